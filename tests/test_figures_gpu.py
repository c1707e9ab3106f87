"""Figures on the MI355X: the multi-view resampling kernel against the single-view one, the frame compositor against a
numpy restatement of make_grid + clamp + ``(x * 255).astype(int)``, Generator.render_views against forward(), every
batched figure against its reference-shaped per-frame rendering, HoloGAN's numpy stream across (training step,
figures, training step), and the runner end to end with ``figures=true``.  (What the reference's callbacks do is
restated in tests/test_figures_cpu.py.)"""
import hashlib
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from lightning_gan_zoo_amd import functional as F
from lightning_gan_zoo_amd.config import locate, make_cfg
from lightning_gan_zoo_amd.core.figures import types as T
from lightning_gan_zoo_amd.core.models.hologan_generator import Generator, view_inverse_matrices

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_ARGS = {"elevation_low": 70, "elevation_high": 110, "azimuth_low": 220, "azimuth_high": 320, "scale_low": 1,
             "scale_high": 1, "transX_low": 0, "transX_high": 0, "transY_low": 0, "transY_high": 0, "transZ_low": 0,
             "transZ_high": 0, "batch_size": 32}


def random_views(n, seed):
    """Views beyond the training ranges (any azimuth / elevation, zoom, shifts): clamped corners included."""
    rng = np.random.RandomState(seed)
    v = np.zeros((n, 6))
    v[:, 0] = rng.uniform(0, 2 * math.pi, n)
    v[:, 1] = rng.uniform(-1.2, 1.2, n)
    v[:, 2] = rng.uniform(0.7, 1.3, n)
    v[:, 3:] = rng.uniform(-1.5, 1.5, (n, 3))
    return v


@pytest.mark.parametrize("C", [64, 6])
@pytest.mark.parametrize("V", [1, 5, 40])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_multi_view_resample_is_bit_equal_to_the_single_view_kernel(B, V, C):
    S = 16
    g = torch.Generator().manual_seed(B * 100 + V * 10 + C)
    vox = torch.randn(B, C, S, S, S, generator=g).to(DEV)
    minv = view_inverse_matrices(random_views(B * V, B + V + C)).reshape(B * V, 16).contiguous().to(DEV)
    got = F.rigid_resample_views(vox, minv)
    want = F.rigid_resample(vox.repeat_interleave(V, 0).contiguous(), minv)
    assert got.shape == (B * V, C * S, S, S)
    assert torch.equal(got, want)


def make_grid_np(imgs, ncol, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid(normalize=False) restated over a numpy [n, C, H, W] array -> [3, GH, GW]."""
    if imgs.shape[1] == 1:
        imgs = np.concatenate([imgs] * 3, axis=1)
    n, C, H, W = imgs.shape
    if n == 1:
        return imgs[0]
    xm = min(ncol, n)
    ym = int(math.ceil(n / xm))
    h, w = H + padding, W + padding
    grid = np.full((C, h * ym + padding, w * xm + padding), pad_value, np.float32)
    k = 0
    for y in range(ym):
        for x in range(xm):
            if k >= n:
                break
            grid[:, y * h + padding:(y + 1) * h, x * w + padding:(x + 1) * w] = imgs[k]
            k += 1
    return grid


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("frames,n,ncol", [(1, 16, 4), (3, 7, 3), (2, 5, 8), (2, 1, 4), (40, 16, 4)])
def test_frame_compositor_is_byte_equal_to_numpy(C, frames, n, ncol):
    rng = np.random.RandomState(frames * 31 + n * 7 + C)
    img = rng.uniform(-0.5, 1.5, (frames * n, C, 9, 7)).astype(np.float32)
    exact = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)     # k / 255: truncation edges
    flat = img.reshape(-1)
    m = min(256, flat.size - 4)
    flat[:m] = exact[np.linspace(0, 255, m).astype(int)]
    flat[m:m + 4] = [0.0, 1.0, -0.0, 1.0000001]
    got = F.figure_frames_u8(torch.from_numpy(img).to(DEV), frames, ncol).cpu().numpy()
    for f in range(frames):
        grid = make_grid_np(img[f * n:(f + 1) * n], ncol)
        want = (np.clip(grid.transpose(1, 2, 0), 0, 1).astype(np.float32) * 255).astype(int).astype(np.uint8)
        assert got[f].shape == want.shape
        assert np.array_equal(got[f], want), f


@pytest.mark.parametrize("img_size", [64, 128])
def test_render_views_matches_forward(img_size):
    torch.manual_seed(0)
    g = Generator(8, 3, 16, VIEW_ARGS, img_size, ext128=img_size == 128).to(DEV).eval()
    z = (torch.rand(3, 16) * 2 - 1).to(DEV)
    shared, per = random_views(5, 1), random_views(3 * 4, 2).reshape(3, 4, 6)
    with torch.no_grad():
        r = g.render_views(z, shared)
        assert r.shape == (3, 5, 3, img_size, img_size)
        for b in range(3):
            for v in range(5):
                ref = g(z[b:b + 1], view_in=shared[v:v + 1])[0]
                assert (r[b, v] - ref).abs().max().item() < 1e-5
        r2 = g.render_views(z, torch.from_numpy(per), max_rows=4)          # [B, V, 6] views, one object per chunk
        for b in range(3):
            ref = g(z[b:b + 1].repeat(4, 1), view_in=per[b])
            assert (r2[b] - ref).abs().max().item() < 1e-5


def small_module(expt, tmp_path):
    cfg = make_cfg(expt, features=8, noise_dim=16, batch_size=8)
    torch.manual_seed(1)
    np.random.seed(1)
    return cfg, locate(cfg.model.lm["_target_"])(cfg, logging_dir=str(tmp_path)).to(DEV)


@pytest.mark.parametrize("expt", ["dc_gan", "hologan"])
def test_batched_figures_match_the_per_frame_rendering(tmp_path, expt):
    cfg, module = small_module(expt, tmp_path)
    module.eval()
    figs = T.build_figures(cfg, module, str(tmp_path))
    with torch.no_grad():
        for fig in figs:
            plan = fig.plan(module)
            cells, frames = fig.render(module, plan)
            ref_cells, ref_frames = fig.render_per_frame(module, plan)
            name = type(fig).__name__
            assert cells.shape == ref_cells.shape and frames.shape == ref_frames.shape, name
            assert (cells - ref_cells).abs().max().item() < 1e-5, name
            assert (frames.int() - ref_frames.int()).abs().max().item() <= 1, name


def test_hologan_numpy_stream_across_step_figures_step(tmp_path):
    """(training step, figures, training step): the second step's view is the one a reference-order replay draws --
    figure draws first, then the step's view -- and the "numpy's global generator was used" warning stays silent."""
    from lightning_gan_zoo_amd.harness import Trainer
    from lightning_gan_zoo_amd.run_network import EpochFigures
    cfg, module = small_module("hologan", tmp_path)
    trainer = Trainer(module)
    real = (torch.rand(8, 3, 64, 64) * 2 - 1).to(DEV)
    batch = (real, torch.zeros(8, dtype=torch.int64, device=DEV))
    trainer.step(batch)
    gen = module.generator
    assert gen._prefetched is not None
    before = gen._prefetched[1]
    draw = gen.sample_view
    seen = []
    gen.sample_view = lambda n: seen.append(draw(n)) or seen[-1]
    figures = EpochFigures(T.build_figures(cfg, module, str(tmp_path)), have_fid=False)
    Generator._warned_numpy_touched = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        figures(module, 0, None)
        n_fig = len(seen)
        trainer.step(batch)
    assert module.training and n_fig == 3           # SampleGrid's view, Interpolation3d's p1 and p2
    np.random.set_state(before)
    replay = [draw(16), draw(16), draw(16), draw(8)]
    for a, b in zip(seen[:n_fig + 1], replay):
        assert np.array_equal(a, b)


def gif_frames(path):
    from PIL import Image
    with Image.open(path) as im:
        total = 0
        for i in range(im.n_frames):
            im.seek(i)
            total += im.info["duration"]
    return total // 40


RUN = ("import sys, hashlib, numpy as np, torch\n"
       "from lightning_gan_zoo_amd import run_network as R\n"
       "R.main(sys.argv[1:])\n"
       "s = np.random.get_state()\n"
       "print('RNG', hashlib.sha256(s[1].tobytes()).hexdigest(), s[2], "
       "hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest())\n")


def run_runner(tmp_path, expt, extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-c", RUN, "+expt=" + expt, "dataset=synthetic", "model.noise_dim=16", "train.batch_size=8",
           "log_every=1000", "max_steps=4", "steps_per_epoch=2"]
    cmd += (["train.features_gen=8", "train.features_disc=8"] if expt == "dc_gan"
            else ["generator.in_planes=8", "discriminator.out_planes=8"])
    r = subprocess.run(cmd + extra, env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return [l for l in r.stdout.splitlines() if l.startswith("RNG ")][-1], r.stdout


def test_runner_writes_dc_gan_figures_every_epoch(tmp_path):
    from PIL import Image
    _, out = run_runner(tmp_path, "dc_gan", ["figures=true", "figure_details.save_all=true"])
    assert "monitor is off" in out
    for e in (0, 1):
        d = tmp_path / "output" / "figures" / ("epoch_%d" % e)
        assert sorted(os.listdir(d)) == ["Interpolation.gif", "SampleGrid.png"]
        with Image.open(d / "SampleGrid.png") as im:
            assert im.size == (266, 266)
        assert gif_frames(d / "Interpolation.gif") == 80


def test_runner_writes_hologan_figures_and_is_unchanged_without_them(tmp_path):
    from PIL import Image
    on = tmp_path / "on"
    on.mkdir()
    run_runner(on, "hologan", ["figures=true", "figure_details.save_all=true"])
    for e in (0, 1):
        d = on / "output" / "figures" / ("epoch_%d" % e)
        assert sorted(os.listdir(d)) == ["AzimuthGif.gif", "AzimuthStep.png", "ElevationGif.gif", "ElevationStep.png",
                                         "Interpolation3d.gif", "SampleGrid.png"]
        with Image.open(d / "ElevationStep.png") as im:
            assert im.size == (530, 266)
        with Image.open(d / "AzimuthStep.png") as im:
            assert im.size == (530, 266)
        assert gif_frames(d / "ElevationGif.gif") == 80
    off, default = tmp_path / "off", tmp_path / "default"
    off.mkdir()
    default.mkdir()
    rng_off, _ = run_runner(off, "hologan", ["figures=false"])
    rng_default, _ = run_runner(default, "hologan", [])
    assert rng_off == rng_default
    assert not (off / "output").exists() and not (default / "output").exists()

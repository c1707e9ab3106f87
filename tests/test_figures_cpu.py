"""Figures on the host: the plan (host random draws, views, frame / cell order) and the write stage (PNG, GIF, paths)
of lightning_gan_zoo_amd.core.figures.types against restatements of the reference's callbacks, and the runner's
``figures`` key.  The generator here is a small elementwise torch function: no product kernel runs.

What the reference does (core/figures/types.py; restated, not imported):
  * Figure.__init__ (:43-51): ``save_dir = parent_dir/cfg.dir``, ``filename = cfg.filename or ClassName.png``
    (AnimationFigure :97-98: ``.gif``), best metric starts at inf.
  * on_validation_end (:78-91): with a monitor, draw only when ``metric < best`` (strict), which becomes the best.
  * Figure.save (:61-71): ``(array * 255).astype(int)`` then imageio.imwrite, whose ``image_as_uint`` stretches an
    integer array's min..max to 0..255 (``(im - mi) / (ma - mi) * 255 + 0.499999999`` in float64, then uint8; a
    constant array is cast as it is); with ``save_all`` under ``epoch_<current_epoch>/`` (:75).
  * AnimationFigure.save (:109-130): ``(array * 255).astype('uint8')[:, :, :3]`` per frame, PIL RGB images, saved with
    ``save_all=True, append_images=frames[1:], optimize=False, duration=n_frames, loop=0``; the frame list is
    ``frames + frames[::-1]`` (:258, :287, :316, :353).
  * SampleGrid (:174-180): one z of ncol**2 (noise_distn.sample), generator(z) -- HoloGAN draws its view inside.
  * Interpolation (:245-259): z1, z2 of 16 each; frames over np.linspace(0, 1, n_frames), 16 images, rows of 4.
  * Interpolation3d (:270-288): z1, z2, p1 = sample_view(16), p2 = sample_view(16); frame view p2 * t + p1 * (1 - t).
  * ElevationStep (:223-239): one z of n_objs; for i in torch.linspace(el_low, el_high, n_steps) the view
    ``torch.tensor([fixed_azimuth * pi / 180, i * pi / 180, 1.0, 0, 0, 0])`` repeated; rows = objects (permute(1, 0)),
    make_grid nrow = n_steps.
  * ElevationGif (:300-322): one z of num_objs; the same views over torch.linspace(el_low, el_high, 40); 4 x 4 grid.
  * AzimuthStep / AzimuthGif (:188-215, :330-359): z of n_objs / ncol**2; their cameras do not exist for HoloGAN.
    This package's deviation: azimuth over torch.linspace(az_low, az_high, n), elevation at the middle, views built
    like ElevationStep's (``torch.tensor([i * pi / 180, fixed_elevation * pi / 180, 1.0, 0, 0, 0])``).
"""
import io
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from lightning_gan_zoo_amd.config import make_cfg, to_cfg
from lightning_gan_zoo_amd.core.figures import types as T
from lightning_gan_zoo_amd.core.models.hologan_generator import Generator as HoloGenerator

VIEW_ARGS = {"elevation_low": 70, "elevation_high": 110, "azimuth_low": 220, "azimuth_high": 320, "scale_low": 1,
             "scale_high": 1, "transX_low": 0, "transX_high": 0, "transY_low": 0, "transY_high": 0, "transZ_low": 0,
             "transZ_high": 0, "batch_size": 32}
Z = 8


class FakeGenerator(torch.nn.Module):
    """Per-image elementwise function of its latent (and view): [n, 3, 6, 5] in about [-1, 1]."""

    def __init__(self, views):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.5, 3 * 6 * 5).reshape(1, 3, 6, 5))
        self.view_args = VIEW_ARGS
        self.has_views = views

    def forward(self, z, view_in=None):
        base = z[:, :1, None, None] * self.w + z[:, 1:2, None, None]
        if self.has_views:
            v = torch.as_tensor(view_in).float()
            base = base + v[:, :1, None, None] - v[:, 1:2, None, None]
        return torch.tanh(base)

    def render_views(self, z, views):
        views = torch.as_tensor(views)
        return torch.stack([torch.stack([self(z[b:b + 1], views[v:v + 1])[0] for v in range(len(views))])
                            for b in range(len(z))])


class FakeModule:
    def __init__(self, views):
        self.generator = FakeGenerator(views)
        if views:
            self.generator.sample_view = lambda n: HoloGenerator.sample_view(self.generator, n)
        self.noise_distn = torch.distributions.uniform.Uniform(-1, 1)
        self.cfg = to_cfg({"model": {"noise_dim": Z}, "generator": {"view_args": VIEW_ARGS}})


def details(**kw):
    d = {"dir": "figures", "filename": "", "fid_callback": True, "save_all": False, "img_size": 64,
         "data_mean": 0.5, "data_std": 0.5, "channels_img": 3}
    d.update(kw)
    return to_cfg(d)


def seed(s=3):
    torch.manual_seed(s)
    np.random.seed(s)


def states():
    return torch.get_rng_state(), np.random.get_state()


def assert_same_states(a, b):
    assert torch.equal(a[0], b[0])
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def sample(n):
    return torch.distributions.uniform.Uniform(-1, 1).sample((n, Z))


# ---- restatements of the reference's draw code ----------------------------------------------------------------------
def ref_step_views(low, high, n, fixed, azimuth):
    out = []
    for i in torch.linspace(low, high, n):
        if azimuth:
            out.append(torch.tensor([i * math.pi / 180, fixed * math.pi / 180, 1.0, 0, 0, 0]))
        else:
            out.append(torch.tensor([fixed * math.pi / 180, i * math.pi / 180, 1.0, 0, 0, 0]))
    return out


def ref_sample_view(n):
    return HoloGenerator.sample_view(FakeGenerator(True), n)


@pytest.mark.parametrize("views", [False, True])
def test_sample_grid_draws(tmp_path, views):
    m = FakeModule(views)
    seed()
    plan = T.SampleGrid(details(), str(tmp_path), ncol=3).plan(m)
    got = states()
    seed()
    z = sample(9)
    v = ref_sample_view(9) if views else None
    assert_same_states(got, states())
    assert torch.equal(plan["z"], z) and plan["frames"] == 1 and plan["ncol"] == 3
    assert (plan["views"] is None) if not views else np.array_equal(plan["views"], v)


def test_interpolation_draws_and_frame_order(tmp_path):
    m = FakeModule(False)
    fig = T.Interpolation(details(), str(tmp_path))
    seed()
    plan = fig.plan(m)
    got = states()
    seed()
    z1, z2 = sample(16), sample(16)
    assert_same_states(got, states())
    assert torch.equal(plan["z1"], z1) and torch.equal(plan["z2"], z2) and plan["frames"] == 40
    # the reference's per-frame loop: generator(interpolate_sphere(z1, z2, t)) for t in np.linspace(0, 1, 40)
    from lightning_gan_zoo_amd.core.utils.utils import interpolate_sphere
    want = torch.cat([m.generator(interpolate_sphere(z1, z2, float(t)))[:16] for t in np.linspace(0, 1, 40)])
    assert torch.equal(fig.render_cells(m, plan), want)
    assert torch.equal(fig.render_cells_per_frame(m, plan), want)


def test_interpolation3d_draws_and_float64_views(tmp_path):
    m = FakeModule(True)
    fig = T.Interpolation3d(details(), str(tmp_path))
    seed()
    plan = fig.plan(m)
    got = states()
    seed()
    z1, z2 = sample(16), sample(16)
    p1, p2 = ref_sample_view(16), ref_sample_view(16)
    assert_same_states(got, states())
    assert torch.equal(plan["z1"], z1) and torch.equal(plan["z2"], z2)
    frames = fig.frame_views(plan)
    assert len(frames) == 40
    for t, p in zip(np.linspace(0, 1, 40), frames):
        ref = p2 * t + p1 * (1 - t)
        assert p.dtype == np.float64 and np.array_equal(p, ref)
    from lightning_gan_zoo_amd.core.utils.utils import interpolate_sphere
    want = torch.cat([m.generator(interpolate_sphere(z1, z2, float(t)), view_in=p2 * t + p1 * (1 - t))
                      for t in np.linspace(0, 1, 40)])
    assert torch.equal(fig.render_cells(m, plan), want)


@pytest.mark.parametrize("cls,azimuth", [(T.ElevationStep, False), (T.AzimuthStep, True)])
def test_step_grid_draws_views_and_cell_order(tmp_path, cls, azimuth):
    m = FakeModule(True)
    fig = cls(details(), str(tmp_path), n_steps=5, n_objs=3)
    seed()
    plan = fig.plan(m)
    got = states()
    seed()
    z = sample(3)
    assert_same_states(got, states())                    # the views consume nothing
    fixed = (110 + 70) / 2 if azimuth else (320 + 220) / 2
    ref = ref_step_views(220, 320, 5, fixed, True) if azimuth else ref_step_views(70, 110, 5, fixed, False)
    assert torch.equal(plan["z"], z) and plan["views"].dtype == torch.float32
    assert all(torch.equal(plan["views"][i], ref[i]) for i in range(5))     # bit for bit: fp32 / fp64 rounding
    # rows = objects, columns = steps: stack(columns).permute(1, 0, ...) then cat(rows)
    cols = [m.generator(z, view_in=v.repeat(3, 1)) for v in ref]
    want = torch.cat(list(torch.stack(cols).permute(1, 0, 2, 3, 4)))
    assert torch.equal(fig.render_cells(m, plan), want)
    assert torch.equal(fig.render_cells_per_frame(m, plan), want)
    assert plan["ncol"] == 5 and plan["frames"] == 1


@pytest.mark.parametrize("cls,azimuth", [(T.ElevationGif, False), (T.AzimuthGif, True)])
def test_view_gif_draws_views_and_frame_order(tmp_path, cls, azimuth):
    m = FakeModule(True)
    fig = cls(details(), str(tmp_path))
    seed()
    plan = fig.plan(m)
    got = states()
    seed()
    z = sample(16)
    assert_same_states(got, states())
    fixed = (110 + 70) / 2 if azimuth else (320 + 220) / 2
    ref = ref_step_views(220, 320, 40, fixed, True) if azimuth else ref_step_views(70, 110, 40, fixed, False)
    assert torch.equal(plan["z"], z) and all(torch.equal(plan["views"][i], ref[i]) for i in range(40))
    want = torch.cat([m.generator(z, view_in=v.repeat(16, 1))[:16] for v in ref])       # frame after frame, 16 cells
    assert torch.equal(fig.render_cells(m, plan), want)
    assert torch.equal(fig.render_cells_per_frame(m, plan), want)
    assert plan["frames"] == 40 and plan["ncol"] == 4


def test_small_configs_and_three_d_figures_need_views(tmp_path):
    assert T.SampleGrid(details(), str(tmp_path), ncol=3).ncol == 3              # sample_grid_small.yaml
    g = T.AzimuthGif(details(), str(tmp_path), ncol=2)                            # azimuth_gif_small.yaml
    seed()
    assert g.plan(FakeModule(True))["z"].shape == (4, Z)
    for cls in (T.Interpolation3d, T.ElevationStep, T.AzimuthStep, T.ElevationGif, T.AzimuthGif):
        with pytest.raises(ValueError, match="3-D figure"):
            cls(details(), str(tmp_path)).check_generator(FakeGenerator(False))


# ---- write -----------------------------------------------------------------------------------------------------------
def imageio_stretch(im):
    """imageio 2.9 core/util.py image_as_uint for an int64 array, restated."""
    im = np.asarray(im)
    mi, ma = np.nanmin(im), np.nanmax(im)
    if ma == mi:
        return im.astype(np.uint8)
    im = im.astype("float64")
    return ((im - mi) / (ma - mi) * (np.power(2.0, 8) - 1) + 0.499999999).astype(np.uint8)


def pre_encoding(grid_float):
    return (np.clip(grid_float, 0, 1).astype(np.float32) * 255).astype(int)


@pytest.mark.parametrize("case", ["random", "constant", "one_channel"])
def test_png_pixels_are_the_stretched_integer_array(tmp_path, case):
    rng = np.random.RandomState(0)
    if case == "random":
        grid = rng.uniform(0.1, 0.8, (14, 10, 3)).astype(np.float32)
    elif case == "constant":
        grid = np.full((14, 10, 3), 0.3, np.float32)
    else:
        grid = np.repeat(rng.uniform(-0.5, 1.5, (14, 10, 1)).astype(np.float32), 3, axis=2)   # make_grid's repeat
    arr = pre_encoding(grid)
    fig = T.SampleGrid(details(), str(tmp_path))
    path = fig.write(arr.astype(np.uint8)[None], epoch=0)
    assert path == os.path.join(str(tmp_path), "figures", "SampleGrid.png")
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (10, 14)
        assert np.array_equal(np.asarray(im), imageio_stretch(arr))
    if case == "constant":
        assert np.array_equal(np.asarray(Image.open(path)), arr.astype(np.uint8))      # no stretch at all


def test_gif_is_byte_equal_to_the_reference_call(tmp_path):
    rng = np.random.RandomState(1)
    frames = (rng.uniform(0, 1, (40, 12, 16, 3)).astype(np.float32) * 255).astype("uint8")
    fig = T.Interpolation(details(save_all=True), str(tmp_path))
    path = fig.write(frames, epoch=3)
    assert path == os.path.join(str(tmp_path), "figures", "epoch_3", "Interpolation.gif")
    seq = list(frames) + list(frames)[::-1]
    pil = [Image.fromarray(a[:, :, :3], "RGB") for a in seq]
    buf = io.BytesIO()
    pil[0].save(buf, format="GIF", save_all=True, append_images=pil[1:], optimize=False, duration=40, loop=0)
    with open(path, "rb") as f:
        assert f.read() == buf.getvalue()
    assert len(seq) == 80
    with Image.open(path) as im:
        assert gif_frames(im) == 80 and im.info["loop"] == 0


def gif_frames(im):
    """Frames of 40 ms in a GIF written with duration=40: PIL merges consecutive identical frames (the turning point
    of ``frames + frames[::-1]``) into one frame of their summed duration."""
    total = 0
    for i in range(im.n_frames):
        im.seek(i)
        total += im.info["duration"]
    assert total % 40 == 0
    return total // 40


def test_file_names_and_epoch_directories(tmp_path):
    d = details(dir="figs")
    assert T.ElevationGif(d, str(tmp_path)).out_path(0) == os.path.join(str(tmp_path), "figs", "ElevationGif.gif")
    assert T.AzimuthStep(d, str(tmp_path)).out_path(5) == os.path.join(str(tmp_path), "figs", "AzimuthStep.png")
    assert os.path.isdir(os.path.join(str(tmp_path), "figs"))           # created at construction, as the reference
    named = T.SampleGrid(details(filename="grid.png", save_all=True), str(tmp_path))
    assert named.out_path(2) == os.path.join(str(tmp_path), "figures", "epoch_2", "grid.png")


def test_monitor_rule(tmp_path, capsys):
    fig = T.SampleGrid(details(), str(tmp_path), monitor="fid")
    assert [fig.should_draw(s) for s in (30.0, 31.0, 30.0, 29.5, 12.0, 12.0)] == [True, False, False, True, True,
                                                                                 False]
    assert fig.current_best_metric == 12.0
    assert "Skipping figures" in capsys.readouterr().out
    free = T.SampleGrid(details(fid_callback=False), str(tmp_path), monitor=None)
    assert all(free.should_draw(s) for s in (3.0, 4.0, None))
    assert all(fig.should_draw(None) for _ in range(3))             # no FID produced: every epoch


# ---- configuration and runner ----------------------------------------------------------------------------------------
def test_hologan_instantiates_six_figures_in_defaults_order(tmp_path):
    from lightning_gan_zoo_amd.core.models.hologan_generator import Generator
    cfg = make_cfg("hologan", features=4, noise_dim=8)

    class M:
        generator = Generator(4, 3, 8, cfg.generator.view_args, 64)

    figs = T.build_figures(cfg, M, str(tmp_path))
    assert [type(f).__name__ for f in figs] == ["SampleGrid", "Interpolation3d", "AzimuthStep", "ElevationStep",
                                                "AzimuthGif", "ElevationGif"]
    assert all(f.monitor == "fid" for f in figs)
    assert [type(f).__name__ for f in T.build_figures(make_cfg("wgan"), M, str(tmp_path))] == ["SampleGrid",
                                                                                               "Interpolation"]


def test_three_d_figures_for_a_generator_without_views_fail_at_construction(tmp_path):
    from lightning_gan_zoo_amd.core.models.standard_networks import Generator
    cfg = make_cfg("hologan", features=4, noise_dim=8)

    class M:
        generator = Generator(8, 3, 4)

    with pytest.raises(ValueError, match="Interpolation3d is a 3-D figure"):
        T.build_figures(cfg, M, str(tmp_path))


def test_runner_key_figures_defaults_off():
    from lightning_gan_zoo_amd import run_network as R
    assert R.parse_overrides(["+expt=dc_gan"])[3]["figures"] is False
    _, _, rest, run = R.parse_overrides(["+expt=dc_gan", "figures=true", "figure_details.save_all=true"])
    assert run["figures"] is True and rest == ["+expt=dc_gan", "figure_details.save_all=true"]
    cfg = R.compose(None, "dc_gan", rest, run)
    assert cfg.figure_details.save_all is True and list(cfg.figures) == ["sample_grid", "interpolation"]


def test_dropping_the_prefetched_view_restores_numpy_state():
    g = HoloGenerator(4, 3, 8, VIEW_ARGS, 64)
    np.random.seed(5)
    before = np.random.get_state()
    g.prefetch_view(6)
    assert not np.array_equal(np.random.get_state()[1], before[1]) or np.random.get_state()[2] != before[2]
    g.drop_prefetched_view()
    assert_same_states((torch.zeros(1), np.random.get_state()), (torch.zeros(1), before))
    assert g._prefetched is None
    g.drop_prefetched_view()                                         # nothing pending: no-op

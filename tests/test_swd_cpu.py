"""The numpy yardsticks of the sliced Wasserstein distance (eval.laplacian_pyramid, swd_descriptors, sliced_wasserstein, swd),
the plan's draws, the runner's keys and the C ABI's argument checks -- everything of the metric that needs no GPU.  The
device kernels are held to these yardsticks in tests/test_swd_gpu.py; tests/swd_support.py derives the bounds."""
import ctypes

import numpy as np
import pytest
import torch

from lightning_gan_zoo_amd import eval as E
from swd_support import (END_TO_END_CASES, PYRAMID_CASES, end_to_end_bound, end_to_end_inputs, host_end_to_end,
                         host_pyramid, pyramid_fp32, ternary_images)


def _small_sets(seed=0, n=6, c=3, s=32):
    rng = np.random.RandomState(seed)
    a = rng.randn(n, c, s, s)
    b = np.cumsum(rng.randn(n, c, s, s), axis=3) * 0.3
    plan = E.SwdPlan(s, c, n, patches=12, dirs=6, repeats=3, seed=seed + 1)
    return a, b, plan


def test_the_distance_of_a_set_to_itself_is_exactly_zero():
    a, _, plan = _small_sets()
    out = E.swd(a, a, plan.positions, plan.directions, plan.repeats)
    assert set(out) == {"swd_32", "swd_16", "swd"}
    assert all(v == 0.0 for v in out.values())


def test_the_statistic_is_symmetric_in_the_two_sets():
    a, b, plan = _small_sets(1)
    ab = E.swd(a, b, plan.positions, plan.directions, plan.repeats)
    ba = E.swd(b, a, plan.positions, plan.directions, plan.repeats)
    assert ab == ba and ab["swd"] > 10.0
    assert ab["swd"] == pytest.approx(np.mean([ab["swd_32"], ab["swd_16"]]), rel=1e-15)


def test_a_per_channel_affine_map_of_one_set_changes_nothing():
    """What normalisation promises: x -> scale_c x + shift_c commutes with the (linear, tap sum 1) pyramid and cancels in
    (d - mean_c) / std_c.  The Laplacian levels lose the shift, the coarsest level keeps it; both are covered."""
    a, b, plan = _small_sets(2)
    scale, shift = np.array([2.0, 0.5, 3.0])[None, :, None, None], np.array([0.25, -1.0, 4.0])[None, :, None, None]
    want = E.swd(a, b, plan.positions, plan.directions, plan.repeats)
    got = E.swd(a, scale * b + shift, plan.positions, plan.directions, plan.repeats)
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-11), key


def test_one_dimensional_sets_give_the_closed_form():
    rng = np.random.RandomState(3)
    a, b = rng.randn(101, 1), 0.5 + 2.0 * rng.randn(101, 1)
    want = np.abs(np.sort(a[:, 0]) - np.sort(b[:, 0])).mean()
    assert E.sliced_wasserstein(a, b, np.array([[1.0]])) == pytest.approx(want, rel=1e-15)
    assert E.sliced_wasserstein(a, b, np.array([[1.0], [-1.0]]), repeats=2) == pytest.approx(want, rel=1e-15)
    with pytest.raises(ValueError, match="equal shapes"):
        E.sliced_wasserstein(a, b[:-1], np.array([[1.0]]))


def test_a_collapsed_channel_divides_by_one_and_stays_finite():
    desc = np.concatenate([np.random.RandomState(4).randn(20, 49), np.full((20, 49), 0.3)], axis=1)
    x = E.swd_normalise(desc, 2)
    assert np.isfinite(x).all() and (x[:, 49:] == 0.0).all()
    assert x[:, :49].std() == pytest.approx(1.0, rel=1e-12)


@pytest.mark.parametrize("size", [16, 32, 33])
def test_mirror_borders_are_torchs_reflect_padding(size):
    """down = conv2d(reflect-pad 2, taps x taps) at stride 2; up = zero insertion, then conv2d(reflect-pad 2, 4 taps x
    taps).  An odd size too: the yardstick's filter does not care, and n -> n - 2 is then checked at an odd border."""
    x = torch.from_numpy(np.random.RandomState(size).randn(2, 3, size, size))
    taps = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16.0
    kernel = (taps[:, None] * taps[None, :])[None, None].repeat(3, 1, 1, 1)
    padded = torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect")
    full = torch.nn.functional.conv2d(padded, kernel, groups=3)
    got = E._swd_filter(E._swd_filter(x.numpy(), -1, E.SWD_TAPS), -2, E.SWD_TAPS)
    assert np.abs(got - full.numpy()).max() < 1e-14
    if size % 2 == 0:
        assert np.abs(E.swd_down(x.numpy()) - full[..., ::2, ::2].numpy()).max() < 1e-14
        y = torch.from_numpy(E.swd_down(x.numpy()))
        z = torch.zeros(2, 3, size, size, dtype=torch.float64)
        z[..., ::2, ::2] = y
        up = torch.nn.functional.conv2d(torch.nn.functional.pad(z, (2, 2, 2, 2), mode="reflect"), 4.0 * kernel, groups=3)
        assert np.abs(E.swd_up(y.numpy()) - up.numpy()).max() < 1e-14


def test_descriptors_are_ordered_channel_dy_dx():
    level = np.arange(2 * 3 * 16 * 16, dtype=np.float64).reshape(2, 3, 16, 16)
    pos = np.array([[[3, 3], [12, 5]], [[7, 12], [3, 12]]])
    d = E.swd_descriptors(level, pos)
    assert d.shape == (4, 147)
    for row, (image, (cy, cx)) in enumerate([(0, (3, 3)), (0, (12, 5)), (1, (7, 12)), (1, (3, 12))]):
        for c, dy, dx in ((0, 0, 0), (1, 3, 3), (2, 6, 0), (2, 6, 6), (0, 2, 5)):
            assert d[row, (c * 7 + dy) * 7 + dx] == level[image, c, cy - 3 + dy, cx - 3 + dx]
    with pytest.raises(ValueError, match="centres"):
        E.swd_descriptors(level, np.array([[[2, 3]], [[3, 3]]]))
    with pytest.raises(ValueError, match="centres"):
        E.swd_descriptors(level, np.array([[[3, 13]], [[3, 3]]]))


@pytest.mark.parametrize("case", PYRAMID_CASES, ids=str)
def test_ternary_pyramids_are_exact_in_fp32_up_to_size_64(case):
    """Values in {-1, 0, 1}: every intermediate of the pyramid is a multiple of a power of two small enough for 24 bits
    up to three levels, so fp32 arithmetic in ANY summation order gives the fp64 values: the GPU test may ask for equal
    bits there.  At S = 128 the level G_2 - up(G_3) needs more bits; there (only) fp32 differs."""
    want = host_pyramid("ternary", case)
    exact = [np.array_equal(f.astype(np.float64), w) and np.array_equal(r.astype(np.float64), w)
             for f, r, w in zip(pyramid_fp32(ternary_images(case)), pyramid_fp32(ternary_images(case), reverse=True), want)]
    assert len(want) == {16: 1, 32: 2, 64: 3, 128: 4}[case[2]]
    if case[2] <= 64:
        assert all(exact)
    else:
        assert exact == [True, True, False, True]
    if case[2] == 16:
        assert np.array_equal(want[0], ternary_images(case).astype(np.float64))       # the single level is the image


def test_the_plan_draws_from_its_own_generator_and_leaves_the_global_ones_alone():
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg("dc_gan", batch_size=4, features=8, noise_dim=16)
    torch.manual_seed(7)
    np.random.seed(7)
    module = locate(cfg.model.lm["_target_"])(cfg, None)
    t0, n0 = torch.get_rng_state().clone(), np.random.get_state()
    plan = E.SwdPlan(64, 3, 10, patches=5, dirs=4, repeats=2, seed=9, module=module)
    again = E.SwdPlan(64, 3, 10, patches=5, dirs=4, repeats=2, seed=9, module=module)
    other = E.SwdPlan(64, 3, 10, patches=5, dirs=4, repeats=2, seed=10, module=module)
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    assert plan.sizes == [64, 32, 16] and plan.latents.shape == (10, 16)
    for h, pos, dirs in zip(plan.sizes, plan.positions, plan.directions):
        assert pos.shape == (10, 5, 2) and pos.dtype == np.int32 and pos.min() >= 3 and pos.max() <= h - 4
        assert dirs.shape == (8, 147) and dirs.dtype == np.float32
        assert np.abs(np.sqrt((dirs.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    assert torch.equal(plan.latents, again.latents) and not torch.equal(plan.latents, other.latents)
    assert all(np.array_equal(a, b) for a, b in zip(plan.positions + plan.directions, again.positions + again.directions))
    assert E.SwdPlan(16, 1, 2).latents is None
    with pytest.raises(ValueError):
        E.SwdPlan(48, 3, 2)
    with pytest.raises(ValueError):
        E.SwdPlan(32, 2, 2)


def test_an_evaluation_leaves_the_generators_and_the_mode_alone(monkeypatch):
    """evaluate_swd around stand-ins for the device calls (the real ones: tests/test_swd_gpu.py): a generator that draws
    from numpy's global generator in every call, as HoloGAN's sample_view does, sees the plan's seed and leaves no trace."""
    from lightning_gan_zoo_amd import functional as F
    seen = []

    class Generator(torch.nn.Module):
        def forward(self, z):
            seen.append(np.random.randint(0, 1 << 30))
            torch.rand(3)
            return torch.zeros(len(z), 1, 16, 16)

        def drop_prefetched_view(self):
            seen.append("dropped")

    class Module(torch.nn.Module):
        device = "cpu"

        def __init__(self):
            super().__init__()
            self.generator = Generator()

    class Real:
        def sorted(self, l):
            return "real%d" % l

    plan = E.SwdPlan(16, 1, 5, patches=2, dirs=2, repeats=1, seed=11)
    plan.latents = torch.zeros(5, 4)
    plan.on = lambda device: (["pos"], ["dirs"])
    monkeypatch.setattr(F, "_req", lambda t, name="tensor": t)
    monkeypatch.setattr(E, "laplacian_pyramid_device", lambda x: [x])
    monkeypatch.setattr(E, "swd_sorted_projections_device", lambda level, pos, dirs: "fake")
    monkeypatch.setattr(E, "swd_distance_device", lambda a, b, rows, repeats: 0.25 if (a, b) == ("fake", "real0") else -1)

    class Pos:
        shape = (10, 2)

    plan.on = lambda device: ([Pos()], ["dirs"])
    module = Module().train()
    np.random.seed(3)
    torch.manual_seed(3)
    t0, n0 = torch.get_rng_state().clone(), np.random.get_state()
    first = E.evaluate_swd(module, plan, Real(), batch=2)
    draws, seen[:] = list(seen), []
    second = E.evaluate_swd(module, plan, Real(), batch=2)
    assert first == second == {"swd_16": 250.0, "swd": 250.0}
    assert draws == seen and draws[0] == "dropped" and len(draws) == 4          # 3 batches, the same views every time
    assert module.training and module.generator.training
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    module.eval()
    E.evaluate_swd(module, plan, Real())
    assert not module.training
    with pytest.raises(ValueError, match="no latents"):
        E.evaluate_swd(module, E.SwdPlan(16, 1, 5), Real())


def test_the_device_functions_refuse_host_tensors():
    x = torch.zeros(2, 3, 32, 32)
    for call in (lambda: E.laplacian_pyramid_device(x), lambda: E.swd_device(x, x, [], []),
                 lambda: E.sliced_wasserstein_device(x, x, None, None), lambda: E.laplacian_pyramid_device(x.numpy())):
        with pytest.raises(RuntimeError, match="no fallback"):
            call()


def test_runner_keys_parse_and_are_checked():
    from lightning_gan_zoo_amd import run_network as R
    run = R.parse_overrides(["+expt=dc_gan"])[3]
    assert [run[k] for k in ("swd", "swd_images", "swd_patches", "swd_dirs", "swd_repeats", "swd_seed", "swd_cache_gb")] \
        == [False, 16384, 128, 128, 4, 0, 16]
    run = R.parse_overrides(["+expt=dc_gan", "swd=true", "+swd_images=256", "swd_patches=8", "swd_dirs=16", "swd_repeats=2",
                             "swd_seed=5", "swd_cache_gb=0.5"])[3]
    assert [run[k] for k in ("swd", "swd_images", "swd_patches", "swd_dirs", "swd_repeats", "swd_seed", "swd_cache_gb")] \
        == [True, 256, 8, 16, 2, 5, 0.5]
    assert run["inception_weights"] is None and run["eval_on_device"] is False       # neither is needed
    for bad in ("swd=maybe", "swd_images=0", "swd_patches=-1", "swd_dirs=1.5", "swd_repeats=0", "swd_seed=-1",
                "swd_cache_gb=-2", "swd_images=true"):
        with pytest.raises(SystemExit, match=bad.split("=")[0]):
            R.parse_overrides(["+expt=dc_gan", bad])


def test_the_monitor_is_swd_only_without_an_fid_evaluator(tmp_path):
    from lightning_gan_zoo_amd import run_network as R
    on, off = {"swd": True}, {"swd": False}
    assert R.checkpoint_monitor(False, on) == "swd"
    assert R.checkpoint_monitor(True, on) == "fid"               # FID keeps the monitor when both are on
    assert R.checkpoint_monitor(False, off) == "fid" and R.checkpoint_monitor(True, off) == "fid"
    keeper = R.CheckpointKeeper(str(tmp_path), monitor="swd", filename="model_best-{swd:.2f}")
    written = []
    save = lambda path: (written.append(path), open(path, "w").close())  # noqa: E731
    assert keeper.update({"swd": 31.256, "swd_16": 1.0}, 10, save).endswith("model_best-swd=31.26.ckpt")
    assert keeper.update({"swd": 40.0}, 20, save) is None
    assert keeper.update({"swd": 12.5}, 30, save).endswith("model_best-swd=12.50.ckpt")
    assert [p.name for p in tmp_path.iterdir()] == ["model_best-swd=12.50.ckpt"]


def test_wants_evaluator_widens_wants_fid_and_keeps_its_answers():
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.config import to_cfg
    folder = to_cfg({"dataset": {"_target_": "torchvision.datasets.ImageFolder", "val": {"root": "/v"}}})
    plain = to_cfg({"dataset": {"_target_": "lightning_gan_zoo_amd.run_network.SyntheticImages"}})
    for cfg in (folder, plain):
        for weights in (None, "w.pth"):
            run = dict(R.RUNNER_KEYS, inception_weights=weights)
            assert R.wants_evaluator(cfg, run) == R.wants_fid(cfg, run)                  # today's key sets: unchanged
            assert R.wants_evaluator(cfg, dict(run, swd=True)) is True
    assert R.wants_fid(folder, dict(R.RUNNER_KEYS, inception_weights="w.pth")) is True
    assert R.wants_fid(plain, dict(R.RUNNER_KEYS, swd=True)) is False


def test_the_evaluators_print_the_levels_and_fid_stays_on_the_same_line(monkeypatch, capsys):
    from lightning_gan_zoo_amd import run_network as R
    result = {"fid": 1.0, "kid": 2.0, "kid_std": 0.5}
    monkeypatch.setattr(E, "RealStatistics", lambda *a, **k: "real")
    monkeypatch.setattr(E, "evaluate_device", lambda *a, **k: dict(result))

    class Scorer:
        sizes = [32, 16]
        text = R.SwdScorer.text

        def __call__(self, module):
            return {"swd_32": 12.345, "swd_16": 7.0, "swd": 9.6725}

    class Features:
        device = "net"

    class Module:
        training = False

    both = R.device_fid_evaluator("dump", Features(), "act", "cuda", swd=Scorer())(Module(), 3)
    alone = R.swd_evaluator(Scorer())(Module(), 4)
    assert both == dict(result, swd_32=12.345, swd_16=7.0, swd=9.6725) and alone == Scorer()(None)
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["epoch 3 FID: 1.0000 KID mean: 2.000000 KID stddev: 0.500000 SWD 32: 12.35 16: 7.00 avg: 9.67",
                     "epoch 4 SWD 32: 12.35 16: 7.00 avg: 9.67"]


@pytest.mark.parametrize("case", END_TO_END_CASES, ids=str)
def test_the_end_to_end_bound_is_below_a_thousandth_of_the_value(case):
    """Otherwise the GPU comparison would show nothing.  Values and bounds (1000 x distance): S = 32: 402.3 +- 0.091 and
    376.3 +- 0.101; S = 64: 286.1 +- 0.081, 352.2 +- 0.322 and 405.7 +- 0.232."""
    a, b, plan = end_to_end_inputs(case)
    assert a.shape == b.shape == (8, 3, case[2], case[2]) and (plan.patches, plan.dirs, plan.repeats) == (16, 8, 2)
    value, bound = host_end_to_end(case), end_to_end_bound(case)
    print(case, {k: (round(value[k], 3), round(bound[k], 4)) for k in value})
    assert set(value) == set(bound) == {"swd_%d" % s for s in plan.sizes} | {"swd"}
    for key in value:
        assert 0.0 < bound[key] < 1e-3 * value[key], key


def test_header_declares_the_entry_points_and_they_check_their_arguments():
    from lightning_gan_zoo_amd._lib import lib, parse_header
    protos = parse_header()
    ptr, i32, i64, size = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert protos["gz_swd_pyramid_describe"] == (i32, [i32, i32, i32, ptr, ptr])
    assert protos["gz_swd_pyramid"] == (i32, [ptr, i32, i32, i32, ptr, i64, ptr])
    assert protos["gz_swd_channel_stats"] == (i32, [ptr, i32, i32, i32, ptr, i32, ptr, ptr, size, ptr])
    assert protos["gz_swd_project"] == (i32, [ptr, i32, i32, i32, ptr, i32, ptr, ptr, i32, ptr, i64, ptr])
    assert protos["gz_swd_sort_plan"] == (i32, [i64, ptr, ptr, ptr, ptr])
    assert protos["gz_swd_sort_columns"] == (i32, [ptr, i64, i32, i64, ptr])
    assert protos["gz_swd_distance"] == (i32, [ptr, i64, ptr, i64, i32, i32, i64, ptr, ptr, size, ptr])
    BAD, UNSUPPORTED, WORKSPACE = -1, -2, -3
    p = [ctypes.c_void_p(0x10000 + 0x1000 * i) for i in range(8)]      # never dereferenced: every call is refused
    levels, offsets = ctypes.c_int(0), (ctypes.c_longlong * 5)()
    assert lib.gz_swd_pyramid_describe(2, 3, 128, ctypes.byref(levels), offsets) == 0
    assert levels.value == 4 and list(offsets) == [0, 6 * 16384, 6 * 20480, 6 * 21504, 6 * 21760]
    assert lib.gz_swd_pyramid_describe(1, 1, 16, ctypes.byref(levels), offsets) == 0 and levels.value == 1
    for s in (8, 48, 256, 0):
        assert lib.gz_swd_pyramid_describe(2, 3, s, ctypes.byref(levels), offsets) == UNSUPPORTED
        assert lib.gz_swd_pyramid(p[0], 2, 3, s, p[1], 1 << 40, None) == UNSUPPORTED
    assert lib.gz_swd_pyramid(p[0], 2, 2, 32, p[1], 1 << 40, None) == BAD
    assert lib.gz_swd_pyramid(p[0], 0, 3, 32, p[1], 1 << 40, None) == BAD
    assert lib.gz_swd_pyramid(None, 2, 3, 32, p[1], 1 << 40, None) == BAD
    assert lib.gz_swd_pyramid(p[0], 2, 3, 32, p[1], 6 * 1280 - 1, None) == WORKSPACE
    assert lib.gz_swd_channel_stats_workspace_bytes(4, 3, 32, 0) == 0
    assert lib.gz_swd_channel_stats_workspace_bytes(4, 3, 48, 5) == 0
    need = lib.gz_swd_channel_stats_workspace_bytes(4, 3, 32, 5)
    assert need > 0 and need % 8 == 0
    assert lib.gz_swd_channel_stats(p[0], 4, 3, 32, p[1], 0, p[2], p[3], 1 << 40, None) == BAD
    assert lib.gz_swd_channel_stats(p[0], 4, 3, 32, p[1], 5, p[2], p[3], need - 1, None) == WORKSPACE
    assert lib.gz_swd_project(p[0], 4, 3, 32, p[1], 0, p[2], p[3], 8, p[4], 32, None) == BAD
    assert lib.gz_swd_project(p[0], 4, 3, 32, p[1], 5, p[2], p[3], 0, p[4], 32, None) == BAD
    assert lib.gz_swd_project(p[0], 4, 3, 32, p[1], 5, p[2], p[3], 8, p[4], 31, None) == BAD       # 20 rows pad to 32
    assert lib.gz_swd_sort_columns(p[0], 0, 3, 64, None) == BAD
    assert lib.gz_swd_sort_columns(p[0], 37, 3, 63, None) == BAD and lib.gz_swd_sort_columns(p[0], 37, 3, 66, None) == BAD
    assert lib.gz_swd_sort_columns(ctypes.c_void_p(0x10004), 37, 3, 64, None) == BAD
    assert lib.gz_swd_distance_workspace_bytes(0, 4, 2) == 0 and lib.gz_swd_distance_workspace_bytes(100, 4, 2) == 64
    assert lib.gz_swd_distance(p[0], 100, p[1], 99, 4, 2, 128, p[2], p[3], 1 << 40, None) == BAD    # unequal set sizes
    assert lib.gz_swd_distance(p[0], 100, p[1], 100, 4, 2, 128, p[2], p[3], 63, None) == WORKSPACE


def test_the_sort_plan_counts_the_passes():
    block, padded, bp, gp = E.swd_sort_plan(1)
    assert block == 16384 and (padded, bp, gp) == (1, 1, 0)
    assert E.swd_sort_plan(37)[1:] == (64, 1, 0)
    assert E.swd_sort_plan(block)[1:] == (block, 1, 0) and E.swd_sort_plan(block + 1)[1:] == (2 * block, 2, 1)
    # a phase's global strides go two to a pass while two are left: 1 + 1 + 2 passes for the 1 + 2 + 3 strides of 8 blocks
    assert E.swd_sort_plan(4 * block + 5)[1:] == (8 * block, 4, 4)
    assert E.swd_sort_plan(16384 * 128)[1:] == (1 << 21, 8, 16)          # the default evaluation: 2^21 rows, 28 strides
    with pytest.raises(RuntimeError):
        E.swd_sort_plan(0)


def test_swd_is_refused_with_the_resident_training_set():
    from lightning_gan_zoo_amd import run_network as R
    with pytest.raises(SystemExit, match="resident_data"):
        R.parse_overrides(["+expt=dc_gan", "swd=true", "resident_data=true"])
    assert R.parse_overrides(["+expt=dc_gan", "swd=false", "resident_data=true"])[3]["resident_data"] is True


def _folder_cfg(root, val_root=None, top_level=False):
    from lightning_gan_zoo_amd.config import to_cfg
    node = {"_target_": "torchvision.datasets.ImageFolder", "root": root}
    if not top_level:
        node["train"] = {"root": root}
    if val_root:
        node["val"] = {"root": val_root}
    return to_cfg({"train": {"batch_size": 4, "img_size": 16, "channels_img": 3, "data_mean": 0.5, "data_std": 0.25},
                   "dataset": node})


def test_the_real_images_come_in_dataset_order_through_the_input_step(tmp_path, monkeypatch):
    """run_network.swd_real_images on the host: the device half of the input step (functional.normalize_u8_images) is
    replaced by its formula, everything else is the runner's own code -- the loader's host half, the count and its
    clamp, the validation root's precedence, the training root where ``build_data`` finds it."""
    from PIL import Image
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd import run_network as R
    from test_resident_data import make_folder
    root, val = str(tmp_path / "train"), str(tmp_path / "val")
    make_folder(root)                                              # 6 images, mixed sizes
    (tmp_path / "val" / "only").mkdir(parents=True)
    Image.fromarray(np.full((16, 16, 3), 200, dtype=np.uint8)).save(str(tmp_path / "val" / "only" / "a.png"))
    calls = []

    def normalize(u8, mean, std):
        calls.append(len(u8))
        return (u8.permute(0, 3, 1, 2).double() / 255 - mean) / std

    monkeypatch.setattr(F, "normalize_u8_images", normalize)
    loader = R.ImageFolderImages(root, 4, 16, 3, 0.5, 0.25, "cpu")
    host = loader.host_batches()
    want = normalize(torch.from_numpy(np.concatenate([next(host)[0], next(host)[0]])), 0.5, 0.25)
    assert want.shape == (6, 3, 16, 16)
    for cfg in (_folder_cfg(root), _folder_cfg(root, top_level=True), _folder_cfg(root, val_root=root)):
        for asked, n in ((5, 5), (4, 4), (100, 6)):
            del calls[:]
            got = R.swd_real_images(cfg, dict(R.RUNNER_KEYS, swd_images=asked), "the loader", "cpu")
            assert torch.equal(got, want[:n]) and sum(calls) == n, (asked, calls)
    got = R.swd_real_images(_folder_cfg(root, val_root=val), dict(R.RUNNER_KEYS, swd_images=5), None, "cpu")
    assert got.shape == (1, 3, 16, 16) and torch.equal(got, torch.full_like(got, (200 / 255 - 0.5) / 0.25))
    from lightning_gan_zoo_amd.config import to_cfg
    with pytest.raises(SystemExit, match="ImageFolder-shaped"):
        R.swd_real_images(to_cfg({"train": {}, "dataset": {"_target_": "torchvision.datasets.MNIST"}}),
                          dict(R.RUNNER_KEYS), None, "cpu")


def test_synthetic_and_tensor_file_sets_give_their_own_rows(tmp_path):
    """Dispatch on the data object ``build_data`` made, before the config is looked at: a synthetic run over a folder
    config stays synthetic."""
    from lightning_gan_zoo_amd import run_network as R
    cfg = _folder_cfg(str(tmp_path), val_root=str(tmp_path))       # never opened
    synthetic = R.SyntheticImages(8, 3, 16, "cpu", 1)
    assert torch.equal(R.swd_real_images(cfg, dict(R.RUNNER_KEYS, swd_images=5), synthetic, "cpu"), synthetic.real[:5])
    assert len(R.swd_real_images(cfg, dict(R.RUNNER_KEYS, swd_images=256), synthetic, "cpu")) == 8
    rows = torch.rand(7, 3, 16, 16) * 2 - 1
    path = str(tmp_path / "rows.pt")
    torch.save(rows, path)
    data = R.TensorFileImages(path, 4, "cpu")
    assert torch.equal(R.swd_real_images(cfg, dict(R.RUNNER_KEYS, swd_images=5), data, "cpu"), rows[:5])
    assert torch.equal(R.swd_real_images(cfg, dict(R.RUNNER_KEYS, swd_images=50), data, "cpu"), rows)


def test_the_scorer_draws_its_plan_for_the_images_it_is_given(monkeypatch):
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg("dc_gan", batch_size=4, features=8, img_size=32, noise_dim=16)
    module = locate(cfg.model.lm["_target_"])(cfg, None)
    run = dict(R.RUNNER_KEYS, swd=True, swd_patches=6, swd_dirs=5, swd_repeats=2, swd_seed=4, swd_cache_gb=0.5)
    made = []
    monkeypatch.setattr(E, "RealPyramid", lambda images, plan, cache_gb: made.append((images, plan, cache_gb)) or "real")
    monkeypatch.setattr(E, "evaluate_swd", lambda mod, plan, real, batch: {"swd_32": 3.0, "swd_16": 1.0, "swd": 2.0,
                                                                           "args": (mod, plan, real, batch)})
    scorer = R.SwdScorer(cfg, run, module)
    assert scorer.sizes == [32, 16] and scorer.plan is None
    t0 = torch.get_rng_state().clone()
    scorer.load_real(torch.zeros(9, 3, 32, 32))
    assert torch.equal(torch.get_rng_state(), t0)
    plan = made[0][1]
    assert made[0][2] == 0.5 and (plan.n, plan.size, plan.channels, plan.patches, plan.dirs, plan.repeats, plan.seed) \
        == (9, 32, 3, 6, 5, 2, 4) and plan.latents.shape == (9, 16)
    m = scorer("mod")
    assert m["args"] == ("mod", plan, "real", 250) and scorer.text(m) == "SWD 32: 3.00 16: 1.00 avg: 2.00"
    with pytest.raises(ValueError):
        R.SwdScorer(make_cfg("dc_gan", img_size=256), run, module)

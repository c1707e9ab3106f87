"""The sliced Wasserstein distance's kernels (csrc/gz_swd.hip) against the numpy yardsticks (eval.laplacian_pyramid,
swd_descriptors, sliced_wasserstein, swd) on the cases and within the bounds of tests/swd_support.py: the pyramid (equal bits
on ternary images up to size 64), the channel statistics, the projection, the column sort (bit-exact against np.sort), the
distance, the whole statistic, equal bits of two calls into NaN-prefilled outputs and workspaces, refusals that touch
nothing, and evaluate_swd on a small DCGAN module.

Measured on the MI355X: largest |device - yardstick| / bound 0.34 (pyramid), 0.12 (projection), 1.1e-4 (end to end); the 66
tests take under 3 s of test time in all, the slowest (130 columns of 65541 keys against np.sort) 0.22 s."""
import ctypes

import numpy as np
import pytest
import torch

from lightning_gan_zoo_amd import eval as E
from swd_support import (END_TO_END_CASES, PROJECT_CASES, PYRAMID_CASES, SORT_CONTENTS, bounds_of, end_to_end_bound,
                         end_to_end_inputs, host_end_to_end, host_projection, host_pyramid, project_inputs, pyramid_bounds,
                         random_images, sort_input, ternary_images)

pytestmark = pytest.mark.gpu
NAN = float("nan")
BAD, UNSUPPORTED, WORKSPACE = -1, -2, -3


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _lib():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    return F, check, lib


def _pyramid(images, calls=2):
    """gz_swd_pyramid into a NaN-prefilled buffer, ``calls`` times -> per call the list of levels as numpy arrays."""
    F, check, lib = _lib()
    n, c, s, _ = images.shape
    x = _dev(images)
    count, offsets = ctypes.c_int(0), (ctypes.c_longlong * 5)()
    check(lib.gz_swd_pyramid_describe(n, c, s, ctypes.byref(count), offsets), "describe")
    out = []
    for _ in range(calls):
        buf = torch.full((offsets[count.value] + 3,), NAN, dtype=torch.float32, device="cuda")
        check(lib.gz_swd_pyramid(F._p(x), n, c, s, F._p(buf), offsets[count.value], F._stream()), "pyramid")
        host = buf.cpu().numpy()
        assert np.isnan(host[offsets[count.value]:]).all()                  # nothing behind the last level
        out.append([host[offsets[l]:offsets[l + 1]].reshape(n, c, s >> l, s >> l) for l in range(count.value)])
    return out


@pytest.mark.parametrize("case", PYRAMID_CASES, ids=str)
def test_ternary_pyramids_equal_the_yardsticks_bits_up_to_size_64(case):
    """tests/test_swd_cpu.py shows that fp32 is exact there in any order.  S = 16 is the single-level identity; at S = 128
    the level G_2 - up(G_3) is held to the bound instead."""
    images = ternary_images(case)
    first, second = _pyramid(images)
    want = host_pyramid("ternary", case)
    assert len(first) == len(want)
    bounds = bounds_of(images)
    for l, (a, b, w) in enumerate(zip(first, second, want)):
        assert _same_bits(a, b)
        if case[2] <= 64 or l != 2:
            assert np.array_equal(a.astype(np.float64), w), l
        else:
            assert (np.abs(a - w) <= bounds[l]).all()
    if case[2] == 16:
        assert _same_bits(first[0], np.asarray(images))


@pytest.mark.parametrize("case", PYRAMID_CASES, ids=str)
def test_random_pyramids_lie_within_the_composed_bound(case):
    first, second = _pyramid(random_images(case))
    worst = 0.0
    for a, b, w, bound in zip(first, second, host_pyramid("random", case), pyramid_bounds(case)):
        assert _same_bits(a, b)
        err = np.abs(a - w)
        assert (err <= bound).all()
        if bound.max() > 0:
            worst = max(worst, float((err / bound).max()))
    print("pyramid %s: largest |device - yardstick| / bound %.3g" % (case, worst))


def test_the_python_pyramid_returns_views_of_one_buffer():
    x = _dev(random_images(PYRAMID_CASES[2]))
    levels = E.laplacian_pyramid_device(x)
    assert [tuple(l.shape) for l in levels] == [(2, 3, 64, 64), (2, 3, 32, 32), (2, 3, 16, 16)]
    for l, w, bound in zip(levels, host_pyramid("random", PYRAMID_CASES[2]), pyramid_bounds(PYRAMID_CASES[2])):
        assert (np.abs(l.cpu().numpy() - w) <= bound).all()
    with pytest.raises(ValueError):
        E.laplacian_pyramid_device(torch.zeros(1, 3, 48, 48, device="cuda"))
    with pytest.raises(ValueError):
        E.laplacian_pyramid_device(torch.zeros(1, 2, 32, 32, device="cuda"))


def _stats(level, pos, calls=2):
    F, check, lib = _lib()
    n, c, h, _ = level.shape
    p = pos.shape[1]
    x, q = _dev(level), _dev(pos.reshape(-1, 2))
    ws_bytes = lib.gz_swd_channel_stats_workspace_bytes(n, c, h, p)
    out = []
    for _ in range(calls):
        stats = torch.full((2 * c,), NAN, dtype=torch.float64, device="cuda")
        ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
        check(lib.gz_swd_channel_stats(F._p(x), n, c, h, F._p(q), p, F._p(stats), F._p(ws), ws_bytes, F._stream()), "stats")
        out.append(stats.cpu().numpy())
    return out


@pytest.mark.parametrize("case", PROJECT_CASES, ids=str)
def test_channel_statistics_match_and_a_constant_channel_has_deviation_zero(case):
    """The device adds N = rows * 49 shifted values v - v0 per channel in fp64: each sum is within N 2^-53 of the sum of its
    terms' magnitudes, so the mean errs by at most N 2^-53 r (r = max|v - v0|), the variance s2 / N - (s1 / N)^2 by at most
    3 N 2^-53 r^2 and the deviation by half of that over itself; the yardstick's own sums obey the same bounds: twice."""
    level, pos, _ = project_inputs(case)
    first, second = _stats(level, pos)
    assert _same_bits(first, second)
    mean, std = host_projection(case)[2]
    c = level.shape[1]
    desc = E.swd_descriptors(level, pos).reshape(-1, c, 49)
    r = np.abs(desc - desc[0:1, :, 0:1]).max(axis=(0, 2))
    nu = desc.shape[0] * 49 * 2.0 ** -53
    assert (np.abs(first[:c] - mean) <= 2 * nu * r).all()
    assert (np.abs(first[c:] - std) <= 2 * 1.5 * nu * r * r / np.where(std == 0, 1.0, std)).all()
    if c == 3:
        assert first[5] == 0.0 and first[2] == np.float64(np.float32(0.3))


def _project(case, stats, gap=8, calls=2):
    """gz_swd_project with the given (mean, std) into NaN-prefilled [ndirs][padded + gap] -> numpy arrays, and padded."""
    F, check, lib = _lib()
    level, pos, dirs = project_inputs(case)
    n, c, h, p, ndirs = case
    padded = E.swd_sort_plan(n * p)[1]
    x, q, w, st = _dev(level), _dev(pos.reshape(-1, 2)), _dev(dirs), _dev(np.concatenate(stats))
    out = []
    for _ in range(calls):
        proj = torch.full((ndirs, padded + gap), NAN, dtype=torch.float32, device="cuda")
        check(lib.gz_swd_project(F._p(x), n, c, h, F._p(q), p, F._p(st), F._p(w), ndirs, F._p(proj), padded + gap,
                                 F._stream()), "project")
        out.append(proj.cpu().numpy())
    return out, padded


@pytest.mark.parametrize("case", PROJECT_CASES, ids=str)
def test_projections_lie_within_the_bound_and_the_padding_is_inf(case):
    """Corner patches (centres 3 and H - 4), D = 49 and 147, 1 / 5 / 128 / 130 directions, 10 / 129 / 128 / 385 rows against a
    tile of 128, a shifted channel and (C = 3) a constant one.  The yardstick's statistics are passed in, so the bound is
    the projection's alone."""
    want, bound, stats = host_projection(case)
    (first, second), padded = _project(case, stats)
    assert _same_bits(first, second)
    rows = want.shape[0]
    got = first[:, :rows].T.astype(np.float64)
    ratio = np.abs(got - want) / bound
    print("project %s: largest |device - yardstick| / bound %.3g" % (case, ratio.max()))
    assert (ratio <= 1.0).all()
    assert padded >= rows and (first[:, rows:padded] == np.inf).all()
    assert np.isnan(first[:, padded:]).all()                                        # the gap behind the padded length


def _sort(x, rows, gap, calls=2):
    """gz_swd_sort_columns on [cols][pitch]: the keys, NaN in rows .. padded - 1 (the launcher owes +inf there) and -7 in
    the gap behind padded (the pitch is a multiple of 4, ``gap`` beyond the padded length rounded up to one)."""
    F, check, lib = _lib()
    cols = x.shape[0]
    padded = E.swd_sort_plan(rows)[1]
    pitch = (padded + 3) // 4 * 4 + gap
    host = np.full((cols, pitch), NAN, dtype=np.float32)
    host[:, :rows] = x
    host[:, padded:] = -7.0
    out = []
    for _ in range(calls):
        data = _dev(host)
        check(lib.gz_swd_sort_columns(F._p(data), rows, cols, pitch, F._stream()), "sort")
        out.append(data.cpu().numpy())
    return out, padded


def _check_sorted(x, rows, gap):
    (first, second), padded = _sort(x, rows, gap)
    assert _same_bits(first, second)
    want = np.sort(x, axis=1)
    assert _same_bits(first[:, :rows].copy().view(np.uint32), want.view(np.uint32))
    assert (first[:, rows:padded] == np.inf).all() and (first[:, padded:] == -7.0).all()


SORT_BLOCK = 16384
SORT_ROWS = [1, 2, 37, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, 2 * SORT_BLOCK, 4 * SORT_BLOCK + 5]


def test_the_plans_block_length_is_the_one_the_sizes_are_placed_around():
    assert E.swd_sort_plan(100)[0] == SORT_BLOCK


@pytest.mark.parametrize("cols", [1, 3, 130])
@pytest.mark.parametrize("rows", SORT_ROWS)
def test_random_columns_sort_to_np_sorts_bits(rows, cols):
    """Every row count around the block length times every column count; the pitch equals the padded length for one
    column and exceeds it by 4 and 12 for 3 and 130."""
    _check_sorted(sort_input("random", rows, cols), rows, {1: 0, 3: 4, 130: 12}[cols])


@pytest.mark.parametrize("content", [c for c in SORT_CONTENTS if c != "random"])
@pytest.mark.parametrize("rows", [37, SORT_BLOCK + 1, 4 * SORT_BLOCK + 5])
def test_special_contents_sort_to_np_sorts_bits(rows, content):
    """All equal, already sorted, reversed, about nine distinct keys, and +-inf / -0.0 / denormals / the largest finite
    keys -- in one block, in two (one global stride) and in eight (six strides in four passes, fused ones among them)."""
    _check_sorted(sort_input(content, rows, 3), rows, 8)


@pytest.mark.parametrize("rows,per,repeats", [(1, 1, 1), (37, 3, 1), (20001, 5, 3), (16385, 1, 2)])
def test_the_distance_is_the_fp64_sum(rows, per, repeats):
    F, check, lib = _lib()
    rng = np.random.RandomState(rows)
    pitch = rows + 3
    a, b = rng.randn(per * repeats, pitch).astype(np.float32), rng.randn(per * repeats, pitch).astype(np.float32)
    want = np.abs(a[:, :rows].astype(np.float64) - b[:, :rows]).reshape(repeats, -1).sum(axis=1)
    da, db = _dev(a), _dev(b)
    ws_bytes = lib.gz_swd_distance_workspace_bytes(rows, per, repeats)
    got = []
    for _ in range(2):
        out = torch.full((repeats,), NAN, dtype=torch.float64, device="cuda")
        ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
        check(lib.gz_swd_distance(F._p(da), rows, F._p(db), rows, per, repeats, pitch, F._p(out), F._p(ws), ws_bytes,
                                  F._stream()), "distance")
        got.append(out.cpu().numpy())
    assert _same_bits(got[0], got[1])
    assert (np.abs(got[0] - want) <= rows * per * 2.0 ** -52 * want).all()


@pytest.mark.parametrize("case", END_TO_END_CASES, ids=str)
def test_the_whole_statistic_lies_within_the_bound_of_the_yardstick(case):
    """swd_device against swd: n = 8, C = 3, P = 16, 8 directions x 2 repeats.  The bound (tests/swd_support.py) is the sum
    of both sets' worst projection errors: sorted sequences move by at most the largest change of any key."""
    a, b, plan = end_to_end_inputs(case)
    want, bound = host_end_to_end(case), end_to_end_bound(case)
    first = E.swd_device(_dev(a), _dev(b), plan.positions, plan.directions, plan.repeats)
    second = E.swd_device(_dev(a), _dev(b), plan.positions, plan.directions, plan.repeats)
    assert first == second and set(first) == set(want)
    print("end to end %s: %s" % (case, {k: "%.4f vs %.4f, |diff| / bound %.3g" % (first[k], want[k], abs(first[k] - want[k])
                                                                                  / bound[k]) for k in want}))
    for key in want:
        assert abs(first[key] - want[key]) <= bound[key], key


def test_the_real_side_gives_equal_bits_cached_and_uncached():
    case = END_TO_END_CASES[0]
    a, b, plan = end_to_end_inputs(case)
    cached, uncached = E.RealPyramid(_dev(b), plan, cache_gb=16), E.RealPyramid(_dev(b), plan, cache_gb=0)
    assert cached.cached and not uncached.cached and cached.cache_bytes == 2 * 16 * 128 * 4
    levels = E.laplacian_pyramid_device(_dev(a))
    pos, dirs = plan.on(levels[0].device)
    for l, level in enumerate(levels):
        fake = E.swd_sorted_projections_device(level, pos[l], dirs[l])
        assert cached.sorted(l) is cached.sorted(l) and uncached.sorted(l) is not uncached.sorted(l)
        assert torch.equal(cached.sorted(l), uncached.sorted(l))
        values = [E.swd_distance_device(fake, real.sorted(l), 128, plan.repeats) for real in (cached, uncached, cached)]
        assert values[0] == values[1] == values[2]
        assert 1000.0 * values[0] == E.swd_device(_dev(a), _dev(b), plan.positions, plan.directions,
                                                  plan.repeats)["swd_%d" % plan.sizes[l]]


def test_refusals_return_their_code_and_touch_nothing():
    F, check, lib = _lib()
    x = torch.zeros((2, 3, 32, 32), dtype=torch.float32, device="cuda")
    out = torch.full((2 * 3 * 1280,), NAN, dtype=torch.float32, device="cuda")
    assert lib.gz_swd_pyramid(F._p(x), 2, 3, 48, F._p(out), out.numel(), F._stream()) == UNSUPPORTED    # S not in the list
    assert lib.gz_swd_pyramid(F._p(x), 2, 3, 32, F._p(out), out.numel() - 1, F._stream()) == WORKSPACE
    pos = torch.full((8, 2), 5, dtype=torch.int32, device="cuda")
    stats = torch.full((6,), NAN, dtype=torch.float64, device="cuda")
    ws = torch.full((64,), NAN, dtype=torch.float64, device="cuda")
    need = lib.gz_swd_channel_stats_workspace_bytes(2, 3, 32, 4)
    assert 0 < need <= 64 * 8
    assert lib.gz_swd_channel_stats(F._p(x), 2, 3, 32, F._p(pos), 0, F._p(stats), F._p(ws), 512, F._stream()) == BAD   # P = 0
    assert lib.gz_swd_channel_stats(F._p(x), 2, 3, 32, F._p(pos), 4, F._p(stats), F._p(ws), need - 1, F._stream()) == WORKSPACE
    dirs = torch.zeros((4, 147), dtype=torch.float32, device="cuda")
    proj = torch.full((4, 8), NAN, dtype=torch.float32, device="cuda")
    good = torch.zeros((6,), dtype=torch.float64, device="cuda")
    assert lib.gz_swd_project(F._p(x), 2, 3, 32, F._p(pos), 0, F._p(good), F._p(dirs), 4, F._p(proj), 8, F._stream()) == BAD
    assert lib.gz_swd_project(F._p(x), 2, 3, 32, F._p(pos), 4, F._p(good), F._p(dirs), 4, F._p(proj), 7, F._stream()) == BAD
    assert lib.gz_swd_sort_columns(F._p(proj), 8, 4, 6, F._stream()) == BAD
    dist = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    assert lib.gz_swd_distance(F._p(proj), 8, F._p(proj), 7, 2, 2, 8, F._p(dist), F._p(ws), 512, F._stream()) == BAD   # unequal
    assert lib.gz_swd_distance(F._p(proj), 8, F._p(proj), 8, 2, 2, 8, F._p(dist), F._p(ws), 31, F._stream()) == WORKSPACE
    torch.cuda.synchronize()
    for t in (out, stats, ws, proj, dist):
        assert torch.isnan(t).all()
    with pytest.raises(ValueError, match="equal shapes"):
        E.swd_device(x, x[:1], [], [])


def test_evaluate_swd_scores_a_dcgan_module_and_leaves_it_as_it_was():
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg("dc_gan", batch_size=4, features=8, img_size=32, noise_dim=16)
    torch.manual_seed(1)
    module = locate(cfg.model.lm["_target_"])(cfg, None).cuda().train()
    plan = E.SwdPlan(32, 3, 12, patches=8, dirs=4, repeats=2, seed=3, module=module)
    images = torch.rand(12, 3, 32, 32, device="cuda") * 2 - 1
    real = E.RealPyramid(images, plan, cache_gb=1)
    np.random.seed(5)
    torch.manual_seed(5)
    t0, g0, n0 = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), np.random.get_state()
    first = E.evaluate_swd(module, plan, real, batch=5)
    second = E.evaluate_swd(module, plan, real, batch=12)
    assert set(first) == {"swd_32", "swd_16", "swd"} and all(np.isfinite(v) and v > 0 for v in first.values())
    assert first["swd"] == pytest.approx((first["swd_32"] + first["swd_16"]) / 2, rel=1e-12)
    assert module.training and module.generator.training
    assert torch.equal(torch.get_rng_state(), t0) and torch.equal(torch.cuda.get_rng_state(), g0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]
    # the same launches on the images the sweep makes (eval mode, the raw tanh output) give the same bits
    module.eval()
    with torch.no_grad():
        fake = module.generator(plan.latents.cuda()).float()
    module.train()
    assert float(fake.min()) < 0.0                                              # not clamped to [0, 1]
    assert second == E.swd_device(fake, images, plan.positions, plan.directions, plan.repeats)


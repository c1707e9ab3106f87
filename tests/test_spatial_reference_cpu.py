"""tests/spatial_reference.py and tests/spatial_cases.py held to account without a GPU: the fp64 reference agrees with
an independent witness (torch on the CPU in float64) over the whole table but the looping cases; forward and backward
references are adjoint; every pool row's plan text is what gz_pool2d_plan (host arithmetic) answers, under the default
switches and under both experiment settings; every branch and every loop is named by a row; the recorded bilinear
constants are what `--measure` gives; the tolerances are small against the outputs; and at those tolerances the
comparator rejects each of a list of plausible kernel mistakes while it accepts the float32 rounding of the true value."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spatial_cases as sc
import spatial_reference as R

F64 = torch.float64


def _close(ours, theirs, what):
    ours, theirs = np.asarray(ours, dtype=np.float64), theirs.detach().double().numpy().reshape(np.shape(ours))
    err = np.abs(ours - theirs).max() / max(np.abs(theirs).max(), 1e-300)
    assert err <= 1e-12, (what, err)


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


SMALL_POOL = [c for c in sc.POOL_ROWS if not c.loop]


# ---------------------------------------------------------------------------
# witnesses
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", SMALL_POOL, ids=[c.id for c in SMALL_POOL])
def test_pool2d_agrees_with_torch(c):
    x = sc.pool_host(c)
    for mode in c.modes:
        y, scale, n = R.pool2d(x, c.KS, c.S, c.P, mode)
        t = _t(x)[None]
        if mode == 0:
            w = F.max_pool2d(t, c.KS, c.S, c.P)
        else:
            w = F.avg_pool2d(t, c.KS, c.S, c.P, count_include_pad=mode == 2)
        _close(y, w, (c, mode))
        assert n.min() >= 1 and n.max() <= c.KS * c.KS and (scale >= np.abs(y) * (1 - 1e-12)).all()
        ones = F.avg_pool2d(torch.ones(1, 1, c.H, c.W, dtype=F64), c.KS, c.S, c.P, divisor_override=1)
        _close(n, ones, (c, "taps inside the image"))


SMALL_SPATIAL = [c for c in sc.SPATIAL_CASES if not c.loop]


@pytest.mark.parametrize("c", SMALL_SPATIAL, ids=[c.id for c in SMALL_SPATIAL])
def test_spatial_ops_agree_with_torch(c):
    a = sc.spatial_host(c)
    x = torch.zeros(1, c.planes, c.H, c.W, dtype=F64, requires_grad=True)
    if c.kind.startswith("avgpool3s2"):
        y = F.avg_pool2d(x if c.kind.endswith("bwd") else _t(a)[None], 3, 2, 1, count_include_pad=True)
    else:
        y = F.interpolate(x if c.kind.endswith("bwd") else _t(a)[None], scale_factor=2)
    if c.kind.endswith("fwd"):
        ours = R.avgpool3s2_fwd(a)[0] if c.kind == "avgpool3s2_fwd" else R.upsample2_fwd(a)
        _close(ours, y, c)
    else:
        w, = torch.autograd.grad(y, [x], _t(a)[None])
        ours = R.avgpool3s2_bwd(a, c.H, c.W)[0] if c.kind == "avgpool3s2_bwd" else R.upsample2_bwd(a)[0]
        _close(ours, w, c)


def _torch_bilinear(x, c):
    """ATen's kernel with the scale handed over as the reference forms it: the float32 quotient."""
    sh, sw = float(np.float32(c.H) / np.float32(c.OH)), float(np.float32(c.W) / np.float32(c.OW))
    return torch._C._nn.upsample_bilinear2d(x, [c.OH, c.OW], False, 1.0 / sh, 1.0 / sw)


SMALL_RESIZE = [c for c in sc.RESIZE_CASES if not c.loop]


@pytest.mark.parametrize("c", SMALL_RESIZE, ids=[c.id for c in SMALL_RESIZE])
def test_resize_agrees_with_torch(c):
    x = sc.resize_host(c)
    y, scale, spread, coord = R.resize_bilinear(x, c.OH, c.OW, c.mul, c.add)
    _close(y, _torch_bilinear(_t(x)[None], c) * c.mul + c.add, c)
    assert (scale >= np.abs(y) * (1 - 1e-12) - 1e-300).all() and spread.min() >= 0 and coord.min() >= 1
    for p in sc.constant_planes(c):
        assert not spread[p].any()
        assert np.abs(y[p] - (sc.CONSTANT * c.mul + c.add)).max() <= 1e-15


SMALL_SAMPLES = [c for c in sc.SAMPLES_CASES if c.loop != "samples_x"]


@pytest.mark.parametrize("c", SMALL_SAMPLES, ids=[c.id for c in SMALL_SAMPLES])
def test_samples_to_inception_agrees_with_torch_and_the_host_quantiser(c):
    from eval_device_support import host_quantise
    x = sc.samples_host(c)
    u8 = host_quantise(x)                                   # [N, H, W, C]
    assert np.array_equal(R.grey_level(x), np.transpose(u8, (0, 3, 1, 2)))
    q = torch.from_numpy(u8).permute(0, 3, 1, 2).double() / 255.0
    q = q.expand(-1, 3, -1, -1) if c.C == 1 else q
    _close(R.samples_to_inception(x, c.OH, c.OW, c.mul, c.add)[0], _torch_bilinear(q.contiguous(), c) * c.mul + c.add, c)


def test_activation_and_residual_tail_agree_with_torch():
    c = sc.ACT_CASES[1]
    a, b = sc.ew_host(c)
    with np.errstate(over="ignore"):
        for act, slope in sc.ACTS:
            w = F.relu(_t(a)) if act == sc.ACT_RELU else F.leaky_relu(_t(a), float(np.float32(slope)))
            assert np.array_equal(R.act_fwd(a, act, slope)[0], w.numpy())
        out, scale = R.axpby(a, sc.AXPBY_ALPHA, b, sc.AXPBY_BETA)
        assert np.array_equal(out, (_t(a) * sc.c32(sc.AXPBY_ALPHA) + _t(b) * sc.c32(sc.AXPBY_BETA)).numpy())
        assert np.isfinite(out).all() and np.abs(out).max() > 3.2e38 and (scale >= np.abs(out)).all()
        assert np.array_equal(R.axpby(a, 0.5, None, 7.0)[0], 0.5 * a.astype(np.float64))
    assert set(sc.f32(sc.EDGES).view(np.uint32)) <= set(a.view(np.uint32)), "every edge value is in the input"


# ---------------------------------------------------------------------------
# adjointness, on the references only
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", sc.SPATIAL_HW)
def test_forward_and_backward_references_are_adjoint(H, W):
    r = sc.rng("adjoint", H, W)
    x = r.standard_normal((5, H, W))
    g = r.standard_normal((5, (H - 1) // 2 + 1, (W - 1) // 2 + 1))
    lhs, rhs = (R.avgpool3s2_fwd(x)[0] * g).sum(), (x * R.avgpool3s2_bwd(g, H, W)[0]).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    g = r.standard_normal((5, 2 * H, 2 * W))
    lhs, rhs = (R.upsample2_fwd(x) * g).sum(), (x * R.upsample2_bwd(g)[0]).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


# ---------------------------------------------------------------------------
# the table: plan texts, branches, loops
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.POOL_ROWS, ids=[c.id for c in sc.POOL_ROWS])
def test_pool_rows_carry_the_plan_the_library_answers(c):
    assert sc.pool_plan(c) == c.plan
    assert sc.plan_loops(c, c.plan) == (c.loop is not None)
    for knobs in sc.KNOBS:
        assert sc.pool_plan(c, knobs).split()[0] == sc.pool_branch_under(c, knobs), knobs
    if c.misaligned:                                        # alignment is what keeps it off the butterfly kernel
        aligned = copy.copy(c)
        aligned.misaligned = False
        assert sc.pool_plan(aligned).startswith("global_avg<16>")


def test_every_branch_and_every_loop_is_named_by_a_row():
    assert {c.plan.split()[0] for c in sc.POOL_ROWS} == set(sc.BRANCHES)
    for knobs, only in (("no_group", {"plane", "flat"}), ("no_group_no_plane", {"flat"})):
        assert {sc.pool_branch_under(c, knobs) for c in sc.POOL_ROWS} == only
    assert {c.loop for c in sc.CASES if c.loop} == set(sc.LOOPS)
    for op in sc.SPATIAL_OPS + ("act", "axpby", "resize"):
        assert any(c.loop for c in sc.CASES if c.kind == op), op
    for c in sc.SPATIAL_CASES:                              # rn_grid: 4096 workgroups of 256 items
        items = c.planes * (c.H * c.W if c.kind != "avgpool3s2_fwd" else ((c.H - 1) // 2 + 1) * ((c.W - 1) // 2 + 1))
        assert (items > 4096 * 256) == (c.loop is not None), c
    for c in sc.ACT_CASES + sc.AXPBY_CASES:
        assert (c.count // 4 > 4096 * 256) == (c.loop is not None), c
    for c in sc.RESIZE_CASES:
        assert (c.planes * c.OH * c.OW > 4096 * 256) == (c.loop is not None), c
    for c in sc.SAMPLES_CASES:
        loop = "samples_x" if -(-c.OH * c.OW // 256) > 4096 else "samples_planes" if c.N * 3 > 65535 else None
        assert c.loop == loop, c
    ragged = [c for c in sc.POOL_ROWS if c.loop == "group_ragged"][0]
    G = int(ragged.plan.split()[1][2:])
    assert ragged.P == 1 and ragged.planes % G and ragged.planes // G >= 8192


def test_pool_inputs_hold_the_planes_the_borders_need():
    for c in sc.POOL_ROWS:
        if c.big:
            continue
        x = sc.pool_host(c)
        assert x[0].max() <= -1.0 and x[0].min() >= -3.0 and (c.planes == 2 or x[-1].max() <= -1.0)
        if c.planes >= 2:
            assert x[1, 0, 0] == sc.CORNER and (np.abs(x[1]) > 10).sum() <= 2


# ---------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------
def test_the_recorded_constants_are_the_measured_ones():
    """`python tests/spatial_reference.py --measure`: K is twice the RECORDED ratio rounded up; measuring again gives the
    recorded ratios to 10 %, and the emulation stays within K."""
    assert (R.constant(R.MEASURED["K1"]), R.constant(R.MEASURED["K2"])) == (R.K1, R.K2)
    got = R.measure(k1=R.K1)
    for k, v in got.items():
        assert abs(v - R.MEASURED[k]) <= 0.1 * R.MEASURED[k], (k, v)
    assert got["K1"] <= R.K1 and got["K2"] <= R.K2


def _reference_outs(c):
    """Every Out of a case, as the GPU test compares it."""
    if c.kind == "pool":
        x = sc.pool_host(c)
        return [R.pool2d_out(x, c.KS, c.S, c.P, m) for m in c.modes]
    if c.kind in sc.SPATIAL_OPS:
        a = sc.spatial_host(c)
        if c.kind == "avgpool3s2_fwd":
            return [R.sum_out(*R.avgpool3s2_fwd(a), "spatial_sum")]
        if c.kind == "avgpool3s2_bwd":
            return [R.sum_out(*R.avgpool3s2_bwd(a, c.H, c.W), "spatial_sum")]
        if c.kind == "upsample2_bwd":
            return [R.sum_out(*R.upsample2_bwd(a), 4, "spatial_sum")]
        return [R.Out(R.upsample2_fwd(a), None, "upsample2_fwd")]
    if c.kind == "resize":
        return [R.resize_out(sc.resize_host(c), c.OH, c.OW, c.mul, c.add)]
    if c.kind == "samples":
        return [R.samples_out(sc.samples_host(c), c.OH, c.OW, c.mul, c.add)]
    a, b = sc.ew_host(c)
    if c.kind == "act":
        return [R.act_out(a, act, slope) for act, slope in sc.ACTS]
    return [R.axpby_out(a, sc.AXPBY_ALPHA, b, sc.AXPBY_BETA)]


SMALL = [c for c in sc.CASES if not c.loop]


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_tolerances_are_small_against_the_outputs(c):
    """The largest tolerance of a case is below 1e-5 of its largest output: a K that could hide a wrong tap fails here.
    The bilinear tolerance has a second term, the float32 coordinate's own error times the tap spread, which is no
    arithmetic slack but the conditioning of the operation (a +-1 checkerboard sampled at x = 399 moves by 2e-4 when
    the coordinate moves by its last bit): there the arithmetic term K1 u scale is held to 1e-5 of the output, and the
    coordinate term K2 u max(fy, fx, 1) to 1e-3 -- of the spread, where a wrong tap is an error of the order of the
    spread itself."""
    for o in _reference_outs(c):
        if o.tol is None:
            continue
        mag = np.abs(o.value).max()
        if c.kind in ("resize", "samples"):
            x = sc.resize_host(c) if c.kind == "resize" else None
            ref = (R.resize_bilinear(x, c.OH, c.OW, c.mul, c.add) if c.kind == "resize"
                   else R.samples_to_inception(sc.samples_host(c), c.OH, c.OW, c.mul, c.add))
            _, scale, spread, coord = ref
            assert (R.U * R.K1 * scale).max() <= 1e-5 * mag
            assert R.U * R.K2 * coord.max() <= 1e-3
        else:
            assert o.tol.max() <= 1e-5 * mag, (c, o.tol.max(), mag)


# ---------------------------------------------------------------------------
# mutants: each plausible mistake violates the tolerance somewhere in the table; the rounded truth never does
# ---------------------------------------------------------------------------
def _violations(cases, outs_of, mutation):
    """The ids of the cases at which the float32 of the mistaken value falls outside the true reference's tolerance."""
    bad = []
    for c in cases:
        true = outs_of(c)
        with R.wrong(mutation):
            mistaken = outs_of(c)
        for o in true:
            assert not R.compare(o.value.astype(np.float32), o, "the rounded truth, %s" % c)
        if any(R.compare(m.value.astype(np.float32), o, c.id) for m, o in zip(mistaken, true)):
            bad.append(c.id)
    return bad


def _pool_outs(c):
    return _reference_outs(c)


def test_rejects_the_divisor_ks2_in_mode_1():
    padded = [c for c in SMALL_POOL if c.P > 0 and 1 in c.modes]
    assert padded and _violations(padded, _pool_outs, "mode1_divides_by_ks2") == [c.id for c in padded]
    unpadded = [c for c in SMALL_POOL if c.P == 0][:5]
    assert not _violations(unpadded, _pool_outs, "mode1_divides_by_ks2")


def test_rejects_a_zero_border_for_max():
    """Plane 0 is negative throughout: a zero border wins every padded window of it."""
    padded = [c for c in SMALL_POOL if c.P > 0 and 0 in c.modes]
    assert padded and _violations(padded, _pool_outs, "max_border_zero") == [c.id for c in padded]


def test_rejects_a_window_shifted_at_the_right_edge():
    rows = [c for c in SMALL_POOL if c.planes * c.H * c.W < 100000]
    assert _violations(rows, _pool_outs, "right_edge_window_shifted") == [c.id for c in rows]


def test_rejects_a_lower_tap_without_its_clamp():
    """(Wherever rows are added: the last output rows then lie past the centre of the last input row, and their lower
    tap is that row again.  A downscale never reaches the clamp, an identity reaches it with weight zero.)"""
    rows = [c for c in SMALL_RESIZE if c.H > 1]
    up = [c.id for c in rows if c.OH > c.H]
    assert up and [i for i in _violations(rows, _reference_outs, "y1_without_clamp")] == up
    rows = [c for c in sc.SAMPLES_CASES if c.H > 1 and c.OH <= 299]
    assert rows and _violations(rows, _reference_outs, "y1_without_clamp") == [c.id for c in rows]


def test_rejects_align_corners_coordinates():
    """(Identity sizes and single-pixel sources have the same coordinates under both rules; a constant plane the same
    value.)"""
    rows = [c for c in SMALL_RESIZE if (c.H, c.W) != (c.OH, c.OW) and (c.H, c.W) != (1, 1)]
    assert rows and _violations(rows, _reference_outs, "align_corners_coordinates") == [c.id for c in rows]
    same = [c for c in SMALL_RESIZE if (c.H, c.W) == (c.OH, c.OW) or (c.H, c.W) == (1, 1)]
    assert same and not _violations(same, _reference_outs, "align_corners_coordinates")


def test_rejects_an_avgpool3s2_backward_without_its_last_row():
    rows = [c for c in SMALL_SPATIAL if c.kind == "avgpool3s2_bwd"]
    assert rows and _violations(rows, _reference_outs, "avgpool3s2_bwd_drops_last_row") == [c.id for c in rows]


def test_every_listed_mutation_is_exercised():
    import inspect
    import sys
    text = inspect.getsource(sys.modules[__name__])
    for name in R.MUTATIONS:
        assert text.count('"%s"' % name) >= 1, name


def test_exact_outputs_are_compared_bit_for_bit():
    c = sc.SPATIAL_CASES[3]
    o = R.Out(R.upsample2_fwd(sc.spatial_host(c)), None, "upsample2_fwd")
    good = o.value.astype(np.float32)
    assert not R.compare(good, o, "y")
    moved = good.copy()
    moved.reshape(-1)[3] = np.nextafter(moved.reshape(-1)[3], np.float32(0))
    assert R.compare(moved, o, "y")
    assert R.compare(-good * 0, R.Out(good * 0, None, "zeros"), "the sign of a zero")

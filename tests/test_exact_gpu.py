"""Exact-integer parity of the multiply-add kernels ("Exact-integer parity"): integer operands with
sum |a||b| < 2^24 per output element make every product and partial sum exact in fp32 whatever the summation order, so
each HIP result must EQUAL the fp64 CPU operator bit for bit -- a wrong index, a dropped or doubled term, a truncated
operand, a narrow accumulator or an unwritten element changes bits.  One operand of every multiply-add case carries
|v| <= 4095 (12 bits).  tests/test_exact_cases.py checks the cases themselves (precondition, torch's fp32 operator alone,
sensitivity, plan-form coverage) without a GPU.

Left to the 1e-3 tests because they are inexact on integers by design: tanh, LeakyReLU's production slope 0.2, the
norms, BCE.  gz_pair_loss mode 0 is the one entry point of this module that is inexact by design (log1pf(expf(-|x|)),
csrc/gz_loss.hip:59-60, and the sigmoid of its backward, :77): it is held to fp64 at the project's 1e-5 instead."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

import exact_support as S
from exact_support import assert_bits_equal, assert_exact_precondition, int_operands

pytestmark = pytest.mark.gpu


def _F():
    from lightning_gan_zoo_amd import functional as F
    return F


def _lib():
    from lightning_gan_zoo_amd._lib import check, lib
    return lib, check


def _geom(c):
    return _F().Geom(c.k, c.k, c.s, c.p)


def _off4(t):
    """The same values on the GPU, 4 bytes off a 16-byte boundary."""
    v = torch.empty(t.numel() + 1, device="cuda")[1:].view_as(t).copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _run_conv(c, op, a, b, bias=None, act=None, slope=0.0):
    F = _F()
    act = F.ACT_NONE if act is None else act
    if op == "F":
        return F._conv_fwd_raw(a, b, bias, _geom(c), act, slope)
    if op == "Dg":
        return F._conv_dgrad_raw(a, b, bias, _geom(c), S.map_sides(c)[0], act, slope)
    assert bias is None and act == F.ACT_NONE
    return F._conv_wgrad_raw(a, b, _geom(c))


_act64 = S.act64


def _act_args(name):
    F = _F()
    return {"none": F.ACT_NONE, "relu": F.ACT_RELU}.get(name, F.ACT_LRELU), S.SLOPES[name]


# ---------------------------------------------------------------------------------------------------------------------
# a. conv2d forward, input gradient and weight gradient at every plan form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.CONV_ROWS, ids=S.row_id)
def test_conv2d_at_every_plan_form(row):
    c, op, form, split = row
    text = S.conv2d_plan(op, *c)
    assert S.plan_form(text) == form, "the case moved off its kernel: " + text
    a, b, ref = S.conv_ref(c, op)
    assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda()), ref, "%s  [%s]" % (S.row_id(row), text))


# ---------------------------------------------------------------------------------------------------------------------
# b. epilogues and fused forms
# ---------------------------------------------------------------------------------------------------------------------
EPILOGUE_ROWS = [r for r in S.CONV_ROWS if (tuple(r[0]), r[1]) in {
    ((2, 16, 8, 40, 3, 1, 1), "F"), ((8, 16, 64, 132, 1, 1, 0), "F"), ((32, 16, 64, 132, 4, 2, 1), "F"),
    ((16, 16, 64, 3, 3, 1, 1), "F"), ((1, 1024, 4, 1024, 5, 2, 2), "F"), ((1, 3, 32, 40, 4, 2, 1), "F"),
    ((64, 16, 32, 3, 3, 1, 1), "F"), ((1, 256, 4, 1024, 5, 2, 2), "F"),
    ((1, 3, 8, 40, 4, 2, 1), "Dg"), ((1, 3, 8, 16, 5, 2, 2), "Dg"), ((2, 64, 16, 64, 4, 2, 1), "Dg"),
    ((1, 1024, 64, 64, 4, 2, 1), "Dg"), ((1, 512, 4, 1024, 5, 2, 2), "Dg"), ((2, 1024, 64, 128, 1, 1, 0), "Dg"),
    ((16, 3, 64, 16, 3, 1, 1), "Dg"), ((2, 64, 8, 16, 3, 1, 1), "Dg")}]


def test_the_epilogue_rows_are_all_there():
    assert len(EPILOGUE_ROWS) == 16


@pytest.mark.parametrize("row", EPILOGUE_ROWS, ids=S.row_id)
def test_conv2d_bias_and_activation_epilogues(row):
    """Integer bias, ReLU, LeakyReLU with slopes 0.5 and 0.25 (powers of two keep it exact)."""
    c, op, form, split = row
    a, b, ref = S.conv_ref(c, op)
    nb = c.K if op == "F" else c.C
    bias = int_operands((nb,), 7, 1.0, 77 + nb)
    assert_exact_precondition(S.conv_apply(c, op, a.double().abs(), b.double().abs()) + 7.0, S.row_id(row))
    ad, bd, biasd = a.cuda(), b.cuda(), bias.cuda()
    with_bias = ref + bias.double().view(1, -1, 1, 1)
    for name in ("none", "relu", "lrelu0.5", "lrelu0.25"):
        act, slope = _act_args(name)
        assert_bits_equal(_run_conv(c, op, ad, bd, biasd, act, slope), _act64(with_bias, name), "%s bias + %s" % (S.row_id(row), name))
    assert_bits_equal(_run_conv(c, op, ad, bd, None, *_act_args("lrelu0.5")), _act64(ref, "lrelu0.5"), "no bias + lrelu0.5")


@pytest.mark.parametrize("case", S.DGRAD_ACT_CASES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_input_gradient_with_the_activation_mask_formed_on_load(case, name):
    """gz_conv2d_dgrad_act: d/dx of act(conv(x, w) + b) with frozen weights, against the transposed convolution of the
    masked gradient in fp64."""
    F = _F()
    lib, _ = _lib()
    N, C, H, K = case
    act, slope = _act_args(name)
    assert lib.gz_conv2d_dgrad_act_fuses(N, C, H, H, K, H // 2, H // 2, 4, 4, 2, 1, act)
    x, w, b, gy, y, ref = S.dgrad_act_case(case, name)
    xd = x.cuda().requires_grad_()
    out = F.conv2d(xd, w.cuda(), b.cuda(), F.K4S2P1, act, slope)
    assert_bits_equal(out, y, "forward")
    out.backward(gy.cuda())
    assert_bits_equal(xd.grad, ref, "dgrad_act %s %s" % (case, name))


@pytest.mark.parametrize("case", S.WGRAD_ACT_CASES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_weight_and_bias_gradient_with_the_activation_mask_formed_on_load(case, name):
    """gz_conv2d_wgrad_act_partial: the critics' first layer with sinks on, applied to two batches before one flush."""
    F = _F()
    lib, _ = _lib()
    N, C, H, K = case
    act, slope = _act_args(name)
    assert lib.gz_conv2d_wgrad_act_fuses(N, C, H, H, K, H // 2, H // 2, 4, 4, 2, 1, act) == 1
    xs, gys, w0, b0, dw_ref, db_ref = S.wgrad_act_case(case, name)
    w, b = torch.nn.Parameter(w0.cuda()), torch.nn.Parameter(b0.cuda())
    prev = F.set_grad_sinks(True)
    try:
        for x, gy in zip(xs, gys):
            F.conv2d(x.cuda(), w, b, F.K4S2P1, act, slope).backward(gy.cuda())
        assert w.grad is None and b.grad is None          # nothing went through autograd's accumulation
        F.flush_grad_sinks()
    finally:
        F.set_grad_sinks(*prev)
    assert_bits_equal(w.grad, dw_ref, "dw")
    assert_bits_equal(b.grad, db_ref, "db")


@pytest.mark.parametrize("row", [r for r in S.CONV_ROWS if r[1] == "Wg" and S.conv_terms(r[0], "Wg") * r[0].K < 3e7],
                         ids=S.row_id)
def test_weight_gradient_with_the_bias_gradient(row):
    """gz_conv2d_wgrad's fused bias gradient (where gz_conv2d_wgrad_fuses_bias says so; gz_channel_sum elsewhere)."""
    c = row[0]
    a, b, ref = S.conv_ref(c, "Wg")
    assert_exact_precondition(b.double().abs().sum((0, 2, 3)), "db")
    dw, db = _F()._conv_wgrad_raw(a.cuda(), b.cuda(), _geom(c), with_bias=True)
    assert_bits_equal(dw, ref, "dw")
    assert_bits_equal(db, b.double().sum((0, 2, 3)), "db")


def test_some_weight_gradient_case_fuses_its_bias_gradient():
    lib, _ = _lib()
    fused = [r for r in S.CONV_ROWS if r[1] == "Wg" and S.conv_terms(r[0], "Wg") * r[0].K < 3e7 and lib.gz_conv2d_wgrad_fuses_bias(
        r[0].N, r[0].C, r[0].H, r[0].H, r[0].K, S.out_side(r[0].H, r[0].k, r[0].s, r[0].p),
        S.out_side(r[0].H, r[0].k, r[0].s, r[0].p), r[0].k, r[0].k, r[0].s, r[0].p) == 1]
    assert fused, "no exact case takes the fused bias gradient"


@pytest.mark.parametrize("case", S.STATS_CASES, ids=S.case_id)
@pytest.mark.parametrize("op", ["F", "Dg"])
def test_batchnorm_statistics_epilogue(case, op):
    """conv2d_with_stats / conv_transpose2d_with_stats: the output is exact on the 12-bit operands; on operands thinned
    until the per-channel sum of y^2 stays below 2^24, the partial rows add up to sum y and sum y^2 exactly."""
    F = _F()
    c = case
    fn = F.conv2d_with_stats if op == "F" else F.conv_transpose2d_with_stats
    a, b, ref = S.conv_ref(c, op)
    y, stats = fn(a.cuda(), b.cuda(), _geom(c))
    assert_bits_equal(y, ref, "output (wide operands)")
    a, b, y64 = S.stats_reference(tuple(c), op)
    y, stats = fn(a.cuda(), b.cuda(), _geom(c))
    assert_bits_equal(y, y64, "output (thin operands)")
    rows = getattr(_lib()[0], "gz_conv2d_fwd_stats_rows" if op == "F" else "gz_conv2d_dgrad_stats_rows")(
        c.N, c.C, c.H, c.H, c.K, c.H // 2, c.H // 2, 4, 4, 2, 1)
    assert rows > 0, "the case no longer carries the statistics"
    assert tuple(stats.shape) == (rows, y64.shape[1], 2)
    # every partial row is a sum of integers below 2^24 (exact in fp32, so an integer itself, and sum y^2 >= |sum y|), and
    # the rows add up, in fp64, to the sums over all pixels; which pixels a row holds is the launch's own business
    assert torch.equal(stats, stats.round()) and bool((stats[:, :, 1] >= stats[:, :, 0].abs()).all())
    tot = stats.double().sum(0).cpu()
    assert_bits_equal(tot[:, 0], y64.sum((0, 2, 3)), "sum y")
    assert_bits_equal(tot[:, 1], (y64 * y64).sum((0, 2, 3)), "sum y^2")


# ---------------------------------------------------------------------------------------------------------------------
# c. split reductions
# ---------------------------------------------------------------------------------------------------------------------
SINK_ROWS = [r for r in S.CONV_ROWS if (tuple(r[0]), r[1]) in {
    ((16, 3, 64, 64, 4, 2, 1), "Wg"), ((2, 72, 64, 96, 1, 1, 0), "Wg"), ((64, 3, 4, 96, 4, 2, 1), "Wg"),
    ((2, 1024, 64, 128, 4, 2, 1), "Wg"), ((1, 512, 8, 1024, 4, 2, 1), "Wg"), ((16, 3, 64, 3, 3, 1, 1), "Wg"),
    ((1, 4, 16, 96, 3, 1, 1), "Wg"), ((64, 3, 32, 3, 3, 1, 1), "Wg")}]


@pytest.mark.parametrize("row", SINK_ROWS, ids=S.row_id)
def test_weight_gradient_slabs_summed_by_reduce_multi(row):
    """gz_conv2d_wgrad_partial + gz_reduce_multi: two launches per parameter into a fresh gradient (beta 0), then a third
    onto the existing one (beta 1)."""
    F = _F()
    c = row[0]
    a, b, ref = S.conv_ref(c, "Wg")
    assert_exact_precondition(3 * S.conv_apply(c, "Wg", a.double().abs(), b.double().abs()), "three passes")
    w = torch.nn.Parameter(torch.zeros(c.K, c.C, c.k, c.k, device="cuda"))
    ad, bd = a.cuda(), b.cuda()
    prev = F.set_grad_sinks(True)
    try:
        for _ in range(2):
            F.conv2d(ad, w, None, _geom(c)).backward(bd)
        F.flush_grad_sinks()
        assert_bits_equal(w.grad, 2 * ref, "beta 0, two sources")
        F.conv2d(ad, w, None, _geom(c)).backward(bd)
        F.flush_grad_sinks()
    finally:
        F.set_grad_sinks(*prev)
    assert_bits_equal(w.grad, 3 * ref, "beta 1")


def test_the_sink_rows_are_all_there():
    assert len(SINK_ROWS) == 8 and any(r[3] for r in SINK_ROWS) and any(not r[3] for r in SINK_ROWS)


@pytest.mark.parametrize("case", S.SPLIT_K_CASES, ids=S.case_id)
def test_conv_split_k(case):
    lib, _ = _lib()
    c = case
    OH = S.out_side(c.H, c.k, c.s, c.p)
    assert lib.gz_conv2d_fwd_workspace_bytes(c.N, c.C, c.H, c.H, c.K, OH, OH, c.k, c.k, c.s, c.p) > 0, "case no longer splits"
    assert lib.gz_conv2d_dgrad_workspace_bytes(c.N, c.C, c.H, c.H, c.K, OH, OH, c.k, c.k, c.s, c.p) > 0
    for op, nb in (("F", c.K), ("Dg", c.C)):
        a, b, ref = S.conv_ref(c, op)
        bias = int_operands((nb,), 7, 1.0, 43)
        assert_exact_precondition(S.conv_apply(c, op, a.double().abs(), b.double().abs()) + 7.0, op)
        assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda()), ref, op)
        assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda(), bias.cuda(), *_act_args("lrelu0.5")),
                          _act64(ref + bias.double().view(1, -1, 1, 1), "lrelu0.5"), op + " bias + lrelu0.5")


@pytest.mark.parametrize("row", [r for r in S.EXTRA_ROWS if r[0] in S.UNALIGNED_CASES], ids=S.extra_id)
def test_conv_operands_four_bytes_off_alignment(row):
    """gz_conv2d_fwd / _dgrad / _wgrad with their activation operands 4 bytes off a 16-byte boundary: the fallback
    loaders."""
    c, op = row
    a, b, ref = S.conv_ref(c, op)
    assert op != "F" or "F igemm2<" in S.conv2d_plan(op, *c)
    assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda()), ref, "aligned")
    assert_bits_equal(_run_conv(c, op, _off4(a), _off4(b) if op == "Wg" else b.cuda()), ref, "4 bytes off")
    if op == "Wg":
        assert_bits_equal(_run_conv(c, op, a.cuda(), _off4(b)), ref, "gy 4 bytes off")


# ---------------------------------------------------------------------------------------------------------------------
# d. conv3d
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.CONV3_ROWS, ids=S.row3_id)
def test_conv3d_family(row):
    F = _F()
    c, op, form = row
    text = S.conv3d_plan(op, *c)
    assert S.plan_form(text) == form, "the case moved off its kernel: " + text
    a, b, ref = S.conv3_reference(tuple(c), op)
    ad, bd = a.cuda(), b.cuda()
    if op == "F":
        got = F._conv3d_fwd_raw(ad, bd, None, F.ACT_NONE, 0.0)
    elif op == "Dg":
        got = F._conv3d_dgrad_raw(ad, bd, None, F.ACT_NONE, 0.0)
    else:
        got = F._conv3d_wgrad_raw(ad, bd, 3)
    assert_bits_equal(got, ref, "%s  [%s]" % (S.row3_id(row), text))
    if op != "Wg" and c.N * c.C * c.K < 2e6:
        nb = c.K if op == "F" else c.C
        bias = int_operands((nb,), 7, 1.0, 5)
        assert_exact_precondition(S.conv3_apply(c, op, a.double().abs(), b.double().abs()) + 7.0, "bias")
        fn = F._conv3d_fwd_raw if op == "F" else F._conv3d_dgrad_raw
        assert_bits_equal(fn(ad, bd, bias.cuda(), F.ACT_RELU, 0.0), torch.relu(ref + bias.double().view(1, -1, 1, 1, 1)),
                          "bias + relu")


# ---------------------------------------------------------------------------------------------------------------------
# d2. rectangular maps (H != W) and box volumes: the same launches where an image boundary falls inside a tile, H is not
# W and a vertical halo row is not the neighbouring image's (tests/exact_support.py, RECT_ROWS / BOX3_ROWS)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.RECT_ROWS, ids=S.row_id)
def test_conv2d_rectangular_at_every_plan_form(row):
    c, op, form, split = row
    text = S.conv2d_plan(op, *c)
    assert S.plan_form(text) == form, "the case moved off its kernel: " + text
    a, b, ref = S.conv_ref(c, op)
    assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda()), ref, "%s  [%s]" % (S.row_id(row), text))


def _epilogue_group(row):
    """(direction, loader family) of a row; the direct kernels by their own names."""
    form = row[2]
    fam = S.loader_family(form)
    return row[1], form.split(" direct ")[1].split("<")[0] if fam == "direct" else fam


def _rect_epilogue_rows():
    """The cheapest rectangular row of every loader family (and of every direct kernel) in the two directions that have
    an epilogue."""
    best = {}
    for row in S.RECT_ROWS:
        if row[1] != "Wg" and "ConvDg5A2" not in row[2]:      # (ConvDg5A2 hands a launch with an epilogue to ConvDgTapA2)
            g = _epilogue_group(row)
            if g not in best or S.case_macs(row[0]) < S.case_macs(best[g][0]):
                best[g] = row
    return [best[g] for g in sorted(best)]


RECT_EPILOGUE_ROWS = _rect_epilogue_rows()


def test_the_rectangular_epilogue_rows_are_all_there():
    # F: ConvFwdA2, ConvTapA2, Row4, K4V, Tap, the plain loader, two direct kernels; Dg: ConvDgA2, ConvDgTapA2, Row4, Tap, the
    # plain loader, four direct kernels
    assert len(RECT_EPILOGUE_ROWS) == 17
    assert any(r[0].H > r[0].W for r in RECT_EPILOGUE_ROWS) and any(r[0].H < r[0].W for r in RECT_EPILOGUE_ROWS)


@pytest.mark.parametrize("row", RECT_EPILOGUE_ROWS, ids=S.row_id)
def test_conv2d_rectangular_bias_and_activation_epilogues(row):
    test_conv2d_bias_and_activation_epilogues(row)


@pytest.mark.parametrize("case", S.RECT_STATS_CASES, ids=S.case_id)
@pytest.mark.parametrize("op", ["F", "Dg"])
def test_rectangular_batchnorm_statistics_epilogue(case, op):
    """test_batchnorm_statistics_epilogue's assertions on rectangular maps: which rows of an image a partial row of the
    statistics owns is where H and W part ways."""
    F = _F()
    c = case
    fn = F.conv2d_with_stats if op == "F" else F.conv_transpose2d_with_stats
    a, b, ref = S.conv_ref(c, op)
    y, stats = fn(a.cuda(), b.cuda(), _geom(c))
    assert_bits_equal(y, ref, "output (wide operands)")
    a, b, y64 = S.stats_reference(tuple(c), op)
    y, stats = fn(a.cuda(), b.cuda(), _geom(c))
    assert_bits_equal(y, y64, "output (thin operands)")
    rows = getattr(_lib()[0], "gz_conv2d_fwd_stats_rows" if op == "F" else "gz_conv2d_dgrad_stats_rows")(
        c.N, c.C, c.H, c.W, c.K, c.H // 2, c.W // 2, 4, 4, 2, 1)
    assert rows > 0, "the case no longer carries the statistics"
    assert tuple(stats.shape) == (rows, y64.shape[1], 2)
    assert torch.equal(stats, stats.round()) and bool((stats[:, :, 1] >= stats[:, :, 0].abs()).all())
    tot = stats.double().sum(0).cpu()
    assert_bits_equal(tot[:, 0], y64.sum((0, 2, 3)), "sum y")
    assert_bits_equal(tot[:, 1], (y64 * y64).sum((0, 2, 3)), "sum y^2")


@pytest.mark.parametrize("case", S.RECT_DGRAD_ACT_CASES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_rectangular_input_gradient_with_the_activation_mask_formed_on_load(case, name):
    F = _F()
    lib, _ = _lib()
    N, C, H, W, K = case
    act, slope = _act_args(name)
    assert lib.gz_conv2d_dgrad_act_fuses(N, C, H, W, K, H // 2, W // 2, 4, 4, 2, 1, act)
    x, w, b, gy, y, ref = S.dgrad_act_case(case, name)
    xd = x.cuda().requires_grad_()
    out = F.conv2d(xd, w.cuda(), b.cuda(), F.K4S2P1, act, slope)
    assert_bits_equal(out, y, "forward")
    out.backward(gy.cuda())
    assert_bits_equal(xd.grad, ref, "dgrad_act %s %s" % (case, name))


@pytest.mark.parametrize("case", S.RECT_WGRAD_ACT_CASES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_rectangular_weight_and_bias_gradient_with_the_activation_mask_formed_on_load(case, name):
    """gz_conv2d_wgrad_act_partial through the sinks, two batches before one flush."""
    F = _F()
    lib, _ = _lib()
    N, C, H, W, K = case
    act, slope = _act_args(name)
    assert lib.gz_conv2d_wgrad_act_fuses(N, C, H, W, K, H // 2, W // 2, 4, 4, 2, 1, act) == 1
    xs, gys, w0, b0, dw_ref, db_ref = S.wgrad_act_case(case, name)
    w, b = torch.nn.Parameter(w0.cuda()), torch.nn.Parameter(b0.cuda())
    prev = F.set_grad_sinks(True)
    try:
        for x, gy in zip(xs, gys):
            F.conv2d(x.cuda(), w, b, F.K4S2P1, act, slope).backward(gy.cuda())
        assert w.grad is None and b.grad is None
        F.flush_grad_sinks()
    finally:
        F.set_grad_sinks(*prev)
    assert_bits_equal(w.grad, dw_ref, "dw")
    assert_bits_equal(b.grad, db_ref, "db")


RECT_WG_BIAS_ROWS = [r for r in S.RECT_ROWS if r[1] == "Wg" and S.conv_terms(r[0], "Wg") * r[0].K < 3e7]


@pytest.mark.parametrize("row", RECT_WG_BIAS_ROWS, ids=S.row_id)
def test_rectangular_weight_gradient_with_the_bias_gradient(row):
    test_weight_gradient_with_the_bias_gradient(row)


def test_some_rectangular_weight_gradient_case_fuses_its_bias_gradient():
    lib, _ = _lib()
    fused = []
    for c, _, _, _ in RECT_WG_BIAS_ROWS:
        (H, W), (OH, OW) = S.map_sides(c)
        if lib.gz_conv2d_wgrad_fuses_bias(c.N, c.C, H, W, c.K, OH, OW, c.k, c.k, c.s, c.p) == 1:
            fused.append(c)
    assert fused, "no rectangular exact case takes the fused bias gradient"


def _rect_sink_rows():
    """The cheapest rectangular weight-gradient row of every loader family and direct kernel, and of each family the
    split and the unsplit launch where the table has both below 3e9 multiply-adds (the test takes three fp64 passes)."""
    best = {}
    for row in S.RECT_ROWS:
        if row[1] == "Wg" and S.case_macs(row[0]) < 3e9:
            g = _epilogue_group(row) + (row[3],)
            if g not in best or S.case_macs(row[0]) < S.case_macs(best[g][0]):
                best[g] = row
    return [best[g] for g in sorted(best)]


RECT_SINK_ROWS = _rect_sink_rows()


def test_the_rectangular_sink_rows_are_all_there():
    # direct: fewk, fewc, smallch (split); WgImgBG, WgALoaderRow, WgALoader: split and unsplit; igemm2r, WgImgB2: unsplit
    assert len(RECT_SINK_ROWS) == 11 and any(r[3] for r in RECT_SINK_ROWS) and any(not r[3] for r in RECT_SINK_ROWS)
    assert any(r[0].H > r[0].W for r in RECT_SINK_ROWS) and any(r[0].H < r[0].W for r in RECT_SINK_ROWS)


@pytest.mark.parametrize("row", RECT_SINK_ROWS, ids=S.row_id)
def test_rectangular_weight_gradient_slabs_summed_by_reduce_multi(row):
    test_weight_gradient_slabs_summed_by_reduce_multi(row)


@pytest.mark.parametrize("case", S.RECT_SPLIT_K_CASES, ids=S.case_id)
def test_rectangular_conv_split_k(case):
    lib, _ = _lib()
    c = case
    (H, W), (OH, OW) = S.map_sides(c)
    assert lib.gz_conv2d_fwd_workspace_bytes(c.N, c.C, H, W, c.K, OH, OW, c.k, c.k, c.s, c.p) > 0, "case no longer splits"
    assert lib.gz_conv2d_dgrad_workspace_bytes(c.N, c.C, H, W, c.K, OH, OW, c.k, c.k, c.s, c.p) > 0
    for op, nb in (("F", c.K), ("Dg", c.C)):
        a, b, ref = S.conv_ref(c, op)
        bias = int_operands((nb,), 7, 1.0, 43)
        assert_exact_precondition(S.conv_apply(c, op, a.double().abs(), b.double().abs()) + 7.0, op)
        assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda()), ref, op)
        assert_bits_equal(_run_conv(c, op, a.cuda(), b.cuda(), bias.cuda(), *_act_args("lrelu0.5")),
                          _act64(ref + bias.double().view(1, -1, 1, 1), "lrelu0.5"), op + " bias + lrelu0.5")
    a, b, ref = S.conv_ref(c, "Wg")
    assert_bits_equal(_run_conv(c, "Wg", a.cuda(), b.cuda()), ref, "Wg  [%s]" % S.conv2d_plan("Wg", *c))


@pytest.mark.parametrize("row", [r for r in S.RECT_EXTRA_ROWS if r[0] in S.RECT_UNALIGNED_CASES], ids=S.extra_id)
def test_rectangular_conv_operands_four_bytes_off_alignment(row):
    test_conv_operands_four_bytes_off_alignment(row)


@pytest.mark.parametrize("row", S.BOX3_ROWS, ids=S.row3_id)
def test_conv3d_box_at_every_plan_form(row):
    test_conv3d_family(row)


# ---------------------------------------------------------------------------------------------------------------------
# e. gz_gemm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.GEMM_CASES + S.GEMM_SPLIT_CASES)
def test_gemm_all_transposes_bias_and_split_k(shape):
    F = _F()
    lib, _ = _lib()
    M, N, K = shape
    if shape in S.GEMM_SPLIT_CASES:
        assert lib.gz_gemm_workspace_bytes(M, N, K) > 0, "case no longer splits"
    a, b, bias, ref = S.gemm_reference(M, N, K)
    ad, bd, at, bt = a.cuda(), b.cuda(), a.t().contiguous().cuda(), b.t().contiguous().cuda()
    assert_bits_equal(F.gemm(ad, bd), ref, "NN")
    assert_bits_equal(F.gemm(at, bd, trans_a=True), ref, "TN")
    assert_bits_equal(F.gemm(ad, bt, trans_b=True), ref, "NT")
    assert_bits_equal(F.gemm(at, bt, trans_a=True, trans_b=True), ref, "TT")
    ref_b = torch.relu(ref + bias.double())
    assert_bits_equal(F.gemm(ad, bd, bias.cuda(), act=F.ACT_RELU), ref_b, "NN bias relu")
    assert_bits_equal(F.gemm(at, bt, bias.cuda(), trans_a=True, trans_b=True, act=F.ACT_RELU), ref_b, "TT bias relu")
    assert_bits_equal(F.gemm(ad, bt, bias.cuda(), trans_b=True, act=F.ACT_LRELU, slope=0.5),
                      TF.leaky_relu(ref + bias.double(), 0.5), "NT bias lrelu0.5")


# ---------------------------------------------------------------------------------------------------------------------
# f. gz_conv2d_fwd_any
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FWD_ANY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_fwd_any(case):
    """Through the raw entry point into an output prefilled with NaN: equality also proves every element was written."""
    F = _F()
    lib, check = _lib()
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = case
    x, w, b, ref = S.fwd_any_reference(case)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    wp = torch.empty(lib.gz_conv2d_pack_fwd_any_elems(K, C, KH, KW), device="cuda")
    check(lib.gz_conv2d_pack_fwd_any(F._p(wd), F._p(wp), K, C, KH, KW, F._stream()), "pack")
    OH, OW = ref.shape[2:]
    y = torch.full((N, K, OH, OW), float("nan"), device="cuda")
    nb = lib.gz_conv2d_fwd_any_workspace_bytes(N, C, H, W, K, OH, OW, KH, KW, SH, SW, PH, PW)
    ws = torch.empty(max(nb // 4, 1), device="cuda")
    check(lib.gz_conv2d_fwd_any(F._p(xd), F._p(wp), F._p(bd), F._p(y), F._p(ws), nb, N, C, H, W, K, OH, OW, KH, KW, SH, SW,
                                PH, PW, F.ACT_RELU, 0.0, F._stream()), "fwd_any")
    assert_bits_equal(y, ref, "fwd_any %s" % (case,))
    if N >= 40:          # the igemm2 launches also write into a channel slice of a wider tensor
        before, after = 24, 40
        wide = torch.full((N, before + K + after, OH, OW), float("nan"), device="cuda")
        dst = wide[:, before:before + K]
        rc = lib.gz_conv2d_fwd_any_into(F._p(xd), F._p(wp), F._p(bd), ctypes.c_void_p(dst.data_ptr()), before + K + after,
                                        N, C, H, W, K, OH, OW, KH, KW, SH, SW, PH, PW, F.ACT_RELU, 0.0, F._stream())
        assert rc == 0, rc
        assert_bits_equal(dst, ref, "fwd_any_into")
        assert bool(torch.isnan(wide[:, :before]).all()) and bool(torch.isnan(wide[:, before + K:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# g. the FMA tails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.LINEAR_MULTI_SHAPES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "none"])
@pytest.mark.parametrize("with_bias", [True, False])
def test_linear_act_multi_forward_and_backward(shape, name, with_bias):
    F = _F()
    N, K, Js = shape
    x, ws, bs, Gs, outs, dx, dws, dbs = S.linear_case(N, K, Js, name, with_bias, 300)
    xd = x.cuda().requires_grad_()
    wd = [w.cuda().requires_grad_() for w in ws]
    bd = [None if b is None else b.cuda().requires_grad_() for b in bs]
    got = F.linear_act_multi(xd, list(zip(wd, bd)), *_act_args(name))
    sum((o * G.cuda()).sum() for o, G in zip(got, Gs)).backward()
    for j in range(len(Js)):
        assert_bits_equal(got[j], outs[j], "out %d" % j)
        assert_bits_equal(wd[j].grad, dws[j], "dW %d" % j)
        if with_bias:
            assert_bits_equal(bd[j].grad, dbs[j], "db %d" % j)
    assert_bits_equal(xd.grad, dx, "dx")


@pytest.mark.parametrize("shape", S.LINEAR_SHAPES)
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "none"])
def test_linear_act_forward_and_backward(shape, name):
    F = _F()
    N, K, Js = shape
    x, ws, bs, Gs, outs, dx, dws, dbs = S.linear_case(N, K, Js, name, True, 400)
    xd, wd, bd = x.cuda().requires_grad_(), ws[0].cuda().requires_grad_(), bs[0].cuda().requires_grad_()
    out = F.linear_act(xd, wd, bd, *_act_args(name))
    (out * Gs[0].cuda()).sum().backward()
    assert_bits_equal(out, outs[0], "out")
    assert_bits_equal(xd.grad, dx, "dx")
    assert_bits_equal(wd.grad, dws[0], "dW")
    assert_bits_equal(bd.grad, dbs[0], "db (gz_colsum)")


@pytest.mark.parametrize("shape", S.COLSUM_SHAPES)
def test_colsum(shape):
    F = _F()
    lib, check = _lib()
    R, L = shape
    x, ref = S.colsum_case(shape)
    xd = x.cuda()
    out = torch.full((L,), float("nan"), device="cuda")
    check(lib.gz_colsum(F._p(xd), F._p(out), R, L, F._stream()), "colsum")
    assert_bits_equal(out, ref, "colsum %s" % (shape,))


@pytest.mark.parametrize("shape", S.ROWDOT_SHAPES)
def test_rowdot_broadcast_and_not(shape):
    F = _F()
    a, b, ref, ref_bcast = S.rowdot_case(shape)
    assert_bits_equal(F._rowdot_raw(a.cuda(), b.cuda(), False), ref, "rowdot")
    assert_bits_equal(F._rowdot_raw(a.cuda(), b[0].contiguous().cuda(), True), ref_bcast, "rowdot broadcast")


@pytest.mark.parametrize("shape", S.COLDOT_SHAPES)
def test_coldot_and_its_partial_form(shape):
    """gz_coldot and gz_coldot_partial: sum_r g[r] x[r, :], with R below and at or above 64."""
    F = _F()
    lib, check = _lib()
    R, L = shape
    x, g, ref = S.coldot_case(shape)
    xd, gd = x.cuda(), g.cuda()
    assert_bits_equal(F._coldot_raw(gd, xd), ref, "coldot %s" % (shape,))
    nbytes = lib.gz_coldot_workspace_bytes(R, L)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), device="cuda")
    out = torch.full((L,), float("nan"), device="cuda")
    nz = ctypes.c_int(0)
    check(lib.gz_coldot_partial(F._p(gd), F._p(xd), F._p(out), F._p(ws), nbytes, R, L, ctypes.byref(nz), F._stream()), "partial")
    if nz.value > 1:
        slices = ws[:nz.value * L].view(nz.value, L)
        assert torch.equal(slices, slices.round())
        assert_bits_equal(slices.double().sum(0), ref, "coldot_partial (%d slices)" % nz.value)
    else:
        assert_bits_equal(out, ref, "coldot_partial (one slice)")


@pytest.mark.parametrize("shape", S.LERP_SHAPES)
def test_lerp_rows_rowscale_and_row_sumsq(shape):
    F = _F()
    R = shape[0]
    a, b, al, s, lerp64, scaled64, u, v, half, ss64, du64, dv64 = S.lerp_case(shape)
    assert_bits_equal(F.lerp_rows(a.cuda(), b.cuda(), al.cuda()), lerp64, "lerp_rows")
    assert_bits_equal(F.row_scale(a.cuda(), s.cuda()), scaled64, "row_scale")
    ud, vd = u.cuda().requires_grad_(), v.cuda().requires_grad_()
    ss = F.row_sumsq(F.lerp_rows(ud, vd, half.cuda()).reshape(R, -1))
    assert_bits_equal(ss, ss64, "row_sumsq")
    ss.sum().backward()
    assert_bits_equal(ud.grad, du64, "d row_sumsq / da")
    assert_bits_equal(vd.grad, dv64, "d row_sumsq / db")


@pytest.mark.parametrize("shape", S.CHANNEL_SUM_SHAPES)
def test_channel_sum(shape):
    g, ref = S.channel_sum_case(shape)
    assert_bits_equal(_F()._channel_sum_raw(g.cuda()), ref, "channel_sum %s" % (shape,))


@pytest.mark.parametrize("shape", S.FULL_DOT_SHAPES)
def test_full_dot_conv_and_its_two_gradients(shape):
    F = _F()
    x, w, G, out64, dx64, dw64 = S.full_dot_case(shape)
    xd, wd = x.cuda().requires_grad_(), w.cuda().requires_grad_()
    out = F.full_dot_conv(xd, wd)
    (out * G.cuda()).sum().backward()
    assert_bits_equal(out, out64, "full_dot_conv")
    assert_bits_equal(xd.grad, dx64, "dx")
    assert_bits_equal(wd.grad, dw64, "dw")


# ---------------------------------------------------------------------------------------------------------------------
# h. second order
# ---------------------------------------------------------------------------------------------------------------------
def test_conv_second_order_closure():
    """conv -> LeakyReLU(0.5) -> conv, gx = d out.sum() / dx with the graph kept, penalty sum(gx^2) + sum(out^2): gx and
    both weight gradients (and the output) against fp64 torch autograd."""
    F = _F()
    leaves = [o.cuda().requires_grad_() for o in S.second_order_conv_operands()]
    got = S.second_order_conv_graph(*leaves, lambda t, w: F.conv2d(t, w, None, F.K4S2P1),
                                    lambda t: F.activation(t, F.ACT_LRELU, 0.5))
    for name, g, ref in zip(("gx", "d pen / d w1", "d pen / d w2", "out"), got, S.second_order_conv_reference()):
        assert_bits_equal(g, ref, "separate activation: " + name)
    leaves = [o.cuda().requires_grad_() for o in S.second_order_conv_operands()]
    x, w1, w2 = leaves
    h = F.conv2d(x, w1, None, F.K4S2P1, F.ACT_LRELU, 0.5)              # the fused epilogue, as the models call it
    out = F.conv2d(h, w2, None, F.K4S2P1)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    ga, gb = torch.autograd.grad(gx.pow(2).sum() + out.pow(2).sum(), (w1, w2))
    for name, g, ref in zip(("gx", "d pen / d w1", "d pen / d w2", "out"), (gx, ga, gb, out), S.second_order_conv_reference()):
        assert_bits_equal(g, ref, "fused activation: " + name)


def test_full_dot_conv_second_order_closure():
    F = _F()
    leaves = [o.cuda().requires_grad_() for o in S.second_order_dot_operands()]
    got = S.second_order_dot_graph(*leaves, F.full_dot_conv)
    for name, g, ref in zip(("out", "gx", "d pen / dx", "d pen / dw"), got, S.second_order_dot_reference()):
        assert_bits_equal(g, ref, name)


# ---------------------------------------------------------------------------------------------------------------------
# i. the pair loss head (gz_pair_loss / gz_pair_loss_bwd)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_each", S.PAIR_MEAN_N)
@pytest.mark.parametrize("weights", S.PAIR_MEAN_WEIGHTS)
def test_weighted_half_means_is_exact_on_integer_logits(n_each, weights):
    """Mode 1: t0 * mean(first) + t1 * mean(second); n_each a power of two, upstream factor 0.25."""
    F = _F()
    x, ref, grad = S.pair_mean_case(n_each, weights)
    xd = x.cuda().requires_grad_()
    out = F.weighted_half_means(xd, *weights)
    (out * 0.25).backward()
    assert out.dim() == 0
    assert_bits_equal(out, ref, "value")
    assert_bits_equal(xd.grad, grad, "gradient")


@pytest.mark.parametrize("n_each", [1, 7, 64, 513, 33])
@pytest.mark.parametrize("targets", [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)])
def test_bce_logits_pair_mean_against_fp64(n_each, targets):
    """Mode 0 (inexact by design: expf / log1pf, csrc/gz_loss.hip pair_loss_kernel): value and gradient against fp64
    binary_cross_entropy_with_logits at the project's 1e-5 of test_fused_loss_heads, logits of +-30 included."""
    F = _F()
    g = torch.Generator().manual_seed(201 + n_each)
    x = torch.randn(2 * n_each, generator=g) * 3
    if n_each > 1:
        x[1], x[-2] = 30.0, -30.0
    x64 = x.double().requires_grad_()
    ref = (TF.binary_cross_entropy_with_logits(x64[:n_each], torch.full((n_each,), targets[0], dtype=torch.float64))
           + TF.binary_cross_entropy_with_logits(x64[n_each:], torch.full((n_each,), targets[1], dtype=torch.float64))) / 2
    (ref * 0.37).backward()
    xd = x.cuda().requires_grad_()
    out = F.bce_logits_pair_mean(xd.reshape(-1, 1), *targets)
    (out * 0.37).backward()

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))

    err_v, err_g = rel(out.detach(), ref.detach()), rel(xd.grad, x64.grad)
    print("n_each %d targets %s: value %.2e gradient %.2e" % (n_each, targets, err_v, err_g))
    assert out.dim() == 0 and err_v < 1e-5 and err_g < 1e-5

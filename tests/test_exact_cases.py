"""The exact-integer cases of tests/test_exact_gpu.py, checked where there is no GPU: every case satisfies the
precondition (sum |a||b| < 2^24, by the fp64 operator on absolute operands), torch's own fp32 CPU operator passes the
comparison on them, a subtly wrong kernel (10-bit or 7-bit operands, a dropped term, a narrow accumulator) does not,
every case takes the plan form it names, and no plan form of tests/golden/dispatch_plan.json is left out."""
import json
import os

import pytest
import torch

import exact_support as S

HERE = os.path.dirname(os.path.abspath(__file__))
S.set_threads()

# the fp32 CPU operator is run on every case below this many multiply-adds; the larger ones keep the precondition here
# and meet their reference in the GPU module
FP32_MACS = 3.0e9


def _macs(c):
    OH = S.out_side(c.H, c.k, c.s, c.p)
    return c.N * OH * OH * c.K * c.C * c.k * c.k


def _fails(got, ref64):
    with pytest.raises(AssertionError):
        S.assert_bits_equal(got, ref64, "sensitivity")


@pytest.mark.parametrize("row", S.CONV_ROWS, ids=S.row_id)
def test_conv2d_case_precondition_plan_and_reference_alone(row):
    c, op, form, split = row
    text = S.conv2d_plan(op, *c)
    assert S.plan_form(text) == form, text
    a, b, ref = S.conv_ref(c, op)                  # asserts the precondition
    assert float(a.abs().max()) == S.WIDE and bool((a % 2 == 1).any())
    if _macs(c) <= FP32_MACS:
        S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32 " + S.row_id(row))


@pytest.mark.parametrize("row", S.EXTRA_ROWS, ids=S.extra_id)
def test_split_k_and_unaligned_case_precondition_and_reference_alone(row):
    c, op = row
    a, b, ref = S.conv_ref(c, op)
    S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32 " + S.extra_id(row))


@pytest.mark.parametrize("case", S.STATS_CASES, ids=S.case_id)
@pytest.mark.parametrize("op", ["F", "Dg"])
def test_batchnorm_statistics_case_precondition(case, op):
    a, b, y = S.stats_reference(tuple(case), op)
    assert float((y * y).sum((0, 2, 3)).max()) < S.TWO24 and float(y.abs().max()) > 0
    S.assert_bits_equal(S.conv_apply(case, op, a, b), y, "torch fp32")


@pytest.mark.parametrize("case", S.FWD_ANY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fwd_any_case_precondition_and_reference_alone(case):
    x, w, b, ref = S.fwd_any_reference(case)
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = case
    S.assert_bits_equal(torch.relu(torch.nn.functional.conv2d(x, w, b, (SH, SW), (PH, PW))), ref, "torch fp32")


@pytest.mark.parametrize("row", S.CONV3_ROWS, ids=S.row3_id)
def test_conv3d_case_precondition_plan_and_reference_alone(row):
    c, op, form = row
    assert S.plan_form(S.conv3d_plan(op, *c)) == form
    a, b, ref = S.conv3_reference(tuple(c), op)
    if c.N * (c.D // 2) ** 3 * c.C * c.K * 27 <= FP32_MACS:
        S.assert_bits_equal(S.conv3_apply(c, op, a, b), ref, "torch fp32 " + S.row3_id(row))


@pytest.mark.parametrize("shape", S.GEMM_CASES + S.GEMM_SPLIT_CASES)
def test_gemm_case_precondition_and_reference_alone(shape):
    a, b, bias, ref = S.gemm_reference(*shape)
    S.assert_bits_equal(a @ b, ref, "torch fp32 gemm")
    S.assert_bits_equal(torch.relu(a @ b + bias), torch.relu(ref + bias.double()), "torch fp32 gemm + bias")


# the fused forms and the FMA tails: building a case asserts its preconditions
@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_activation_mask_case_preconditions(name):
    for case in S.DGRAD_ACT_CASES:
        S.dgrad_act_case(case, name)
    for case in S.WGRAD_ACT_CASES:
        S.wgrad_act_case(case, name)


@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "none"])
def test_linear_case_preconditions_and_reference_alone(name):
    for N, K, Js in S.LINEAR_MULTI_SHAPES + S.LINEAR_SHAPES:
        for with_bias in (True, False):
            x, ws, bs, Gs, outs, dx, dws, dbs = S.linear_case(N, K, Js, name, with_bias, 300)
            for w, b, o in zip(ws, bs, outs):
                S.assert_bits_equal(S.act64(torch.nn.functional.linear(x, w, b), name), o, "torch fp32 linear")


def test_tail_case_preconditions_and_reference_alone():
    for shape in S.COLSUM_SHAPES:
        x, ref = S.colsum_case(shape)
        S.assert_bits_equal(x.sum(0), ref, "torch fp32 colsum")
    for shape in S.ROWDOT_SHAPES:
        a, b, ref, _ = S.rowdot_case(shape)
        S.assert_bits_equal((a * b).sum(1), ref, "torch fp32 rowdot")
    for shape in S.COLDOT_SHAPES:
        x, g, ref = S.coldot_case(shape)
        S.assert_bits_equal(g @ x, ref, "torch fp32 coldot")
    for shape in S.LERP_SHAPES:
        S.lerp_case(shape)
    for shape in S.CHANNEL_SUM_SHAPES:
        S.channel_sum_case(shape)
    for shape in S.FULL_DOT_SHAPES:
        S.full_dot_case(shape)
    for n in S.PAIR_MEAN_N:
        for wts in S.PAIR_MEAN_WEIGHTS:
            S.pair_mean_case(n, wts)


def test_second_order_case_preconditions():
    S.second_order_conv_reference()
    S.second_order_dot_reference()


def test_no_golden_plan_form_is_left_out():
    """Every form of the pinned dispatch table, 2-D and 3-D, is the form of an exact case; the allowed share left out
    is zero."""
    golden = json.load(open(os.path.join(HERE, "golden", "dispatch_plan.json")))
    want = {S.plan_form(v) for cfg in golden.values() for v in cfg.values()}
    assert len(want) == 44, len(want)              # today's count: a new form needs a case of its own
    have = {S.plan_form(S.conv2d_plan(op, *c)) for c, op, _, _ in S.CONV_ROWS}
    have |= {S.plan_form(S.conv3d_plan(op, *c)) for c, op, _ in S.CONV3_ROWS}
    missing = sorted(want - have)
    assert not missing, "golden plan forms without an exact case:\n" + "\n".join(missing)


def test_no_plan_form_of_the_existing_case_tables_is_left_out():
    """The forms that the module-level case tables of test_ops_gpu.py reach, in all three directions."""
    import test_ops_gpu as T
    shapes = [(N, C, H, K) + T.GEOMS[g] for g in T.GEOMS for (N, C, H, K) in T.CONV_CASES]
    shapes += [(N, C, 2 * OH, K, 5, 2, 2) for (N, K, C, OH) in T.DG5_CASES]
    shapes += [(N, C, 2 * OH, K, 4, 2, 1) for (N, K, OH, C, _) in T.IGEMM2_DG_CASES]
    shapes += [(N, C, H, K, 4, 2, 1) for (N, C, H, K, _) in T.IGEMM2_F_CASES]
    shapes += [(N, C, H, K, 4, 2, 1) for (N, C, H, K) in T.IGEMM2_WG_CASES + T.UNALIGNED_CASES]
    shapes += [tuple(c) for c in T.IGEMM2_TAP_CASES + T.IGEMM2WG_CASES + T._random_gather_cases(14, 7)]
    shapes += [(N, C, H, K, 5, 2, 2) for (N, C, H, K) in T.IGEMM2_TAP_DG_CASES]
    shapes += [(N, C, H, K, k, 1, pd) for (N, C, H, K, k, pd) in T.IGEMM2_TAP_DG_S1_CASES]
    want = {S.plan_form(S.conv2d_plan(op, *sh)) for sh in shapes for op in S.OPS}
    have = {S.plan_form(S.conv2d_plan(op, *c)) for c, op, _, _ in S.CONV_ROWS}
    missing = sorted(want - have)
    assert len(want) > 44 and not missing, "plan forms of the existing tables without an exact case:\n" + "\n".join(missing)


def test_every_launch_the_planner_offers_in_the_enumeration_has_a_row():
    """One case per (form, split / unsplit) where the planner offers both: every key that S.enumerate_plans() reaches
    (N, C, H, K lists x four geometries x three directions, up to 1.5e10 multiply-adds) is the key of a row."""
    have = {(form, split) for _, _, form, split in S.CONV_ROWS}
    missing = sorted(k for k in S.enumerate_plans() if k not in have)
    assert not missing, "launches without an exact case:\n" + "\n".join("%s split=%s" % k for k in missing)


def test_split_and_unsplit_launches_are_what_the_table_says():
    for c, op, form, split in S.CONV_ROWS:
        assert (S.split_count(S.conv2d_plan(op, *c)) > 1) == split, (c, op)


# every path through the four launchers' shared host code (make_grid, launch_big_lds, launch_splitk_finish) that a
# launcher has: the arithmetic a comparison of device code does not see
LAUNCH_PATHS = [(L, p) for L in ("igemm", "igemm2") for p in
                ("unsplit", "split: finish<4>", "split: finish<8>", "split: epilogue slabs", "phases unsplit",
                 "phases split: finish<4>", "phases split: finish<8>")]
LAUNCH_PATHS.remove(("igemm2", "split: epilogue slabs"))      # (its weight gradients are igemm2w / igemm2r)
LAUNCH_PATHS += [("igemm2", "KG=2 unsplit"), ("igemm2", "KG=2 split: finish<4>"), ("igemm2", "KG=2 split: finish<8>"),
                 ("igemm2r", "unsplit"), ("igemm2r", "split: epilogue slabs"),
                 ("igemm2w", "unsplit"), ("igemm2w", "split: epilogue slabs")]


def test_every_path_through_the_launchers_has_a_case():
    have = S.launch_paths()
    missing = [k for k in LAUNCH_PATHS if not have.get(k)]
    assert not missing, "launcher paths without an exact case: %s" % missing


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: what a subtly wrong kernel would return is NOT equal -- one case per direction and the GEMM
# ---------------------------------------------------------------------------------------------------------------------
SENSITIVITY = [(S.ConvCase(2, 16, 8, 40, 3, 1, 1), "F"), (S.ConvCase(2, 64, 16, 64, 4, 2, 1), "Dg"),
               (S.ConvCase(2, 72, 64, 96, 1, 1, 0), "Wg")]


def _halves(c, op, a, b):
    """The two halves of the reduction as separate fp32 results: F / Dg split the reduced channels, Wg the batch."""
    if op == "Wg":
        h = c.N // 2
        return [S.conv_apply(c._replace(N=n), op, aa, bb) for n, aa, bb in ((h, a[:h], b[:h]), (c.N - h, a[h:], b[h:]))]
    if op == "F":
        h = c.C // 2
        return [S.conv_apply(c, op, a[:, :h], b[:, :h]), S.conv_apply(c, op, a[:, h:], b[:, h:])]
    h = c.K // 2
    return [S.conv_apply(c, op, a[:, :h], b[:h]), S.conv_apply(c, op, a[:, h:], b[h:])]


@pytest.mark.parametrize("case,op", SENSITIVITY, ids=lambda v: v if isinstance(v, str) else S.case_id(v))
def test_a_subtly_wrong_conv_kernel_is_not_equal(case, op):
    c = case
    assert any(r[0] == c and r[1] == op for r in S.CONV_ROWS)
    a, b, ref = S.conv_ref(c, op)
    S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32")
    for bits in (10, 7):                                            # a reduced-precision operand path
        _fails(S.conv_apply(c, op, S.round_mantissa(a, bits), b), ref)
    parts = _halves(c, op, a, b)
    S.assert_bits_equal(parts[0] + parts[1], ref, "two halves in fp32")
    _fails((parts[0].half() + parts[1].half()).float(), ref)        # a narrow accumulator
    # the last term of the reduction dropped: the last pixel (Wg) or the last (channel, tap) (F, Dg)
    a2, b2 = a.clone(), b.clone()
    if op == "Wg":
        assert float(a[-1, :, -1, -1].abs().max()) > 0 and float(b[-1, :, -1, -1].abs().max()) > 0
        b2[-1, :, -1, -1] = 0
    elif op == "F":
        b2[:, -1, -1, -1] = 0
    else:
        b2[-1, :, -1, -1] = 0
    assert not torch.equal(b2, b)
    _fails(S.conv_apply(c, op, a2, b2), ref)


def test_a_subtly_wrong_gemm_is_not_equal():
    a, b, bias, ref = S.gemm_reference(100, 512, 300)
    for bits in (10, 7):
        _fails(S.round_mantissa(a, bits) @ b, ref)
    h = a.shape[1] // 2
    p0, p1 = a[:, :h] @ b[:h], a[:, h:] @ b[h:]
    S.assert_bits_equal(p0 + p1, ref, "two halves in fp32")
    _fails((p0.half() + p1.half()).float(), ref)
    _fails(a[:, :-1] @ b[:-1], ref)                                 # the last term dropped


def test_the_helpers_themselves():
    t = S.int_operands((64, 64), 4095, 0.5, 3)
    assert torch.equal(t, t.round()) and float(t.abs().max()) == 4095 and 0.4 < float((t != 0).float().mean()) < 0.6
    assert torch.equal(t, S.int_operands((64, 64), 4095, 0.5, 3)) and not torch.equal(t, S.int_operands((64, 64), 4095, 0.5, 4))
    assert S.plan_form("F igemm2<256x64> X slabs=12 bn_stats_rows=1 wave_groups=2") == \
        "F igemm2<256x64> X slabs= bn_stats_rows= wave_groups=2"
    assert S.plan_form("Dg igemm<64x64> Y splits=3 slabs=27") == "Dg igemm<64x64> Y splits= slabs="
    assert float(S.round_mantissa(torch.tensor([4095.0]), 10)) == 4096.0
    assert float(S.round_mantissa(torch.tensor([4095.0]), 7)) == 4096.0
    assert float(S.round_mantissa(torch.tensor([1025.0]), 10)) == 1025.0
    with pytest.raises(AssertionError):
        S.assert_exact_precondition(torch.tensor([2.0 ** 24]))
    nan = torch.full((2, 2), float("nan"))
    with pytest.raises(AssertionError, match="4 of 4 elements differ"):
        S.assert_bits_equal(nan, torch.zeros(2, 2, dtype=torch.float64), "unwritten")

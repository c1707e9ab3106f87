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


# ---------------------------------------------------------------------------------------------------------------------
# rectangular maps and box volumes ("Exact-integer parity": what squares and cubes cannot see)
# ---------------------------------------------------------------------------------------------------------------------
def _row_is_mid(c, op, form):
    _, (OH, OW) = S.map_sides(c)
    return S.mid_tile(c.N, OH * OW, S.tile_pixels(form, op))


@pytest.mark.parametrize("row", S.RECT_ROWS, ids=S.row_id)
def test_rectangular_case_precondition_plan_and_reference_alone(row):
    c, op, form, split = row
    assert c.H != c.W
    text = S.conv2d_plan(op, *c)
    assert S.plan_form(text) == form and (S.split_count(text) > 1) == split, text
    a, b, ref = S.conv_ref(c, op)                  # asserts the precondition
    assert float(a.abs().max()) == S.WIDE and bool((a % 2 == 1).any())
    if S.case_macs(c) <= FP32_MACS:
        S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32 " + S.row_id(row))


@pytest.mark.parametrize("row", S.RECT_EXTRA_ROWS, ids=S.extra_id)
def test_rectangular_split_k_and_unaligned_case_precondition_and_reference_alone(row):
    c, op = row
    a, b, ref = S.conv_ref(c, op)
    if S.case_macs(c) <= FP32_MACS:
        S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32 " + S.extra_id(row))


def _tall_wide_and_mid(shapes, tile=256):
    """``shapes``: (N, H, W, pixels per image) -- a tall one, a wide one and a mid-tile one are among them."""
    return (any(H > W for _, H, W, _ in shapes) and any(H < W for _, H, W, _ in shapes)
            and any(S.mid_tile(N, px, tile) for N, _, _, px in shapes))


def test_rectangular_split_k_and_unaligned_cases_split_and_cover_both_orientations():
    from lightning_gan_zoo_amd._lib import lib
    for c in S.RECT_SPLIT_K_CASES:
        (H, W), (OH, OW) = S.map_sides(c)
        assert lib.gz_conv2d_fwd_workspace_bytes(c.N, c.C, H, W, c.K, OH, OW, c.k, c.k, c.s, c.p) > 0, c
        assert lib.gz_conv2d_dgrad_workspace_bytes(c.N, c.C, H, W, c.K, OH, OW, c.k, c.k, c.s, c.p) > 0, c
    assert sum(S.split_count(S.conv2d_plan("Wg", *c)) > 1 for c in S.RECT_SPLIT_K_CASES) >= 2
    for c in S.RECT_UNALIGNED_CASES:
        assert "F igemm2<" in S.conv2d_plan("F", *c)
    assert any("Dg igemm2<" in S.conv2d_plan("Dg", *c) and "Wg igemm2w<" in S.conv2d_plan("Wg", *c)
               for c in S.RECT_UNALIGNED_CASES)
    for cases in (S.RECT_SPLIT_K_CASES, S.RECT_UNALIGNED_CASES):
        assert _tall_wide_and_mid([(c.N, c.H, c.W, (c.H // c.s) * (c.W // c.s)) for c in cases])


@pytest.mark.parametrize("case", S.RECT_STATS_CASES, ids=S.case_id)
@pytest.mark.parametrize("op", ["F", "Dg"])
def test_rectangular_batchnorm_statistics_case_precondition(case, op):
    from lightning_gan_zoo_amd._lib import lib
    c = case
    fn = lib.gz_conv2d_fwd_stats_rows if op == "F" else lib.gz_conv2d_dgrad_stats_rows
    assert fn(c.N, c.C, c.H, c.W, c.K, c.H // 2, c.W // 2, 4, 4, 2, 1) > 0, "the case does not carry the statistics"
    a, b, y = S.stats_reference(tuple(c), op)
    assert float((y * y).sum((0, 2, 3)).max()) < S.TWO24 and float(y.abs().max()) > 0
    S.assert_bits_equal(S.conv_apply(c, op, a, b), y, "torch fp32")


def test_rectangular_statistics_and_activation_cases_cover_both_orientations():
    from lightning_gan_zoo_amd._lib import lib
    assert _tall_wide_and_mid([(c.N, c.H, c.W, c.H // 2 * (c.W // 2)) for c in S.RECT_STATS_CASES])
    assert any("igemm2<" in S.conv2d_plan("F", *c) for c in S.RECT_STATS_CASES)
    assert any("igemm2<" in S.conv2d_plan("Dg", *c) for c in S.RECT_STATS_CASES)
    for cases, fuses in ((S.RECT_DGRAD_ACT_CASES, lib.gz_conv2d_dgrad_act_fuses), (S.RECT_WGRAD_ACT_CASES, lib.gz_conv2d_wgrad_act_fuses)):
        assert _tall_wide_and_mid([(N, H, W, H // 2 * (W // 2)) for N, C, H, W, K in cases])
        for N, C, H, W, K in cases:
            assert C in (3, 4) and H != W
            for act in (1, 2):             # ACT_RELU, ACT_LRELU
                assert fuses(N, C, H, W, K, H // 2, W // 2, 4, 4, 2, 1, act) == 1, (N, C, H, W, K)


@pytest.mark.parametrize("name", ["relu", "lrelu0.5", "lrelu0.25"])
def test_rectangular_activation_mask_case_preconditions(name):
    for case in S.RECT_DGRAD_ACT_CASES:
        S.dgrad_act_case(case, name)
    for case in S.RECT_WGRAD_ACT_CASES:
        S.wgrad_act_case(case, name)


@pytest.mark.parametrize("row", S.BOX3_ROWS, ids=S.row3_id)
def test_conv3d_box_case_precondition_plan_and_reference_alone(row):
    c, op, form = row
    assert len({c.D, c.H, c.W}) == 3, "D, H, W pairwise different (every form of the table admits it)"
    assert S.plan_form(S.conv3d_plan(op, *c)) == form
    a, b, ref = S.conv3_reference(tuple(c), op)
    if S.row3_macs(c) <= FP32_MACS:
        S.assert_bits_equal(S.conv3_apply(c, op, a, b), ref, "torch fp32 " + S.row3_id(row))


def test_every_launch_the_planner_offers_on_a_rectangle_has_a_row():
    """Every (form, split) key S.enumerate_rect_plans() reaches is the key of a rectangular row: the allowed share left
    out is zero.  The keys of CONV_ROWS without a rectangular row are exactly S.RECT_UNREACHED, and the enumeration reaches
    none of them, so that list cannot hide a gap."""
    reached = S.enumerate_rect_plans()
    have = {(form, split) for _, _, form, split in S.RECT_ROWS}
    missing = sorted(k for k in reached if k not in have)
    assert not missing, "launches without a rectangular case:\n" + "\n".join("%s split=%s" % k for k in missing)
    square = {(form, split) for _, _, form, split in S.CONV_ROWS}
    assert sorted(square - have) == sorted(S.RECT_UNREACHED)
    assert not [k for k in S.RECT_UNREACHED if k in reached]
    assert len(S.RECT_UNREACHED) <= 6
    # the counts recorded next to the table: keys reached, and keys whose row holds a mid-tile image boundary -- every key
    # that has such a shape in the enumeration
    assert len(reached) == S.RECT_KEYS == len(have)
    mid_rows = {(form, split) for c, op, form, split in S.RECT_ROWS if _row_is_mid(c, op, form)}
    assert mid_rows == {k for k, (_, mid) in reached.items() if mid is not None}
    assert len(mid_rows) == S.RECT_MID_KEYS


def test_rectangular_rows_cover_both_orientations_of_every_loader_family():
    tall = sum(1 for c, _, _, _ in S.RECT_ROWS if c.H > c.W)
    assert abs(2 * tall - len(S.RECT_ROWS)) <= len(S.RECT_ROWS) // 10, "orientations out of balance: %d tall" % tall
    for fam in S.LOADER_FAMILIES:
        for op in S.OPS:
            rows = [c for c, o, form, _ in S.RECT_ROWS if o == op and S.loader_family(form) == fam]
            if rows and fam != "igemm2r":      # (2-pixel feature rows, W = 4 with OH a multiple of 8: tall maps only)
                assert any(c.H > c.W for c in rows) and any(c.H < c.W for c in rows), (fam, op)
    named = ["ConvFwdA2", "ConvDgA2", "ConvDg5A2", "ConvTapA2", "ConvDgTapA2", "WgImgB2", "WgImgBG", "Row4", "K4V", "ALoaderTap", "direct"]
    assert all(any(S.loader_family(form) == fam for _, _, form, _ in S.RECT_ROWS) for fam in named)


def test_every_conv3d_form_the_planner_offers_on_a_box_has_a_row():
    reached = S.enumerate_box_plans()
    have = {form for _, _, form in S.BOX3_ROWS}
    missing = sorted(f for f in reached if f not in have)
    assert not missing, "conv3d forms without a box case:\n" + "\n".join(missing)
    cubes = {form for _, _, form in S.CONV3_ROWS}
    assert sorted(cubes - have) == sorted(S.BOX3_UNREACHED)
    assert not [f for f in S.BOX3_UNREACHED if f in reached]
    assert len(reached) == S.BOX3_FORMS == len(have) and len(have - cubes) >= 5
    mid_rows = {form for c, op, form in S.BOX3_ROWS if S.mid_tile(c.N, S.box_pixels(c), S.tile_pixels(form, op))}
    assert mid_rows == {f for f, (_, mid) in reached.items() if mid is not None} and len(mid_rows) == S.BOX3_MID_FORMS


RECT_SENSITIVITY = [(S.RectCase(3, 16, 12, 8, 40, 5, 2, 2), "F"), (S.RectCase(3, 64, 12, 8, 64, 4, 2, 1), "Dg"),
                    (S.RectCase(3, 4, 6, 16, 65, 3, 1, 1), "Wg")]


@pytest.mark.parametrize("case,op", RECT_SENSITIVITY, ids=lambda v: v if isinstance(v, str) else S.case_id(v))
def test_a_kernel_that_confuses_the_sides_of_a_rectangle_is_not_equal(case, op):
    """What a square case cannot see: (a) H and W exchanged, (b) no padding between the images of a batch (a vertical
    halo row fetched from the neighbouring image), (c) the last image row dropped."""
    c = case
    assert any(r[0] == c and r[1] == op for r in S.RECT_ROWS) and c.N > 1 and c.k > 1 and c.p > 0
    a, b, ref = S.conv_ref(c, op)
    S.assert_bits_equal(S.conv_apply(c, op, a, b), ref, "torch fp32")
    maps = [a] + ([b] if op == "Wg" else [])            # the operands that are maps: x (and gy); the other is the filter
    # (a) the same memory viewed with the sides exchanged, the result viewed back
    swapped = [t.reshape(t.shape[0], t.shape[1], t.shape[3], t.shape[2]) for t in maps]
    for t, t2 in zip(maps, swapped):
        assert not torch.equal(t2, t.transpose(2, 3)) and float(t[:, :, 1:].abs().max()) > 0
    got = S.conv_apply(c._replace(H=c.W, W=c.H), op, swapped[0], swapped[1] if op == "Wg" else b)
    _fails(got.reshape(ref.shape), ref)
    # (b) the batch as one tall image of N * H rows: rows next to an image boundary see the neighbour, not padding
    for t in maps:
        assert float(t[1:, :, 0].abs().max()) > 0 and float(t[:-1, :, -1].abs().max()) > 0
    tall = [t.transpose(0, 1).reshape(1, t.shape[1], c.N * t.shape[2], t.shape[3]) for t in maps]
    got = S.conv_apply(c._replace(N=1, H=c.N * c.H), op, tall[0], tall[1] if op == "Wg" else b)
    if op != "Wg":                                      # sliced back per image
        got = got.reshape(got.shape[1], c.N, -1, got.shape[3]).transpose(0, 1)
    _fails(got, ref)
    # (c) the last row of every image dropped
    cut = [t.clone() for t in maps]
    for t in cut:
        assert float(t[:, :, -1].abs().max()) > 0
        t[:, :, -1] = 0
    _fails(S.conv_apply(c, op, cut[0], cut[1] if op == "Wg" else b), ref)


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

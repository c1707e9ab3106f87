"""Exact-integer parity ("Exact-integer parity"): operands, precondition, assertion and the case tables that
tests/test_exact_cases.py (CPU) and tests/test_exact_gpu.py share.  Importable without a GPU.

With integer operands and sum |a||b| < 2^24 per output element, every product and every partial sum of a multiply-add
kernel is an integer below 2^24: fp32 holds it exactly in any summation order, with or without FMA, through any
split-K slab sum and any MFMA shape, and fp64 on the CPU (below 2^53) does too.  So the comparison is torch.equal."""
import ctypes
import functools
import re
from collections import namedtuple

import torch
import torch.nn.functional as TF

TWO24 = float(2 ** 24)
WIDE = 4095          # 12 significant bits, odd: a 10-bit (TF32 / fp16) or 7-bit (bf16) operand path cannot carry it
OPS = ("F", "Dg", "Wg")


def int_operands(shape, amp, density, seed):
    """Seeded integer-valued fp32 tensor: a fraction ``density`` of the entries is uniform in [-amp, amp] \\ {0}, the
    rest is 0.  The first entry is +-amp itself (amp is odd in every wide operand), so the widest value is there at any
    size and density."""
    g = torch.Generator().manual_seed(int(seed))
    mag = torch.randint(1, int(amp) + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    keep = torch.rand(tuple(shape), generator=g) < float(density)
    out = (mag * sign * keep).to(torch.float32)
    out.view(-1)[0] = float(amp) if seed % 2 else -float(amp)
    return out


def assert_exact_precondition(abs_result, what=""):
    """``abs_result``: the same operator in fp64 on |a|, |b| (and |bias|).  A case that fails this is a broken case."""
    top = float(abs_result.max())
    assert top < TWO24, "%s: sum |a||b| reaches %.0f >= 2^24: the case is not exact in fp32 (thin its operands)" % (what, top)
    assert top > 0, "%s: all-zero case" % what
    return top


def assert_bits_equal(got, ref64, what=""):
    got64 = got.detach().double().cpu()
    assert got64.shape == ref64.shape, "%s: shape %s, reference %s" % (what, tuple(got64.shape), tuple(ref64.shape))
    if torch.equal(got64, ref64):
        return
    bad = ~(got64 == ref64)                  # NaN (an element nobody wrote) differs from everything
    idx = bad.nonzero()
    diff = (got64 - ref64).abs()
    lines = ["%s: %d of %d elements differ (largest difference %s, largest reference magnitude %g)"
             % (what, int(bad.sum()), bad.numel(), float(torch.nan_to_num(diff, nan=float("inf")).max()),
                float(ref64.abs().max()))]
    for i in idx[:8]:
        t = tuple(int(v) for v in i)
        lines.append("    %s: got %r, reference %r" % (t, float(got64[t]), float(ref64[t])))
    raise AssertionError("\n".join(lines))


def plan_form(text):
    """The plan text with the counts behind splits= / slabs= / bn_stats_rows= removed (wave_groups=2 stays: it is a
    different launch)."""
    return re.sub(r"\b(splits|slabs|bn_stats_rows)=\d+", r"\1=", text)


def round_mantissa(t, bits):
    """``t`` rounded to ``bits`` explicit mantissa bits (10: TF32 / fp16 class, 7: bf16), round to nearest even."""
    drop = 23 - bits
    i = t.contiguous().view(torch.int32).to(torch.int64)
    i = i + ((1 << (drop - 1)) - 1) + ((i >> drop) & 1)
    return ((i >> drop) << drop).to(torch.int32).view(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# plans (host-only logic of the library)
# ---------------------------------------------------------------------------------------------------------------------
def out_side(H, k, s, p):
    return (H + 2 * p - k) // s + 1


def conv2d_plan(op, *shape):
    """``shape``: N C H K k s p (a ConvCase: the square map H x H) or N C H W K k s p (a RectCase)."""
    from lightning_gan_zoo_amd._lib import lib
    buf = ctypes.create_string_buffer(512)
    N, C, H, W, K, k, s, p = shape if len(shape) == 8 else shape[:3] + (shape[2],) + shape[3:]
    rc = lib.gz_conv2d_plan(OPS.index(op), N, C, H, W, K, out_side(H, k, s, p), out_side(W, k, s, p), k, k, s, p, buf, 512)
    assert rc >= 0, (op, shape, rc)
    return buf.value.decode()


def conv3d_plan(op, *shape):
    """The Conv3d view (make_dispatch_golden.py): image side [N, C, D, H, W], feature side [N, K, D/2, H/2, W/2], k3 s2
    p1.  ``shape``: N C D K (a Conv3Case: the cube D^3) or N C D H W K (a Box3Case)."""
    from lightning_gan_zoo_amd._lib import lib
    buf = ctypes.create_string_buffer(512)
    N, C, D, H, W, K = shape if len(shape) == 6 else shape[:3] + (shape[2], shape[2]) + shape[3:]
    rc = lib.gz_conv3d_plan(OPS.index(op), N, C, D, H, W, K, D // 2, H // 2, W // 2, 3, 2, 1, buf, 512)
    assert rc >= 0, (op, shape, rc)
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------------------------
# operands of a multiply-add case: one WIDE operand (|v| <= 4095, 12 bits), one small ({-1, 0, 1} .. +-3), thinned
# until the longest reduction stays below 2^24
# ---------------------------------------------------------------------------------------------------------------------
def thin(terms, target=2.0 ** 21):
    """(density of each operand, amplitude of the small one) for a reduction of ``terms`` products: the expected
    sum |a||b| = terms * (WIDE + 1) / 2 * (amp + 1) / 2 * density^2 stays near ``target`` = 2^24 / 8 (the margin is for
    the largest of many output elements; assert_exact_precondition checks the case itself).  The density is lowered
    first, with the small operand at +-3; only where that would leave fewer than one entry in four does the small operand
    go down to {-1, 0, 1}, and the density goes on from there.  The wide operand keeps 4095."""
    for amp in (3, 1):
        d2 = target / (terms * (WIDE + 1) / 2.0 * (amp + 1) / 2.0)
        if d2 >= 1.0 / 16 or amp == 1:
            return min(1.0, max(d2, 1e-4) ** 0.5), amp


def pair(shape_wide, shape_small, terms, seed):
    d, amp = thin(terms)
    return int_operands(shape_wide, WIDE, d, seed), int_operands(shape_small, amp, d, seed + 1)


def split_count(text):
    return max([int(v) for v in re.findall(r"(?:splits|slabs)=(\d+)", text)], default=0)


def launch_path(text, op, phases):
    """(launcher, path) a plan text stands for, in the terms of csrc/gz_igemm_core.h make_grid: which of launch_igemm /
    launch_igemm2 / launch_igemm2r / launch_igemm2w, unsplit or how the split reduction is finished (the weight
    gradient's epilogue writes its own slabs; the others go through raw slabs and splitk_finish_kernel<Epi, 8> above 16
    slabs, <Epi, 4> up to 16), ``phases`` = the launch passes per-phase chunk counts (GridMap::var_chunks), and the
    two-wave-group kernel.  None: a direct kernel."""
    m = re.search(r"\b(igemm2w|igemm2r|igemm2|igemm)<", text)
    if not m:
        return None
    n = split_count(text) or 1
    if n == 1:
        path = "unsplit"
    elif op == "Wg":
        path = "split: epilogue slabs"
    else:
        path = "split: finish<8>" if n > 16 else "split: finish<4>"
    return m.group(1), ("phases " if phases else "") + ("KG=2 " if "wave_groups=2" in text else "") + path


def launch_paths():
    """{(launcher, path): [test ids]} over the conv2d and conv3d case tables (host only).  Per-phase chunk counts: the 2-D
    input gradients of the tap-major loaders at stride 2 with other than 4x4 taps (run_dgrad*: 9 / 6 / 6 / 4 taps per
    phase at 5x5), every 3-D input gradient."""
    out = {}
    for c, op, form, split in CONV_ROWS:
        text = conv2d_plan(op, *c)
        phases = op == "Dg" and c.s == 2 and c.k != 4 and "Tap" in text
        out.setdefault(launch_path(text, op, phases), []).append("test_conv2d_at_every_plan_form[%s]" % row_id((c, op)))
    for c, op, form in CONV3_ROWS:
        text = conv3d_plan(op, *c)
        out.setdefault(launch_path(text, op, op == "Dg"), []).append("test_conv3d_family[%s]" % row3_id((c, op)))
    out.pop(None, None)
    return out


ENUM_NS = [1, 2, 3, 4, 8, 16, 32, 33, 50, 64, 128, 131, 256, 512]
ENUM_CS = [1, 2, 3, 4, 6, 16, 20, 32, 64, 72, 128, 132, 256, 384, 512, 1024]
ENUM_HS = [4, 8, 12, 16, 24, 32, 64]
ENUM_KS = [3, 4, 7, 16, 32, 40, 64, 72, 96, 128, 132, 160, 256, 512, 1024]
ENUM_GEOMS = [(4, 2, 1), (5, 2, 2), (3, 1, 1), (1, 1, 0)]


def enumerate_plans(max_macs=1.5e10):
    """{(plan form, split): (multiply-adds, shape, direction)} with the cheapest shape per key, over N, C, H, K of the
    lists above, the four layer geometries and the three directions (host only).  tools/find_exact_cases.py prints it;
    tests/test_exact_cases.py holds the case table to it: what the planner offers here has a row."""
    import itertools
    best = {}
    for (k, s, p), N, C, H, K in itertools.product(ENUM_GEOMS, ENUM_NS, ENUM_CS, ENUM_HS, ENUM_KS):
        if H + 2 * p < k:
            continue
        OH = out_side(H, k, s, p)
        macs = N * OH * OH * K * C * k * k
        if macs > max_macs or N * C * H * H > 1.4e8 or N * K * OH * OH > 1.4e8:
            continue
        for op in OPS:
            text = conv2d_plan(op, N, C, H, K, k, s, p)
            key = (plan_form(text), split_count(text) > 1)
            if key not in best or macs < best[key][0]:
                best[key] = (macs, (N, C, H, K, k, s, p), op)
    return best


# Rectangular maps (H != W) and box volumes.  The chooser selects most fast loaders by OW alone, and a square power-of-two
# map has 16 .. 4096 pixels -- always a divisor or a multiple of a 128- / 256- / 512-pixel tile -- so only a rectangle puts
# an image boundary inside a tile at a position that is no tile boundary ("mid-tile" below).
RECT_SIDES = [4, 6, 8, 10, 12, 16, 24, 32, 48, 64, 96]
# (shorter than ENUM_*: with 110 (H, W) pairs the scan is 5 s; the full ENUM_* lists with the odd channel counts of
# _CONV_TABLE -- 40 s -- reach the same 170 keys, 163 of them mid-tile)
RECT_NS = [1, 2, 3, 16, 50, 128, 512]
RECT_CS = [1, 2, 3, 4, 6, 16, 64, 72, 132, 384, 512, 1024]
RECT_KS = [3, 16, 32, 40, 64, 65, 128, 132, 256, 1024]


def tile_pixels(form, op):
    """Pixels along the tile's row dimension: the first number of igemm<AxB> / igemm2<AxB> for F and Dg.  The weight
    gradient's tile has no pixel dimension (pixels are its reduction) and a direct kernel has no tile: 256 for both, the
    workgroup size and the smallest igemm2 tile."""
    m = re.search(r"igemm2?<(\d+)x", form)
    return int(m.group(1)) if m and op != "Wg" else 256


# the loader families as the plan text names them, most specific first (loader_family() takes the first that matches)
LOADER_FAMILIES = ["direct", "ConvFwdA2", "ConvDg5A2", "ConvDgA2", "ConvDgTapA2", "ConvTapA2", "WgImgB2", "WgImgBG",
                   "igemm2r", "Row4", "K4V", "ALoaderTap", "WgALoaderRow", "WgALoader", "ConvFwdALoader", "ConvDgALoader"]


def loader_family(form):
    return next(f for f in LOADER_FAMILIES if f in form)


def orientation(shape):
    """Of a RectCase (or its tuple): "tall" (H > W) or "wide"."""
    return "tall" if shape[2] > shape[3] else "wide"


def mid_tile(N, pixels, tile):
    """More than one image, and the feature map (per-phase grid of a stride-2 input gradient) neither divides the tile nor
    is a multiple of it: some tile holds an image boundary that is no tile boundary."""
    return N > 1 and pixels % tile != 0 and tile % pixels != 0


@functools.lru_cache(maxsize=2)
def _rect_scan(max_macs):
    """{(plan form, split): {(orientation, mid-tile): (multiply-adds, shape, direction)}}: the cheapest shape per key,
    orientation ("tall": H > W, "wide": H < W) and whether the shape is mid-tile."""
    import itertools
    from lightning_gan_zoo_amd._lib import lib
    buf = ctypes.create_string_buffer(512)
    keys, best = {}, {}
    pairs = [(H, W) for H in RECT_SIDES for W in RECT_SIDES if H != W]
    for (k, s, p), (H, W) in itertools.product(ENUM_GEOMS, pairs):
        OH, OW = out_side(H, k, s, p), out_side(W, k, s, p)
        pixels = (H // s) * (W // s)             # = OH * OW on these even sides: the input gradient's per-phase grid
        orient = "tall" if H > W else "wide"
        for N, C, K in itertools.product(RECT_NS, RECT_CS, RECT_KS):
            macs = N * OH * OW * K * C * k * k
            if macs > max_macs or N * C * H * W > 1.4e8 or N * K * OH * OW > 1.4e8:
                continue
            for i, op in enumerate(OPS):
                rc = lib.gz_conv2d_plan(i, N, C, H, W, K, OH, OW, k, k, s, p, buf, 512)
                assert rc >= 0, (op, N, C, H, W, K, k, s, p, rc)
                text = buf.value
                key = keys.get(text)
                if key is None:
                    t = text.decode()
                    key = keys[text] = (plan_form(t), split_count(t) > 1)
                slot = best.setdefault(key, {})
                which = (orient, mid_tile(N, pixels, tile_pixels(key[0], op)))
                if which not in slot or macs < slot[which][0]:
                    slot[which] = (macs, (N, C, H, W, K, k, s, p), op)
    return best


def _cheapest(entries):
    entries = [e for e in entries if e is not None]
    return min(entries, key=lambda e: (e[0], e[1])) if entries else None


def enumerate_rect_plans(max_macs=1.5e10, orientation=None):
    """{(plan form, split): (cheapest, mid)} over the (H, W) pairs of RECT_SIDES with H != W, both orientations (or the
    one asked for), N, C, K of the RECT_* lists, the four layer geometries and the three directions (host only).
    ``cheapest``: (multiply-adds, shape, direction) of the cheapest rectangle of the key; ``mid``: the same for the
    cheapest one that is mid_tile(), None where the key has none.  tools/find_exact_cases.py --rect prints the rows."""
    out = {}
    for key, slot in _rect_scan(max_macs).items():
        sides = ("tall", "wide") if orientation is None else (orientation,)
        cheapest = _cheapest([slot.get((o, m)) for o in sides for m in (False, True)])
        if cheapest is not None:
            out[key] = (cheapest, _cheapest([slot.get((o, True)) for o in sides]))
    return out


BOX_SIDES = [4, 6, 8, 10, 12, 16, 24, 32]
BOX_NS = [1, 2, 5, 16, 24, 64]
BOX_CS = [1, 4, 16, 64, 72, 128, 130]
BOX_KS = [8, 20, 64, 72, 128, 512]


@functools.lru_cache(maxsize=2)
def _box_scan(max_macs):
    """{plan form: {(pairwise different sides, mid-tile): (multiply-adds, shape, direction)}} over the boxes that are no
    cubes."""
    import itertools
    best = {}
    boxes = [b for b in itertools.product(BOX_SIDES, repeat=3) if len(set(b)) > 1]
    for (D, H, W), N, C, K in itertools.product(boxes, BOX_NS, BOX_CS, BOX_KS):
        pixels = (D // 2) * (H // 2) * (W // 2)
        macs = N * pixels * C * K * 27
        if macs > max_macs or N * C * D * H * W > 1.4e8:
            continue
        for op in OPS:
            form = plan_form(conv3d_plan(op, N, C, D, H, W, K))
            which = (len({D, H, W}) == 3, mid_tile(N, pixels, tile_pixels(form, op)))
            slot = best.setdefault(form, {})
            if which not in slot or macs < slot[which][0]:
                slot[which] = (macs, (N, C, D, H, W, K), op)
    return best


def enumerate_box_plans(max_macs=1.5e10):
    """{plan form: (cheapest, mid)} of conv3d over the boxes of BOX_SIDES^3 that are no cubes, like enumerate_rect_plans
    (the 3-D table pins the form alone).  Shapes with D, H, W pairwise different are preferred where the form has one."""
    out = {}
    for form, slot in _box_scan(max_macs).items():
        diff = any(k[0] for k in slot)
        out[form] = (_cheapest([slot.get((d, m)) for d in ((True,) if diff else (False,)) for m in (False, True)]),
                     _cheapest([slot.get((d, True)) for d in ((True,) if diff else (False,))]))
    return out


# A conv2d case: x [N, C, H, H], w [K, C, k, k], feature side [N, K, OH, OH].
ConvCase = namedtuple("ConvCase", "N C H K k s p")
# The same on a rectangular map: x [N, C, H, W], feature side [N, K, OH, OW].  Every helper below takes either.
RectCase = namedtuple("RectCase", "N C H W K k s p")


def conv_case(key):
    """The case a plain tuple stands for (the lru_cache keys): 7 fields a ConvCase, 8 a RectCase."""
    return RectCase(*key) if len(key) == 8 else ConvCase(*key)


def map_sides(c):
    """(H, W) of the image side and (OH, OW) of the feature side."""
    H, W = c.H, getattr(c, "W", c.H)
    return (H, W), (out_side(H, c.k, c.s, c.p), out_side(W, c.k, c.s, c.p))


def case_id(c):
    if len(c) == 8:
        return "N%d_C%d_H%dxW%d_K%d_k%ds%dp%d" % tuple(c)
    return "N%d_C%d_H%d_K%d_k%ds%dp%d" % tuple(c[:7])


def case_macs(c):
    _, (OH, OW) = map_sides(c)
    return c.N * OH * OW * c.K * c.C * c.k * c.k


def conv_terms(c, op):
    _, (OH, OW) = map_sides(c)
    if op == "F":
        return c.C * c.k * c.k
    if op == "Dg":
        return c.K * ((c.k + c.s - 1) // c.s) ** 2
    return c.N * OH * OW


def conv_operands(c, op):
    """(a, b) of direction ``op``: F (x wide, w small), Dg (gy wide, w small), Wg (x wide, gy small)."""
    (H, W), (OH, OW) = map_sides(c)
    xs, ws, gs = (c.N, c.C, H, W), (c.K, c.C, c.k, c.k), (c.N, c.K, OH, OW)
    seed = 1000 + 7 * OPS.index(op) + (c.N * 31 + c.C * 17 + c.H * 13 + c.K * 11 + c.k + (W * 19 if len(c) == 8 else 0)) % 997
    shapes = {"F": (xs, ws), "Dg": (gs, ws), "Wg": (xs, gs)}[op]
    return pair(shapes[0], shapes[1], conv_terms(c, op), seed)


def conv_apply(c, op, a, b, bias=None):
    """Direction ``op`` of the case by torch's CPU operator in the dtype of the operands."""
    if op == "F":
        return TF.conv2d(a, b, bias, c.s, c.p)
    if op == "Dg":
        sides, outs = map_sides(c)
        return TF.conv_transpose2d(a, b, bias, c.s, c.p,
                                   output_padding=tuple(h - ((o - 1) * c.s - 2 * c.p + c.k) for h, o in zip(sides, outs)))
    return torch.nn.grad.conv2d_weight(a, (c.K, c.C, c.k, c.k), b, stride=c.s, padding=c.p)


def set_threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@functools.lru_cache(maxsize=4)
def conv_reference(c_key, op):
    """(a, b, ref64) with the precondition asserted; computed once per (case, direction) and shared."""
    c = conv_case(c_key)
    set_threads()
    a, b = conv_operands(c, op)
    assert_exact_precondition(conv_apply(c, op, a.double().abs(), b.double().abs()), "%s %s" % (case_id(c), op))
    return a, b, conv_apply(c, op, a.double(), b.double())


def conv_ref(c, op):
    return conv_reference(tuple(c), op)


# ---------------------------------------------------------------------------------------------------------------------
# conv2d case table: the smallest shape found for every plan form (tests/test_exact_cases.py re-checks the forms and
# that no form of tests/golden/dispatch_plan.json is missing)
# ---------------------------------------------------------------------------------------------------------------------
# Rows: (shape, direction, plan form the launch must take, whether its reduction is split).  The form is asserted
# through gz_conv2d_plan before the launch, so a threshold edit cannot quietly move a case off the kernel it was chosen
# for.  Found by enumerating N, C, H, K over the four geometries and keeping the cheapest shape per (form, split / unsplit);
# the last blocks are the full-chip direct kernels, the ragged companions of the igemm2 families (a partly empty last
# pixel tile, 72 channels, 96 / 132 / 160 columns) and the wave_groups=2 launches.
_CONV_TABLE = [
    ((16, 3, 64, 16, 3, 1, 1), 'Dg', 'Dg direct conv3x3_smallch<mfma16x16x4>', False),
    ((1, 3, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=1>', False),
    ((1, 3, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=4>', False),
    ((1, 3, 8, 40, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=8>', False),
    ((1, 4, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=1>', False),
    ((1, 4, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=4>', False),
    ((1, 4, 8, 40, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=8>', False),
    ((1, 3, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=4>', False),
    ((1, 3, 8, 40, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=8>', False),
    ((1, 4, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=4,KS=4>', False),
    ((1, 4, 8, 40, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=4,KS=8>', False),
    ((1, 3, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=3>', False),
    ((1, 4, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=4>', False),
    ((1, 512, 4, 1024, 5, 2, 2), 'Dg', 'Dg igemm2<256x64> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', True),
    ((32, 72, 64, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x128> ConvDgALoader splits= bn_stats_rows=', False),
    ((32, 72, 64, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((1, 3, 4, 256, 1, 1, 0), 'Dg', 'Dg igemm<128x32> ConvDgALoader splits= bn_stats_rows=', True),
    ((1, 3, 4, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x32> ConvDgALoader splits= bn_stats_rows=', False),
    ((1, 16, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x32> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((1, 16, 8, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x32> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((1, 3, 4, 40, 5, 2, 2), 'Dg', 'Dg igemm<128x32> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((1, 3, 4, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x32> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((1, 64, 4, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoader splits= bn_stats_rows=', True),
    ((1, 64, 4, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x64> ConvDgALoader splits= bn_stats_rows=', False),
    ((1, 64, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((1, 64, 8, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((1, 64, 4, 40, 5, 2, 2), 'Dg', 'Dg igemm<128x64> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((1, 64, 4, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x64> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((2, 64, 8, 256, 1, 1, 0), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', True),
    ((2, 64, 8, 3, 1, 1, 0), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', False),
    ((2, 64, 16, 64, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((2, 64, 16, 3, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((2, 64, 8, 40, 3, 1, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((2, 64, 8, 16, 3, 1, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((16, 16, 64, 3, 3, 1, 1), 'F', 'F direct conv3x3_fewk<fma>', False),
    ((64, 16, 32, 3, 3, 1, 1), 'F', 'F direct conv3x3_smallch<mfma16x16x4>', False),
    ((8, 16, 64, 132, 1, 1, 0), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', False),
    ((1, 1024, 4, 1024, 5, 2, 2), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', True),
    ((1, 256, 4, 1024, 5, 2, 2), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', True),
    ((1, 256, 4, 132, 1, 1, 0), 'F', 'F igemm<128x128> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((1, 3, 4, 132, 1, 1, 0), 'F', 'F igemm<128x128> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((1, 16, 4, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((1, 3, 4, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((1, 16, 4, 132, 5, 2, 2), 'F', 'F igemm<128x128> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((1, 16, 4, 132, 3, 1, 1), 'F', 'F igemm<128x128> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((1, 256, 4, 3, 1, 1, 0), 'F', 'F igemm<128x32> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((1, 3, 4, 3, 1, 1, 0), 'F', 'F igemm<128x32> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((1, 16, 4, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((1, 3, 4, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((1, 16, 32, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((1, 3, 32, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((1, 16, 4, 3, 5, 2, 2), 'F', 'F igemm<128x32> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((1, 16, 4, 3, 3, 1, 1), 'F', 'F igemm<128x32> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((1, 256, 4, 40, 1, 1, 0), 'F', 'F igemm<128x64> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((1, 3, 4, 40, 1, 1, 0), 'F', 'F igemm<128x64> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((1, 16, 4, 40, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((1, 3, 4, 40, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((1, 16, 4, 40, 5, 2, 2), 'F', 'F igemm<128x64> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((1, 16, 4, 40, 3, 1, 1), 'F', 'F igemm<128x64> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((2, 256, 8, 40, 1, 1, 0), 'F', 'F igemm<64x64> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((2, 3, 8, 40, 1, 1, 0), 'F', 'F igemm<64x64> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((2, 16, 16, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((2, 3, 16, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((1, 16, 32, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((1, 3, 32, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((2, 20, 8, 40, 3, 1, 1), 'F', 'F igemm<64x64> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((2, 16, 8, 40, 3, 1, 1), 'F', 'F igemm<64x64> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((16, 3, 64, 3, 3, 1, 1), 'Wg', 'Wg direct wgrad_k3_fewk<fma> slabs=', True),
    ((16, 3, 64, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=1> slabs=', True),
    ((16, 3, 64, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=4> slabs=', True),
    ((16, 4, 64, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=1> slabs=', True),
    ((16, 4, 64, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=4> slabs=', True),
    ((64, 3, 32, 3, 3, 1, 1), 'Wg', 'Wg direct wgrad_smallch_k3<mfma16x16x4> slabs=', True),
    ((1, 512, 8, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', False),
    ((1, 1024, 4, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', False),
    ((2, 72, 64, 96, 1, 1, 0), 'Wg', 'Wg igemm<128x128> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((1, 3, 16, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((1, 3, 4, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((64, 3, 4, 96, 4, 2, 1), 'Wg', 'Wg igemm<128x64> WgALoader+WgBLoader slabs=', True),
    ((1, 3, 4, 96, 4, 2, 1), 'Wg', 'Wg igemm<128x64> WgALoader+WgBLoader slabs=', False),
    ((1, 4, 16, 96, 3, 1, 1), 'Wg', 'Wg igemm<128x64> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((1, 4, 4, 96, 3, 1, 1), 'Wg', 'Wg igemm<128x64> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((64, 3, 4, 3, 4, 2, 1), 'Wg', 'Wg igemm<64x64> WgALoader+WgBLoader slabs=', True),
    ((1, 3, 4, 3, 4, 2, 1), 'Wg', 'Wg igemm<64x64> WgALoader+WgBLoader slabs=', False),
    ((1, 4, 16, 3, 3, 1, 1), 'Wg', 'Wg igemm<64x64> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((1, 4, 4, 3, 3, 1, 1), 'Wg', 'Wg igemm<64x64> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((256, 3, 64, 64, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=4>', False),
    ((256, 3, 64, 64, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=4>', False),
    ((32, 3, 64, 1024, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=8>', False),
    ((2, 1024, 64, 256, 5, 2, 2), 'Dg', 'Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, aligned tensors; else the gather loader)', False),
    ((1, 512, 64, 1024, 5, 2, 2), 'Dg', 'Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, aligned tensors; else the gather loader)', True),
    ((2, 1024, 64, 64, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((2, 1024, 64, 128, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', False),
    ((2, 1024, 64, 128, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', True),
    ((2, 1024, 64, 128, 1, 1, 0), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', False),
    ((1, 1024, 64, 64, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((3, 256, 64, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', True),
    ((1, 1024, 64, 128, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', False),
    ((1, 512, 64, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', True),
    ((64, 64, 64, 64, 4, 2, 1), 'Dg', 'Dg igemm2<512x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((2, 1024, 64, 64, 3, 1, 1), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows= wave_groups=2', False),
    ((32, 16, 64, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', False),
    ((3, 512, 64, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', True),
    ((2, 512, 64, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', True),
    ((32, 64, 64, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', False),
    ((8, 64, 64, 132, 3, 1, 1), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', False),
    ((1, 128, 64, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', True),
    ((4, 64, 64, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', False),
    ((4, 16, 64, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', False),
    ((3, 20, 64, 1024, 5, 2, 2), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', False),
    ((64, 3, 64, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((512, 3, 64, 64, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((512, 3, 64, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=4> slabs=', True),
    ((16, 72, 64, 128, 5, 2, 2), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', True),
    ((1, 512, 32, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', False),
    ((1, 256, 64, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', True),
    ((1, 512, 16, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', False),
    ((1, 1024, 16, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', False),
    ((3, 72, 64, 512, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', True),
    ((1, 1024, 8, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', False),
    ((131, 132, 16, 72, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((50, 132, 24, 72, 3, 1, 1), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows= wave_groups=2', False),
    ((131, 132, 16, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', True),
    ((50, 72, 24, 132, 3, 1, 1), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', False),
    ((131, 132, 16, 160, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', True),
    ((131, 72, 16, 160, 5, 2, 2), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', True),
    ((128, 64, 32, 128, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', False),
    ((128, 64, 32, 128, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    # forms that only the odd shapes of the existing case tables reach: 1- and 2-channel images, feature rows that
    # are no multiple of 4 (the generic weight-gradient loaders), the 256x256 tile
    ((3, 1, 8, 6, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=1>', False),
    ((512, 1, 64, 193, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=4>', False),
    ((2, 2, 16, 9, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=1>', False),
    ((512, 2, 64, 65, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=4>', False),
    ((33, 2, 64, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=8>', False),
    ((33, 2, 64, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=2> slabs=', True),
    ((2, 1, 32, 24, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=1,KS=4>', False),
    ((5, 2, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=2,KS=4>', False),
    ((128, 384, 16, 72, 4, 2, 1), 'Dg', 'Dg igemm2<256x256> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((16, 1, 64, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=1> slabs=', True),
    ((24, 4, 64, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=2> slabs=', True),
    ((16, 72, 24, 72, 1, 1, 0), 'Wg', 'Wg igemm<128x128> WgALoader+WgBLoader slabs=', True),
    ((3, 6, 12, 10, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoader+WgBLoader slabs=', True),
    ((1, 4, 12, 7, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoader+WgBLoader slabs=', False),
    ((1, 132, 12, 40, 5, 2, 2), 'Dg', 'Dg igemm<128x128> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((3, 512, 32, 1024, 1, 1, 0), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', False),
    ((3, 1024, 32, 512, 1, 1, 0), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', True),
    # the other launch (split / unsplit) of forms above and the remaining forms the enumeration of enumerate_plans()
    # reaches; the last three: ConvDg5A2 with a partly empty last pixel tile (2368 pixels per phase) and 1056 columns
    ((1, 1, 8, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=8>', False),
    ((1, 1, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=1,KS=8>', False),
    ((1, 2, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=2,KS=8>', False),
    ((1, 1, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=1>', False),
    ((1, 2, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=2>', False),
    ((131, 132, 8, 512, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', True),
    ((2, 132, 64, 512, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', True),
    ((131, 132, 16, 160, 5, 2, 2), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', True),
    ((50, 132, 12, 512, 3, 1, 1), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows= wave_groups=2', True),
    ((131, 384, 12, 40, 5, 2, 2), 'Dg', 'Dg igemm2<256x64> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', False),
    ((1, 132, 4, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoader splits= bn_stats_rows=', True),
    ((1, 132, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((1, 132, 4, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x128> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((131, 512, 8, 132, 3, 1, 1), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', True),
    ((131, 64, 8, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', True),
    ((8, 1024, 64, 72, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((16, 1, 64, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=2> slabs=', True),
    ((16, 1, 64, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=4> slabs=', True),
    ((16, 2, 64, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=1> slabs=', True),
    ((16, 2, 64, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=4> slabs=', True),
    ((16, 3, 64, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=2> slabs=', True),
    ((64, 1024, 8, 160, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', True),
    ((512, 72, 8, 160, 5, 2, 2), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', True),
    ((64, 256, 8, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', True),
    ((16, 256, 16, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', True),
    ((512, 16, 8, 1024, 5, 2, 2), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', True),
    ((256, 16, 8, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', True),
    ((37, 256, 16, 1024, 5, 2, 2), 'Dg', 'Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, aligned tensors; else the gather loader)', True),
    ((37, 1024, 16, 256, 5, 2, 2), 'Dg', 'Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, aligned tensors; else the gather loader)', False),
    ((2, 1056, 64, 256, 5, 2, 2), 'Dg', 'Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, aligned tensors; else the gather loader)', False),
    # launch_igemm2 with more than 16 slabs (22: the eight-wavefront finish pass), one wave group, equal phases -- the one
    # path of launch_paths() that only the wave_groups=2 and the per-phase launches above reached
    ((33, 512, 8, 256, 5, 2, 2), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', True),
    # a square with 12-pixel rows per phase (H = 24): no tile of 64 or 128 pixels holds whole rows, so the k4 s2 p1 input
    # gradient stays off ConvDgALoaderRow4 (found by the rectangular table below)
    ((3, 64, 24, 3, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', False),
]
CONV_ROWS = [(ConvCase(*sh), op, form, split) for sh, op, form, split in _CONV_TABLE]


def row_id(row):
    return "%s-%s" % (row[1], case_id(row[0]))


# conv3d (ConvTranspose3d k3 s2 p1 op1; the Conv3d view): (N, C image side, D image side, K feature side)
Conv3Case = namedtuple("Conv3Case", "N C D K")
# test_conv3d_family's shapes, (N, Cin, D, Cout) of conv_transpose3d(x [N, Cin, D^3], w [Cin, Cout, 3, 3, 3]), in the
# Conv3d view (N, C = Cout, D image side = 2 D, K = Cin)
# (case, direction, plan form the launch must take): all three directions at every shape; each row asserts its form
# through gz_conv3d_plan, so a threshold edit cannot move it off its kernel unnoticed
_CONV3_TABLE = [
    ((2, 4, 8, 8), 'F', 'F igemm<128x32> Conv3DFwdALoader splits= slabs='),
    ((2, 4, 8, 8), 'Dg', 'Dg igemm<128x32> Conv3DDgALoader splits= slabs='),
    ((2, 4, 8, 8), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
    ((3, 12, 8, 20), 'F', 'F igemm<128x32> Conv3DFwdALoader splits= slabs='),
    ((3, 12, 8, 20), 'Dg', 'Dg igemm<128x32> Conv3DDgALoader splits= slabs='),
    ((3, 12, 8, 20), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
    ((4, 16, 16, 64), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((4, 16, 16, 64), 'Dg', 'Dg igemm<128x32> Conv3DDgALoader splits= slabs='),
    ((4, 16, 16, 64), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
    ((2, 130, 8, 128), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 130, 8, 128), 'Dg', 'Dg igemm<64x64> Conv3DDgALoader splits= slabs='),
    ((2, 130, 8, 128), 'Wg', 'Wg igemm2r<128x256> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((8, 128, 8, 512), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((8, 128, 8, 512), 'Dg', 'Dg igemm2<256x128> Conv3DDgTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((8, 128, 8, 512), 'Wg', 'Wg igemm2r<256x128> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((8, 64, 16, 128), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((8, 64, 16, 128), 'Dg', 'Dg igemm<128x64> Conv3DDgALoader splits= slabs='),
    ((8, 64, 16, 128), 'Wg', 'Wg igemm2r<128x256> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((3, 64, 8, 64), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((3, 64, 8, 64), 'Dg', 'Dg igemm<64x64> Conv3DDgALoader splits= slabs='),
    ((3, 64, 8, 64), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
    ((2, 192, 8, 192), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 192, 8, 192), 'Dg', 'Dg igemm<64x64> Conv3DDgALoader splits= slabs='),
    ((2, 192, 8, 192), 'Wg', 'Wg igemm2r<128x256> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((5, 64, 16, 72), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((5, 64, 16, 72), 'Dg', 'Dg igemm<64x64> Conv3DDgALoader splits= slabs='),
    ((5, 64, 16, 72), 'Wg', 'Wg igemm<128x128> WgALoader+Wg3DBLoader splits= slabs='),
    ((5, 128, 8, 72), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((5, 128, 8, 72), 'Dg', 'Dg igemm2<256x128> Conv3DDgTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((5, 128, 8, 72), 'Wg', 'Wg igemm<128x128> WgALoader+Wg3DBLoader splits= slabs='),
    ((2, 20, 6, 24), 'F', 'F igemm<128x32> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 20, 6, 24), 'Dg', 'Dg igemm<128x32> Conv3DDgALoader splits= slabs='),
    ((2, 20, 6, 24), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
    ((64, 128, 8, 512), 'F', 'F igemm2<256x128> Conv3DTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((64, 128, 8, 512), 'Dg', 'Dg igemm2<256x128> Conv3DDgTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((64, 128, 8, 512), 'Wg', 'Wg igemm2r<256x128> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((24, 72, 10, 512), 'F', 'F igemm2<256x64> Conv3DTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((24, 72, 10, 512), 'Dg', 'Dg igemm<128x64> Conv3DDgALoader splits= slabs='),
    ((24, 72, 10, 512), 'Wg', 'Wg igemm2r<256x128> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
]
CONV3_ROWS = [(Conv3Case(*c), op, form) for c, op, form in _CONV3_TABLE]


# The same on a box: image side [N, C, D, H, W] (even sides), feature side [N, K, D/2, H/2, W/2].
Box3Case = namedtuple("Box3Case", "N C D H W K")


def conv3_case(key):
    return Box3Case(*key) if len(key) == 6 else Conv3Case(*key)


def box_sides(c):
    return (c.D, c.H, c.W) if len(c) == 6 else (c.D, c.D, c.D)


def row3_id(row):
    if len(row[0]) == 6:
        return "%s-N%d_C%d_D%dxH%dxW%d_K%d" % ((row[1],) + tuple(row[0]))
    return "%s-N%d_C%d_D%d_K%d" % ((row[1],) + tuple(row[0]))


def box_pixels(c):
    D, H, W = box_sides(c)
    return (D // 2) * (H // 2) * (W // 2)


def row3_macs(c):
    return c.N * box_pixels(c) * c.C * c.K * 27


def conv3_terms(c, op):
    return {"F": c.C * 27, "Dg": c.K * 8, "Wg": c.N * box_pixels(c)}[op]


def conv3_operands(c, op):
    D, H, W = box_sides(c)
    xs, ws, gs = (c.N, c.C, D, H, W), (c.K, c.C, 3, 3, 3), (c.N, c.K, D // 2, H // 2, W // 2)
    shapes = {"F": (xs, ws), "Dg": (gs, ws), "Wg": (xs, gs)}[op]
    seed = 3000 + OPS.index(op) + c.N + c.C + c.K + (3 * D + 5 * H + 7 * W if len(c) == 6 else 0)
    return pair(shapes[0], shapes[1], conv3_terms(c, op), seed)


def conv3_apply(c, op, a, b, bias=None):
    if op == "F":
        return TF.conv3d(a, b, bias, 2, 1)
    if op == "Dg":
        return TF.conv_transpose3d(a, b, bias, 2, 1, output_padding=1)
    return torch.nn.grad.conv3d_weight(a, (c.K, c.C, 3, 3, 3), b, stride=2, padding=1)


@functools.lru_cache(maxsize=4)
def conv3_reference(key, op):
    c = conv3_case(key)
    set_threads()
    a, b = conv3_operands(c, op)
    assert_exact_precondition(conv3_apply(c, op, a.double().abs(), b.double().abs()), "3d %s %s" % (key, op))
    return a, b, conv3_apply(c, op, a.double(), b.double())


# ---------------------------------------------------------------------------------------------------------------------
# rectangular maps and box volumes: one row per (form, split) key that enumerate_rect_plans() reaches -- all 162 keys of
# _CONV_TABLE and 8 that no square of it reaches -- as printed by tools/find_exact_cases.py --rect.  A row is the cheapest
# mid-tile shape of its key (N > 1, the feature map neither a divisor nor a multiple of the tile's pixel count), or the
# cheapest rectangle where the key has none ("no mid-tile").  RECT_MID_KEYS of the RECT_KEYS keys have a mid-tile row.
# The orientation alternates down the table; every loader family has a tall (H > W) and a wide row per direction, for
# which ConvFwdALoaderRow4 needs a second row (its tall maps, 16- or 32-pixel rows and >= 24 of them, are whole tiles).
# "sq": a square row of the same key is cheaper than this rectangle, which is over 3e9 multiply-adds.
# ---------------------------------------------------------------------------------------------------------------------
RECT_KEYS, RECT_MID_KEYS = 170, 163
_DG5A2 = ('Dg igemm2<256x(4 phases x 32)> ConvDg5A2(row-shared, LDS-DMA 16B, 12 k-steps) slabs= (no bias / activation, '
          'aligned tensors; else the gather loader)')
_RECT_TABLE = [
    ((128, 1, 6, 96, 16, 3, 1, 1), 'Dg', 'Dg direct conv3x3_smallch<mfma16x16x4>', False),
    ((2, 1, 6, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=1>', False),
    ((2, 1, 10, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=4>', False),
    ((2, 1, 6, 8, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=1,KS=8>', False),
    ((2, 2, 10, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=1>', False),
    ((2, 2, 6, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=4>', False),
    ((2, 2, 10, 8, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=2,KS=8>', False),
    ((2, 3, 6, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=1>', False),
    ((2, 3, 10, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=4>', False),
    ((2, 3, 6, 8, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=3,KS=8>', False),
    ((2, 4, 10, 8, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=1>', False),
    ((2, 4, 6, 8, 16, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=4>', False),
    ((2, 4, 10, 8, 32, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc4_k4s2p1<C=4,KS=8>', False),
    ((512, 1, 96, 64, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=1,KS=1>', False),        # no mid-tile
    ((2, 1, 10, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=1,KS=4>', False),
    ((2, 1, 6, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=1,KS=8>', False),
    ((512, 2, 96, 64, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=2,KS=1>', False),        # no mid-tile
    ((2, 2, 6, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=2,KS=4>', False),
    ((2, 2, 10, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=2,KS=8>', False),
    ((512, 3, 96, 64, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=1>', False),        # no mid-tile
    ((2, 3, 10, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=4>', False),
    ((2, 3, 6, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=3,KS=8>', False),
    ((512, 4, 96, 64, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=4,KS=1>', False),        # no mid-tile
    ((2, 4, 6, 8, 16, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=4,KS=4>', False),
    ((2, 4, 10, 8, 32, 5, 2, 2), 'Dg', 'Dg direct dgrad_smallc4_k5s2p2<C=4,KS=8>', False),
    ((2, 1, 4, 6, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=1>', False),
    ((2, 2, 6, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=2>', False),
    ((2, 3, 4, 6, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=3>', False),
    ((2, 4, 6, 4, 3, 4, 2, 1), 'Dg', 'Dg direct dgrad_smallc_k4s2p1<C=4>', False),
    ((50, 384, 12, 64, 128, 5, 2, 2), 'Dg', _DG5A2, False),
    ((3, 1024, 24, 16, 1024, 5, 2, 2), 'Dg', _DG5A2, True),
    ((50, 132, 10, 64, 64, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((50, 132, 24, 16, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', True),
    ((50, 132, 10, 64, 128, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', False),
    ((50, 132, 10, 32, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x128> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', True),
    ((50, 132, 6, 96, 128, 1, 1, 0), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', False),
    ((50, 132, 32, 24, 132, 5, 2, 2), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', True),
    ((50, 132, 6, 96, 64, 3, 1, 1), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows= wave_groups=2', False),
    ((50, 132, 24, 12, 256, 3, 1, 1), 'Dg', 'Dg igemm2<256x128> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows= wave_groups=2', True),
    ((50, 384, 10, 64, 64, 4, 2, 1), 'Dg', 'Dg igemm2<256x256> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((50, 1024, 10, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),
    ((128, 384, 6, 8, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', True),
    ((50, 1024, 10, 8, 128, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', False),
    ((3, 1024, 6, 64, 256, 4, 2, 1), 'Dg', 'Dg igemm2<256x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows= wave_groups=2', True),
    ((3, 1024, 96, 24, 40, 5, 2, 2), 'Dg', 'Dg igemm2<256x64> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', False),
    ((2, 384, 4, 6, 1024, 5, 2, 2), 'Dg', 'Dg igemm2<256x64> ConvDgTapA2(gather, LDS-DMA 4B) splits= bn_stats_rows=', True),
    ((512, 64, 48, 16, 64, 4, 2, 1), 'Dg', 'Dg igemm2<512x64> ConvDgA2(row-shared, LDS-DMA 16B) splits= bn_stats_rows=', False),        # 6.4e9; sq 4.3e9
    ((2, 132, 4, 6, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x128> ConvDgALoader splits= bn_stats_rows=', False),
    ((2, 132, 6, 4, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoader splits= bn_stats_rows=', True),
    ((2, 132, 6, 8, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((2, 132, 10, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x128> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((2, 132, 4, 6, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x128> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((2, 132, 6, 4, 32, 5, 2, 2), 'Dg', 'Dg igemm<128x128> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((2, 1, 4, 6, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x32> ConvDgALoader splits= bn_stats_rows=', False),
    ((2, 1, 6, 4, 256, 1, 1, 0), 'Dg', 'Dg igemm<128x32> ConvDgALoader splits= bn_stats_rows=', True),
    ((2, 6, 6, 8, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x32> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((2, 6, 10, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x32> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((2, 1, 4, 6, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x32> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((2, 1, 6, 4, 32, 5, 2, 2), 'Dg', 'Dg igemm<128x32> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((2, 64, 4, 6, 3, 1, 1, 0), 'Dg', 'Dg igemm<128x64> ConvDgALoader splits= bn_stats_rows=', False),
    ((2, 64, 6, 4, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoader splits= bn_stats_rows=', True),
    ((2, 64, 6, 8, 3, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((2, 64, 10, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<128x64> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((2, 64, 4, 6, 16, 5, 2, 2), 'Dg', 'Dg igemm<128x64> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((2, 64, 6, 4, 32, 5, 2, 2), 'Dg', 'Dg igemm<128x64> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((3, 64, 4, 6, 3, 1, 1, 0), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', False),
    ((3, 64, 6, 4, 256, 1, 1, 0), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', True),
    ((3, 64, 6, 16, 3, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderRow4 splits= bn_stats_rows=', False),
    ((3, 64, 12, 8, 64, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderRow4 splits= bn_stats_rows=', True),
    ((3, 64, 4, 6, 16, 3, 1, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderTap splits= bn_stats_rows=', False),
    ((3, 64, 6, 4, 32, 3, 1, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoaderTap splits= bn_stats_rows=', True),
    ((16, 16, 96, 64, 3, 3, 1, 1), 'F', 'F direct conv3x3_fewk<fma>', False),        # no mid-tile
    ((128, 16, 6, 96, 3, 3, 1, 1), 'F', 'F direct conv3x3_smallch<mfma16x16x4>', False),
    ((512, 16, 10, 32, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', False),
    ((128, 384, 12, 8, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', True),
    ((50, 64, 10, 64, 1024, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', False),        # 8.4e9; sq 4.4e9
    ((50, 512, 10, 16, 132, 4, 2, 1), 'F', 'F igemm2<256x128> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', True),
    ((50, 16, 6, 96, 132, 1, 1, 0), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', False),
    ((50, 1024, 12, 6, 132, 3, 1, 1), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', True),
    ((50, 64, 6, 96, 132, 3, 1, 1), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', False),
    ((2, 1024, 6, 4, 1024, 5, 2, 2), 'F', 'F igemm2<256x128> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', True),
    ((50, 16, 10, 32, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', False),
    ((3, 132, 48, 32, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows=', True),
    ((50, 64, 10, 32, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', False),
    ((3, 384, 24, 16, 1024, 4, 2, 1), 'F', 'F igemm2<256x64> ConvFwdA2(raw rows, LDS-DMA 16B) slabs= bn_stats_rows= wave_groups=2', True),
    ((3, 512, 10, 96, 1024, 1, 1, 0), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', False),
    ((3, 1024, 48, 10, 1024, 1, 1, 0), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows=', True),
    ((3, 64, 10, 96, 1024, 3, 1, 1), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', False),
    ((2, 384, 6, 4, 1024, 5, 2, 2), 'F', 'F igemm2<256x64> ConvTapA2(gather, LDS-DMA 4B) slabs= bn_stats_rows= wave_groups=2', True),
    ((2, 1, 4, 6, 132, 1, 1, 0), 'F', 'F igemm<128x128> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((2, 384, 6, 4, 132, 1, 1, 0), 'F', 'F igemm<128x128> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((2, 1, 4, 6, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((3, 1, 6, 32, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((3, 16, 6, 32, 132, 4, 2, 1), 'F', 'F igemm<128x128> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((2, 16, 4, 6, 132, 3, 1, 1), 'F', 'F igemm<128x128> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 132, 5, 2, 2), 'F', 'F igemm<128x128> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((2, 1, 4, 6, 3, 1, 1, 0), 'F', 'F igemm<128x32> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((2, 384, 6, 4, 3, 1, 1, 0), 'F', 'F igemm<128x32> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((2, 1, 4, 6, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((2, 1, 6, 32, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((2, 16, 6, 32, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((2, 16, 4, 6, 3, 3, 1, 1), 'F', 'F igemm<128x32> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 3, 5, 2, 2), 'F', 'F igemm<128x32> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((2, 1, 4, 6, 40, 1, 1, 0), 'F', 'F igemm<128x64> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((2, 384, 6, 4, 40, 1, 1, 0), 'F', 'F igemm<128x64> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((2, 1, 4, 6, 40, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 40, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((512, 1, 10, 64, 65, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((1, 16, 4, 32, 40, 4, 2, 1), 'F', 'F igemm<128x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),        # no mid-tile
    ((2, 16, 4, 6, 40, 3, 1, 1), 'F', 'F igemm<128x64> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((2, 16, 6, 4, 40, 5, 2, 2), 'F', 'F igemm<128x64> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((3, 1, 4, 6, 40, 1, 1, 0), 'F', 'F igemm<64x64> ConvFwdALoader slabs= bn_stats_rows=', False),
    ((3, 384, 6, 4, 40, 1, 1, 0), 'F', 'F igemm<64x64> ConvFwdALoader slabs= bn_stats_rows=', True),
    ((3, 1, 4, 24, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', False),
    ((3, 16, 12, 8, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderK4V slabs= bn_stats_rows=', True),
    ((2, 1, 6, 32, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    ((2, 16, 6, 32, 40, 4, 2, 1), 'F', 'F igemm<64x64> ConvFwdALoaderRow4 slabs= bn_stats_rows=', True),
    ((3, 16, 4, 6, 40, 3, 1, 1), 'F', 'F igemm<64x64> ConvFwdALoaderTap slabs= bn_stats_rows=', False),
    ((3, 16, 12, 8, 40, 5, 2, 2), 'F', 'F igemm<64x64> ConvFwdALoaderTap slabs= bn_stats_rows=', True),
    ((128, 1, 8, 64, 3, 3, 1, 1), 'Wg', 'Wg direct wgrad_k3_fewk<fma> slabs=', True),        # no mid-tile
    ((50, 1, 48, 32, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=1> slabs=', True),
    ((128, 1, 6, 96, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=2> slabs=', True),
    ((50, 1, 48, 32, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=1,KT=4> slabs=', True),
    ((128, 2, 6, 96, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=1> slabs=', True),
    ((50, 2, 48, 32, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=2> slabs=', True),
    ((128, 2, 6, 96, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=2,KT=4> slabs=', True),
    ((50, 3, 48, 32, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=1> slabs=', True),
    ((128, 3, 6, 96, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=2> slabs=', True),
    ((50, 3, 48, 32, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=3,KT=4> slabs=', True),
    ((128, 4, 6, 96, 16, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=1> slabs=', True),
    ((50, 4, 48, 32, 32, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=2> slabs=', True),
    ((128, 4, 6, 96, 64, 4, 2, 1), 'Wg', 'Wg direct wgrad_k4s2p1_fewc<mfma16x16x4,C=4,KT=4> slabs=', True),
    ((128, 1, 6, 96, 3, 3, 1, 1), 'Wg', 'Wg direct wgrad_smallch_k3<mfma16x16x4> slabs=', True),
    # igemm2r on 2-D maps: feature rows of 2 pixels (W = 4, OH a multiple of 8), so tall maps only
    ((128, 384, 96, 4, 128, 4, 2, 1), 'Wg', 'Wg igemm2r<128x256> WgALoaderRow+WgBLoaderRow(register-staged) slabs=', True),
    ((2, 512, 48, 4, 1024, 4, 2, 1), 'Wg', 'Wg igemm2r<256x128> WgALoaderRow+WgBLoaderRow(register-staged) slabs=', False),
    ((128, 384, 48, 4, 256, 4, 2, 1), 'Wg', 'Wg igemm2r<256x128> WgALoaderRow+WgBLoaderRow(register-staged) slabs=', True),
    ((16, 384, 48, 32, 128, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', True),        # 4.8e9; sq 4.3e9
    ((128, 384, 24, 8, 128, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', True),        # 4.8e9; sq 2.7e9
    ((16, 384, 96, 16, 128, 4, 2, 1), 'Wg', 'Wg igemm2w<128x256> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', True),        # 4.8e9; sq 2.8e9
    ((50, 64, 10, 96, 128, 3, 1, 1), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', True),
    ((512, 64, 24, 4, 128, 3, 1, 1), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', True),        # 3.6e9; sq 2.4e9
    ((512, 64, 12, 16, 128, 5, 2, 2), 'Wg', 'Wg igemm2w<128x256> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', True),        # 5.0e9; sq 2.4e9
    ((2, 512, 6, 32, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', False),
    ((16, 512, 6, 96, 256, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=16>(both operands LDS-DMA) slabs=', True),        # 4.8e9; sq 4.3e9
    ((2, 512, 24, 8, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', False),
    ((16, 384, 96, 8, 256, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=4>(both operands LDS-DMA) slabs=', True),        # 4.8e9; sq 4.3e9
    ((2, 512, 24, 16, 1024, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', False),
    ((50, 512, 12, 16, 256, 4, 2, 1), 'Wg', 'Wg igemm2w<256x128> WgImgB2<CW=8>(both operands LDS-DMA) slabs=', True),        # 5.0e9; sq 4.3e9
    ((2, 384, 6, 32, 1024, 5, 2, 2), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', False),
    ((128, 16, 6, 96, 256, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=16>(both operands LDS-DMA) slabs=', True),
    ((2, 1024, 12, 4, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', False),
    ((50, 16, 96, 4, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=4>(both operands LDS-DMA) slabs=', True),
    ((2, 1024, 10, 8, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', False),
    ((512, 16, 6, 8, 1024, 3, 1, 1), 'Wg', 'Wg igemm2w<256x128> WgImgBG<CW=8>(both operands LDS-DMA) slabs=', True),        # 3.6e9; sq 2.4e9
    ((128, 72, 12, 6, 65, 1, 1, 0), 'Wg', 'Wg igemm<128x128> WgALoader+WgBLoader slabs=', True),
    ((16, 72, 6, 96, 65, 1, 1, 0), 'Wg', 'Wg igemm<128x128> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((2, 1, 6, 4, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoader+WgBLoader slabs=', False),
    ((3, 1, 4, 24, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoader+WgBLoader slabs=', True),
    ((2, 1, 12, 4, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((3, 1, 6, 16, 3, 1, 1, 0), 'Wg', 'Wg igemm<128x32> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((2, 3, 6, 4, 65, 4, 2, 1), 'Wg', 'Wg igemm<128x64> WgALoader+WgBLoader slabs=', False),
    ((3, 4, 4, 24, 65, 3, 1, 1), 'Wg', 'Wg igemm<128x64> WgALoader+WgBLoader slabs=', True),
    ((2, 4, 12, 4, 65, 3, 1, 1), 'Wg', 'Wg igemm<128x64> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((3, 4, 6, 16, 65, 3, 1, 1), 'Wg', 'Wg igemm<128x64> WgALoaderRow+WgBLoaderRow slabs=', True),
    ((2, 3, 6, 4, 3, 4, 2, 1), 'Wg', 'Wg igemm<64x64> WgALoader+WgBLoader slabs=', False),
    ((3, 4, 4, 24, 3, 3, 1, 1), 'Wg', 'Wg igemm<64x64> WgALoader+WgBLoader slabs=', True),
    ((2, 4, 12, 4, 3, 3, 1, 1), 'Wg', 'Wg igemm<64x64> WgALoaderRow+WgBLoaderRow slabs=', False),
    ((3, 4, 6, 16, 3, 3, 1, 1), 'Wg', 'Wg igemm<64x64> WgALoaderRow+WgBLoaderRow slabs=', True),
    # second row of its key: ConvFwdALoaderRow4 on a tall map (whole tiles: no mid-tile shape exists)
    ((1, 1, 48, 32, 3, 4, 2, 1), 'F', 'F igemm<128x32> ConvFwdALoaderRow4 slabs= bn_stats_rows=', False),
    # second row of its key: 12-pixel rows of the per-phase grid, which ConvDgALoaderRow4 took until this table found that a
    # tile starting inside such a row (64 % 12 != 0) reads its first pixel's left neighbour from outside the tile
    ((3, 64, 4, 24, 3, 4, 2, 1), 'Dg', 'Dg igemm<64x64> ConvDgALoader splits= bn_stats_rows=', False),
]
RECT_ROWS = [(RectCase(*sh), op, form, split) for sh, op, form, split in _RECT_TABLE]
# keys of _CONV_TABLE that no rectangle of the enumeration reaches (tests/test_exact_cases.py asserts that it does not)
RECT_UNREACHED = []

# conv3d on boxes that are no cubes: one row per form enumerate_box_plans() reaches (tools/find_exact_cases.py --box) -- the
# 13 forms of _CONV3_TABLE and 7 that no cube of it reaches (F igemm<128x128 | 128x64 | 64x64> Conv3DFwdALoader, F igemm
# <128x64 | 128x128> Conv3DFwdALoaderTap, Dg igemm<128x128> Conv3DDgALoader, Wg igemm<128x32>).  D, H, W are pairwise
# different in every row, and every row is mid-tile (BOX3_MID_FORMS of BOX3_FORMS).
BOX3_FORMS, BOX3_MID_FORMS = 20, 20
_BOX3_TABLE = [
    ((2, 128, 4, 6, 8, 20), 'Dg', 'Dg igemm2<256x128> Conv3DDgTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((24, 130, 6, 10, 12, 8), 'Dg', 'Dg igemm<128x128> Conv3DDgALoader splits= slabs='),
    ((2, 1, 4, 6, 8, 8), 'Dg', 'Dg igemm<128x32> Conv3DDgALoader splits= slabs='),
    ((24, 72, 6, 10, 12, 8), 'Dg', 'Dg igemm<128x64> Conv3DDgALoader splits= slabs='),
    ((2, 64, 4, 6, 8, 8), 'Dg', 'Dg igemm<64x64> Conv3DDgALoader splits= slabs='),
    ((64, 16, 6, 10, 32, 512), 'F', 'F igemm2<256x128> Conv3DTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((64, 16, 4, 10, 24, 512), 'F', 'F igemm2<256x64> Conv3DTapA2(gather, LDS-DMA 4B) splits= slabs='),
    ((64, 1, 6, 24, 32, 72), 'F', 'F igemm<128x128> Conv3DFwdALoader splits= slabs='),
    ((64, 16, 6, 24, 32, 72), 'F', 'F igemm<128x128> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 1, 4, 6, 8, 8), 'F', 'F igemm<128x32> Conv3DFwdALoader splits= slabs='),
    ((2, 16, 4, 6, 8, 8), 'F', 'F igemm<128x32> Conv3DFwdALoaderTap splits= slabs='),
    ((64, 1, 6, 12, 32, 72), 'F', 'F igemm<128x64> Conv3DFwdALoader splits= slabs='),
    ((64, 16, 6, 12, 32, 72), 'F', 'F igemm<128x64> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 1, 4, 6, 8, 64), 'F', 'F igemm<64x64> Conv3DFwdALoader splits= slabs='),
    ((2, 16, 4, 6, 8, 64), 'F', 'F igemm<64x64> Conv3DFwdALoaderTap splits= slabs='),
    ((2, 1, 4, 6, 8, 128), 'Wg', 'Wg igemm2r<128x256> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((2, 1, 4, 6, 8, 512), 'Wg', 'Wg igemm2r<256x128> WgALoader+Wg3DBLoader(register-staged) splits= slabs='),
    ((2, 4, 4, 6, 8, 72), 'Wg', 'Wg igemm<128x128> WgALoader+Wg3DBLoader splits= slabs='),
    ((2, 1, 4, 6, 8, 8), 'Wg', 'Wg igemm<128x32> WgALoader+Wg3DBLoader splits= slabs='),
    ((2, 4, 4, 6, 8, 8), 'Wg', 'Wg igemm<64x64> WgALoader+Wg3DBLoader splits= slabs='),
]
BOX3_ROWS = [(Box3Case(*c), op, form) for c, op, form in _BOX3_TABLE]
BOX3_UNREACHED = []


# ---------------------------------------------------------------------------------------------------------------------
# GEMM: c[M, N] = a[M, K] @ b[K, N] (+ bias): the shapes of test_gemm_all_transposes and test_gemm_split_k
# ---------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [(5, 7, 9), (128, 100, 256), (100, 512, 300), (512, 16384, 100), (33, 1, 64)]
GEMM_SPLIT_CASES = [(64, 128, 8192), (64, 1, 8192), (3, 70, 4100), (200, 130, 2048)]        # (M, N, K)


@functools.lru_cache(maxsize=4)
def gemm_reference(M, N, K):
    set_threads()
    a, b = pair((M, K), (K, N), K, 5000 + M + N + K)
    bias = int_operands((N,), 7, 1.0, 5001 + M)
    assert_exact_precondition(a.double().abs() @ b.double().abs() + bias.double().abs(), "gemm %s" % ((M, N, K),))
    return a, b, bias, a.double() @ b.double()


# ---------------------------------------------------------------------------------------------------------------------
# further conv2d shapes of the GPU module whose plan form is not pinned: test_conv_split_k's, the shapes whose operands
# are moved 4 bytes off alignment, and the shapes of the fused BatchNorm statistics
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_K_CASES = [ConvCase(64, 512, 4, 512, 3, 1, 1), ConvCase(16, 96, 8, 200, 3, 1, 1), ConvCase(64, 256, 8, 512, 5, 2, 2),
                 ConvCase(32, 256, 8, 512, 4, 2, 1), ConvCase(8, 512, 4, 512, 1, 1, 0)]
UNALIGNED_CASES = [ConvCase(64, 16, 32, 256, 4, 2, 1), ConvCase(128, 64, 32, 128, 4, 2, 1)]
EXTRA_ROWS = [(c, op) for c in SPLIT_K_CASES for op in ("F", "Dg")] + [(c, op) for c in UNALIGNED_CASES for op in OPS]
STATS_CASES = [ConvCase(N, C, H, K, 4, 2, 1) for (N, C, H, K) in
               [(2, 3, 16, 5), (4, 8, 16, 16), (3, 20, 8, 40), (8, 64, 16, 128), (16, 32, 32, 96), (64, 16, 32, 256),
                (128, 64, 32, 128), (37, 24, 16, 72)]]


# the same on rectangular maps, each list with a tall, a wide and a mid-tile shape (24, 96, 80, 160, 192 and 384 pixels
# per image, N > 1)
RECT_SPLIT_K_CASES = [RectCase(50, 512, 4, 6, 512, 3, 1, 1), RectCase(16, 96, 12, 8, 200, 3, 1, 1),
                      RectCase(50, 256, 8, 12, 512, 5, 2, 2), RectCase(3, 256, 12, 8, 512, 4, 2, 1),
                      RectCase(3, 512, 6, 4, 512, 1, 1, 0)]
RECT_UNALIGNED_CASES = [RectCase(128, 64, 48, 32, 128, 4, 2, 1), RectCase(50, 16, 10, 32, 1024, 4, 2, 1)]
RECT_EXTRA_ROWS = [(c, op) for c in RECT_SPLIT_K_CASES + RECT_UNALIGNED_CASES for op in OPS]
RECT_STATS_CASES = [RectCase(N, C, H, W, K, 4, 2, 1) for (N, C, H, W, K) in
                    [(3, 3, 24, 16, 5), (4, 8, 16, 24, 16), (3, 20, 12, 8, 40), (8, 64, 24, 16, 128), (16, 32, 48, 32, 96),
                     (50, 16, 48, 32, 256), (50, 128, 10, 64, 64), (50, 128, 48, 16, 64), (37, 24, 12, 16, 72)]]


def extra_id(row):
    return "%s-%s" % (row[1], case_id(row[0]))


@functools.lru_cache(maxsize=2)
def stats_reference(c_key, op):
    """Operands thin enough for the sums of the BatchNorm epilogue: (a, b, y64) with the per-channel sum over ALL pixels
    of y^2 (hence of every partial row, and of |y|) below 2^24 -- thinned until it is."""
    c = conv_case(c_key)
    set_threads()
    (H, W), (OH, OW) = map_sides(c)
    shape_a = (c.N, c.C, H, W) if op == "F" else (c.N, c.K, OH, OW)
    for step, density in enumerate((1.0, 0.5, 0.25, 0.12, 0.06, 0.03, 0.015, 0.008, 0.004)):
        a = int_operands(shape_a, 3, density, 7000 + step)
        b = int_operands((c.K, c.C, c.k, c.k), 1, density, 7100 + step)
        y_abs = conv_apply(c, op, a.double().abs(), b.double().abs())
        if float((y_abs * y_abs).sum((0, 2, 3)).max()) < TWO24:
            return a, b, conv_apply(c, op, a.double(), b.double())
    raise AssertionError("no density makes the statistics of %s %s exact" % (case_id(c), op))


# ---------------------------------------------------------------------------------------------------------------------
# gz_conv2d_fwd_any (run-time geometry, bias + ReLU): N, C, H, W, K, KH, KW, SH, SW, PH, PW -- test_conv2d_fwd_any's 1x7,
# 7x1, 5x5 p2 and stride-2 shapes, on the igemm kernel (N = 2 / 16) and on the igemm2 skeleton (N >= 40)
# ---------------------------------------------------------------------------------------------------------------------
FWD_ANY_CASES = [
    (2, 128, 17, 17, 128, 1, 7, 1, 1, 0, 3), (2, 160, 17, 17, 192, 7, 1, 1, 1, 3, 0), (2, 48, 35, 35, 64, 5, 5, 1, 1, 2, 2),
    (2, 288, 35, 35, 384, 3, 3, 2, 2, 0, 0), (16, 192, 17, 17, 192, 3, 3, 2, 2, 0, 0), (2, 20, 13, 9, 7, 2, 4, 2, 1, 1, 2),
    (72, 128, 17, 17, 192, 1, 7, 1, 1, 0, 3), (72, 160, 17, 17, 192, 7, 1, 1, 1, 3, 0), (48, 48, 35, 35, 64, 5, 5, 1, 1, 2, 2),
    (40, 72, 17, 17, 320, 1, 7, 1, 1, 0, 3),
]


@functools.lru_cache(maxsize=2)
def fwd_any_reference(case):
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = case
    set_threads()
    x, w = pair((N, C, H, W), (K, C, KH, KW), C * KH * KW, 9000 + sum(case))
    b = int_operands((K,), 7, 1.0, 9001 + sum(case))
    assert_exact_precondition(TF.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), (SH, SW), (PH, PW)),
                              "fwd_any %s" % (case,))
    return x, w, b, torch.relu(TF.conv2d(x.double(), w.double(), b.double(), (SH, SW), (PH, PW)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the fused forms and of the FMA tails: operands, fp64 results, preconditions asserted.  The GPU module
# launches them; tests/test_exact_cases.py builds every one of them where there is no GPU.
# ---------------------------------------------------------------------------------------------------------------------
SLOPES = {"none": 0.0, "relu": 0.0, "lrelu0.5": 0.5, "lrelu0.25": 0.25}        # powers of two keep LeakyReLU exact


def act64(t, name):
    return {"none": t, "relu": torch.relu(t), "lrelu0.5": TF.leaky_relu(t, 0.5), "lrelu0.25": TF.leaky_relu(t, 0.25)}[name]


DGRAD_ACT_CASES = [(4, 3, 64, 16), (128, 3, 64, 64), (3, 4, 32, 40)]            # (N, C, H, K), k4 s2 p1
WGRAD_ACT_CASES = [(16, 3, 64, 64), (20, 4, 64, 32), (128, 3, 64, 64)]
# the same on rectangular maps, (N, C, H, W, K): tall, wide and mid-tile (N > 1, H/2 * W/2 neither divides 256 nor is a
# multiple of it: 384, 96 and 12 pixels; 384 and 144) shapes at which gz_conv2d_dgrad_act_fuses / _wgrad_act_fuses say yes
RECT_DGRAD_ACT_CASES = [(2, 3, 48, 32, 16), (4, 3, 48, 64, 16), (3, 4, 24, 16, 40), (5, 3, 6, 8, 16), (24, 4, 48, 64, 32)]
RECT_WGRAD_ACT_CASES = [(50, 3, 48, 32, 64), (128, 4, 6, 96, 16), (24, 4, 48, 64, 32), (50, 4, 48, 32, 32)]


def act_case_shape(case):
    """(N, C, H, W, K) of a (N, C, H, K) or (N, C, H, W, K) case of the two tables above."""
    return tuple(case) if len(case) == 5 else (case[0], case[1], case[2], case[2], case[3])


@functools.lru_cache(maxsize=2)
def dgrad_act_case(case, name):
    """d/dx of act(conv(x, w) + b): (x, w, b, gy, y64, dx64).  The masked gradient holds multiples of the slope, so the
    bound is 2^24 * slope."""
    N, C, H, W, K = act_case_shape(case)
    slope = SLOPES[name]
    set_threads()
    x, w, b = int_operands((N, C, H, W), 3, 1.0, 1), int_operands((K, C, 4, 4), 1, 1.0, 2), int_operands((K,), 7, 1.0, 3)
    gy = int_operands((N, K, H // 2, W // 2), WIDE, 1.0, 4)
    y = act64(TF.conv2d(x.double(), w.double(), b.double(), 2, 1), name)
    g_pre = gy.double() * torch.where(y > 0, 1.0, slope).double()
    assert_exact_precondition(TF.conv_transpose2d(g_pre.abs(), w.double().abs(), None, 2, 1) / (slope or 1.0), "dgrad_act")
    return x, w, b, gy, y, TF.conv_transpose2d(g_pre, w.double(), None, 2, 1)


@functools.lru_cache(maxsize=2)
def wgrad_act_case(case, name):
    """Weight and bias gradient of act(conv(x, w) + b) over two batches: (xs, gys, w, b, dw64, db64)."""
    N, C, H, W, K = act_case_shape(case)
    slope = SLOPES[name]
    set_threads()
    d, amp = thin(2 * N * (H // 2) * (W // 2))
    w0, b0 = int_operands((K, C, 4, 4), 1, 1.0, 12), int_operands((K,), 7, 1.0, 13)
    xs = [int_operands((N, C, H, W), WIDE, d, 10 + i) for i in (0, 100)]
    gys = [int_operands((N, K, H // 2, W // 2), amp, d, 11 + i) for i in (0, 100)]
    dw_ref, db_ref, dw_abs = 0, 0, 0
    for x, gy in zip(xs, gys):
        y = act64(TF.conv2d(x.double(), w0.double(), b0.double(), 2, 1), name)
        assert_exact_precondition(TF.conv2d(x.double().abs(), w0.double().abs(), b0.double().abs(), 2, 1), "forward")
        g_pre = gy.double() * torch.where(y > 0, 1.0, slope).double()
        dw_ref = dw_ref + torch.nn.grad.conv2d_weight(x.double(), (K, C, 4, 4), g_pre, stride=2, padding=1)
        dw_abs = dw_abs + torch.nn.grad.conv2d_weight(x.double().abs(), (K, C, 4, 4), g_pre.abs(), stride=2, padding=1)
        db_ref = db_ref + g_pre.sum((0, 2, 3))
    assert_exact_precondition(dw_abs / (slope or 1.0), "wgrad_act")
    assert_exact_precondition(sum(gy.double().abs().sum((0, 2, 3)) for gy in gys) / (slope or 1.0), "wgrad_act db")
    return xs, gys, w0, b0, dw_ref, db_ref


LINEAR_MULTI_SHAPES = [(64, 128, (256, 128, 132)), (5, 7, (3, 70)), (130, 33, (65,))]         # N, K, Js: ragged N, K and J
LINEAR_SHAPES = [(6, 40, (24,)), (70, 64, (1,)), (64, 100, (36,))]


def linear_case(N, K, Js, name, with_bias, seed):
    """[act(x W_j^T + b_j)] with the loss sum_j <G_j, out_j>, x the 12-bit operand: (x, ws, bs, Gs, outs64, dx64, dws64,
    dbs64)."""
    slope = SLOPES[name]
    d, amp = thin(max(N, K))
    x = int_operands((N, K), WIDE, d, seed)
    ws = [int_operands((J, K), amp, d, seed + 1 + i) for i, J in enumerate(Js)]
    bs = [int_operands((J,), 7, 1.0, seed + 20 + i) if with_bias else None for i, J in enumerate(Js)]
    Gs = [int_operands((N, J), 1, 1.0, seed + 40 + i) for i, J in enumerate(Js)]
    xa = x.double().abs()
    frac = slope or 1.0
    for w, G in zip(ws, Gs):
        assert_exact_precondition((xa @ w.double().abs().t() + (7.0 if with_bias else 0.0)) / frac, "linear out")
        assert_exact_precondition((G.double().abs().t() @ xa) / frac, "linear dW")
    assert_exact_precondition(sum(G.double().abs() @ w.double().abs() for w, G in zip(ws, Gs)) / frac, "linear dx")
    x64 = x.double().requires_grad_()
    w64 = [w.double().requires_grad_() for w in ws]
    b64 = [None if b is None else b.double().requires_grad_() for b in bs]
    outs = [act64(TF.linear(x64, w, b), name) for w, b in zip(w64, b64)]
    sum((o * G.double()).sum() for o, G in zip(outs, Gs)).backward()
    return x, ws, bs, Gs, [o.detach() for o in outs], x64.grad, [w.grad for w in w64], [None if b is None else b.grad for b in b64]


COLSUM_SHAPES = [(1, 4), (16, 24), (70, 1), (130, 68), (1000, 36), (33, 1025)]                # (R, L)
ROWDOT_SHAPES = [(1, 4), (6, 512), (5, 192), (70, 1024), (130, 36), (3, 8192)]
COLDOT_SHAPES = [(1, 4), (6, 512), (63, 192), (64, 192), (70, 1024), (513, 36), (2048, 512)]  # R below, at and above 64
LERP_SHAPES = [(5, 3, 8, 8), (1, 4), (64, 3, 64, 64), (7, 100)]
CHANNEL_SUM_SHAPES = [(8, 16, 32, 32), (3, 5, 4, 4), (16, 64, 8, 8, 8), (2, 7, 6, 10), (130, 3, 64, 64)]
FULL_DOT_SHAPES = [(6, 32, 4, 4), (1, 3, 4, 4), (70, 64, 4, 4), (130, 512, 4, 4)]


def colsum_case(shape):
    R, L = shape
    x = int_operands((R, L), WIDE, min(1.0, 2.0 ** 21 / (R * 2048.0)), 500 + R)
    assert_exact_precondition(x.double().abs().sum(0), "colsum")
    return x, x.double().sum(0)


def rowdot_case(shape):
    R, L = shape
    a, b = pair((R, L), (R, L), L, 600 + L)
    assert_exact_precondition((a.double().abs() * b.double().abs()).sum(1), "rowdot")
    return a, b, (a.double() * b.double()).sum(1), a.double() @ b[0].double()


def coldot_case(shape):
    R, L = shape
    x, g = pair((R, L), (R,), R, 700 + R)
    assert_exact_precondition(g.double().abs() @ x.double().abs(), "coldot")
    return x, g, g.double() @ x.double()


def lerp_case(shape):
    """lerp_rows / row_scale with factors that are multiples of 1/8 on 12-bit operands (three fractional bits: 4095 * 8 <
    2^24), and row_sumsq of a lerp with factors 0, 1/2, 1 on small integers with the gradients of the chain."""
    R = shape[0]
    view = (R,) + (1,) * (len(shape) - 1)
    a, b = int_operands(shape, WIDE, 1.0, 800), int_operands(shape, WIDE, 1.0, 801)
    al = torch.randint(0, 9, (R,), generator=torch.Generator().manual_seed(802)).float() / 8
    s = torch.randint(-16, 17, (R,), generator=torch.Generator().manual_seed(803)).float() / 8
    lerp64 = a.double() * al.double().view(view) + b.double() * (1 - al.double().view(view))
    assert_exact_precondition((a.double().abs() + b.double().abs()) * 8 * 2, "lerp_rows / row_scale")
    L = a.numel() // R
    amp = min(31, max(1, int((2.0 ** 20 / L) ** 0.5)))
    u, v = int_operands(shape, amp, 1.0, 804), int_operands(shape, amp, 1.0, 805)
    half = torch.randint(0, 3, (R,), generator=torch.Generator().manual_seed(806)).float() / 2
    u64, v64 = u.double().requires_grad_(), v.double().requires_grad_()
    mix = u64 * half.double().view(view) + v64 * (1 - half.double().view(view))
    ss64 = mix.reshape(R, -1).pow(2).sum(1)
    assert_exact_precondition((u.double().abs() + v.double().abs()).reshape(R, -1).pow(2).sum(1) * 4, "row_sumsq")
    ss64.sum().backward()
    return a, b, al, s, lerp64, a.double() * s.double().view(view), u, v, half, ss64.detach(), u64.grad, v64.grad


def channel_sum_case(shape):
    terms = shape[0] * int(torch.tensor(shape[2:]).prod())
    g = int_operands(shape, WIDE, min(1.0, 2.0 ** 21 / (terms * 2048.0)), 900)
    dims = [i for i in range(len(shape)) if i != 1]
    assert_exact_precondition(g.double().abs().sum(dims), "channel_sum")
    return g, g.double().sum(dims)


def full_dot_case(shape):
    N, C, H, W = shape
    x, w = pair(shape, (1, C, H, W), C * H * W, 950 + N)
    G = int_operands((N, 1, 1, 1), 1, 1.0, 951)
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    out64 = TF.conv2d(x64, w64, None, 2, 0)
    (out64 * G.double()).sum().backward()
    assert_exact_precondition(TF.conv2d(x.double().abs(), w.double().abs(), None, 2, 0), "full_dot_conv")
    assert_exact_precondition((x.double().abs() * G.double().abs()).sum(0), "full_dot_conv dw")
    return x, w, G, out64.detach(), x64.grad, w64.grad


def second_order_conv_operands():
    return (int_operands((3, 3, 16, 16), 1, 0.5, 21), int_operands((8, 3, 4, 4), 1, 0.5, 22),
            int_operands((6, 8, 4, 4), 1, 0.5, 23))


def second_order_conv_graph(x, w1, w2, conv, act):
    """conv -> act -> conv; gx = d out.sum() / dx with the graph kept; penalty sum(gx^2) + sum(out^2), no sqrt."""
    h = act(conv(x, w1))
    out = conv(h, w2)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    ga, gb = torch.autograd.grad(gx.pow(2).sum() + out.pow(2).sum(), (w1, w2))
    return gx.detach(), ga, gb, out.detach()


def second_order_conv_reference():
    """fp64 torch autograd with LeakyReLU(0.5); the precondition from the same graph on absolute operands with the
    activation replaced by the identity (|act'| <= 1), times 4 for the two fractional bits slope^2 brings."""
    def leaf(t, absolute):
        return (t.abs() if absolute else t).double().requires_grad_()
    ops = second_order_conv_operands()
    conv = lambda t, w: TF.conv2d(t, w, None, 2, 1)
    for t in second_order_conv_graph(*[leaf(o, True) for o in ops], conv, lambda t: t):
        assert_exact_precondition(t * 4, "second order")
    return second_order_conv_graph(*[leaf(o, False) for o in ops], conv, lambda t: TF.leaky_relu(t, 0.5))


def second_order_dot_operands():
    return int_operands((6, 32, 4, 4), 1, 1.0, 51), int_operands((1, 32, 4, 4), 1, 1.0, 52)


def second_order_dot_graph(x, w, dot):
    out = dot(x, w)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    return (out.detach(), gx.detach()) + torch.autograd.grad(gx.pow(2).sum() + out.pow(2).sum(), (x, w))


def second_order_dot_reference():
    ops = second_order_dot_operands()
    dot = lambda t, w: TF.conv2d(t, w, None, 2, 0)
    for t in second_order_dot_graph(*[o.abs().double().requires_grad_() for o in ops], dot):
        assert_exact_precondition(t, "second order")
    return second_order_dot_graph(*[o.double().requires_grad_() for o in ops], dot)


PAIR_MEAN_N = [1, 64, 512]                  # n_each: powers of two keep the means exact
PAIR_MEAN_WEIGHTS = [(-1.0, 1.0), (0.5, -2.0)]


def pair_mean_case(n_each, weights):
    """t0 * mean(first) + t1 * mean(second) with the upstream factor 0.25: (x, value64, gradient64)."""
    x = int_operands((2 * n_each, 1), WIDE, 1.0, 1200 + n_each)
    assert_exact_precondition(x.double().abs().view(2, -1).sum(1) * 8, "pair loss")
    x64 = x.double().requires_grad_()
    ref = weights[0] * x64[:n_each].mean() + weights[1] * x64[n_each:].mean()
    (ref * 0.25).backward()
    return x, ref.detach(), x64.grad

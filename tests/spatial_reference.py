"""The fp64 reference of the pooling, resize and ResNet spatial kernels (csrc/gz_infer.hip, first half of
csrc/gz_resnet.hip): numpy only, no torch, no GPU, no import of the library.  Every function is written from the
operation, not from the kernel that serves it, and returns with the value what its tolerance needs.

Tolerances are  |got - ref| <= K u scale  with u = 2^-24 (the unit roundoff of float32) and `scale` the sum of the
magnitudes that enter the element.

  sums (average pools, avgpool3s2 forward and backward, upsample2 backward, the global average): n float32 terms summed
    in any order cost n - 1 additions, each with a relative error of at most u in a partial sum whose magnitude the sum
    of |term| bounds; then one scaling (the division, or the product with the constant) and one rounded constant
    (1.f / 9.f; 1 / 64 is exact and only makes the bound generous), each u; one to spare.  K = n + 2, n the number of
    taps inside the image (SUM_SPARE = 2).
  axpby: alpha a and beta b are one rounding each (u |alpha a|, u |beta b|: together u scale), their sum one more
    (u |out| <= u scale); a fused multiply-add only removes one of them.  2, and one to spare: K = 3.
  act_fwd, leaky: one product, one rounding: K = 1.  Below the normal range a rounding is absolute, not relative: every
    non-exact tolerance carries TINY = 2^-149, one denormal step.
  exact, bit for bit: max pooling, upsample2 forward, relu, the identity resize with mul 1 add 0.

Bilinear (resize_bilinear, samples_to_inception) has no such count: the float32 source coordinate is off by a few
u max(f, 1), and that error is multiplied by the slope of the interpolant, which `spread` (the largest difference among
the four taps) bounds.  tol = u (K1 scale + K2 max(fy, fx, 1) spread |mul|) + TINY, with K1 and K2 measured by
`python tests/spatial_reference.py --measure`: a numpy float32 emulation of the operation over the inputs of the case
table (spatial_cases.py), in both spellings of the kernel source (the pinned one with its explicit fused operations, the
plain expression) and, for the plain one, with every choice of which product the compiler fuses into which sum.  K1 is
measured on the outputs whose four taps are equal or whose coordinate is exact in either arithmetic (spread term zero or
coordinate term zero), K2 on all outputs with K1 in place.  K is twice the worst ratio seen, rounded up to an integer.
The kernel's output is never used to choose K.

Measured (worst ratios of the emulation):  K1 3.333 -> K1 = 7;  K2 1.603 -> K2 = 4."""
import itertools
import sys

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
SUM_SPARE = 2
K_AXPBY = 3
K_ACT = 1
MEASURED = {"K1": 3.333, "K2": 1.603}
K1, K2 = 7, 4
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2

MUTATION = None     # test_spatial_reference_cpu.py: a deliberately wrong implementation (see wrong())
MUTATIONS = ("mode1_divides_by_ks2", "max_border_zero", "right_edge_window_shifted", "y1_without_clamp",
             "align_corners_coordinates", "avgpool3s2_bwd_drops_last_row")


class wrong:
    """with wrong(name): the functions below compute the named mistake instead of the operation."""

    def __init__(self, name):
        assert name in MUTATIONS, name
        self.name = name

    def __enter__(self):
        global MUTATION
        MUTATION = self.name

    def __exit__(self, *exc):
        global MUTATION
        MUTATION = None


class Out:
    """One output: the fp64 value and the tolerance of every element (None: the float32 of the value, bit for bit)."""

    def __init__(self, value, tol, kind):
        self.value = np.asarray(value, dtype=np.float64)
        self.tol = None if tol is None else np.broadcast_to(np.asarray(tol, dtype=np.float64), self.value.shape)
        self.kind = kind


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ratios(got, out):
    """|got - ref| / tol per element (0 where both are 0; inf where only the tolerance is)."""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(out.value.shape) - out.value)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / out.tol)


def compare(got, out, what=""):
    """The messages of the elements outside the tolerance (at most one line per output)."""
    got = np.asarray(got, dtype=np.float32).reshape(out.value.shape)
    if out.tol is None:
        bad = np.flatnonzero(bits(got).reshape(-1) != bits(out.value).reshape(-1))
        if bad.size:
            i = bad[0]
            return ["%s: %d of %d words differ, first at %d: got %r, want %r" % (
                what, bad.size, got.size, i, float(got.reshape(-1)[i]), float(out.value.reshape(-1)[i]))]
        return []
    r = ratios(got, out)
    bad = np.flatnonzero(~(r.reshape(-1) <= 1.0))
    if bad.size:
        i = int(bad[np.argmax(r.reshape(-1)[bad])])
        return ["%s: %d of %d elements outside the tolerance, worst at %d: got %r, want %r, %.3g x the tolerance %.3g" % (
            what, bad.size, got.size, i, float(got.reshape(-1)[i]), float(out.value.reshape(-1)[i]), r.reshape(-1)[i],
            out.tol.reshape(-1)[i])]
    return []


def worst(got, out):
    return 0.0 if out.tol is None or not out.value.size else float(ratios(got, out).max())


def f64(a):
    return np.asarray(a, dtype=np.float64)


def out_size(n, KS, S, P):
    return (n + 2 * P - KS) // S + 1


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
def _windows(xp, KS, S, OH, OW):
    """The KS * KS taps of every window of the padded planes xp [planes, HP, WP], each as [planes, OH, OW]."""
    return [xp[:, dy:dy + S * (OH - 1) + 1:S, dx:dx + S * (OW - 1) + 1:S] for dy in range(KS) for dx in range(KS)]


def pool2d(x, KS, S, P, mode):
    """x [planes, H, W] -> (y, scale, n) with y [planes, OH, OW]; mode 0 max, 1 average over the taps inside the image,
    2 average over KS * KS.  scale = sum |tap| / divisor (max: |y|); n = taps inside the image, [OH, OW]."""
    x = f64(x)
    planes, H, W = x.shape
    OH, OW = out_size(H, KS, S, P), out_size(W, KS, S, P)
    assert OH > 0 and OW > 0
    border = -np.inf if mode == 0 and MUTATION != "max_border_zero" else 0.0
    xp = np.full((planes, H + 2 * P, W + 2 * P + 1), border)        # (one spare column for the shifted-window mistake)
    xp[:, P:P + H, P:P + W] = x
    inside = np.zeros((1, H + 2 * P, W + 2 * P + 1))
    inside[:, P:P + H, P:P + W] = 1.0
    taps = _windows(xp, KS, S, OH, OW)
    if MUTATION == "right_edge_window_shifted":         # the last output column reads one column further right
        taps = [np.concatenate([t[:, :, :-1], ts[:, :, -1:]], axis=2)
                for t, ts in zip(taps, _windows(xp[:, :, 1:], KS, S, OH, OW))]
    n = sum(_windows(inside, KS, S, OH, OW))[0]
    if mode == 0:
        y = taps[0]
        for t in taps[1:]:
            y = np.maximum(y, t)
        return y, np.abs(y), n
    div = n if mode == 1 and MUTATION != "mode1_divides_by_ks2" else float(KS * KS)
    return sum(taps) / div, sum(np.abs(t) for t in taps) / div, n


def pool2d_out(x, KS, S, P, mode):
    y, scale, n = pool2d(x, KS, S, P, mode)
    if mode == 0:
        return Out(y, None, "pool_max")
    return Out(y, (n + SUM_SPARE) * U * scale + TINY, "pool_avg")


# ---------------------------------------------------------------------------
# AvgPool2d(3, stride 2, padding 1) with count_include_pad, nearest 2x upsampling, and their adjoints
# ---------------------------------------------------------------------------
def avgpool3s2_fwd(x):
    """x [planes, H, W] -> (y, scale, n), y [planes, (H - 1) // 2 + 1, (W - 1) // 2 + 1]: the mean over the 3 x 3 window
    centred on (2 oh, 2 ow), taps outside the image counting as zero, always divided by 9."""
    x = f64(x)
    planes, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp, inside = np.zeros((planes, 2 * OH + 1, 2 * OW + 1)), np.zeros((1, 2 * OH + 1, 2 * OW + 1))
    xp[:, 1:H + 1, 1:W + 1] = x
    inside[:, 1:H + 1, 1:W + 1] = 1.0
    y, scale, n = 0.0, 0.0, 0.0
    for dy, dx in itertools.product(range(3), range(3)):
        sl = (slice(None), slice(dy, dy + 2 * OH - 1, 2), slice(dx, dx + 2 * OW - 1, 2))
        y, scale, n = y + xp[sl] / 9.0, scale + np.abs(xp[sl]) / 9.0, n + inside[sl]
    return y, scale, n[0]


def avgpool3s2_bwd(gy, H, W):
    """The transpose of avgpool3s2_fwd: every gy[oh][ow] / 9 is scattered into its window, what falls outside the
    image is dropped.  gy [planes, OH, OW] -> (gx [planes, H, W], scale, n)."""
    gy = f64(gy)
    planes, OH, OW = gy.shape
    assert OH == (H - 1) // 2 + 1 and OW == (W - 1) // 2 + 1
    if MUTATION == "avgpool3s2_bwd_drops_last_row":
        gy = gy.copy()
        gy[:, -1, :] = 0.0
    gp, sp, np_ = (np.zeros((planes, 2 * OH + 1, 2 * OW + 1)) for _ in range(3))
    for dy, dx in itertools.product(range(3), range(3)):
        sl = (slice(None), slice(dy, dy + 2 * OH - 1, 2), slice(dx, dx + 2 * OW - 1, 2))
        gp[sl] += gy / 9.0
        sp[sl] += np.abs(gy) / 9.0
        np_[sl] += 1.0
    crop = (slice(None), slice(1, H + 1), slice(1, W + 1))
    return gp[crop], sp[crop], np_[crop][0]


def upsample2_fwd(x):
    """y[2h + a][2w + b] = x[h][w]."""
    return np.repeat(np.repeat(f64(x), 2, axis=1), 2, axis=2)


def upsample2_bwd(gy):
    """The transpose: gx[h][w] = the sum of the four gy it was copied to.  -> (gx, scale)."""
    gy = f64(gy)
    p, H2, W2 = gy.shape
    g = gy.reshape(p, H2 // 2, 2, W2 // 2, 2)
    return g.sum((2, 4)), np.abs(g).sum((2, 4))


def sum_out(value, scale, n, kind):
    return Out(value, (n + SUM_SPARE) * U * scale + TINY, kind)


# ---------------------------------------------------------------------------
# activation, residual tail
# ---------------------------------------------------------------------------
def act_fwd(x, act, slope=0.0):
    """-> (y, exact): relu max(x, 0) with relu(-0) = +0; leaky relu x for x > 0, slope x otherwise."""
    x = f64(x)
    if act == ACT_RELU:
        return np.where(x > 0, x, 0.0), True
    if act == ACT_LRELU:
        return np.where(x > 0, x, x * float(np.float32(slope))), False
    return x, True


def act_out(x, act, slope=0.0):
    y, exact = act_fwd(x, act, slope)
    return Out(y, None if exact else K_ACT * U * np.abs(y) + TINY, "act")


def axpby(a, alpha, b, beta):
    """alpha a + beta b (b None: alpha a) -> (out, scale); alpha and beta as the C ABI receives them (float32)."""
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    out, scale = alpha * f64(a), np.abs(alpha * f64(a))
    if b is not None:
        out, scale = out + beta * f64(b), scale + np.abs(beta * f64(b))
    return out, scale


def axpby_out(a, alpha, b, beta):
    out, scale = axpby(a, alpha, b, beta)
    return Out(out, K_AXPBY * U * scale + TINY, "axpby")


# ---------------------------------------------------------------------------
# bilinear resize (ATen's align_corners=False rule), generator output -> Inception input
# ---------------------------------------------------------------------------
def _source(n_out, n_in, dt=np.float64):
    """(coordinate, lower tap, upper tap, upper weight) of every output index along one axis; the scale is the float32
    quotient the launcher passes, everything after it in `dt`."""
    scale = dt(np.float32(n_in) / np.float32(n_out))
    o = np.arange(n_out).astype(dt)
    if MUTATION == "align_corners_coordinates":
        f = o * dt((n_in - 1) / max(n_out - 1, 1))
    else:
        f = np.maximum((o + dt(0.5)) * scale - dt(0.5), dt(0))
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = i0 + 1 if MUTATION == "y1_without_clamp" else np.minimum(i0 + 1, n_in - 1)
    return f, i0, i1, f - i0.astype(dt)


def _taps(x, OH, OW):
    """x [planes, H, W] -> the four taps [planes, OH, OW] (a, b top left / right; c, d bottom), and the axis data."""
    planes, H, W = x.shape
    fy, y0, y1, ly = _source(OH, H)
    fx, x0, x1, lx = _source(OW, W)
    if MUTATION == "y1_without_clamp":                  # reads the row after the plane: the next plane's first, or 0
        flat, first = np.concatenate([x.reshape(-1), np.zeros(W + 1)]), (np.arange(planes) * H * W)[:, None, None]
        g = lambda yy, xx: flat[first + (yy[:, None] * W + xx[None, :])[None]]  # noqa: E731
    else:
        g = lambda yy, xx: x[:, yy[:, None], xx[None, :]]            # noqa: E731
    return (g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)), (fy, ly), (fx, lx)


def resize_bilinear(x, OH, OW, mul, add):
    """-> (y, scale, spread, coord): y = bilinear(x) * mul + add;  scale = sum |w_k p_k| |mul| + |add|;  spread = the
    largest |p_i - p_j| over the four taps;  coord = max(fy, fx, 1)."""
    x = f64(x)
    mul, add = float(np.float32(mul)), float(np.float32(add))
    (a, b, c, d), (fy, ly), (fx, lx) = _taps(x, OH, OW)
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = 1.0 - ly, 1.0 - lx
    v = hy * (hx * a + lx * b) + ly * (hx * c + lx * d)
    mag = hy * (hx * np.abs(a) + lx * np.abs(b)) + ly * (hx * np.abs(c) + lx * np.abs(d))
    spread = np.maximum(np.maximum(a, b), np.maximum(c, d)) - np.minimum(np.minimum(a, b), np.minimum(c, d))
    coord = np.maximum(np.maximum(fy[:, None], fx[None, :]), 1.0)[None]
    return v * mul + add, mag * abs(mul) + abs(add), spread, coord


def bilinear_tol(scale, spread, coord, mul, k1=None, k2=None):
    k1, k2 = K1 if k1 is None else k1, K2 if k2 is None else k2
    return U * (k1 * scale + k2 * coord * spread * abs(float(np.float32(mul)))) + TINY


def resize_out(x, OH, OW, mul, add):
    y, scale, spread, coord = resize_bilinear(x, OH, OW, mul, add)
    if x.shape[1:] == (OH, OW) and mul == 1.0 and add == 0.0:
        return Out(y, None, "resize")
    return Out(y, bilinear_tol(scale, spread, coord, mul), "resize")


def grey_level(x):
    """The sample dump's truncation, specified in float32: int(float32(clip(v, 0, 1)) * float32(255))."""
    c = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1))
    return (c * np.float32(255)).astype(np.int64)


def samples_to_inception(x, OH, OW, mul, add):
    """x [N, C, H, W], C 1 or 3 -> (y [N, 3, OH, OW], scale, spread, coord): level / 255, the resize, and for C = 1 the
    one plane in all three channels."""
    N, C, H, W = x.shape
    q = grey_level(x).astype(np.float64) / 255.0
    if C == 1:
        q = np.repeat(q, 3, axis=1)
    y, scale, spread, coord = resize_bilinear(q.reshape(N * 3, H, W), OH, OW, mul, add)
    sh = (N, 3, OH, OW)
    return y.reshape(sh), scale.reshape(sh), spread.reshape(sh), np.broadcast_to(coord, (N * 3, OH, OW)).reshape(sh)


def samples_out(x, OH, OW, mul, add):
    y, scale, spread, coord = samples_to_inception(x, OH, OW, mul, add)
    return Out(y, bilinear_tol(scale, spread, coord, mul), "samples")


def constant_plane_tol(c, mul, add):
    """A constant plane c, |c| <= 1: the weights sum to one whatever they are."""
    return 4 * U * (abs(c * float(np.float32(mul))) + abs(float(np.float32(add))))


# ---------------------------------------------------------------------------
# float32 emulation of the bilinear kernels (for --measure and the CPU test; never for the GPU test)
# ---------------------------------------------------------------------------
F32 = np.float32


def _fma(a, b, c):
    """round(a b + c) for float32 operands: the product is exact in float64, the sum is rounded to 53 bits and then to
    24 (a double rounding that differs from the fused operation in about one case in 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, dtype=np.float32).astype(np.float64)).astype(F32)


def _sum2(p, x, q, y, fuse):
    """p x + q y in float32; fuse 0: both products rounded; 1: fma(p, x, q y); 2: fma(q, y, p x)."""
    if fuse == 0:
        return p * x + q * y
    return _fma(p, x, q * y) if fuse == 1 else _fma(q, y, p * x)


def _source32(n_out, n_in, fused):
    scale = F32(n_in) / F32(n_out)
    o = np.arange(n_out).astype(F32) + F32(0.5)
    f = _fma(o, np.full_like(o, scale), F32(-0.5)) if fused else o * scale - F32(0.5)
    f = np.maximum(f, F32(0))
    i0 = f.astype(np.int64)
    return f, i0, i0 + (i0 < n_in - 1), f - i0.astype(F32)


def emulate(x, OH, OW, mul, add, quantised=False):
    """Yields (name, y float32 [planes, OH, OW]) for every spelling: "pinned", and "plain" with the coordinate fused or
    not, each inner sum and the outer sum with none, the first or the second product fused, the last product fused or
    not.  quantised: x holds grey levels, a tap is float32(level) * float32(1 / 255) as the kernel forms it."""
    x = np.asarray(x, dtype=F32)
    if quantised:
        x = x * (F32(1) / (F32(255) * F32(1)))
    mul, add = F32(mul), F32(add)
    planes, H, W = x.shape
    for cf in (True, False):
        _, y0, y1, ly = _source32(OH, H, cf)
        _, x0, x1, lx = _source32(OW, W, cf)
        a, b = x[:, y0[:, None], x0[None, :]], x[:, y0[:, None], x1[None, :]]
        c, d = x[:, y1[:, None], x0[None, :]], x[:, y1[:, None], x1[None, :]]
        ly3, lx3 = np.broadcast_to(ly[None, :, None], a.shape), np.broadcast_to(lx[None, None, :], a.shape)
        hy3, hx3 = F32(1) - ly3, F32(1) - lx3
        if cf:
            top, bot = _fma(lx3, b, hx3 * a), _fma(hx3, c, lx3 * d)
            yield "pinned", _fma(hy3 * top + ly3 * bot, np.full_like(a, mul), add)
        for ft, fb in itertools.product(range(3), range(3)):
            top, bot = _sum2(hx3, a, lx3, b, ft), _sum2(hx3, c, lx3, d, fb)
            for fo in range(3):
                v = _sum2(hy3, top, ly3, bot, fo)
                yield "plain c%d t%d b%d o%d m0" % (cf, ft, fb, fo), v * mul + add
                yield "plain c%d t%d b%d o%d m1" % (cf, ft, fb, fo), _fma(v, np.full_like(v, mul), add)


def _emulation_runs(cases):
    """(case name, emulated outputs, the reference's (value, scale, spread, coord), mul) per bilinear case."""
    import spatial_cases as sc
    for case in cases:
        if case.kind == "resize":
            x, (OH, OW, mul, add) = sc.resize_host(case), (case.OH, case.OW, case.mul, case.add)
            ref = resize_bilinear(x, OH, OW, mul, add)
            yield case, emulate(x, OH, OW, mul, add), ref
        else:
            x = sc.samples_host(case)
            N, C, H, W = x.shape
            lv = grey_level(x)
            lv = np.repeat(lv, 3, axis=1) if C == 1 else lv
            ref = tuple(r.reshape(N * 3, case.OH, case.OW) for r in
                        samples_to_inception(x, case.OH, case.OW, case.mul, case.add))
            yield case, emulate(lv.reshape(N * 3, H, W), case.OH, case.OW, case.mul, case.add, quantised=True), ref


def measure(cases=None, k1=None):
    """The worst ratios of the emulation: {"K1": ..., "K2": ...}.  K1: err / (u scale) over the outputs whose spread
    term vanishes; K2: (err - u k1 scale) / (u coord spread |mul|) over the others, k1 the constant K1 follows from
    (given, or twice the measured ratio rounded up)."""
    import spatial_cases as sc
    cases = [c for c in (cases or sc.bilinear_cases()) if not c.loop]
    runs, w1 = [], 0.0
    for case, ys, (v, scale, spread, coord) in _emulation_runs(cases):
        err = np.zeros_like(v)
        for _, y in ys:
            err = np.maximum(err, np.abs(y.astype(np.float64) - v))
        flat = spread == 0.0
        if flat.any():
            w1 = max(w1, float((err[flat] / (U * scale[flat] + TINY)).max()))
        runs.append((err, scale, spread, np.broadcast_to(coord, v.shape), abs(float(np.float32(case.mul)))))
    k1 = constant(w1) if k1 is None else k1
    w2 = 0.0
    for err, scale, spread, coord, mul in runs:
        live = spread > 0.0
        if live.any():
            rest = err[live] - U * k1 * scale[live] - TINY
            w2 = max(w2, float((rest / (U * coord[live] * spread[live] * mul)).max()))
    return {"K1": w1, "K2": w2}


def constant(ratio):
    return int(np.ceil(2.0 * ratio))


if __name__ == "__main__":
    if "--measure" in sys.argv:
        got = measure()
        print("worst ratios of the float32 emulation: K1 %.3f  K2 %.3f" % (got["K1"], got["K2"]))
        print("K1 = %d, K2 = %d" % (constant(got["K1"]), constant(got["K2"])))

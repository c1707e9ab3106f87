"""An fp64 reference for every case of tests/test_norm_parent_bits_gpu.py: CPU only, no import of the library.

For each driver of that file (``_rownorm_fwd`` ...) there is a twin here (``REFERENCE["rownorm_fwd"]`` ...) that takes
the same arguments, reads the same seeded host inputs (norm_cases.py) and returns the same keys.  A key maps to an `Out`:
the fp64 value, a condition-aware error scale per element, and what an activation mask needs (below).  The operation is
written plainly in torch float64 -- mean, variance, rsqrt, affine, activation; every gradient by torch.autograd of that
forward graph -- and not as the kernels spell it.

Comparison (compare()):   |got_i - value_i| <= K[kind] * u * scale_i + slack_i,   u = 2^-24.

scale_i: the magnitude of the terms the result is formed from.  It is computed by running the closed formula of the
quantity (the one in the header of csrc/gz_norm.hip: z = x scale + shift, dz = g act'(z), xh = (x - mean) rstd,
dx = scale (dz - k1 - xh k2), ...) in the little error arithmetic of class T, which carries next to every value v a
magnitude s >= |v|:
    a + b, a - b   ->  s_a + s_b                       (a subtraction counts as an addition)
    a * b          ->  s_a |b| + |a| s_b - |a b|       (first order: each factor's error times the other's value; equal
                                                        to |a b| when both factors are exact)
    sum_i a_i      ->  sum_i s_i ;     a * const, a / const  ->  s * |const|
    sqrt(a)        ->  s_a / (2 sqrt|a|) ;     a / b  ->  s_a / |b| + |a| s_b / b^2      (first order; used by
                                                        tail_reference.py, no formula of this module needs them)
    input          ->  s = |v|
so that a result which is a small difference of large terms is allowed the error of the large terms and no more.  Two
quantities enter this arithmetic with a scale of their own:
    mean:  s = sum|x| / n.
    rstd = 1 / sqrt(var + eps):  s = rstd * kappa.  kappa is the condition of the variance as the PATH forms it.
      Row paths (rownorm_act_fused_kernel) use the corrected two-pass formula: x - mean_f is exact to one rounding and
      the correction term removes the error of mean_f, so var has the relative error of a sum of squares: kappa = 1.
      BatchNorm paths (bn_finalize from row_sums_kernel, or from a convolution's partial rows) form
      sum x^2 / n - mean^2 from float32 row sums: an error of u sum x^2 / n against var + eps, so
      kappa = (sum x^2 / n) / (var + eps).
    The running variance carries s = sum x^2 / n + 2 |mean| s_mean - mean^2 by the same rules.

either_i (outputs behind an activation mask): where the fp64 pre-activation z lies in the band
|z| <= B u (|x scale| + |mean scale| + |beta|) a float32 kernel may take the other side.  Such an element also passes
if it matches `alt`, the value with the other mask for that element; and every reduction or group mean the element
feeds gets `slack` = the absolute value of the element's term (with its weight in that reduction) added to its
tolerance.  The derivations stand where the slack is formed (_first_backward, _second_backward).

Untouched words: an output buffer starts at SENTINEL; a word the entry point does not write has value SENTINEL and
scale 0, so it must be there bit for bit.  Integer outputs (nbt, bwd_rc) have kind "int" and are compared exactly.

K and B are MEASURED, not chosen: `python tests/norm_reference.py --measure` replays every case with the same code in
float32 on the CPU -- the variance formed the way the path under test forms it -- and prints, per kind, the largest
|replay - reference| / (u scale); K = 4 x that, rounded up to a power of two (4: the replay sums in torch's order, the
kernels lane-serial, then by xor butterfly, then in fp64 columns; errors of the same size, not equal).  B comes the same
way from the replay's error in z.  The table below is that output; test_norm_reference_cpu.py re-derives it."""
import contextlib
import functools
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

import norm_cases as nc
from norm_cases import ACTS, EPS, MOMENTUM, SENTINEL

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
RED = (1, 3)                # a tensor is viewed [A, B, C, D]: statistics of (a, c) over b and d

# --measure (CPU replay in float32 against this reference, all cases and settings): largest ratio -> K
MEASURED = {'coef': 4.274, 'out': 4.41, 'dx': 3.532, 'affine': 2.654, 'k': 2.424, 'running': 3.295, 'bwd2': 2.807,
            'ew': 1.921}
K = {'coef': 32, 'out': 32, 'dx': 16, 'affine': 16, 'k': 16, 'running': 16, 'bwd2': 16, 'ew': 8}
MEASURED_Z = {'row': 16.627, 'bn': 23.056}      # the replay's error in z over u (|x scale| + |mean scale| + |beta|)
B = {'row': 128, 'bn': 128}

_TRACE = None               # measure_z(): a list that collects the runs of _forward
MUTATION = None             # test_norm_reference_cpu.py: a deliberately wrong reference (mutated())


@contextlib.contextmanager
def mutated(name):
    global MUTATION
    MUTATION = name
    try:
        yield
    finally:
        MUTATION = None


class Out:
    """One output of a case.  kind: a key of K, or "int".  alt / slack: see the module text; either: the band."""

    def __init__(self, value, scale=None, kind="int", alt=None, slack=None, either=None):
        self.kind = kind
        self.value = _np(value)
        self.scale = None if scale is None else np.broadcast_to(_np(scale), self.value.shape)
        self.alt = None if alt is None else _np(alt)
        self.slack = None if slack is None else np.broadcast_to(_np(slack), self.value.shape)
        self.either = None if either is None else _np(either).astype(bool)


def untouched(shape):
    """Words the entry point must not write: SENTINEL, to the bit (scale 0)."""
    return Out(np.full(shape, SENTINEL), np.zeros(shape), "out")


def _np(t):
    if isinstance(t, T):
        t = t.v
    if isinstance(t, torch.Tensor):
        t = t.detach()
        return t.numpy() if t.dtype == torch.int64 or t.dtype == torch.bool else t.double().numpy()
    return np.asarray(t)


class T:
    """A value with the magnitude of the terms it was formed from (module text)."""

    def __init__(self, v, s=None):
        self.v = v.detach()
        self.s = self.v.abs() if s is None else s.detach()

    def __add__(self, o):
        return T(self.v + o.v, self.s + o.s)

    def __sub__(self, o):
        return T(self.v - o.v, self.s + o.s)

    def __mul__(self, o):
        if not isinstance(o, T):
            return T(self.v * o, self.s * abs(o))
        return T(self.v * o.v, self.s * o.v.abs() + self.v.abs() * o.s - (self.v * o.v).abs())

    def __truediv__(self, c):
        if isinstance(c, T):        # first order: s_a / |b| + |a| s_b / b^2
            return T(self.v / c.v, self.s / c.v.abs() + self.v.abs() * c.s / (c.v * c.v))
        return T(self.v / c, self.s / abs(c))

    def sqrt(self):                 # first order: s_a / (2 sqrt|a|); an exact zero stays exact
        r = self.v.abs().sqrt()
        return T(r, torch.where(r > 0, self.s / (2 * r), torch.zeros_like(r)))

    def __neg__(self):
        return T(-self.v, self.s)

    def sum(self, dims, keepdim=True):
        return T(self.v.sum(dims, keepdim=keepdim), self.s.sum(dims, keepdim=keepdim))

    def reshape(self, *shape):
        return T(self.v.reshape(*shape), self.s.reshape(*shape))

    def expand(self, *shape):
        return T(self.v.expand(*shape), self.s.expand(*shape))


def _cat(ts, dim=0):
    return T(torch.cat([t.v for t in ts], dim), torch.cat([t.s for t in ts], dim))


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _inputs(d, dt):
    return {k: _t(v, dt) for k, v in d.items()}


# ---------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------
def _moments(x, n, mode, dt):
    """(mean, biased variance) of x [A, B, C, D] over b and d, in fp64, differentiable.  float64: the plain operation.
    float32 (the replay): formed as the path under test forms them."""
    if MUTATION == "skip_last4":
        xs = x[..., :-4]
        mean = xs.sum(RED, keepdim=True) / n
        return mean.double(), (((xs - mean) ** 2).sum(RED, keepdim=True) / n).double()
    if dt == F64:
        return x.mean(RED, keepdim=True), x.var(RED, unbiased=False, keepdim=True)
    if mode == "twopass":       # rownorm_act_fused_kernel: float32 mean, float32 centred sums, corrected in fp64
        mean_f = x.sum(RED, keepdim=True) / n
        d = x - mean_f
        d0, d1 = d.sum(RED, keepdim=True).double(), (d * d).sum(RED, keepdim=True).double()
        return mean_f.double() + d0 / n, ((d1 - d0 * d0 / n) / n).clamp_min(0.0)
    # "sums": row_sums_kernel + bn_finalize: float32 sums of x and x^2 per row, combined in fp64
    s1 = x.sum(3, keepdim=True).double().sum(1, keepdim=True)
    s2 = (x * x).sum(3, keepdim=True).double().sum(1, keepdim=True)
    mean = s1 / n
    return mean, (s2 / n - mean * mean).clamp_min(0.0)


def _stats(x, n, unb, mode, dt, partials=None):
    """Statistics of x [A, B, C, D] per (a, c).  partials [A, R, C, 2] (float32 partial sums from the caller, `n`
    elements per (a, c)): the VALUES come from their fp64 sums; the derivatives stay those of the statistics of x."""
    st = types.SimpleNamespace()
    A, _, C, _ = x.shape
    whole = MUTATION == "group_stats_whole_batch" and A > 1 and mode == "sums"
    xs = x.reshape(1, -1, C, x.shape[3]) if whole else x
    mean, var = _moments(xs, xs.shape[1] * xs.shape[3], mode, dt)
    with torch.no_grad():
        st.mean_s = xs.abs().double().sum(RED, keepdim=True) / (xs.shape[1] * xs.shape[3])
        st.ex2 = (xs.double() ** 2).sum(RED, keepdim=True) / (xs.shape[1] * xs.shape[3])
    if partials is not None and not whole:
        p = partials.double()
        s1, s2 = p[..., 0].sum(1).reshape(A, 1, C, 1), p[..., 1].sum(1).reshape(A, 1, C, 1)
        mean_p = s1 / n
        var_p = (s2 / n - mean_p * mean_p).clamp_min(0.0)
        mean, var = mean + (mean_p - mean).detach(), var + (var_p - var).detach()
        st.mean_s, st.ex2 = p[..., 0].abs().sum(1).reshape(A, 1, C, 1) / n, s2 / n
    if whole:
        mean, var = mean.expand(A, 1, C, 1), var.expand(A, 1, C, 1)
        st.mean_s, st.ex2 = st.mean_s.expand(A, 1, C, 1), st.ex2.expand(A, 1, C, 1)
    st.mean, st.var_biased = mean, var
    if MUTATION == "swap_unbiased":
        unb = 1 - unb
    st.var = var * (n / (n - 1.0)) if unb and n > 1 else var
    return st


def _mask(z, act):
    name = {v[0]: k for k, v in ACTS.items()}[act[0]]
    if name == "none":
        return torch.ones_like(z), torch.ones_like(z)
    lo = 0.0 if name == "relu" else act[1]
    pos = z > 0
    one, low = torch.ones_like(z), torch.full_like(z, lo)
    return torch.where(pos, one, low), torch.where(pos, low, one)


def _act(z, act, m):
    if MUTATION == "mask_from_xh":
        return z * m
    if act[0] == 1:
        return F.relu(z)
    if act[0] == 2:
        return F.leaky_relu(z, act[1])
    return z


# ---------------------------------------------------------------------------
# the engine: forward, first backward, second backward of one normalisation on a [A, B, C, D] view
# ---------------------------------------------------------------------------
def _forward(x, ga, be, eps, unb, act, dt, mode, path, partials=None, count=None):
    """x [A, B, C, D]; ga, be broadcastable [A or 1, 1, C, 1] (None: 1 and 0); eps a number or [A, 1, 1, 1]."""
    r = types.SimpleNamespace()
    A, Bn, C, D = x.shape
    n = float(count or Bn * D)
    r.n, r.nk, r.path = n, (n - 1.0 if unb and n > 1 else n), path      # nk: the divisor of k2 (header of row_bwd_k)
    if ga is None:
        ga, be = torch.ones(1, 1, C, 1, dtype=dt), torch.zeros(1, 1, C, 1, dtype=dt)
    st = _stats(x, n, unb, mode, dt, partials)
    rstd = (st.var.double() + eps).rsqrt().to(dt)
    mean = st.mean.to(dt)
    sc = ga * rstd
    sh = be - mean * sc
    z = x * sc + sh
    with torch.no_grad():
        # kappa (module text): 1 for the two-pass row path, (sum x^2 / n) / (var + eps) for the sums paths
        kappa = (st.ex2 / (st.var_biased.double() + eps)).clamp_min(1.0)
        if mode == "twopass":
            kappa = torch.ones_like(kappa)
        r.x, r.ga, r.be = T(x), T(ga.expand(ga.shape[0], 1, C, 1)), T(be.expand(be.shape[0], 1, C, 1))
        r.mean = T(mean, st.mean_s.to(dt))
        r.rstd = T(rstd, (rstd.double() * kappa).to(dt))
        r.var_biased = T(st.var_biased.double(), st.ex2 + 2 * mean.double().abs() * st.mean_s - mean.double() ** 2)
        r.sc = r.ga * r.rstd
        r.sh = r.be - r.mean * r.sc
        r.z = r.x * r.sc + r.sh
        r.z.v = z.detach()
        r.zunit = (x * sc).abs() + (mean * sc).abs() + be.abs()
        r.band = (z.abs() <= B[path] * U * r.zunit) if act[0] else torch.zeros_like(z, dtype=torch.bool)
        src = (x - mean) * rstd if MUTATION == "mask_from_xh" else z
        r.m, r.m_alt = _mask(src.detach(), act)
    r.g_out = _act(z, act, r.m)
    r.shape = (A, Bn, C, D)
    if _TRACE is not None:
        _TRACE.append(r)
    return r


def _coef_out(r):
    """[scale | shift | mean | rstd], each flattened over (a, c)."""
    A, _, C, _ = r.shape
    parts = [t.expand(A, 1, C, 1).reshape(-1) for t in (r.sc, r.sh, r.mean, r.rstd)]
    return Out(_cat(parts).v, _cat(parts).s, "coef")


def _fwd_out(r):
    out = r.z * T(r.m)
    return Out(r.g_out, out.s, "out", alt=torch.where(r.band, r.z.v * r.m_alt, r.g_out.detach()), either=r.band)


def _first_backward(r, g, wrt, create_graph=False):
    """Values by autograd of the forward graph with upstream g; scales by the closed formula in T.
    Band elements (j: the kernel may take the other mask): dz_j moves by d_j = |g_j| |m_alt - m|.  That moves
      sum dz by d_j, sum dz xh by d_j |xh_j|  (the slack of dbeta / dgamma / rowsums / dsb),
      k1 by d_j / n, k2 by d_j |xh_j| / n'  (the slack of k),
      and dx_i = scale (dz_i - k1 - xh_i k2) of every i of the statistics group by
      |scale| (d_j / n + |xh_i| d_j |xh_j| / n'),
      and dx_j itself by scale g_j (m_alt - m): the `alt` of dx."""
    r.grads = torch.autograd.grad(r.g_out, wrt, g, create_graph=create_graph, allow_unused=True)
    with torch.no_grad():
        r.g = T(g)
        r.dz = r.g * T(r.m)
        r.xh = (r.x - r.mean) * r.rstd
        r.S1, r.S2 = r.dz.sum(RED), (r.dz * r.xh).sum(RED)
        n, nk = r.n, r.nk
        if MUTATION == "k_whole_count":
            n, nk = n * r.shape[0], nk * r.shape[0]
        r.k1, r.k2 = r.S1 / n, r.S2 / nk
        r.dx = r.sc * (r.dz - r.k1 - r.xh * r.k2)
        r.delta = torch.where(r.band, g.abs() * (r.m_alt - r.m).abs(), torch.zeros_like(g))
        r.sl1, r.sl2 = r.delta.sum(RED, keepdim=True), (r.delta * r.xh.v.abs()).sum(RED, keepdim=True)
        r.dx_slack = r.sc.v.abs() * (r.sl1 / n + r.xh.v.abs() * r.sl2 / nk)
        r.dx_shift = r.sc.v * g * (r.m_alt - r.m)            # dx_j with the other mask, less dx_j
        r.dx_value = r.dx.v if MUTATION == "k_whole_count" else r.grads[0]
        if r.dx_value is not None and r.dx_value.numel() == r.dx.v.numel():
            r.dx_value = r.dx_value.reshape(r.shape)
    return r


def _dx_out(r):
    v = r.dx_value.detach()
    return Out(v, r.dx.s, "dx", alt=torch.where(r.band, v + r.dx_shift, v), slack=r.dx_slack, either=r.band)


def _k_out(r):
    A, _, C, _ = r.shape
    k = _cat([r.k1.reshape(-1), r.k2.reshape(-1)])
    return Out(k.v, k.s, "k", slack=torch.cat([(r.sl1 / r.n).reshape(-1), (r.sl2 / r.nk).reshape(-1)]))


# ---------------------------------------------------------------------------
# row cases
# ---------------------------------------------------------------------------
def _row_affine(d, apr, N, C, leaf=False):
    ga, be = (d["gamma_r"], d["beta_r"]) if apr else (d["gamma_c"], d["beta_c"])
    if leaf:
        ga, be = ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    shape = (N, 1, C, 1) if apr else (1, 1, C, 1)
    return ga, be, ga.reshape(shape), be.reshape(shape)


def ref_rownorm_fwd(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("fwd", N, C, inner), dt), {}
    for apr, unb, act in nc.switches(N, C, inner, nc.FWD_FULL, nc.FWD_FEW):
        _, _, ga, be = _row_affine(d, apr, N, C)
        r = _forward(d["x"].view(N, 1, C, inner), ga, be, EPS, unb, ACTS[act], dt, "twopass", "row")
        tag = "apr%d_unb%d_%s" % (apr, unb, act)
        res[tag + "/coef"], res[tag + "/out"] = _coef_out(r), _shaped(_fwd_out(r), (N, C, inner))
    return res


def _shaped(o, shape):
    for name in ("value", "scale", "alt", "slack", "either"):
        a = getattr(o, name)
        if a is not None:
            setattr(o, name, np.ascontiguousarray(a).reshape(shape))
    return o


def ref_rownorm_stats(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("stats", N, C, inner), dt), {}
    for apr, unb in nc.switches(N, C, inner, nc.STATS_FULL, nc.STATS_FEW):
        _, _, ga, be = _row_affine(d, apr, N, C)
        r = _forward(d["x"].view(N, 1, C, inner), ga, be, EPS, unb, ACTS["none"], dt, "twopass", "row")
        res["apr%d_unb%d/coef" % (apr, unb)] = _coef_out(r)
    return res


def _row_backward(d, N, C, inner, apr, unb, act, dt, second=False):
    x = d["x"].clone().requires_grad_(True)
    ga_l, be_l, ga, be = _row_affine(d, apr, N, C, leaf=True)
    r = _forward(x.view(N, 1, C, inner), ga, be, EPS, unb, ACTS[act], dt, "twopass", "row")
    g = d["g"].view(N, 1, C, inner)
    if second:
        g = g.clone().requires_grad_(True)
    _first_backward(r, g, [x, ga_l, be_l], create_graph=second)
    r.leaves = (x, ga_l, be_l, g)
    return r


def _affine_out(r, per_row, acc_gamma=None, acc_beta=None):
    """(dgamma, dbeta): sum dz xh and sum dz per row, or per channel over the samples; + the seeded accumulators."""
    A, _, C, _ = r.shape
    outs = []
    for S, sl, grad, acc in ((r.S2, r.sl2, r.grads[1], acc_gamma), (r.S1, r.sl1, r.grads[2], acc_beta)):
        if not per_row:
            S, sl = S.sum((0,)), sl.sum((0,), keepdim=True)
        S, sl, v = S.reshape(-1), sl.reshape(-1), grad.detach().reshape(-1)
        if acc is not None and MUTATION != "ignore_accumulate":
            S, v = S + T(acc), v + acc
        outs.append(Out(v, S.s, "affine", slack=sl))
    return outs


def ref_norm_act_bwd_rows_form(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("bwd", N, C, inner), dt), {}
    for apr, unb, act, with_dx in nc.switches(N, C, inner, nc.BWD_FULL, nc.BWD_FEW):
        r = _row_backward(d, N, C, inner, min(apr, 1), unb, act, dt)
        dgamma, dbeta = _affine_out(r, apr != 0)
        tag = "apr%d_unb%d_%s_dx%d" % (apr, unb, act, with_dx)
        if apr == 2:        # packed [N][dgamma C | dbeta C]
            def pack(a, b):
                return np.concatenate([a.reshape(N, C), b.reshape(N, C)], 1).reshape(-1)
            res[tag + "/dgamma"] = Out(pack(dgamma.value, dbeta.value), pack(dgamma.scale, dbeta.scale), "affine",
                                       slack=pack(dgamma.slack, dbeta.slack))
        else:
            res[tag + "/dgamma"], res[tag + "/dbeta"] = dgamma, dbeta
        if with_dx:
            res[tag + "/dx"] = _shaped(_dx_out(r), (N, C, inner))
    return res


def ref_rownorm_bwd_acc(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("acc", N, C, inner), dt), {}
    for acc in (0, 1):
        for act in (ACTS if nc.small(N, C, inner) else ["lrelu"]):
            r = _row_backward(d, N, C, inner, 0, 0, act, dt)
            tag = "acc%d_%s" % (acc, act)
            res[tag + "/dgamma"], res[tag + "/dbeta"] = _affine_out(
                r, False, d["acc_gamma"][:C] if acc else None, d["acc_beta"][:C] if acc else None)
            res[tag + "/dx"] = _shaped(_dx_out(r), (N, C, inner))
    return res


def ref_rownorm_bwd_rows(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("rows", N, C, inner), dt), {}
    for act in (ACTS if nc.small(N, C, inner) else ["relu"]):
        r = _row_backward(d, N, C, inner, 0, 0, act, dt)
        res[act + "/dx"] = _shaped(_dx_out(r), (N, C, inner))
        sums = T(torch.stack([r.S1.v.reshape(-1), r.S2.v.reshape(-1)], 1),
                 torch.stack([r.S1.s.reshape(-1), r.S2.s.reshape(-1)], 1))
        res[act + "/rowsums"] = Out(sums.v, sums.s, "k", slack=torch.stack([r.sl1.reshape(-1), r.sl2.reshape(-1)], 1))
    return res


def _second_backward(r, v):
    """gz_rownorm_act_bwd2: values by autograd through the first backward's dx contracted with v; scales by the closed
    formula of the kernel header in T.  With d_j as in _first_backward (sums over the row, n its length):
      gg_out_i = m_i scale pv_i, pv = v - mean(v) - xh mean(v xh), depends on no other mask: `alt` only;
      t1 = mean(v dz) - mean(v) mean(dz) - c mvx moves by d_j pv_j / n, c = mean(dz xh) by d_j xh_j / n, mean(dz) by
      d_j / n, hence gx_i = -scale rstd (xh_i t1 + c pv_i + mvx (dz_i - mean(dz) - xh_i c)) moves by at most
      |scale rstd| (|xh_i| S1 + |pv_i| S2 + |mvx| (S3 + |xh_i| S2)) / n with S1 = sum d |pv|, S2 = sum d |xh|, S3 = sum d,
      and gx_j itself by -scale rstd mvx g_j (m_alt - m): its `alt`;
      ggamma_c = sum_n rstd n t1 moves by sum_n rstd S1."""
    x, ga_l, _, g = r.leaves
    L = (r.grads[0].reshape(r.shape) * v).sum()
    gg, gx, gga = torch.autograd.grad(L, [g, x, ga_l])
    gg, gx = gg.reshape(r.shape), gx.reshape(r.shape)
    with torch.no_grad():
        n, vT, m = r.n, T(v), T(r.m)
        mv, mg, c = vT.sum(RED) / n, r.dz.sum(RED) / n, (r.dz * r.xh).sum(RED) / n
        mvx, mvg = (vT * r.xh).sum(RED) / n, (vT * r.dz).sum(RED) / n
        t1 = mvg - mv * mg - c * mvx
        pv = vT - mv - r.xh * mvx
        ggT = (m * r.sc) * pv
        gxT = -((r.sc * r.rstd) * (r.xh * t1 + c * pv + mvx * (r.dz - mg - r.xh * c)))
        ggaT = (r.rstd * (t1 * n)).sum((0,))
        S1 = (r.delta * pv.v.abs()).sum(RED, keepdim=True)
        S2, S3 = r.sl2, r.sl1
        srs = (r.sc.v * r.rstd.v)
        gx_slack = srs.abs() * (r.xh.v.abs() * S1 + pv.v.abs() * S2 + mvx.v.abs() * (S3 + r.xh.v.abs() * S2)) / n
        gx_alt = torch.where(r.band, gx - srs * mvx.v * r.g.v * (r.m_alt - r.m), gx)
        gg_alt = torch.where(r.band, r.m_alt * r.sc.v * pv.v, gg.reshape(r.shape))
        gga_slack = (r.rstd.v * S1).sum((0,))
    return (Out(gg.reshape(r.shape), ggT.s, "bwd2", alt=gg_alt, either=r.band),
            Out(gx.reshape(r.shape), gxT.s, "bwd2", alt=gx_alt.reshape(r.shape), slack=gx_slack, either=r.band),
            Out(gga.reshape(-1), ggaT.s.reshape(-1), "bwd2", slack=gga_slack.reshape(-1)))


def ref_rownorm_bwd2(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("bwd2", N, C, inner), dt), {}
    for act in (ACTS if nc.small(N, C, inner) else ["lrelu"]):
        r = _row_backward(d, N, C, inner, 0, 0, act, dt, second=True)
        gg, gx, gga = _second_backward(r, d["v"].view(N, 1, C, inner))
        res[act + "/gg_out"], res[act + "/gx"] = _shaped(gg, (N, C, inner)), _shaped(gx, (N, C, inner))
        res[act + "/ggamma"] = gga
    return res


def ref_rownorm_sigma(N, C, inner, dt=F64):
    d, res = _inputs(nc.rows_host("sigma", N, C, inner), dt), {}
    for groups in (1, 2):
        sigma = _t(nc.f32(nc.SIGMAS[:groups]), dt)
        eps = (torch.tensor(EPS, dtype=dt) * sigma * sigma).repeat_interleave(N // groups).view(N, 1, 1, 1).double()
        r = _forward(d["x"].view(N, 1, C, inner), None, None, eps, 0, ACTS["lrelu"], dt, "twopass", "row")
        res["groups%d_lrelu/coef" % groups] = _coef_out(r)
        res["groups%d_lrelu/out" % groups] = _shaped(_fwd_out(r), (N, C, inner))
    return res


def ref_adain_const(N, C, inner, dt=F64):
    """AdaIN of the shared [C][inner] constant = AdaIN (unbiased variance) of its repeat over the samples; the gradient
    of the constant is the sum over the samples, which autograd takes through the expand."""
    d, res = _inputs(nc.adain_host(N, C, inner), dt), {}
    for act in ("relu", "lrelu"):
        x0, sb = d["x"].clone().requires_grad_(True), d["sb"].clone().requires_grad_(True)
        ga, be = sb[:, :C].reshape(N, 1, C, 1), sb[:, C:].reshape(N, 1, C, 1)
        r = _forward(x0.view(1, 1, C, inner).expand(N, 1, C, inner), ga, be, EPS, 1, ACTS[act], dt, "twopass", "row")
        res[act + "/coef"], res[act + "/out"] = _coef_out(r), _shaped(_fwd_out(r), (N, C, inner))
        rc = nc.GZ_ERR_UNSUPPORTED if inner > 1024 else 0
        res[act + "/bwd_rc"] = Out(np.array([rc], dtype=np.int64))
        if rc == 0:
            _first_backward(r, d["g"].view(N, 1, C, inner), [x0, sb])
            # dx[c] = sum_n dx[n, c]: the scales add, and a band element's own move joins the slack of its sum
            slack = (r.dx_slack + torch.where(r.band, r.dx_shift.abs(), torch.zeros_like(r.dx_shift))).sum(0)
            res[act + "/dx"] = Out(r.grads[0], r.dx.s.sum(0).reshape(C, inner), "dx", slack=slack.reshape(C, inner))
            S = T(torch.cat([r.S2.v.reshape(N, C), r.S1.v.reshape(N, C)], 1),
                  torch.cat([r.S2.s.reshape(N, C), r.S1.s.reshape(N, C)], 1))
            res[act + "/dsb"] = Out(r.grads[1], S.s, "affine",
                                    slack=torch.cat([r.sl2.reshape(N, C), r.sl1.reshape(N, C)], 1))
    return res


ref_adain_const_too_long = ref_adain_const


# ---------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------
def _running_out(r, rm, rv, groups):
    """rm <- (1 - m) rm + m mean, rv <- (1 - m) rv + m var cnt / (cnt - 1), group after group."""
    rm, rv = T(rm.reshape(1, 1, -1, 1)), T(rv.reshape(1, 1, -1, 1))
    unb = 1.0 if MUTATION == "running_var_biased" else r.n / (r.n - 1.0)
    for g in range(groups):
        mean = T(r.mean.v[g:g + 1].to(rm.v.dtype), r.mean.s[g:g + 1].to(rm.v.dtype))
        var = T(r.var_biased.v[g:g + 1].to(rm.v.dtype), r.var_biased.s[g:g + 1].to(rm.v.dtype))
        rm = rm * (1.0 - MOMENTUM) + mean * MOMENTUM
        rv = rv * (1.0 - MOMENTUM) + var * unb * MOMENTUM
    return (Out(rm.v.reshape(-1), rm.s.reshape(-1), "running"), Out(rv.v.reshape(-1), rv.s.reshape(-1), "running"),
            Out(np.array([nc.NBT0 + groups], dtype=np.int64)))


def _bn_run(d, N, C, inner, groups, part, act, affine, dt, partials=None, count=None):
    x = d["x"].clone().requires_grad_(True)
    ga_l = (d["gamma"] if affine else torch.ones(C, dtype=dt)).clone().requires_grad_(True)
    be_l = (d["beta"] if affine else torch.zeros(C, dtype=dt)).clone().requires_grad_(True)
    p = d["partials"].reshape(groups, 2 * N // groups, C, 2) if part else None
    r = _forward(x.view(groups, N // groups, C, inner), ga_l.view(1, 1, C, 1), be_l.view(1, 1, C, 1), EPS, 0, ACTS[act],
                 dt, "sums", "bn", partials=p, count=(N // groups) * inner)
    r.leaves = (x, ga_l, be_l)
    return r


def _bn_bwd(r, d, N, C, inner, groups, acc, with_dx, tag, res):
    _first_backward(r, d["g"].view(groups, N // groups, C, inner), list(r.leaves))
    res[tag + "/dgamma"], res[tag + "/dbeta"] = _affine_out(r, False, d["acc_gamma"] if acc else None,
                                                            d["acc_beta"] if acc else None)
    res[tag + "/k"] = _k_out(r)
    if with_dx:
        res[tag + "/dx"] = _shaped(_dx_out(r), (N, C, inner))


def _bn_fwd(r, d, N, C, inner, groups, run, tag, res):
    res[tag + "/coef"], res[tag + "/out"] = _coef_out(r), _shaped(_fwd_out(r), (N, C, inner))
    if run:
        res[tag + "/running_mean"], res[tag + "/running_var"], res[tag + "/nbt"] = _running_out(r, d["rm"], d["rv"], groups)


def ref_bn_fused(N, C, H, W, dt=F64):
    inner, res = H * W, {}
    d = _inputs(nc.bn_inputs_host("fused", N, C, inner), dt)
    for groups, part, run, act, affine, with_dx in nc.bn_fused_switches():
        r = _bn_run(d, N, C, inner, groups, part, act, affine, dt)
        tag = "groups%d_part%d_run%d_%s" % (groups, part, run, act)
        _bn_fwd(r, d, N, C, inner, groups, run, tag, res)
        _bn_bwd(r, d, N, C, inner, groups, run, with_dx, tag, res)
    return res


def ref_bn_stats_apply(N, C, H, W, dt=F64):
    inner, res = H * W, {}
    d = _inputs(nc.bn_inputs_host("stats", N, C, inner), dt)
    for groups in nc.switches(N, C, inner, (1, 2), (2,)):
        r = _bn_run(d, N, C, inner, groups, 0, "lrelu", True, dt)
        tag = "groups%d_lrelu" % groups
        _bn_fwd(r, d, N, C, inner, groups, True, tag, res)
        _bn_bwd(r, d, N, C, inner, groups, groups - 1, True, tag, res)
    return res


def ref_bn_functional(N, C, H, W, dt=F64):
    inner, res = H * W, {}
    d = _inputs(nc.bn_inputs_host("functional", N, C, inner), dt)
    for groups in (1, 2):
        for part in (0, 1):
            r = _bn_run(d, N, C, inner, groups, part, "relu", True, dt)
            tag, full = "groups%d_part%d_relu" % (groups, part), {}
            _bn_fwd(r, d, N, C, inner, groups, True, tag, full)
            _bn_bwd(r, d, N, C, inner, groups, 0, True, tag, full)
            for k, o in full.items():
                if k.split("/")[1] not in ("coef", "k"):
                    res[k] = _shaped(o, (N, C, H, W)) if k.split("/")[1] in ("out", "dx") else o
    return res


def ref_bn_eval_coef(N, C, H, W, dt=F64):
    """rstd = 1 / sqrt(running_var + eps) (one rounding of each step: kappa = 1), scale = gamma rstd,
    shift = beta - running_mean scale, mean = running_mean."""
    d = _inputs(nc.bn_inputs_host("eval", N, C, H * W), dt)
    rstd = T((d["rv"] + EPS).rsqrt())
    sc = T(d["gamma"]) * rstd
    sh = T(d["beta"]) - T(d["rm"]) * sc
    c = _cat([sc, sh, T(d["rm"]), rstd])
    return {"plain/coef": Out(c.v, c.s, "coef")}


def ref_bn_finalize(rows, groups, dt=F64):
    """gz_batchnorm_finalize_g: everything from the partial rows [rows][C][2], (rows / groups) * per elements a group."""
    C, per = nc.FINALIZE_C, nc.FINALIZE_PER
    d = _inputs(nc.finalize_host(rows, groups), dt)
    Rg = rows // groups
    # only the partial sums exist: a stand-in x carries no values (every value comes from the partials)
    x = torch.zeros(groups, 1, C, 1, dtype=dt)
    r = _forward(x, d["gamma"].view(1, 1, C, 1), d["beta"].view(1, 1, C, 1), EPS, 0, ACTS["none"], dt, "sums", "bn",
                 partials=d["partials"].reshape(groups, Rg, C, 2), count=Rg * per)
    res = {"plain/coef": _coef_out(r)}
    res["plain/running_mean"], res["plain/running_var"], res["plain/nbt"] = _running_out(r, d["rm"], d["rv"], groups)
    return res


def ref_channel_sum(N, C, inner, dt=F64):
    x = T(_t(nc.channel_sum_host(N, C, inner)["x"], dt))
    s = x.sum((0, 2), keepdim=False)
    return {"plain/out": Out(s.v, s.s, "affine")}


def ref_elementwise(count, dt=F64):
    """gz_act_bwd: dx = g act'(.) through the OUTPUT (out > 0 ? 1 : slope; tanh: 1 - out^2); the inputs are exact, so
    no mask is in doubt.  gz_tanh_bwd2: res = v g (-2 out)."""
    d, res = _inputs(nc.elementwise_host(count), dt), {}
    g, v, out = T(d["g"]), T(d["v"]), T(d["out"])
    one = T(torch.ones_like(out.v))
    for name, act in nc.elementwise_acts(count):
        if name == "tanh":
            dx = g * (one - out * out)
        else:
            lo = {"none": 1.0, "relu": 0.0, "lrelu": act[1]}[name]
            dx = g * T(torch.where(out.v > 0, torch.ones_like(out.v), torch.full_like(out.v, lo)))
        res["act_bwd_" + name + "/dx"] = Out(dx.v, dx.s, "ew")
    y = v * g * (out * -2.0)
    res["tanh_bwd2/res"] = Out(y.v, y.s, "ew")
    return res


REFERENCE = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("ref_")}


@functools.lru_cache(maxsize=None)
def reference(fn_name, args):
    """The fp64 reference of one case, computed once (the callers leave it unchanged)."""
    return REFERENCE[fn_name](*args)


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def ratios(got, ref, Kk=None):
    """(|got - ref| - slack) / (K u scale) per element, the better of value and alt; inf where scale is 0 and the word
    differs, or where got is not finite."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.value.shape)
    Kk = K[ref.kind] if Kk is None else Kk

    def one(want):
        excess = np.abs(got - want) - (0.0 if ref.slack is None else ref.slack)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(excess <= 0, 0.0, excess / (Kk * U * ref.scale))
        return np.where(np.isfinite(got), q, np.inf)
    q = one(ref.value)
    if ref.alt is not None:
        q = np.minimum(q, one(ref.alt))
    return q


def compare(got, ref, key="", table=None):
    """[] or one message: the key, the count and the first few positions, values and ratios to tolerance.
    table: the K of another reference module that shares this comparator (tail_reference.py)."""
    got, table = np.asarray(got), K if table is None else table
    if got.size != ref.value.size:
        return ["%s: %d elements against %d" % (key, got.size, ref.value.size)]
    if ref.kind == "int":
        same = got.dtype.kind in "iu" and np.array_equal(got.reshape(-1), ref.value.reshape(-1))
        return [] if same else ["%s: %s against %s" % (key, got.reshape(-1)[:4], ref.value.reshape(-1)[:4])]
    q = ratios(got, ref, table[ref.kind])
    bad = np.argwhere(~(q <= 1.0))
    if not bad.size:
        return []
    at = tuple(bad[:4].T)
    return ["%s: %d of %d beyond K = %d (%s), first at %s: got %s, reference %s, ratio to tolerance %s"
            % (key, len(bad), q.size, table[ref.kind], ref.kind, bad[:4].tolist(), got.reshape(ref.value.shape)[at],
               ref.value[at], q[at])]


def worst(got, ref, table=None):
    return 0.0 if ref.kind == "int" else float(ratios(got, ref, (K if table is None else table)[ref.kind]).max())


# ---------------------------------------------------------------------------
# --measure
# ---------------------------------------------------------------------------
def all_cases():
    """(driver name, args) of every case of the default list and of the experiment settings, once each."""
    import test_norm_parent_bits_gpu as bits
    cases = [(fn.__name__.lstrip("_"), args) for _, fn, args in bits.CASES]
    for _, (_, extra) in bits.SETTINGS.items():
        cases += [(fn.__name__.lstrip("_"), args) for _, fn, args in extra]
    return list(dict.fromkeys(cases))


def _pow2_ceil(v):
    return int(2 ** int(np.ceil(np.log2(max(v, 1e-30)))))


def measure_z(cases):
    """B: the float32 replay's error in z over u (|x scale| + |mean scale| + |beta|), per path."""
    global _TRACE
    worst_z = {"row": 0.0, "bn": 0.0}
    try:
        for name, args in cases:
            if name in ("bn_eval_coef", "bn_finalize", "channel_sum", "elementwise"):       # (no z)
                continue
            _TRACE = n64 = []
            REFERENCE[name](*args)
            _TRACE = n32 = []
            REFERENCE[name](*args, dt=F32)
            for a, b in zip(n64, n32):
                q = ((b.z.v.double() - a.z.v).abs() / (U * a.zunit)).max().item()
                worst_z[a.path] = max(worst_z[a.path], q)
    finally:
        _TRACE = None
    return worst_z


def measure(cases=None):
    """({kind: largest replay ratio}, {path: largest z ratio}): the float32 replay against the fp64 reference."""
    cases = all_cases() if cases is None else cases
    big = {k: 0.0 for k in K}
    for name, args in cases:
        ref, rep = reference(name, args), REFERENCE[name](*args, dt=F32)
        assert ref.keys() == rep.keys(), name
        for key, o in ref.items():
            if o.kind != "int":
                big[o.kind] = max(big[o.kind], float(ratios(rep[key].value, o, Kk=1.0).max()))
    return big, measure_z(cases)


def constants(big, big_z):
    return {k: _pow2_ceil(4 * v) for k, v in big.items()}, {k: _pow2_ceil(4 * v) for k, v in big_z.items()}


if __name__ == "__main__":
    assert sys.argv[1:] == ["--measure"], "usage: python tests/norm_reference.py --measure"
    # B first (the band decides which elements count as `either` when K is measured), then K with that B
    _z = measure_z(all_cases())
    B.update(constants({}, _z)[1])
    _big, _z = measure()
    _K, _B = constants(_big, _z)
    print("MEASURED =", {k: round(v, 3) for k, v in _big.items()})
    print("K =", _K)
    print("MEASURED_Z =", {k: round(v, 3) for k, v in _z.items()})
    print("B =", _B)

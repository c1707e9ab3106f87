"""An fp64 reference for the kernels that close every training step (csrc/gz_optim.hip, csrc/gz_loss.hip): CPU only, no
import of the library.  Conventions, comparator and error arithmetic are those of norm_reference.py (`Out`, `T`,
`compare` are imported from there); read its header first.

For each driver of test_tail_fp64_gpu.py (``_adam`` ...) there is a twin here (``REFERENCE["adam"]`` ...) that takes the
same arguments, reads the same seeded host inputs (tail_cases.py) and returns the same keys.  The operations are written
as formulas in torch float64, not as the kernels spell them, from the float32 host inputs and the scalars AS THE C ABI
RECEIVES THEM: lr, beta1, beta2, eps, alpha and grad_scale rounded to float32 first (tail_cases.c32); the step count is
an integer and the bias corrections 1 - beta^t are formed in double from the float32 betas.

    Adam       gv = g gs;  m' = m + (gv - m)(1 - b1);  v' = b2 v + (1 - b2) gv^2;
               p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    RMSprop    v' = a v + (1 - a) gv^2;  p' = p - lr gv / (sqrt(v') + eps)
    tick       {t, 1 - b1^t, sqrt(1 - b2^t)} after k ticks
    slabs      g = the sum of all slabs of all sources (exact in any order: tail_cases.slab_host), then Adam
    BCE        mean(max(x, 0) - x t + log(1 + exp(-|x|))),  dx = (sigmoid(x) - t) gup / n
    MSE        mean((a - b)^2),  da = 2 (a - b) gup / n
    GP         mean((sqrt(s) - 1)^2),  ds = (sqrt(s) - 1) / sqrt(s) gup / n, exactly 0 at s == 0
    vectors    x / max(||x||, eps), ||x||, <x / max(||x||, eps), x>;  <a, b>;  x / sigma
    power      v = normalize(W^T u), u = normalize(W v), sigma = u . (W v)
    sn bwd     dW = (G - (sum rowdots) u v^T) / sigma
    sigma term term[r][l] = sum_g c_g u[g][r] v[g][l],  c_g = -eps sigma_g sum_{rows of g} rstd_row^2 S2_row,
               S2_row the SECOND float of the row's pair in rowsums

Comparison:   |got_i - value_i| <= K[kind] * u * scale_i,   u = 2^-24, no slack and no element excused.  scale_i comes
from running the formula in the error arithmetic `T` (sums of magnitudes; sqrt and quotient to first order).  One term
is added to every scale that is not 0:

    TINY = 2^-126, the smallest normal float32.  Below it a float32 result is a multiple of 2^-149 and its rounding
    error is up to 2^-150 = u TINY whatever its size, so a relative bound cannot hold there; the gradient of BCE at a
    logit of -90 against target 0, sigmoid(-90) gup / n = 8e-40 gup / n, is such a result.

A scale of 0 (a word the entry point must not change, a result that is exactly 0, the step count) means bit for bit;
gradients after the optimizer (unchanged, or exactly zero with zero_grads) are kind "int": the float32 bit patterns.

K is MEASURED, not chosen: `python tests/tail_reference.py --measure` replays every case with this same code in float32
on the CPU (plain torch; the constants rounded where the kernels round them; sums pairwise by element-wise additions,
so that the figures do not depend on the host) and prints, per kind, the largest
|replay - reference| / (u scale); K = 4 x that, rounded up to a power of two (4: another order of summation, and the
device's expf / log1pf / pow in place of the host's).  The table below is that output; test_tail_reference_cpu.py
re-derives it.  K is never taken from a GPU result."""
import contextlib
import functools
import math
import sys

import numpy as np
import torch

import tail_cases as tc
from norm_reference import F32, F64, Out, T, ratios
from norm_reference import compare as _compare
from norm_reference import worst as _worst

TINY = 2.0 ** -126

# --measure (CPU replay in float32 against this reference, all cases): largest ratio -> K
MEASURED = {'adam': 3.183, 'tick': 0.465, 'loss': 1.993, 'lossgrad': 2.163, 'vec': 1.296, 'power': 2.174,
            'sigma_term': 4.089}
K = {'adam': 16, 'tick': 2, 'loss': 8, 'lossgrad': 16, 'vec': 8, 'power': 16, 'sigma_term': 32}

MUTATION = None             # test_tail_reference_cpu.py: a deliberately wrong reference (mutated())
MUTATIONS = ("lerp_weight_beta1", "eps_inside_sqrt", "bc2_without_sqrt", "bias_correction_of_previous_step",
             "grad_scale_on_m_only", "tail_unstepped", "sigma_from_old_u", "v_norm_one_block", "sigma_term_sign",
             "rowsums_first_float", "coef_slice_dropped", "gp_grad_nonzero_at_zero")


@contextlib.contextmanager
def mutated(name):
    global MUTATION
    assert name in MUTATIONS, name
    MUTATION = name
    try:
        yield
    finally:
        MUTATION = None


def compare(got, ref, key=""):
    return _compare(got, ref, key, table=K)


def worst(got, ref):
    return _worst(got, ref, table=K)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _k(c, dt):
    """A constant as a T (magnitude |c|)."""
    return T(torch.tensor(c, dtype=dt))


def _c(x, dt):
    """A derived constant: the replay rounds it to float32 where the kernels hold it as a float."""
    return float(np.float32(x)) if dt == F32 else float(x)


def _o(t, kind, shape=None):
    v, s = t.v.double(), t.s.double()
    s = torch.where(s > 0, s + TINY, torch.zeros_like(s))
    if shape is not None:
        v, s = v.reshape(shape), s.reshape(shape)
    return Out(v, s, kind)


def bits(a):
    """float32 words as integers (kind "int": compared exactly)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.int64)


def _cat(ts):
    return T(torch.cat([t.v.reshape(-1) for t in ts]), torch.cat([t.s.reshape(-1) for t in ts]))


def _sum(t, dim):
    """The sum over one dimension.  The float32 replay adds neighbours pairwise, level by level, with element-wise
    additions only: those round the same on every host, where the order of torch.sum is the host's vector unit's."""
    if t.v.dtype == F64:
        return t.sum((dim,), keepdim=False)
    x = t.v.movedim(dim, -1)
    while x.shape[-1] > 1:
        n = x.shape[-1]
        y = x[..., 0:n - n % 2:2] + x[..., 1:n:2]
        x = torch.cat([y, x[..., n - 1:]], -1) if n % 2 else y
    return T(x[..., 0], t.s.sum(dim))


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------
def _keep_tail(new, old, n):
    """tail_unstepped: the last n % 4 elements keep their old value."""
    if MUTATION == "tail_unstepped" and n % 4:
        new.v[n - n % 4:] = old.v[n - n % 4:]
    return new


def _adam_one(d, g, lr, b1, b2, eps, t, gs, dt):
    """(p', m', v') of one tensor; g: the float32 gradient (host array)."""
    tb = t - 1 if MUTATION == "bias_correction_of_previous_step" and t > 1 else t
    bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
    step_size = float(np.float32(lr) / np.float32(bc1)) if dt == F32 else lr / bc1
    bc2s = _c(bc2 if MUTATION == "bc2_without_sqrt" else math.sqrt(bc2), dt)
    P, G, M, V = (T(_t(a, dt)) for a in (d["p"], g, d["m"], d["v"]))
    gv = G * gs
    gvv = G if MUTATION == "grad_scale_on_m_only" else gv
    m1 = M + (gv - M) * _c(b1 if MUTATION == "lerp_weight_beta1" else 1.0 - b1, dt)
    v1 = V * b2 + (gvv * gvv) * _c(1.0 - b2, dt)
    if MUTATION == "eps_inside_sqrt":
        denom = (v1 + _k(eps, dt)).sqrt() / bc2s
    else:
        denom = v1.sqrt() / bc2s + _k(eps, dt)
    p1 = P - (m1 / denom) * step_size
    n = P.v.numel()
    return _keep_tail(p1, P, n), _keep_tail(m1, M, n), _keep_tail(v1, V, n)


def _rmsprop_one(d, lr, alpha, eps, gs, dt):
    P, G, V = (T(_t(d[k], dt)) for k in ("p", "g", "v"))
    gv = G * gs
    v1 = V * alpha + (gv * gv) * _c(1.0 - alpha, dt)
    p1 = P - (gv / (v1.sqrt() + _k(eps, dt))) * lr
    return p1, v1


def _grad_bits(tensors, zg):
    g = np.concatenate([d["g"] for d in tensors])
    return Out(bits(np.zeros_like(g) if zg else g))


def _adam_outs(tensors, tag, sw, dt, res):
    b1, b2, t, gs, zg = sw
    steps = [_adam_one(d, d["g"], tc.c32(tc.ADAM_LR), tc.c32(b1), tc.c32(b2), tc.c32(tc.ADAM_EPS), t, tc.c32(gs), dt)
             for d in tensors]
    for i, name in enumerate("pmv"):
        res["%s/%s" % (tag, name)] = _o(_cat([s[i] for s in steps]), "adam")
    res[tag + "/g"] = _grad_bits(tensors, zg)


def opt_tensors(layout):
    return [tc.opt_tensor_host(layout, k, n) for k, n in enumerate(tc.opt_numels(layout))]


def ref_adam(entry, layout, dt=F64):
    """gz_adam_step / gz_adam_step_dev: outputs concatenated over the tensors of the layout, per switch setting."""
    tensors, res = opt_tensors(layout), {}
    for sw in tc.adam_switches():
        _adam_outs(tensors, tc.adam_tag(*sw), sw, dt, res)
    return res


def ref_rmsprop(layout, dt=F64):
    tensors, res = opt_tensors(layout), {}
    lr, alpha, eps = tc.c32(tc.RMSPROP_LR), tc.c32(tc.RMSPROP_ALPHA), tc.c32(tc.RMSPROP_EPS)
    for gs, zg in tc.rmsprop_switches():
        steps = [_rmsprop_one(d, lr, alpha, eps, tc.c32(gs), dt) for d in tensors]
        tag = "gs%g_zg%d" % (gs, zg)
        res[tag + "/p"], res[tag + "/v"] = _o(_cat([s[0] for s in steps]), "adam"), _o(_cat([s[1] for s in steps]), "adam")
        res[tag + "/g"] = _grad_bits(tensors, zg)
    return res


TICK_DEV_SWITCH = (0.5, 1)      # (grad_scale, zero_grads) of the gz_adam_step_dev that follows the ticks


def _tick(b1, b2, t, dt):
    """{t, 1 - b1^t, sqrt(1 - b2^t)}: the count exact, the corrections with the magnitudes of their terms."""
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    v = torch.tensor([t, bc1, math.sqrt(bc2)], dtype=F64)
    s = torch.tensor([0.0, 1.0 + b1 ** t, (1.0 + b2 ** t) / (2.0 * math.sqrt(bc2))], dtype=F64)
    return _o(T(v.to(dt), s), "tick")


def ref_tick(b1, b2, dt=F64):
    """gz_adam_tick five times from {0, 0, 0}, then gz_adam_step_dev at t = 5; once from {999, ., .}, then at t = 1000."""
    f1, f2, res = tc.c32(b1), tc.c32(b2), {}
    for k in range(1, 6):
        res["from0/k%d" % k] = _tick(f1, f2, k, dt)
    res["from999/k1"] = _tick(f1, f2, 1000, dt)
    for t in (5, 1000):
        _adam_outs(opt_tensors("tick"), "dev%d" % t, (b1, b2, t) + TICK_DEV_SWITCH, dt, res)
    return res


def ref_slabs(dt=F64):
    """gz_adam_step_from_slabs on twelve parameters: the gradient is the exact sum of the slabs."""
    params = [(tc.slab_host(k, n, nzs), n) for k, (n, nzs) in enumerate(tc.slab_params())]
    grads = [np.sum([s[:, :n].astype(np.float64).sum(0) for s in d["slabs"]], 0) for d, n in params]
    for g in grads:
        assert np.array_equal(g, g.astype(np.float32).astype(np.float64))
    res = {}
    for b1, b2, t, gs in tc.slab_switches():
        steps = [_adam_one(d, tc.f32(g), tc.c32(tc.ADAM_LR), tc.c32(b1), tc.c32(b2), tc.c32(tc.ADAM_EPS), t,
                           tc.c32(gs), dt) for (d, _), g in zip(params, grads)]
        for i, name in enumerate("pmv"):
            res["b%g_%g_t%d_gs%g/%s" % (b1, b2, t, gs, name)] = _o(_cat([s[i] for s in steps]), "adam")
    return res


# ---------------------------------------------------------------------------
# loss tails
# ---------------------------------------------------------------------------
def _own(v):
    """A transcendental's value: known to its own rounding."""
    return T(v)


def _bce_terms(x, t):
    X = T(x)
    return T(x.clamp_min(0)) - X * t + _own(torch.log1p(torch.exp(-x.abs())))


def _sigmoid(x, dt):
    """1 / (1 + e^-x) for x >= 0 and e^x / (1 + e^x) below: neither branch overflows."""
    e = _own(torch.exp(-x.abs()))
    one = _k(1.0, dt)
    pos, neg = one / (one + e), e / (one + e)
    return T(torch.where(x >= 0, pos.v, neg.v), torch.where(x >= 0, pos.s, neg.s))


def ref_bce(n, dt=F64):
    x = _t(tc.bce_host(n)["x"], dt)
    return {"t%d/loss" % t: _o(_sum(_bce_terms(x, float(t)), 0).reshape(1) / float(n), "loss") for t in (0, 1)}


def ref_mse(n, dt=F64):
    d = tc.mse_host(n)
    diff = T(_t(d["a"], dt)) - T(_t(d["b"], dt))
    return {"loss": _o(_sum(diff * diff, 0).reshape(1) / float(n), "loss")}


def ref_gp(n, dt=F64):
    d = T(_t(tc.gp_host(n)["sumsq"], dt)).sqrt() - _k(1.0, dt)
    return {"loss": _o(_sum(d * d, 0).reshape(1) / float(n), "loss")}


def ref_loss_bwd(n, dt=F64):
    """The three gradients under the upstream factor gup = tail_cases.UPSTREAM."""
    res = {}
    d = tc.bce_host(n)
    x, gup = _t(d["x"], dt), T(_t(d["g"], dt))
    for t in (0, 1):
        res["bce_t%d/dx" % t] = _o((_sigmoid(x, dt) - _k(float(t), dt)) * (gup / float(n)), "lossgrad")
    d = tc.mse_host(n)
    res["mse/da"] = _o((T(_t(d["a"], dt)) - T(_t(d["b"], dt))) * (gup * 2.0 / float(n)), "lossgrad")
    d = tc.gp_host(n)
    s = _t(d["sumsq"], dt)
    r = T(s).sqrt()
    safe = T(torch.where(s > 0, r.v, torch.ones_like(r.v)), r.s)
    ds = ((r - _k(1.0, dt)) / safe) * (gup / float(n))
    at0 = gup.v / float(n) if MUTATION == "gp_grad_nonzero_at_zero" else torch.zeros_like(gup.v)
    ds = T(torch.where(s > 0, ds.v, -at0.expand_as(s)), torch.where(s > 0, ds.s, torch.zeros_like(s)))
    res["gp/ds"] = _o(ds, "lossgrad")
    return res


# ---------------------------------------------------------------------------
# vector operations, x / sigma, the spectral-norm backward
# ---------------------------------------------------------------------------
def _dot(a, b):
    return _sum(a * b, 0)


def _normalize(x, eps, dt, norm_of=None):
    """(x / max(||x||, eps), ||x||); norm_of: the part of x the norm is taken from (a mutation)."""
    part = x if norm_of is None else norm_of
    nrm = _dot(part, part).sqrt()
    den = nrm if float(nrm.v) >= eps else _k(eps, dt)
    return x / den, nrm


def ref_vec(n, dt=F64):
    """gz_vec_normalize and gz_vec_normalize_dot in every mode (both destinations hold the same words), gz_vec_dot."""
    res, eps = {}, tc.c32(tc.SN_EPS)
    for mode in tc.VEC_MODES:
        x = T(_t(tc.vec_host(n, zero=mode == "zero")["x"], dt))
        q, nrm = _normalize(x, eps, dt)
        for entry, last, what in (("normalize", nrm, "norm"), ("normalize_dot", _dot(q, x), "dot")):
            tag = "%s/%s/" % (mode, entry)
            res[tag + "out"] = _o(q, "vec")
            if mode != "no_out2":
                res[tag + "out2"] = _o(q, "vec")
            res[tag + what] = _o(last, "vec", (1,))
    d = tc.vec_host(n)
    res["dot/out"] = _o(_dot(T(_t(d["x"], dt)), T(_t(d["b"], dt))), "vec", (1,))
    return res


def ref_mat(R, L, dt=F64):
    """gz_div_scalar: x / sigma; gz_spectral_norm_bwd: (G - (sum rowdots) u v^T) / sigma with G = x."""
    d = {k: T(_t(v, dt)) for k, v in tc.mat_host(R, L).items()}
    return {"div/out": _o(d["x"] / d["sigma"].reshape(()), "vec"), "snbwd/out": _o(sn_bwd(d), "vec")}


def sn_bwd(d):
    """d: T of x (= G) [R][L], rowdots [R], u [R], v [L], sigma [1]."""
    R, L = d["x"].v.shape
    c = _sum(d["rowdots"], 0)
    uv = (d["u"] * c).reshape(R, 1) * d["v"].reshape(1, L)
    return (d["x"] - uv) / d["sigma"].reshape(())


# ---------------------------------------------------------------------------
# power iteration, sigma term
# ---------------------------------------------------------------------------
def _power_step(W, u, eps, dt):
    R, L = W.v.shape
    vraw = _sum(W * u.reshape(R, 1), 0)
    block = T(vraw.v[:1024], vraw.s[:1024]) if MUTATION == "v_norm_one_block" else None
    v, nv = _normalize(vraw, eps, dt, norm_of=block)
    wv = _sum(W * v.reshape(1, L), 1)
    u1, nu = _normalize(wv, eps, dt)
    sigma = _dot(u if MUTATION == "sigma_from_old_u" else u1, wv)
    return u1, v, sigma, (nv, nu)


def ref_power(R, L, dt=F64, zero=False, norms=None):
    """gz_sn_power_iteration twice on the same buffers: the second starts from the first's u (its magnitudes carried)."""
    d, res, eps = tc.power_host(R, L, zero=zero), {}, tc.c32(tc.SN_EPS)
    W, u = T(_t(d["W"], dt)), T(_t(d["u"], dt))
    for it in (1, 2):
        u, v, sigma, nn = _power_step(W, u, eps, dt)
        if norms is not None:
            norms.extend(nn)
        for name, val in (("u", u), ("us", u), ("v", v), ("vs", v)):
            res["it%d/%s" % (it, name)] = _o(val, "power")
        res["it%d/sigma" % it] = _o(sigma, "power", (1,))
    return res


def ref_power_zero(R, L, dt=F64):
    """W == 0: u, v and sigma are exactly 0 (every scale is 0)."""
    return ref_power(R, L, dt, zero=True)


def ref_sigma_term(groups, rpg, R, L, dt=F64):
    d = {k: T(_t(v, dt)) for k, v in tc.sigma_host(groups, rpg, R, L).items()}
    return {"term": _o(sigma_term(d, groups, rpg, R, L), "sigma_term")}


def sigma_term(d, groups, rpg, R, L, eps=tc.c32(tc.SIGMA_EPS)):
    """d: T of rowsums [rows][2], rstd [rows], sigma [groups], u [groups][R], v [groups][L]; rows = groups * rpg."""
    half = 0 if MUTATION == "rowsums_first_float" else 1
    S2 = T(d["rowsums"].v[:, half], d["rowsums"].s[:, half])
    prod = (d["rstd"] * d["rstd"] * S2).reshape(groups, rpg)
    if MUTATION == "coef_slice_dropped":
        per = (rpg + 15) // 16
        prod = T(prod.v[:, per:], prod.s[:, per:])
    sign = 1.0 if MUTATION == "sigma_term_sign" else -1.0
    c = _sum(prod, 1) * d["sigma"] * (sign * eps)
    term = None
    for g in range(groups):
        cu = T(d["u"].v[g], d["u"].s[g]) * T(c.v[g], c.s[g])
        one = cu.reshape(R, 1) * T(d["v"].v[g], d["v"].s[g]).reshape(1, L)
        term = one if term is None else term + one
    return term


REFERENCE = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("ref_")}


@functools.lru_cache(maxsize=None)
def reference(fn_name, args):
    """The fp64 reference of one case, computed once (the callers leave it unchanged)."""
    return REFERENCE[fn_name](*args)


# ---------------------------------------------------------------------------
# --measure
# ---------------------------------------------------------------------------
KINDS = ("adam", "tick", "loss", "lossgrad", "vec", "power", "sigma_term")


def _pow2_ceil(v):
    return int(2 ** int(np.ceil(np.log2(max(v, 1e-30)))))


def measure(cases=None):
    """{kind: largest ratio}: the float32 replay against the fp64 reference."""
    big = {k: 0.0 for k in KINDS}
    for name, args in (tc.CASES if cases is None else cases):
        ref, rep = reference(name, tuple(args)), REFERENCE[name](*args, dt=F32)
        assert ref.keys() == rep.keys(), name
        for key, o in ref.items():
            if o.kind != "int":
                big[o.kind] = max(big[o.kind], float(ratios(rep[key].value.astype(np.float32), o, Kk=1.0).max()))
    return big


def constants(big):
    return {k: max(_pow2_ceil(4 * v), 1) for k, v in big.items()}


if __name__ == "__main__":
    assert sys.argv[1:] == ["--measure"], "usage: python tests/tail_reference.py --measure"
    _big = measure()
    print("MEASURED =", {k: round(v, 3) for k, v in _big.items()})
    print("K =", constants(_big))

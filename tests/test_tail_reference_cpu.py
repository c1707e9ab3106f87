"""tests/tail_reference.py held to account without a GPU: it agrees in float64 with independent witnesses
(torch.optim, torch.nn.utils.spectral_norm and autograd, torch's loss functions); its recorded constants are what
`--measure` gives; the inputs of the power iteration keep its tolerance meaningful; and at those constants the comparator
rejects each of a list of plausible kernel mistakes while it accepts the float32 replay of the true operation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_cases as tc
import tail_reference as R
from norm_reference import T

F64, F32 = torch.float64, torch.float32


def _close(ours, theirs, what):
    ours = np.asarray(ours.v if isinstance(ours, T) else ours, dtype=np.float64).reshape(-1)
    theirs = theirs.detach().double().numpy().reshape(-1)
    err = np.abs(ours - theirs).max() / np.abs(theirs).max()
    assert err <= 1e-12, (what, err)


# ---------------------------------------------------------------------------
# witnesses
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("betas", tc.BETAS)
def test_adam_agrees_with_torch_optim(betas):
    r = tc.rng("witness", "adam", betas)
    lr, b1, b2, eps, gs = tc.c32(tc.ADAM_LR), tc.c32(betas[0]), tc.c32(betas[1]), tc.c32(tc.ADAM_EPS), 0.5
    p = torch.tensor(0.05 * r.randn(37), dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    d = {"p": p.detach().numpy().copy(), "m": np.zeros(37), "v": np.zeros(37)}
    for t in range(1, 6):
        g = 1e-2 * r.randn(37)
        p.grad = torch.from_numpy(g * gs)
        opt.step()
        p1, m1, v1 = R._adam_one(d, g, lr, b1, b2, eps, t, gs, F64)
        _close(p1, p, "p at step %d" % t)
        _close(m1, opt.state[p]["exp_avg"], "m at step %d" % t)
        _close(v1, opt.state[p]["exp_avg_sq"], "v at step %d" % t)
        d = {"p": p1.v.numpy(), "m": m1.v.numpy(), "v": v1.v.numpy()}


def test_rmsprop_agrees_with_torch_optim():
    r = tc.rng("witness", "rmsprop")
    lr, alpha, eps, gs = tc.c32(tc.RMSPROP_LR), tc.c32(tc.RMSPROP_ALPHA), tc.c32(tc.RMSPROP_EPS), 0.5
    p = torch.tensor(0.05 * r.randn(37), dtype=F64, requires_grad=True)
    opt = torch.optim.RMSprop([p], lr=lr, alpha=alpha, eps=eps, foreach=False)
    d = {"p": p.detach().numpy().copy(), "v": np.zeros(37)}
    for t in range(1, 6):
        d["g"] = 1e-2 * r.randn(37)
        p.grad = torch.from_numpy(d["g"] * gs)
        opt.step()
        p1, v1 = R._rmsprop_one(d, lr, alpha, eps, gs, F64)
        _close(p1, p, "p at step %d" % t)
        _close(v1, opt.state[p]["square_avg"], "v at step %d" % t)
        d = {"p": p1.v.numpy(), "v": v1.v.numpy()}


def test_tick_is_the_bias_corrections_of_step_t():
    for b1, b2 in tc.BETAS:
        ref = R.reference("tick", (b1, b2))
        f1, f2 = tc.c32(b1), tc.c32(b2)
        for k in range(1, 6):
            assert ref["from0/k%d" % k].value.tolist() == [k, 1 - f1 ** k, (1 - f2 ** k) ** 0.5]
        assert ref["from999/k1"].value.tolist() == [1000, 1 - f1 ** 1000, (1 - f2 ** 1000) ** 0.5]


def test_power_iteration_and_backward_agree_with_torch_spectral_norm():
    """torch.nn.utils.spectral_norm in train mode on a float64 Conv2d: one forward is one power iteration from the
    module's u; weight = W / sigma; autograd of <weight, G> gives dW with u and v held constant."""
    torch.manual_seed(5)
    eps = tc.c32(tc.SN_EPS)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(3, 5, 2).double(), eps=eps)
    R_, L = 5, 12
    u0 = conv.weight_u.detach().clone()
    W = conv.weight_orig.detach().reshape(R_, L)
    conv.train()
    conv(torch.randn(1, 3, 4, 4, dtype=F64))
    u, v, sigma, _ = R._power_step(T(W), T(u0), eps, F64)
    _close(u, conv.weight_u, "u")
    _close(v, conv.weight_v, "v")
    _close(T(W) / sigma, conv.weight, "W / sigma")
    G = torch.randn(5, 3, 2, 2, dtype=F64)
    dW, = torch.autograd.grad((conv.weight * G).sum(), [conv.weight_orig])
    d = {"x": T(G.reshape(R_, L)), "rowdots": T((G.reshape(R_, L) * (W / sigma.v)).sum(1)), "u": u, "v": v,
         "sigma": sigma.reshape(1)}
    _close(R.sn_bwd(d), dW, "dW")


@pytest.mark.parametrize("groups", [1, 2])
def test_sigma_term_agrees_with_autograd_through_sigma(groups):
    """leaky_relu(instance_norm(conv2d(x, W / sigma_g) + b)) per group g of the batch, sigma_g = u_g^T W v_g with u_g,
    v_g constant: the gradient with respect to W THROUGH SIGMA ONLY.  The kernel's inputs are those of the rescaled form
    IN_{eps sigma^2}(conv2d(x, W)): xh is the same, rstd_row = rstd of the witness's normalisation / sigma_g.
    (eps = 0.05: the normalisation hides sigma except through eps, so autograd forms this gradient as a difference
    1 / eps times its size -- at 1e-5 the witness itself is good to 1e-10 only.)"""
    r = tc.rng("witness", "sigma", groups)
    Cout, Cin, k, per, eps = 3, 2, 2, 2, 0.05
    R_, L, N = Cout, Cin * k * k, groups * 2
    x, b = torch.tensor(r.randn(N, Cin, 5, 5)), torch.tensor(r.randn(Cout))
    W = torch.tensor(r.randn(Cout, Cin, k, k))
    Ws = W.clone().requires_grad_(True)                     # the leaf that reaches the loss through sigma only
    u, v = torch.tensor(r.randn(groups, R_)), torch.tensor(r.randn(groups, L))
    up = torch.tensor(r.randn(N, Cout, 4, 4))
    sigma = torch.stack([u[g] @ Ws.reshape(R_, L) @ v[g] for g in range(groups)])
    assert sigma.abs().min() > 0.1
    loss, rowsums, rstd = 0.0, [], []
    for g in range(groups):
        sl = slice(g * per, (g + 1) * per)
        y = F.conv2d(x[sl], W / sigma[g], b)
        z = F.instance_norm(y, eps=eps).detach().requires_grad_(True)
        loss = loss + (F.leaky_relu(F.instance_norm(y, eps=eps), 0.2) * up[sl]).sum()
        dz, = torch.autograd.grad((F.leaky_relu(z, 0.2) * up[sl]).sum(), [z])
        rowsums.append(torch.stack([torch.full((per * Cout,), tc.WRONG_HALF, dtype=F64),
                                    (dz * z).sum((2, 3)).reshape(-1)], 1))
        rstd.append(((y.var((2, 3), unbiased=False) + eps).rsqrt() / sigma[g]).detach().reshape(-1))
    term, = torch.autograd.grad(loss, [Ws])
    d = {"rowsums": T(torch.cat(rowsums)), "rstd": T(torch.cat(rstd)), "sigma": T(sigma), "u": T(u), "v": T(v)}
    _close(R.sigma_term(d, groups, per * Cout, R_, L, eps=eps), term, "term")


def test_loss_tails_agree_with_torch():
    n, up = 257, float(np.float32(tc.UPSTREAM))
    x = torch.tensor(tc.bce_host(n)["x"], dtype=F64, requires_grad=True)
    bwd = R.reference("loss_bwd", (n,))
    for t in (0, 1):
        loss = F.binary_cross_entropy_with_logits(x, torch.full_like(x, float(t)))
        _close(R.reference("bce", (n,))["t%d/loss" % t].value, loss, "bce")
        _close(bwd["bce_t%d/dx" % t].value, torch.autograd.grad(loss * up, [x])[0], "bce dx")
    d = tc.mse_host(n)
    a, b = torch.tensor(d["a"], dtype=F64, requires_grad=True), torch.tensor(d["b"], dtype=F64)
    loss = F.mse_loss(a, b)
    _close(R.reference("mse", (n,))["loss"].value, loss, "mse")
    _close(bwd["mse/da"].value, torch.autograd.grad(loss * up, [a])[0], "mse da")
    s = torch.tensor(tc.gp_host(n)["sumsq"], dtype=F64, requires_grad=True)
    loss = ((s.sqrt() - 1.0) ** 2).mean()
    _close(R.reference("gp", (n,))["loss"].value, loss, "gp")
    ds, live = torch.autograd.grad(loss * up, [s])[0], (s > 0).detach().numpy()
    _close(bwd["gp/ds"].value[live], ds[torch.from_numpy(live)], "gp ds")
    assert (~live).sum() == 2 and not bwd["gp/ds"].value[~live].any() and not bwd["gp/ds"].scale[~live].any()


def test_vector_operations_agree_with_torch():
    n, eps = 257, tc.c32(tc.SN_EPS)
    d = tc.vec_host(n)
    x, b = torch.tensor(d["x"], dtype=F64), torch.tensor(d["b"], dtype=F64)
    ref = R.reference("vec", (n,))
    _close(ref["plain/normalize/out"].value, F.normalize(x, dim=0, eps=eps), "normalize")
    _close(ref["plain/normalize/norm"].value, x.norm(), "norm")
    _close(ref["plain/normalize_dot/dot"].value, F.normalize(x, dim=0, eps=eps) @ x, "fused dot")
    _close(ref["dot/out"].value, x @ b, "dot")
    for key, o in ref.items():
        if key.startswith("zero/"):
            assert not o.value.any() and not o.scale.any(), key
    m = tc.mat_host(3, 8)
    _close(R.reference("mat", (3, 8))["div/out"].value, torch.tensor(m["x"], dtype=F64) / float(m["sigma"][0]), "div")


def test_slab_gradients_are_exact_and_steps_use_their_sum():
    """ref_slabs asserts that each gradient is a float32; here: it is Adam on that sum (one parameter, by hand)."""
    k, (n, nzs) = 5, tc.slab_params()[5]
    d = tc.slab_host(k, n, nzs)
    g = sum(s[:, :n].astype(np.float64).sum(0) for s in d["slabs"])
    assert len(nzs) == 2 and np.abs(g).max() > 0
    b1, b2, t, gs = tc.slab_switches()[0]
    p1, _, _ = R._adam_one(d, g, tc.c32(tc.ADAM_LR), tc.c32(b1), tc.c32(b2), tc.c32(tc.ADAM_EPS), t, tc.c32(gs), F64)
    first = sum(nn for nn, _ in tc.slab_params()[:k])
    got = R.reference("slabs", ())["b%g_%g_t%d_gs%g/p" % (b1, b2, t, gs)].value[first:first + n]
    assert np.array_equal(got, p1.v.numpy())
    assert sorted({len(z) for _, z in tc.slab_params()}) == [1, 2, 3, 4]
    assert {z for _, zs in tc.slab_params() for z in zs} == set(tc.SLAB_NZ)


# ---------------------------------------------------------------------------
# the inputs keep the tolerance meaningful; the constants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tc.POWER_SHAPES)
def test_power_iteration_norms_are_not_cancellations(shape):
    """||W^T u|| and ||W v|| of both iterations exceed a tenth of their sum-of-magnitudes bound, so that the scale of u,
    v and sigma is within a small factor of their size."""
    norms = []
    R.ref_power(*shape, norms=norms)
    assert len(norms) == 4
    for nrm in norms:
        assert float(nrm.v) > 0.1 * float(nrm.s), (shape, float(nrm.v), float(nrm.s))


def test_the_recorded_constants_are_the_measured_ones():
    """`python tests/tail_reference.py --measure`: K is 4 x the RECORDED ratios rounded up to a power of two, exactly;
    measuring again gives the recorded ratios to 15 % (the last digits of torch's float32 sums are the host's)."""
    assert R.constants(R.MEASURED) == R.K and set(R.K) == set(R.KINDS)
    big = R.measure()
    assert big.keys() == R.MEASURED.keys()
    for k, v in big.items():
        assert abs(v - R.MEASURED[k]) <= 0.15 * R.MEASURED[k], (k, v, R.MEASURED[k])


# ---------------------------------------------------------------------------
# mutation check: against a wrong reference the comparator rejects the float32 replay of the true operation
# ---------------------------------------------------------------------------
def _rejected(name, args, mutation):
    """The keys at which the float32 replay fails against the mutated reference (it passes against the true one)."""
    true, rep = R.reference(name, tuple(args)), R.REFERENCE[name](*args, dt=F32)
    with R.mutated(mutation):
        wrong = R.REFERENCE[name](*args)
    assert wrong.keys() == true.keys() == rep.keys()

    def got(k):
        return rep[k].value.astype(np.int64 if true[k].kind == "int" else np.float32)
    ok = [m for k, o in true.items() for m in R.compare(got(k), o, k)]
    assert not ok, "the replay must pass against the true reference: %s" % ok[:3]
    return {k for k, o in wrong.items() if R.compare(got(k), o, k)}


def _adam_keys(names, keep=lambda b1, b2, t, gs, zg: True):
    return {"%s/%s" % (tc.adam_tag(*sw), n) for sw in tc.adam_switches() if keep(*sw) for n in names}


ADAM = ("adam", ("step", "single"))


def test_rejects_a_lerp_weight_of_beta1():
    """(1 - beta1 == beta1 at 0.5: only the pair with beta1 = 0 can tell.)"""
    assert _rejected(*ADAM, "lerp_weight_beta1") == _adam_keys("pm", lambda b1, *_: b1 == 0.0)


def test_rejects_eps_inside_the_square_root():
    assert _rejected(*ADAM, "eps_inside_sqrt") == _adam_keys("p")


def test_rejects_a_second_bias_correction_without_its_square_root():
    """(1 - beta2^t is 1 to float32 at the late steps: there is nothing to tell.)"""
    late = {(0.5, 100000), (0.0, 1000), (0.0, 100000)}
    assert _rejected(*ADAM, "bc2_without_sqrt") == _adam_keys("p", lambda b1, b2, t, *_: (b1, t) not in late)


def test_rejects_the_bias_correction_of_the_previous_step():
    bad = _rejected(*ADAM, "bias_correction_of_previous_step")
    assert _adam_keys("p", lambda b1, b2, t, *_: t in (2, 10)) <= bad
    assert bad <= _adam_keys("p", lambda b1, b2, t, *_: t > 1)


def test_rejects_grad_scale_on_the_first_moment_only():
    assert _rejected(*ADAM, "grad_scale_on_m_only") == _adam_keys("pv", lambda b1, b2, t, gs, zg: gs != 1.0)


@pytest.mark.parametrize("layout", tc.OPT_LAYOUTS)
def test_rejects_a_tail_left_unstepped(layout):
    assert _rejected("adam", ("step_dev", layout), "tail_unstepped") == _adam_keys("pmv")


@pytest.mark.parametrize("shape", [(3, 8), (65, 1028)])
def test_rejects_sigma_from_the_u_before_the_iteration(shape):
    bad = _rejected("power", shape, "sigma_from_old_u")
    assert "it1/sigma" in bad and not any(k.split("/")[1] in ("u", "v", "us", "vs") for k in bad)


def test_rejects_v_normalised_by_one_column_block():
    for shape in tc.POWER_SHAPES:
        bad = _rejected("power", shape, "v_norm_one_block")
        assert ({"it1/v", "it1/vs", "it2/v", "it2/vs"} <= bad) == (shape[1] > 1024), shape


SIGMA_CASES = [(1, 1, 3, 8), (2, 17, 3, 8), (8, 16, 65, 1028), (2, 4097, 3, 8)]


@pytest.mark.parametrize("mutation", ["sigma_term_sign", "rowsums_first_float", "coef_slice_dropped"])
def test_rejects_a_wrong_sigma_term(mutation):
    for args in SIGMA_CASES:
        assert _rejected("sigma_term", args, mutation) == {"term"}, args


def test_rejects_a_gp_gradient_at_zero():
    for n in (255, 70001):
        assert _rejected("loss_bwd", (n,), "gp_grad_nonzero_at_zero") == {"gp/ds"}
    assert not _rejected("loss_bwd", (1,), "gp_grad_nonzero_at_zero")      # (no row with sumsq == 0 there)


def test_every_listed_mutation_is_exercised():
    import inspect
    import sys
    text = inspect.getsource(sys.modules[__name__])
    for name in R.MUTATIONS:
        assert text.count('"%s"' % name) >= 1, name


def test_untouched_gradient_words_are_compared_bit_for_bit():
    g = tc.opt_tensor_host("single", 0, 8)["g"]
    o = R.Out(R.bits(g))
    assert not R.compare(g.view(np.uint32), o, "g")
    moved = g.copy()
    moved[5] = np.nextafter(moved[5], np.float32(0))
    assert R.compare(moved.view(np.uint32), o, "g")
    assert R.compare(np.zeros(8, dtype=np.float32).view(np.uint32), o, "g")

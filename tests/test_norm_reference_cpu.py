"""tests/norm_reference.py held to account without a GPU: it agrees with torch's own float64 normalisations and their
autograd derivatives; the elements it lets take either side of an activation are few; its recorded constants are what
`--measure` gives; and at those constants the comparator rejects each of a list of plausible kernel mistakes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc
import norm_reference as R
from norm_cases import ACTS, EPS, MOMENTUM, SENTINEL

F64 = torch.float64


def _close(ours, theirs, what):
    ours, theirs = np.asarray(ours, dtype=np.float64).reshape(-1), theirs.detach().double().numpy().reshape(-1)
    err = np.abs(ours - theirs).max() / np.abs(theirs).max()
    assert err <= 1e-12, (what, err)


def _act(z, act):
    return F.relu(z) if act == "relu" else F.leaky_relu(z, ACTS[act][1]) if act == "lrelu" else z


def _d(host):
    return {k: torch.from_numpy(v).to(F64) for k, v in host.items()}


# ---------------------------------------------------------------------------
# cross-check against torch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 8, 8, 8), (6, 5, 8, 8)])
def test_batchnorm_agrees_with_torch(shape):
    """F.batch_norm per statistics group, the running buffers handed from group to group, and its autograd."""
    N, C, H, W = shape
    ref, d = R.reference("bn_fused", shape), _d(nc.bn_inputs_host("fused", N, C, H * W))
    for groups, part, run, act, affine, with_dx in nc.bn_fused_switches():
        if part:
            continue                # statistics from the caller's partial sums: not an operation torch has
        tag = "groups%d_part%d_run%d_%s" % (groups, part, run, act)
        x = d["x"].clone().requires_grad_(True)
        ga = (d["gamma"] if affine else torch.ones(C, dtype=F64)).clone().requires_grad_(True)
        be = (d["beta"] if affine else torch.zeros(C, dtype=F64)).clone().requires_grad_(True)
        rm, rv = d["rm"].clone(), d["rv"].clone()
        out = torch.cat([_act(F.batch_norm(xg, rm, rv, ga, be, True, MOMENTUM, EPS), act) for xg in x.chunk(groups)])
        dx, dga, dbe = torch.autograd.grad(out, [x, ga, be], d["g"])
        _close(ref[tag + "/out"].value, out, tag + "/out")
        if run:
            _close(ref[tag + "/running_mean"].value, rm, tag + "/running_mean")
            _close(ref[tag + "/running_var"].value, rv, tag + "/running_var")
            assert ref[tag + "/nbt"].value.tolist() == [nc.NBT0 + groups]
            dga, dbe = dga + d["acc_gamma"], dbe + d["acc_beta"]
        _close(ref[tag + "/dgamma"].value, dga, tag + "/dgamma")
        _close(ref[tag + "/dbeta"].value, dbe, tag + "/dbeta")
        if with_dx:
            _close(ref[tag + "/dx"].value, dx, tag + "/dx")
        xg = d["x"].view(groups, N // groups, C, H * W)
        mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
        rstd = (var + EPS).rsqrt()
        _close(ref[tag + "/coef"].value, torch.cat([(ga * rstd).reshape(-1), (be - mean * ga * rstd).reshape(-1),
                                                    mean.reshape(-1), rstd.reshape(-1)]), tag + "/coef")


@pytest.mark.parametrize("shape", [(3, 5, 12), (2, 3, 64)])
def test_instancenorm_agrees_with_torch(shape):
    """F.instance_norm with per-channel affine: forward, first derivatives, and the derivatives of <dx, v>."""
    N, C, inner = shape
    for act in ACTS:
        d = _d(nc.rows_host("fwd", N, C, inner))
        out = _act(F.instance_norm(d["x"], weight=d["gamma_c"], bias=d["beta_c"], eps=EPS), act)
        _close(R.reference("rownorm_fwd", shape)["apr0_unb0_%s/out" % act].value, out, act + "/out")

        d = _d(nc.rows_host("bwd", N, C, inner))
        x, ga, be = (d[k].clone().requires_grad_(True) for k in ("x", "gamma_c", "beta_c"))
        out = _act(F.instance_norm(x, weight=ga, bias=be, eps=EPS), act)
        ref = R.reference("norm_act_bwd_rows_form", shape)
        for name, grad in zip(("dx", "dgamma", "dbeta"), torch.autograd.grad(out, [x, ga, be], d["g"])):
            _close(ref["apr0_unb0_%s_dx1/%s" % (act, name)].value, grad, act + "/" + name)

        d = _d(nc.rows_host("bwd2", N, C, inner))
        x, ga, g = (d[k].clone().requires_grad_(True) for k in ("x", "gamma_c", "g"))
        out = _act(F.instance_norm(x, weight=ga, bias=d["beta_c"], eps=EPS), act)
        dx, = torch.autograd.grad(out, [x], g, create_graph=True)
        ref = R.reference("rownorm_bwd2", shape)
        for name, grad in zip(("gg_out", "gx", "ggamma"), torch.autograd.grad((dx * d["v"]).sum(), [g, x, ga])):
            _close(ref["%s/%s" % (act, name)].value, grad, act + "/" + name)


def _adain(features, scale, bias):
    """Adaptive instance normalisation as HoloGAN's generator writes it: moments over the pixels with torch's default
    (unbiased) variance, then the per-sample scale and bias."""
    flat = features.flatten(2)
    mean, var = flat.mean(2, keepdim=True), flat.var(2, keepdim=True)
    return ((flat - mean) * torch.rsqrt(var + EPS) * scale.unsqueeze(2) + bias.unsqueeze(2)).view_as(features)


def test_adain_agrees_with_the_plain_expression():
    N, C, inner = shape = (3, 5, 12)
    d = _d(nc.rows_host("fwd", N, C, inner))
    out = _act(_adain(d["x"], d["gamma_r"].view(N, C), d["beta_r"].view(N, C)), "relu")
    _close(R.reference("rownorm_fwd", shape)["apr1_unb1_relu/out"].value, out, "out")
    d = _d(nc.rows_host("bwd", N, C, inner))
    x, ga, be = (d[k].clone().requires_grad_(True) for k in ("x", "gamma_r", "beta_r"))
    out = _act(_adain(x, ga.view(N, C), be.view(N, C)), "relu")
    dx, dga, dbe = torch.autograd.grad(out, [x, ga, be], d["g"])
    ref = R.reference("norm_act_bwd_rows_form", shape)
    _close(ref["apr1_unb1_relu_dx1/dx"].value, dx, "dx")
    _close(ref["apr1_unb1_relu_dx1/dgamma"].value, dga, "dgamma")
    _close(ref["apr1_unb1_relu_dx1/dbeta"].value, dbe, "dbeta")
    _close(ref["apr2_unb1_relu_dx1/dgamma"].value, torch.cat([dga.view(N, C), dbe.view(N, C)], 1), "packed")

    N, C, inner = shape = (5, 3, 16)         # the constant every sample shares = its repeat
    d = _d(nc.adain_host(N, C, inner))
    x, sb = d["x"].clone().requires_grad_(True), d["sb"].clone().requires_grad_(True)
    out = _act(_adain(x.repeat(N, 1, 1), sb[:, :C], sb[:, C:]), "lrelu")
    dx, dsb = torch.autograd.grad(out, [x, sb], d["g"])
    ref = R.reference("adain_const", shape)
    _close(ref["lrelu/out"].value, out, "const out")
    _close(ref["lrelu/dx"].value, dx, "const dx")
    _close(ref["lrelu/dsb"].value, dsb, "const dsb")
    assert ref["lrelu/bwd_rc"].value.tolist() == [0]
    too_long = R.reference("adain_const_too_long", (3, 2, 1028))
    assert too_long["relu/bwd_rc"].value.tolist() == [nc.GZ_ERR_UNSUPPORTED] and "relu/dx" not in too_long


def test_formula_scales_bound_their_values():
    """The closed formulas that give the scales evaluate to the autograd values, and no scale is below its value."""
    for name, args in [("norm_act_bwd_rows_form", (3, 5, 12)), ("rownorm_bwd2", (2, 3, 64)), ("bn_fused", (4, 8, 8, 8)),
                       ("adain_const", (5, 3, 16))]:
        for key, o in R.reference(name, args).items():
            if o.kind != "int":
                assert (o.scale >= np.abs(o.value) * (1 - 1e-9)).all(), (name, key)


# ---------------------------------------------------------------------------
# the band, the constants
# ---------------------------------------------------------------------------
ALL = R.all_cases()


@pytest.mark.parametrize("name,args", ALL, ids=["%s_%s" % (n, "x".join(map(str, a))) for n, a in ALL])
def test_few_elements_may_take_either_side(name, args):
    """A condition on the inputs, from the reference alone: the band of B u around z = 0 holds at most
    max(2, 1e-4 size) elements of any output."""
    for key, o in R.reference(name, args).items():
        if o.either is not None:
            assert o.either.sum() <= max(2, 1e-4 * o.either.size), (key, int(o.either.sum()), o.either.size)


def test_the_recorded_constants_are_the_measured_ones():
    """`python tests/norm_reference.py --measure`: the float32 replay against the fp64 reference over every case.  K and B
    are 4 x the RECORDED ratios rounded up to a power of two, exactly; measuring again gives the recorded ratios to
    15 % (torch's float32 sums take the order the host's vector unit gives them, so the last digits are the host's)."""
    assert R.constants(R.MEASURED, R.MEASURED_Z) == (R.K, R.B)
    big, big_z = R.measure(ALL)
    for got, recorded in ((big, R.MEASURED), (big_z, R.MEASURED_Z)):
        assert got.keys() == recorded.keys()
        for k, v in got.items():
            assert abs(v - recorded[k]) <= 0.15 * recorded[k], (k, v, recorded[k])


# ---------------------------------------------------------------------------
# mutation check: the comparator at the recorded K rejects a wrong reference
# ---------------------------------------------------------------------------
def _rejected(name, args, mutation, keys=None):
    """The keys at which the mutated reference, taken as a kernel's output, fails against the true one."""
    true = R.reference(name, args)
    with R.mutated(mutation):
        wrong = R.REFERENCE[name](*args)
    assert wrong.keys() == true.keys()
    assert not any(R.compare(o.value, o, k) for k, o in true.items()), "the true reference must pass against itself"
    return {k for k, o in true.items()
            if R.compare(wrong[k].value.astype(np.float32 if o.kind != "int" else np.int64), o, k)}


@pytest.mark.parametrize("shape", [(3, 5, 12), (2, 3, 1280), (1, 2, 4352)])
def test_rejects_statistics_that_skip_the_last_float4(shape):
    bad = _rejected("rownorm_fwd", shape, "skip_last4")
    assert {"apr%d_unb%d_%s/%s" % (apr, unb, act, o) for apr, unb, act in nc.FWD_FULL for o in ("coef", "out")} <= bad
    assert "apr0_unb0/coef" in _rejected("rownorm_stats", shape, "skip_last4")


def test_rejects_swapped_biased_and_unbiased_variance():
    assert _rejected("rownorm_stats", (1, 2, 4352), "swap_unbiased") == {"apr%d_unb%d/coef" % s for s in nc.STATS_FULL}
    assert "apr1_unb1_relu/out" in _rejected("rownorm_fwd", (1, 2, 4352), "swap_unbiased")


def test_rejects_group_statistics_over_the_whole_batch():
    bad = _rejected("bn_fused", (12, 4, 64, 64), "group_stats_whole_batch")
    for groups, part, run, act, affine, with_dx in nc.bn_fused_switches():
        tag = "groups%d_part%d_run%d_%s" % (groups, part, run, act)
        assert ((tag + "/coef") in bad) == (groups == 2), tag
        assert ((tag + "/out") in bad) == (groups == 2), tag


def test_rejects_k_divided_by_the_whole_count():
    bad = _rejected("bn_fused", (12, 4, 64, 64), "k_whole_count")
    for groups, part, run, act, affine, with_dx in nc.bn_fused_switches():
        tag = "groups%d_part%d_run%d_%s" % (groups, part, run, act)
        assert ((tag + "/k") in bad) == (groups == 2), tag
        if with_dx:
            assert ((tag + "/dx") in bad) == (groups == 2), tag


@pytest.mark.parametrize("shape", [(3, 5, 12), (2, 3, 256)])
def test_rejects_a_mask_taken_from_xhat(shape):
    bad = _rejected("rownorm_fwd", shape, "mask_from_xh")
    assert {"apr1_unb%d_%s/out" % (unb, act) for unb in (0, 1) for act in ("relu", "lrelu")} <= bad
    assert not any(k.endswith("_none/out") for k in bad)
    bad = _rejected("norm_act_bwd_rows_form", shape, "mask_from_xh")
    assert {"apr1_unb%d_%s_dx1/%s" % (unb, act, o) for unb in (0, 1) for act in ("relu", "lrelu")
            for o in ("dx", "dgamma", "dbeta")} <= bad


def test_rejects_a_running_variance_from_the_biased_one():
    bad = _rejected("bn_fused", (4, 32, 4, 4), "running_var_biased")
    assert bad == {"groups%d_part%d_run1_%s/running_var" % (g, p, a)
                   for g, p, r, a, _, _ in nc.bn_fused_switches() if r}


def test_rejects_an_ignored_accumulate():
    bad = _rejected("rownorm_bwd_acc", (2, 3, 64), "ignore_accumulate")
    assert bad == {"acc1_%s/%s" % (a, o) for a in ACTS for o in ("dgamma", "dbeta")}
    bad = _rejected("bn_fused", (4, 8, 8, 8), "ignore_accumulate")
    assert bad == {"groups%d_part%d_run1_%s/%s" % (g, p, a, o) for g, p, r, a, _, _ in nc.bn_fused_switches() if r
                   for o in ("dgamma", "dbeta")}


def test_rejects_rows_left_untouched_and_accepts_only_the_sentinel_there():
    """Rows from 262144 on (the second trip of the row loop) left at SENTINEL, at (4, 131080, 4); and the other way
    round: a word that must stay SENTINEL may not move by one bit."""
    shape, first = (4, 131080, 4), 262144
    for name, key in (("rownorm_fwd", "apr1_unb1_lrelu/out"), ("rownorm_bwd_rows", "relu/dx"),
                      ("rownorm_bwd2", "lrelu/gx")):
        o = R.reference(name, shape)[key]
        got = o.value.astype(np.float32).reshape(-1, shape[2])
        assert not R.compare(got, o, key)
        got[first:] = SENTINEL
        assert R.compare(got, o, key), key
    o = R.untouched((8,))
    got = np.full(8, SENTINEL, dtype=np.float32)
    assert not R.compare(got, o, "untouched")
    got[5] = np.nextafter(np.float32(SENTINEL), np.float32(0))
    assert R.compare(got, o, "untouched")


def test_rejects_swapped_affine_gradients():
    for name, args, tag in (("norm_act_bwd_rows_form", (2, 3, 64), "apr0_unb0_relu_dx1"),
                            ("norm_act_bwd_rows_form", (2, 3, 64), "apr1_unb1_lrelu_dx1"),
                            ("bn_fused", (4, 8, 8, 8), "groups2_part0_run1_none")):
        ref = R.reference(name, args)
        dgamma, dbeta = ref[tag + "/dgamma"], ref[tag + "/dbeta"]
        assert R.compare(dbeta.value.astype(np.float32), dgamma, tag + "/dgamma")
        assert R.compare(dgamma.value.astype(np.float32), dbeta, tag + "/dbeta")

"""The normalisation kernels (csrc/gz_norm.hip) against the bits they produced BEFORE their bodies were written once
(row walk, coefficient record, element terms, finalize, slice walk).  The other tests of these kernels hold them to a
relative tolerance that any order of summation satisfies; here every output word of every launch geometry is fixed: fp32 outputs
are compared as uint32, num_batches_tracked as an integer, and not one element may differ.
tests/golden/norm_parent.npz was written by tests/golden/make_norm_golden.py with the library of the commit before that
refactor; the inputs are seeded here (row means away from zero, mixed-sign gradients, both sides of every activation).

The shapes are the smallest that cross each boundary of the code; the comment next to each says which.  A case is one
entry point on one shape and runs that entry point's scalar switches (affine form, biased / unbiased, activation,
accumulate, groups, ...) one after another; an output is keyed ``case/switches/name``.

Fixture size: the outputs of all cases are over 200 MB, the file has to stay under 1 MB.  An output of more than 512
elements is therefore kept as the sha256 of its bytes plus every 257th element, and both are compared; smaller outputs
are kept whole.  Equal digests are equal bits, so nothing is compared more loosely -- only a mismatch in a large output is
reported without its position.

The experiment paths (csrc/gz_knobs.h switches are read once per process) run in one child process per setting, which
writes its outputs to a file that the test compares in the same way."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

from helpers import GOLDEN_DIR  # noqa: E402

pytestmark = pytest.mark.gpu

from norm_cases import (ACTS, ADAIN_SHAPES, BIG_CHANNELS, BN_SHAPES, BWD_FEW, BWD_FULL, EPS,  # noqa: E402,F401
                        EW_COUNTS, FINALIZE_C, FINALIZE_PER, FWD_FEW, FWD_FULL, GZ_ERR_UNSUPPORTED, MOMENTUM, NBT0,
                        ROW_SHAPES, SENTINEL, SIGMAS, STATS_FEW, STATS_FULL, adain_host, bn_fused_switches,
                        bn_inputs_host, channel_sum_host, elementwise_acts, elementwise_host, f32 as _f32,
                        finalize_host, rows_host, small, switches as _switches)

WHOLE_LIMIT = 512           # elements; larger outputs are stored as digest + every 257th element


# ---------------------------------------------------------------------------
# inputs (seeded on the host: norm_cases.py) and plumbing
# ---------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _buf(*shape, fill=SENTINEL):
    import torch
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _lib():
    from lightning_gan_zoo_amd._lib import lib
    return lib


def _ws(N, C):
    """The norm workspace, poisoned: a kernel that reads a part of it that this launch has not written shows up."""
    return _buf(max(_lib().gz_norm_workspace_bytes(N, C) // 4, 1), fill=float("nan"))


def _ok(rc, what):
    assert rc == 0, (what, rc)


def _upload(d):
    return {k: _dev(v) for k, v in d.items()}


def _rows(tag, N, C, inner):
    return _upload(rows_host(tag, N, C, inner))


def _affine(d, apr):
    return (d["gamma_r"], d["beta_r"]) if apr else (d["gamma_c"], d["beta_c"])


def _row_coef(d, N, C, inner, apr=0, unb=0):
    coef = _buf(4 * N * C)
    ga, be = _affine(d, apr)
    _ok(_lib().gz_rownorm_stats(_p(d["x"]), _p(ga), _p(be), _p(coef), None, N, C, inner, EPS, apr, unb, None), "stats")
    return coef


# ---------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------
def _rownorm_fwd(N, C, inner):
    d, res = _rows("fwd", N, C, inner), {}
    for apr, unb, act in _switches(N, C, inner, FWD_FULL, FWD_FEW):
        ga, be = _affine(d, apr)
        coef, out = _buf(4 * N * C), _buf(N, C, inner)
        _ok(_lib().gz_rownorm_act_fwd(_p(d["x"]), _p(ga), _p(be), _p(coef), _p(out), N, C, inner, EPS, apr, unb,
                                      *ACTS[act], None), "rownorm_act_fwd")
        tag = "apr%d_unb%d_%s" % (apr, unb, act)
        res[tag + "/coef"], res[tag + "/out"] = _host(coef), _host(out)
    return res


def _rownorm_stats(N, C, inner):
    d, res = _rows("stats", N, C, inner), {}
    for apr, unb in _switches(N, C, inner, STATS_FULL, STATS_FEW):
        res["apr%d_unb%d/coef" % (apr, unb)] = _host(_row_coef(d, N, C, inner, apr, unb))
    return res


def _norm_act_bwd_rows_form(N, C, inner):
    """gz_norm_act_bwd with per_channel = 0."""
    d, res = _rows("bwd", N, C, inner), {}
    for apr, unb, act, with_dx in _switches(N, C, inner, BWD_FULL, BWD_FEW):
        coef = _row_coef(d, N, C, inner, min(apr, 1), unb)
        dx = _buf(N, C, inner) if with_dx else None
        nga = {0: C, 1: N * C, 2: 2 * N * C}[apr]
        dgamma, dbeta, kbuf, ws = _buf(nga), _buf(nga), _buf(2 * N * C), _ws(N, C)
        dg, db = (dgamma, dgamma[C:]) if apr == 2 else (dgamma, dbeta)
        _ok(_lib().gz_norm_act_bwd(_p(d["g"]), _p(d["x"]), _p(coef), _p(dx), dg.data_ptr(), db.data_ptr(), _p(ws),
                                   _p(kbuf), N, C, inner, 0, apr, unb, *ACTS[act], None), "norm_act_bwd")
        tag = "apr%d_unb%d_%s_dx%d" % (apr, unb, act, with_dx)
        res[tag + "/dgamma"] = _host(dgamma)
        if apr != 2:
            res[tag + "/dbeta"] = _host(dbeta)
        if with_dx:
            res[tag + "/dx"] = _host(dx)
    return res


def _rownorm_bwd_acc(N, C, inner):
    d, res = _rows("acc", N, C, inner), {}
    coef = _row_coef(d, N, C, inner)
    for acc in (0, 1):
        for act in (ACTS if small(N, C, inner) else ["lrelu"]):
            dx, kbuf, ws = _buf(N, C, inner), _buf(2 * N * C), _ws(N, C)
            dgamma, dbeta = d["acc_gamma"][:C].clone(), d["acc_beta"][:C].clone()
            _ok(_lib().gz_rownorm_act_bwd_acc(_p(d["g"]), _p(d["x"]), _p(coef), _p(dx), _p(dgamma), _p(dbeta), _p(ws),
                                              _p(kbuf), N, C, inner, *ACTS[act], acc, None), "rownorm_act_bwd_acc")
            tag = "acc%d_%s" % (acc, act)
            res[tag + "/dx"], res[tag + "/dgamma"], res[tag + "/dbeta"] = _host(dx), _host(dgamma), _host(dbeta)
    return res


def _rownorm_bwd_rows(N, C, inner):
    d, res = _rows("rows", N, C, inner), {}
    coef = _row_coef(d, N, C, inner)
    for act in (ACTS if small(N, C, inner) else ["relu"]):
        dx, sums = _buf(N, C, inner), _buf(N * C, 2)
        _ok(_lib().gz_rownorm_act_bwd_rows(_p(d["g"]), _p(d["x"]), _p(coef), _p(dx), _p(sums), N, C, inner, *ACTS[act],
                                           None), "rownorm_act_bwd_rows")
        res[act + "/dx"], res[act + "/rowsums"] = _host(dx), _host(sums)
    return res


def _rownorm_bwd2(N, C, inner):
    d, res = _rows("bwd2", N, C, inner), {}
    coef = _row_coef(d, N, C, inner)
    for act in (ACTS if small(N, C, inner) else ["lrelu"]):
        gg, gx, ggamma, ws = _buf(N, C, inner), _buf(N, C, inner), _buf(C), _ws(N, C)
        _ok(_lib().gz_rownorm_act_bwd2(_p(d["g"]), _p(d["v"]), _p(d["x"]), _p(coef), _p(gg), _p(gx), _p(ggamma), _p(ws),
                                       N, C, inner, *ACTS[act], None), "rownorm_act_bwd2")
        res[act + "/gg_out"], res[act + "/gx"], res[act + "/ggamma"] = _host(gg), _host(gx), _host(ggamma)
    return res


def _rownorm_sigma(N, C, inner):
    d, res = _rows("sigma", N, C, inner), {}
    for groups in (1, 2):
        sigma = _dev(_f32(SIGMAS[:groups]))
        coef, out = _buf(4 * N * C), _buf(N, C, inner)
        _ok(_lib().gz_rownorm_act_fwd_sigma(_p(d["x"]), _p(sigma), groups, _p(coef), _p(out), N, C, inner, EPS,
                                            *ACTS["lrelu"], None), "rownorm_act_fwd_sigma")
        res["groups%d_lrelu/coef" % groups], res["groups%d_lrelu/out" % groups] = _host(coef), _host(out)
    return res


def _adain_const(N, C, inner):
    """gz_adain_const_fwd and gz_adain_const_bwd: x is the [C][inner] constant every sample shares, sb the packed
    per-sample [N][scale C | shift C]."""
    d, res = _upload(adain_host(N, C, inner)), {}
    x, sb, g = d["x"], d["sb"], d["g"]
    for act in ("relu", "lrelu"):
        coef, out = _buf(4 * N * C), _buf(N, C, inner)
        _ok(_lib().gz_adain_const_fwd(_p(x), _p(sb), _p(coef), _p(out), N, C, inner, EPS, *ACTS[act], None),
            "adain_const_fwd")
        dx, dsb = _buf(C, inner), _buf(N, 2 * C)
        rc = _lib().gz_adain_const_bwd(_p(g), _p(x), _p(coef), _p(dx), _p(dsb), N, C, inner, *ACTS[act], None)
        res[act + "/coef"], res[act + "/out"] = _host(coef), _host(out)
        res[act + "/bwd_rc"] = np.array([rc], dtype=np.int64)
        if rc == 0:
            res[act + "/dx"], res[act + "/dsb"] = _host(dx), _host(dsb)
    return res


def _adain_const_too_long(N, C, inner):
    res = _adain_const(N, C, inner)
    assert all(int(res[a + "/bwd_rc"][0]) == GZ_ERR_UNSUPPORTED for a in ("relu", "lrelu")), res
    return res


# ---------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------
def _bn_inputs(tag, N, C, inner):
    return _upload(bn_inputs_host(tag, N, C, inner))


def _running(d, on):
    import torch
    if not on:
        return None, None, None
    return d["rm"].clone(), d["rv"].clone(), torch.full((1,), NBT0, dtype=torch.int64, device="cuda")


def _bn_bwd(d, coef, N, C, inner, groups, act, acc, with_dx, tag, res):
    dx = _buf(N, C, inner) if with_dx else None
    dgamma, dbeta = d["acc_gamma"].clone(), d["acc_beta"].clone()
    kbuf, ws = _buf(2 * groups * C), _ws(N, C)
    _ok(_lib().gz_batchnorm_act_bwd_g(_p(d["g"]), _p(d["x"]), _p(coef), _p(dx), _p(dgamma), _p(dbeta), _p(ws), _p(kbuf),
                                      N, C, inner, *ACTS[act], groups, acc, None), "batchnorm_act_bwd_g")
    res[tag + "/dgamma"], res[tag + "/dbeta"], res[tag + "/k"] = _host(dgamma), _host(dbeta), _host(kbuf)
    if with_dx:
        res[tag + "/dx"] = _host(dx)


def _bn_fused(N, C, H, W):
    """gz_batchnorm_act_fwd_fused, then gz_batchnorm_act_bwd_g on its coefficients.  Switches: groups, partial rows
    from the caller (two per sample) or none, running buffers and nbt or none; accumulate follows `running`; the
    affine parameters are null once and dx is null once (the backward then takes bn_bwd_finalize_kernel)."""
    inner, res = H * W, {}
    d = _bn_inputs("fused", N, C, inner)
    for groups, part, run, act, affine, with_dx in bn_fused_switches():
        rm, rv, nbt = _running(d, run)
        coef, out = _buf(4 * groups * C), _buf(N, C, inner)
        ws = None if part else _ws(N, C)
        _ok(_lib().gz_batchnorm_act_fwd_fused(
            _p(d["x"]), _p(d["partials"]) if part else None, 2 * N if part else 0, (N // groups) * inner if part else 0,
            _p(d["gamma"]) if affine else None, _p(d["beta"]) if affine else None, _p(coef), _p(rm), _p(rv), _p(nbt),
            _p(ws), _p(out), N, C, inner, EPS, MOMENTUM, groups, *ACTS[act], None), "batchnorm_act_fwd_fused")
        tag = "groups%d_part%d_run%d_%s" % (groups, part, run, act)
        res[tag + "/coef"], res[tag + "/out"] = _host(coef), _host(out)
        if run:
            res[tag + "/running_mean"], res[tag + "/running_var"], res[tag + "/nbt"] = _host(rm), _host(rv), _host(nbt)
        _bn_bwd(d, coef, N, C, inner, groups, act, run, with_dx, tag, res)
    return res


def _bn_stats_apply(N, C, H, W):
    """gz_batchnorm_stats_g + gz_norm_act_fwd_g (+ gz_batchnorm_act_bwd_g for the large-C case's apply index)."""
    inner, res = H * W, {}
    d = _bn_inputs("stats", N, C, inner)
    for groups in _switches(N, C, inner, (1, 2), (2,)):
        rm, rv, nbt = _running(d, True)
        coef, out, ws = _buf(4 * groups * C), _buf(N, C, inner), _ws(N, C)
        _ok(_lib().gz_batchnorm_stats_g(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), _p(coef), _p(rm), _p(rv), _p(nbt),
                                        _p(ws), N, C, inner, EPS, MOMENTUM, groups, None), "batchnorm_stats_g")
        _ok(_lib().gz_norm_act_fwd_g(_p(d["x"]), _p(coef), _p(out), N, C, inner, 1, groups, *ACTS["lrelu"], None),
            "norm_act_fwd_g")
        tag = "groups%d_lrelu" % groups
        res[tag + "/coef"], res[tag + "/out"] = _host(coef), _host(out)
        res[tag + "/running_mean"], res[tag + "/running_var"], res[tag + "/nbt"] = _host(rm), _host(rv), _host(nbt)
        _bn_bwd(d, coef, N, C, inner, groups, "lrelu", groups - 1, True, tag, res)
    return res


def _bn_eval_coef(N, C, H, W):
    d = _bn_inputs("eval", N, C, H * W)
    coef = _buf(4 * C)
    _ok(_lib().gz_batchnorm_eval_coef(_p(d["gamma"]), _p(d["beta"]), _p(d["rm"]), _p(d["rv"]), _p(coef), C, EPS, None),
        "batchnorm_eval_coef")
    return {"plain/coef": _host(coef)}


def _bn_finalize(rows, groups):
    """gz_batchnorm_finalize_g on partial rows of 32 elements each: <= 512 rows per group is the one-wavefront image,
    more the eight-wavefront one."""
    C, per = FINALIZE_C, FINALIZE_PER
    d = _upload(finalize_host(rows, groups))
    partials = d["partials"]
    rm, rv, nbt = _running(d, True)
    coef = _buf(4 * groups * C)
    _ok(_lib().gz_batchnorm_finalize_g(_p(partials), rows, (rows // groups) * per, _p(d["gamma"]), _p(d["beta"]),
                                       _p(coef), _p(rm), _p(rv), _p(nbt), C, EPS, MOMENTUM, groups, None),
        "batchnorm_finalize_g")
    return {"plain/coef": _host(coef), "plain/running_mean": _host(rm), "plain/running_var": _host(rv),
            "plain/nbt": _host(nbt)}


def _channel_sum(N, C, inner):
    x = _dev(channel_sum_host(N, C, inner)["x"])
    out, ws = _buf(C), _ws(N, C)
    _ok(_lib().gz_channel_sum(_p(x), _p(out), _p(ws), N, C, inner, None), "channel_sum")
    return {"plain/out": _host(out)}


def _elementwise(count):
    d, res = _upload(elementwise_host(count)), {}
    g, v, out = d["g"], d["v"], d["out"]
    for name, act in elementwise_acts(count):
        dx = _buf(count)
        _ok(_lib().gz_act_bwd(_p(g), _p(out), _p(dx), count, *act, None), "act_bwd")
        res["act_bwd_" + name + "/dx"] = _host(dx)
    y = _buf(count)
    _ok(_lib().gz_tanh_bwd2(_p(v), _p(g), _p(out), _p(y), count, None), "tanh_bwd2")
    res["tanh_bwd2/res"] = _host(y)
    return res


def _bn_functional(N, C, H, W):
    """functional.batch_norm_act and its backward under the Python-side switch that keeps bn_finalize a launch of its
    own: without statistics from a convolution (gz_batchnorm_stats_g) and with (gz_batchnorm_finalize_g)."""
    import torch
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd.functional import _base
    assert _base._NORM_UNFUSED, "the separate-finalize switch was not honoured"
    inner, res = H * W, {}
    d = _bn_inputs("functional", N, C, inner)
    for groups in (1, 2):
        for part in (0, 1):
            x = d["x"].view(N, C, H, W).clone().requires_grad_(True)
            gamma, beta = torch.nn.Parameter(d["gamma"].clone()), torch.nn.Parameter(d["beta"].clone())
            rm, rv, nbt = _running(d, True)
            out = F.batch_norm_act(x, gamma, beta, rm, rv, nbt[0], True, MOMENTUM, EPS, *ACTS["relu"],
                                   stats=d["partials"] if part else None, groups=groups)
            out.backward(d["g"].view(N, C, H, W))
            tag = "groups%d_part%d_relu" % (groups, part)
            res[tag + "/out"], res[tag + "/dx"] = _host(out.detach()), _host(x.grad)
            res[tag + "/dgamma"], res[tag + "/dbeta"] = _host(gamma.grad), _host(beta.grad)
            res[tag + "/running_mean"], res[tag + "/running_var"], res[tag + "/nbt"] = _host(rm), _host(rv), _host(nbt)
    return res


def _case(fn, args):
    return ("%s_%s" % (fn.__name__.lstrip("_"), "x".join(str(a) for a in args)), fn, args)


ROW_ENTRY_POINTS = [_rownorm_fwd, _rownorm_stats, _norm_act_bwd_rows_form, _rownorm_bwd_acc, _rownorm_bwd_rows,
                    _rownorm_bwd2]
CASES = ([_case(fn, s) for fn in ROW_ENTRY_POINTS for s in ROW_SHAPES]
         + [_case(_rownorm_sigma, (4, 6, 64))]
         + [_case(_adain_const, s) for s in ADAIN_SHAPES] + [_case(_adain_const_too_long, (3, 2, 1028))]
         + [_case(_bn_fused, s) for s in BN_SHAPES]
         + [_case(_bn_stats_apply, (4, 8, 8, 8)), _case(_bn_stats_apply, BIG_CHANNELS + (1,))]
         + [_case(_bn_eval_coef, (4, 8, 8, 8)), _case(_bn_finalize, (16, 2)), _case(_bn_finalize, (1040, 2)),
            _case(_channel_sum, (70, 5, 4))]
         + [_case(_elementwise, (n,)) for n in EW_COUNTS])

# Experiment paths: {setting: (environment, cases)}.  `unfused` is the three-launch backward (norm_bwd_rowsums_kernel,
# row_bwd_finalize_kernel, bn_bwd_finalize_kernel, norm_bwd_apply_kernel); `bwd_cache16` the backward's CACHE = 16
# image; `finalize_launch` the Python-side separate bn_finalize launch.
SETTINGS = {
    "unfused": ({"GZ_EXPERIMENTS": "1", "GZ_NORM_UNFUSED": "1"},
                [_case(_norm_act_bwd_rows_form, s) for s in [(3, 5, 4), (3, 5, 12), (2, 3, 1280), (4, 131080, 4)]]
                + [_case(_rownorm_bwd_acc, (2, 3, 256)), _case(_bn_fused, (4, 8, 8, 8)), _case(_bn_fused, (6, 5, 8, 8)),
                   _case(_bn_stats_apply, BIG_CHANNELS + (1,))]),
    "bwd_cache16": ({"GZ_EXPERIMENTS": "1", "GZ_NORM_BWD_CACHE": "16"},
                    [_case(fn, s) for fn in (_norm_act_bwd_rows_form, _rownorm_bwd_rows)
                     for s in [(2, 3, 1280), (1, 2, 4096)]]),
    "finalize_launch": ({"GZ_EXPERIMENTS": "1", "GZ_BN_FINALIZE_LAUNCH": "1"}, [_case(_bn_functional, (4, 8, 8, 8))]),
}


# ---------------------------------------------------------------------------
# stored form, comparison
# ---------------------------------------------------------------------------
def stored(arrays):
    """{golden key: array} in the form the file keeps: small outputs whole, large ones as digest + every 257th."""
    blob = {}
    for key, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float32, np.int64), (key, a.dtype)
        if a.size > WHOLE_LIMIT:
            blob[key + "#sha256"] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
            blob[key + "#every257"] = a.reshape(-1)[::257].copy()
            blob[key + "#shape"] = np.array(a.shape, dtype=np.int64)
            blob[key + "#signs"] = np.array([(a <= 0).sum(), (a > 0).sum()], dtype=np.int64)    # (for the guard test)
        else:
            blob[key] = a
    return blob


def outputs(name, fn, args, prefix=""):
    return stored({prefix + name + "/" + key: v for key, v in fn(*args).items()})


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def mismatches(got, want_all):
    """What differs between one case's stored outputs and the golden file's, as a list of messages."""
    bad = []
    for key, value in got.items():
        if key not in want_all:
            bad.append("%s: not in the golden file" % key)
            continue
        want = want_all[key]
        if value.dtype.kind == "U":
            if str(value) != str(want):
                bad.append("%s: digest differs" % key)
        elif value.shape != want.shape or value.dtype != want.dtype:
            bad.append("%s: %s %s against %s %s" % (key, value.dtype, value.shape, want.dtype, want.shape))
        else:
            differ = np.argwhere(_bits(value) != _bits(want))
            if differ.size:
                at = tuple(differ[:4].T)
                bad.append("%s: %d elements differ, first at %s: %s against %s"
                           % (key, len(differ), differ[:4].tolist(), value[at], want[at]))
    return bad


def pack(blob):
    """{key: array} as the six arrays the golden file holds (a zip member per output would cost more than the outputs):
    names, shapes and kinds of the entries, and their values end to end by kind (fp32 bits, integers, digests)."""
    keys = sorted(blob)
    kind = ["s" if blob[k].dtype.kind == "U" else "f" if blob[k].dtype == np.float32 else "i" for k in keys]

    def cat(which, dtype):
        return np.concatenate([np.zeros(0, dtype)] + [blob[k].reshape(-1) for k, c in zip(keys, kind) if c == which])
    return {"keys": np.array(keys), "kinds": np.array(kind),
            "shapes": np.array([",".join(str(n) for n in blob[k].shape) for k in keys]),
            "f32_bits": cat("f", np.float32).view(np.uint32), "i64": cat("i", np.int64),
            "text": np.array([str(blob[k]) for k, c in zip(keys, kind) if c == "s"])}


def unpack(z):
    at, blob = {"f": 0, "i": 0, "s": 0}, {}
    flat = {"f": z["f32_bits"].view(np.float32), "i": z["i64"], "s": z["text"]}
    for key, kind, shape in zip(z["keys"], z["kinds"], z["shapes"]):
        kind, shape = str(kind), tuple(int(n) for n in str(shape).split(",") if n)
        n = 1 if kind == "s" else int(np.prod(shape))
        a = flat[kind][at[kind]:at[kind] + n]
        at[kind] += n
        blob[str(key)] = np.array(str(a[0])) if kind == "s" else a.reshape(shape)
    return blob


_golden = {}


def _parent():
    if not _golden:
        with np.load(os.path.join(GOLDEN_DIR, "norm_parent.npz")) as z:
            _golden.update(unpack(z))
    return _golden


def run_setting(setting, out_path, env=None):
    """The cases of one experiment setting in a fresh process with that setting's environment; returns what the child
    stored ({golden key: array}, keys prefixed with ``setting:``)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), setting, out_path],
                       env=dict(os.environ if env is None else env, **SETTINGS[setting][0]), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, (setting, r.stdout[-3000:])
    with np.load(out_path) as z:
        return unpack(z)


def _case_names():
    return {name for name, _, _ in CASES} | {s + ":" + name for s, (_, cases) in SETTINGS.items() for name, _, _ in cases}


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------
def test_the_golden_file_holds_exactly_the_cases():
    """Exactly the cases of the lists; every stored number finite; every output behind an activation has lanes on both
    sides of it; no stored rstd is 1 / sqrt(eps) of a variance that was clamped to zero (rstd < 0.5 / sqrt(eps): the
    inputs have variance ~0.5, so rstd ~1.4, and under sigma <= 1.3 a clamped one would be >= 1 / (1.3 sqrt(eps)))."""
    gold = _parent()
    keys = set(gold) - {"library_digest"}
    assert {k.split("/")[0] for k in keys} == _case_names()
    for k in sorted(keys):
        a = gold[k]
        if a.dtype.kind == "U":
            continue
        assert a.dtype in (np.float32, np.int64) and np.isfinite(a).all(), k
        base, _, form = k.partition("#")
        switches, name = base.split("/")[1:]
        if "relu" in switches and name in ("out", "dx") and form in ("", "signs"):
            assert (a > 0).all() if form == "signs" else (a <= 0).any() and (a > 0).any(), k
        if name == "coef" and form in ("", "every257"):
            if form == "every257":
                n = int(np.prod(gold[base + "#shape"]))
                rstd = a[np.arange(0, n, 257) >= 3 * (n // 4)]
            else:
                rstd = a.reshape(4, -1)[3]
            assert rstd.size and (rstd > 0).all() and (rstd < 0.5 / np.sqrt(EPS)).all(), (k, rstd.max())


@pytest.mark.parametrize("name,fn,args", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_parents(name, fn, args):
    bad = mismatches(outputs(name, fn, args), _parent())
    assert not bad, bad


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_experiment_paths_equal_the_parents(setting):
    with tempfile.TemporaryDirectory() as tmp:
        got = run_setting(setting, os.path.join(tmp, setting + ".npz"))
    assert {k.split("/")[0] for k in got} == {setting + ":" + name for name, _, _ in SETTINGS[setting][1]}
    bad = mismatches(got, _parent())
    assert not bad, bad


if __name__ == "__main__":      # the child of run_setting: python test_norm_parent_bits_gpu.py <setting> <out.npz>
    _setting, _out = sys.argv[1:3]
    assert all(os.environ.get(k) == v for k, v in SETTINGS[_setting][0].items()), "started without the environment"
    _blob = {}
    for _c in SETTINGS[_setting][1]:
        _blob.update(outputs(*_c, prefix=_setting + ":"))
    np.savez_compressed(_out, **pack(_blob))

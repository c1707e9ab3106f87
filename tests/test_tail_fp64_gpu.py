"""The kernels that close every training step (csrc/gz_optim.hip, csrc/gz_loss.hip) against the fp64 reference of
tail_reference.py, through the C ABI, at every boundary of their launch geometry (tail_cases.py says which size is which
boundary).  Element by element:  |got - ref| <= K u scale, integers and untouched words exactly.  K is a constant measured
on the CPU (`python tests/tail_reference.py --measure`), never fitted to what the kernels give.

Every buffer a launch may write lies in an arena with 64 sentinel words in front of and behind it, and those words are
compared bit for bit afterwards (Arena.read), as are the inputs a launch must leave alone: a stray write to an in-bounds
neighbour fails the case.  Promises between outputs (the second destination holds the same words; a job's result does not
depend on the table it stands in) are bit comparisons too.

As a script (`python tests/test_tail_fp64_gpu.py`) it runs every case and prints the worst ratio to tolerance per kind."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import tail_cases as tc  # noqa: E402
import tail_reference as R  # noqa: E402
from tail_cases import GUARD, GZ_ERR_BAD_SHAPE, GZ_ERR_UNSUPPORTED, SENTINEL, c32, f32  # noqa: E402

pytestmark = pytest.mark.gpu

VIOLATIONS = []             # sentinel words, inputs and bit-equality promises: messages of the case that is running
REPORT = {}                 # {kind: (worst ratio to tolerance, where)}


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------
def _lib():
    from lightning_gan_zoo_amd._lib import lib
    return lib


def _ok(rc, what):
    from lightning_gan_zoo_amd._lib import check
    check(rc, what)


class Arena:
    """Host arrays side by side in one device buffer: [GUARD sentinels | array (+ offset floats) | pad to 4 | GUARD] ...
    Every array starts 16-byte aligned unless its offset says otherwise; at least 2 * GUARD sentinels lie between two."""

    def __init__(self, arrays, offsets=None):
        import torch
        arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        self.slots, pos = [], 0
        for a, off in zip(arrays, offsets or [0] * len(arrays)):
            start = pos + GUARD + off
            self.slots.append((start, a.size))
            pos = (start + a.size + 3) // 4 * 4 + GUARD
        self.host = np.full(pos, SENTINEL, dtype=np.float32)
        self.outside = np.ones(pos, dtype=bool)
        for (s, n), a in zip(self.slots, arrays):
            self.host[s:s + n] = a
            self.outside[s:s + n] = False
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, k=0):
        return self.dev.data_ptr() + 4 * self.slots[k][0]

    def read(self, what):
        """The arrays as the device holds them now; a sentinel that moved is a violation."""
        got = self.dev.cpu().numpy()
        moved = np.flatnonzero((got.view(np.uint32) != self.host.view(np.uint32)) & self.outside)
        if moved.size:
            VIOLATIONS.append("%s: %d sentinel words written, first at word %d of the arena (slots %s)"
                              % (what, moved.size, moved[0], self.slots[:4]))
        return [got[s:s + n].copy() for s, n in self.slots]

    def unchanged(self, what):
        """An input, or the buffers of a refused call: every word as uploaded."""
        got = self.dev.cpu().numpy()
        if not np.array_equal(got.view(np.uint32), self.host.view(np.uint32)):
            VIOLATIONS.append("%s: written to" % what)


def _out(*shape):
    return np.full(shape, SENTINEL, dtype=np.float32)


def _same_bits(a, b, what):
    if not np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)):
        VIOLATIONS.append("%s: not the same bits" % what)


def _ptrs(arena, idxs):
    return (ctypes.c_void_p * len(idxs))(*[arena.ptr(k) for k in idxs])


# ---------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------
def _host_tick(b1, b2, t):
    return f32([t, 1.0 - c32(b1) ** t, math.sqrt(1.0 - c32(b2) ** t)])


def _opt_run(layout, names, call, tag):
    """Uploads the tensors of the layout (one arena per array name), calls `call(count, {name: pointer array}, numel)`
    once for all tensors ("single": once per tensor) and returns {name: the outputs concatenated over the tensors}."""
    tensors, offsets = R.opt_tensors(layout), tc.opt_offsets(layout)
    arenas = {name: Arena([d[name] for d in tensors], offsets) for name in names}
    every = list(range(len(tensors)))
    for idxs in ([[k] for k in every] if layout == "single" else [every]):
        numel = (ctypes.c_longlong * len(idxs))(*[tensors[k]["p"].size for k in idxs])
        _ok(call(len(idxs), {name: _ptrs(a, idxs) for name, a in arenas.items()}, numel), tag)
    return {name: np.concatenate(a.read("%s/%s" % (tag, name))) for name, a in arenas.items()}, arenas


def _adam_call(entry, sw, tick_ptr=None):
    b1, b2, t, gs, zg = sw
    lib = _lib()

    def call(count, p, numel):
        if entry == "step":
            return lib.gz_adam_step(count, p["p"], p["g"], p["m"], p["v"], numel, tc.ADAM_LR, b1, b2, tc.ADAM_EPS, t, gs,
                                    zg, None)
        return lib.gz_adam_step_dev(count, p["p"], p["g"], p["m"], p["v"], numel, tc.ADAM_LR, b1, b2, tc.ADAM_EPS,
                                    tick_ptr, gs, zg, None)
    return call


def _adam(entry, layout):
    res = {}
    for sw in tc.adam_switches():
        tag = tc.adam_tag(*sw)
        tick = Arena([_host_tick(sw[0], sw[1], sw[2])])
        got, _ = _opt_run(layout, "pgmv", _adam_call(entry, sw, tick.ptr()), tag)
        tick.unchanged(tag + "/tick")
        for name in "pmv":
            res["%s/%s" % (tag, name)] = got[name]
        res[tag + "/g"] = got["g"].view(np.uint32)
    return res


def _rmsprop(layout):
    res, lib = {}, _lib()
    for gs, zg in tc.rmsprop_switches():
        def call(count, p, numel):
            return lib.gz_rmsprop_step(count, p["p"], p["g"], p["v"], numel, tc.RMSPROP_LR, tc.RMSPROP_ALPHA,
                                       tc.RMSPROP_EPS, gs, zg, None)
        tag = "gs%g_zg%d" % (gs, zg)
        got, _ = _opt_run(layout, "pgv", call, tag)
        res[tag + "/p"], res[tag + "/v"], res[tag + "/g"] = got["p"], got["v"], got["g"].view(np.uint32)
    return res


def _tick(b1, b2):
    """Five ticks from {0, 0, 0}, one from {999, ., .}; after each chain gz_adam_step_dev on the DEVICE's tick, held to
    the reference at that step and, at the same tolerance, to gz_adam_step (not bit for bit: the device's pow is not
    the host's)."""
    res, lib, ref = {}, _lib(), R.reference("tick", (b1, b2))

    def chain(start, ticks, name, t):
        tick = Arena([f32(start)])
        for k in range(1, ticks + 1):
            _ok(lib.gz_adam_tick(tick.ptr(), b1, b2, None), "adam_tick")
            res["%s/k%d" % (name, k)] = tick.read("tick")[0]
        sw = (b1, b2, t) + R.TICK_DEV_SWITCH
        dev, _ = _opt_run("tick", "pgmv", _adam_call("step_dev", sw, tick.ptr()), "dev%d" % t)
        host, _ = _opt_run("tick", "pgmv", _adam_call("step", sw), "step%d" % t)
        for n in "pmv":
            res["dev%d/%s" % (t, n)] = dev[n]
            o = ref["dev%d/%s" % (t, n)]
            VIOLATIONS.extend(R.compare(dev[n], R.Out(host[n], o.scale, o.kind), "dev%d/%s against gz_adam_step" % (t, n)))
        res["dev%d/g" % t] = dev["g"].view(np.uint32)
        _same_bits(dev["g"], host["g"], "dev%d/g against gz_adam_step" % t)

    chain([0.0, 0.0, 0.0], 5, "from0", 5)
    chain([999.0, 0.125, 0.25], 1, "from999", 1000)
    return res


def _slab_table(lib, params, P, M, V, S):
    """The host table of the twelve parameters; S: the arena of every (parameter, source) slab array in order."""
    table = (ctypes.c_char * lib.gz_adam_src_table_bytes())()
    q = 0
    for k, (d, n) in enumerate(params):
        for s in d["slabs"]:
            _ok(lib.gz_adam_src_add(table, P.ptr(k), M.ptr(k), V.ptr(k), n, S.ptr(q), s.shape[0], s.shape[1]), "src_add")
            q += 1
    return table


def _slabs():
    res, lib = {}, _lib()
    params = [(tc.slab_host(k, n, nzs), n) for k, (n, nzs) in enumerate(tc.slab_params())]
    assert len(params) == lib.gz_adam_src_max_tensors() == tc.SLAB_MAX_TENSORS
    S = Arena([s for d, _ in params for s in d["slabs"]])
    for b1, b2, t, gs in tc.slab_switches():
        P, M, V = (Arena([d[name] for d, _ in params]) for name in "pmv")
        table = _slab_table(lib, params, P, M, V, S)
        _ok(lib.gz_adam_step_from_slabs(table, tc.ADAM_LR, b1, b2, tc.ADAM_EPS, t, gs, None), "adam_step_from_slabs")
        for name, a in (("p", P), ("m", M), ("v", V)):
            res["b%g_%g_t%d_gs%g/%s" % (b1, b2, t, gs, name)] = np.concatenate(a.read("slabs/" + name))
    S.unchanged("the slabs")
    return res


# ---------------------------------------------------------------------------
# loss tails
# ---------------------------------------------------------------------------
def _bce(n):
    x, res = Arena([tc.bce_host(n)["x"]]), {}
    for t in (0, 1):
        loss = Arena([_out(1)])
        _ok(_lib().gz_bce_logits_mean(x.ptr(), loss.ptr(), n, float(t), None), "bce_logits_mean")
        res["t%d/loss" % t] = loss.read("bce loss")[0]
    x.unchanged("bce x")
    return res


def _mse(n):
    d = tc.mse_host(n)
    ab, loss = Arena([d["a"], d["b"]]), Arena([_out(1)])
    _ok(_lib().gz_mse_mean(ab.ptr(0), ab.ptr(1), loss.ptr(), n, None), "mse_mean")
    ab.unchanged("mse inputs")
    return {"loss": loss.read("mse loss")[0]}


def _gp(n):
    s, loss = Arena([tc.gp_host(n)["sumsq"]]), Arena([_out(1)])
    _ok(_lib().gz_gp_penalty(s.ptr(), loss.ptr(), n, None), "gp_penalty")
    s.unchanged("gp sumsq")
    return {"loss": loss.read("gp loss")[0]}


def _loss_bwd(n):
    res, lib = {}, _lib()
    d = tc.bce_host(n)
    inp = Arena([d["x"], d["g"]])
    for t in (0, 1):
        dx = Arena([_out(n)])
        _ok(lib.gz_bce_logits_mean_bwd(inp.ptr(0), inp.ptr(1), dx.ptr(), n, float(t), None), "bce_logits_mean_bwd")
        res["bce_t%d/dx" % t] = dx.read("bce dx")[0]
    inp.unchanged("bce inputs")
    d = tc.mse_host(n)
    inp, da = Arena([d["a"], d["b"], d["g"]]), Arena([_out(n)])
    _ok(lib.gz_mse_mean_bwd(inp.ptr(0), inp.ptr(1), inp.ptr(2), da.ptr(), n, None), "mse_mean_bwd")
    res["mse/da"] = da.read("mse da")[0]
    inp.unchanged("mse inputs")
    d = tc.gp_host(n)
    inp, ds = Arena([d["sumsq"], d["g"]]), Arena([_out(n)])
    _ok(lib.gz_gp_penalty_bwd(inp.ptr(0), inp.ptr(1), ds.ptr(), n, None), "gp_penalty_bwd")
    res["gp/ds"] = ds.read("gp ds")[0]
    inp.unchanged("gp inputs")
    return res


# ---------------------------------------------------------------------------
# vector operations, x / sigma, the spectral-norm backward
# ---------------------------------------------------------------------------
def _vec(n):
    res, lib = {}, _lib()
    for mode in tc.VEC_MODES:
        host = tc.vec_host(n, zero=mode == "zero")["x"]
        for entry, what in (("normalize", "norm"), ("normalize_dot", "dot")):
            x, outs, last = Arena([host]), Arena([_out(n), _out(n)]), Arena([_out(1)])
            out = x.ptr() if mode == "inplace" else outs.ptr(0)
            out2 = None if mode == "no_out2" else outs.ptr(1)
            fn = lib.gz_vec_normalize if entry == "normalize" else lib.gz_vec_normalize_dot
            _ok(fn(x.ptr(), out, out2, last.ptr(), n, tc.SN_EPS, None), "vec_" + entry)
            tag = "%s/%s/" % (mode, entry)
            o0, o1 = outs.read(tag + "out")
            if mode == "inplace":
                _same_bits(o0, _out(n), tag + "the destination not given")
                o0 = x.read(tag + "x")[0]
            else:
                x.unchanged(tag + "x")
            res[tag + "out"] = o0
            if mode == "no_out2":
                _same_bits(o1, _out(n), tag + "the destination not given")
            else:
                res[tag + "out2"] = o1
                _same_bits(o0, o1, tag + "out2 against out")
            res[tag + what] = last.read(tag + what)[0]
    d = tc.vec_host(n)
    ab, out = Arena([d["x"], d["b"]]), Arena([_out(1)])
    _ok(lib.gz_vec_dot(ab.ptr(0), ab.ptr(1), out.ptr(), n, None), "vec_dot")
    ab.unchanged("vec_dot inputs")
    res["dot/out"] = out.read("vec_dot")[0]
    return res


def _mat(R_, L):
    d, lib = tc.mat_host(R_, L), _lib()
    inp = Arena([d[k] for k in ("x", "sigma", "rowdots", "u", "v")])
    div, bwd = Arena([_out(R_, L)]), Arena([_out(R_, L)])
    _ok(lib.gz_div_scalar(inp.ptr(0), inp.ptr(1), div.ptr(), R_ * L, None), "div_scalar")
    _ok(lib.gz_spectral_norm_bwd(inp.ptr(0), inp.ptr(2), inp.ptr(3), inp.ptr(4), inp.ptr(1), bwd.ptr(), R_, L, None),
        "spectral_norm_bwd")
    inp.unchanged("mat inputs")
    return {"div/out": div.read("div")[0].reshape(R_, L), "snbwd/out": bwd.read("snbwd")[0].reshape(R_, L)}


# ---------------------------------------------------------------------------
# power iteration, sigma term
# ---------------------------------------------------------------------------
class _PowerJob:
    """The buffers of one job: W; the outputs u, v, us, vs, sigma in one arena; the workspace, poisoned, in another."""

    def __init__(self, R_, L, zero=False):
        d = tc.power_host(R_, L, zero=zero)
        self.R, self.L = R_, L
        self.W = Arena([d["W"]])
        self.out = Arena([d["u"], d["v"], _out(R_), _out(L), _out(1)])
        self.ws = Arena([np.full(_lib().gz_sn_workspace_floats(R_, L), np.nan, dtype=np.float32)])

    def add(self, table):
        o = self.out
        return _lib().gz_sn_add(table, self.W.ptr(), o.ptr(0), o.ptr(1), o.ptr(2), o.ptr(3), o.ptr(4), self.ws.ptr(),
                                self.R, self.L)

    def read(self, what):
        u, v, us, vs, sigma = self.out.read(what)
        self.ws.read(what + " workspace")
        self.W.unchanged(what + " W")
        _same_bits(u, us, what + ": us against u")
        _same_bits(v, vs, what + ": vs against v")
        return {"u": u, "us": us, "v": v, "vs": vs, "sigma": sigma}


def _power_table(jobs):
    table = (ctypes.c_char * _lib().gz_sn_table_bytes())()
    for jb in jobs:
        _ok(jb.add(table), "sn_add")
    return table


def _power(R_, L, zero=False):
    """One job, two iterations on the same buffers."""
    jb, res = _PowerJob(R_, L, zero), {}
    for it in (1, 2):
        _ok(_lib().gz_sn_power_iteration(_power_table([jb]), tc.SN_EPS, None), "sn_power_iteration")
        for k, a in jb.read("power %dx%d it%d" % (R_, L, it)).items():
            res["it%d/%s" % (it, k)] = a
    return res


def _power_zero(R_, L):
    return _power(R_, L, zero=True)


@functools.lru_cache(maxsize=None)
def _power_single(R_, L):
    return _power(R_, L)


def _sigma_term(groups, rpg, R_, L):
    d, lib = tc.sigma_host(groups, rpg, R_, L), _lib()
    inp = Arena([d[k] for k in ("rowsums", "rstd", "sigma", "u", "v")])
    coefs = Arena([np.full(lib.gz_sn_sigma_coef_floats(groups), np.nan, dtype=np.float32)])
    term = Arena([_out(R_, L)])
    _ok(lib.gz_sn_sigma_term(inp.ptr(0), inp.ptr(1), inp.ptr(2), inp.ptr(3), inp.ptr(4), coefs.ptr(), term.ptr(),
                             groups * rpg, groups, R_, L, tc.SIGMA_EPS, None), "sn_sigma_term")
    inp.unchanged("sigma term inputs")
    coefs.read("sigma term coefs")
    return {"term": term.read("sigma term")[0].reshape(R_, L)}


DRIVERS = {name[1:]: fn for name, fn in list(globals().items()) if name[1:] in R.REFERENCE and name.startswith("_")}
assert DRIVERS.keys() == R.REFERENCE.keys()


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------
def check(name, args):
    """One case: the mismatches of every key, and what the arenas and the bit comparisons found."""
    del VIOLATIONS[:]
    got = _power_single(*args) if name == "power" else DRIVERS[name](*args)
    ref, what = R.reference(name, tuple(args)), "%s%s" % (name, tuple(args))
    bad = list(VIOLATIONS) + ([] if got.keys() == ref.keys() else ["%s: keys %s" % (what, sorted(set(got) ^ set(ref)))])
    worst = {}
    for key in sorted(set(got) & set(ref)):
        bad += R.compare(got[key], ref[key], what + "/" + key)
        kind = ref[key].kind
        if kind != "int":
            w = R.worst(got[key], ref[key])
            worst[kind] = max(worst.get(kind, 0.0), w)
            if w > REPORT.get(kind, (-1.0, ""))[0]:
                REPORT[kind] = (w, what + "/" + key)
    for kind, w in sorted(worst.items()):
        print("worst ratio to tolerance, %-10s %.4f  (K = %d) in %s" % (kind, w, R.K[kind], what))
    return bad


def _id(case):
    return "%s_%s" % (case[0], "x".join(str(a) for a in case[1]))


@pytest.mark.parametrize("name,args", tc.CASES, ids=[_id(c) for c in tc.CASES])
def test_agrees_with_the_fp64_reference(name, args):
    bad = check(name, args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("order", ["listed", "reversed"])
def test_power_iteration_of_a_job_does_not_depend_on_its_table(order):
    """Four mixed jobs in one table (the job-prefix lookup of all three multi-workgroup launches): each job's words are
    those of its single-job run, since no sum's order depends on the table."""
    del VIOLATIONS[:]
    shapes = tc.POWER_TABLE if order == "listed" else tc.POWER_TABLE[::-1]
    assert len(shapes) == _lib().gz_sn_max_jobs()
    jobs = [_PowerJob(R_, L) for R_, L in shapes]
    _ok(_lib().gz_sn_power_iteration(_power_table(jobs), tc.SN_EPS, None), "sn_power_iteration")
    for jb in jobs:
        got, single = jb.read("table job %dx%d" % (jb.R, jb.L)), _power_single(jb.R, jb.L)
        for k, a in got.items():
            _same_bits(a, single["it1/" + k], "job %dx%d in the %s table, %s against its single-job run"
                       % (jb.R, jb.L, order, k))
    assert not VIOLATIONS, "\n".join(VIOLATIONS)


def test_refused_calls_return_their_code_and_write_nothing():
    del VIOLATIONS[:]
    lib = _lib()
    # optimizers: count 0, count 25, step 0
    tensors = [tc.opt_tensor_host("refused", k, 8) for k in range(tc.OPT_MAX_TENSORS + 1)]
    arenas = {n: Arena([d[n] for d in tensors]) for n in "pgmv"}
    tick = Arena([_host_tick(0.5, 0.999, 3)])
    every = list(range(len(tensors)))
    p = {n: _ptrs(a, every) for n, a in arenas.items()}
    numel = (ctypes.c_longlong * len(every))(*[8] * len(every))
    for count in (0, tc.OPT_MAX_TENSORS + 1):
        assert lib.gz_adam_step(count, p["p"], p["g"], p["m"], p["v"], numel, tc.ADAM_LR, 0.5, 0.999, tc.ADAM_EPS, 3,
                                1.0, 1, None) == GZ_ERR_BAD_SHAPE
        assert lib.gz_adam_step_dev(count, p["p"], p["g"], p["m"], p["v"], numel, tc.ADAM_LR, 0.5, 0.999, tc.ADAM_EPS,
                                    tick.ptr(), 1.0, 1, None) == GZ_ERR_BAD_SHAPE
        assert lib.gz_rmsprop_step(count, p["p"], p["g"], p["v"], numel, tc.RMSPROP_LR, tc.RMSPROP_ALPHA,
                                   tc.RMSPROP_EPS, 1.0, 1, None) == GZ_ERR_BAD_SHAPE
    assert lib.gz_adam_step(1, p["p"], p["g"], p["m"], p["v"], numel, tc.ADAM_LR, 0.5, 0.999, tc.ADAM_EPS, 0, 1.0, 1,
                            None) == GZ_ERR_BAD_SHAPE
    # Adam from slabs: a thirteenth parameter, a fifth source, a numel that is no multiple of 4
    slabs = Arena([_out(8, 16)])
    table = (ctypes.c_char * lib.gz_adam_src_table_bytes())()

    def add(k, numel_k=8):
        return lib.gz_adam_src_add(table, arenas["p"].ptr(k), arenas["m"].ptr(k), arenas["v"].ptr(k), numel_k, slabs.ptr(),
                                   8, 16)
    assert add(0, 6) == GZ_ERR_BAD_SHAPE
    for k in range(tc.SLAB_MAX_TENSORS):
        assert add(k) == 0
    assert add(tc.SLAB_MAX_TENSORS) == GZ_ERR_UNSUPPORTED
    for _ in range(tc.SLAB_MAX_SRC - 1):
        assert add(0) == 0
    assert add(0) == GZ_ERR_UNSUPPORTED
    assert lib.gz_adam_step_from_slabs(table, tc.ADAM_LR, 0.5, 0.999, tc.ADAM_EPS, 0, 1.0, None) == GZ_ERR_BAD_SHAPE
    # power iteration: a fifth job, L % 4 != 0
    jb = _PowerJob(3, 8)
    table = _power_table([jb] * lib.gz_sn_max_jobs())
    assert jb.add(table) == GZ_ERR_UNSUPPORTED
    o = jb.out
    assert lib.gz_sn_add((ctypes.c_char * lib.gz_sn_table_bytes())(), jb.W.ptr(), o.ptr(0), o.ptr(1), o.ptr(2), o.ptr(3),
                         o.ptr(4), jb.ws.ptr(), 4, 6) == GZ_ERR_BAD_SHAPE
    # sigma term: nine groups, rows % groups != 0, L % 4 != 0
    d = tc.sigma_host(9, 2, 3, 8)
    inp = Arena([d[k] for k in ("rowsums", "rstd", "sigma", "u", "v")])
    coefs, term = Arena([_out(9 * 16)]), Arena([_out(3, 8)])
    for rows, groups, L in ((18, 9, 8), (17, 2, 8), (16, 2, 6)):
        assert lib.gz_sn_sigma_term(inp.ptr(0), inp.ptr(1), inp.ptr(2), inp.ptr(3), inp.ptr(4), coefs.ptr(), term.ptr(),
                                    rows, groups, 3, L, tc.SIGMA_EPS, None) == GZ_ERR_BAD_SHAPE
    for what, a in list(arenas.items()) + [("tick", tick), ("slabs", slabs), ("W", jb.W), ("power outputs", jb.out),
                                           ("workspace", jb.ws), ("sigma inputs", inp), ("coefs", coefs), ("term", term)]:
        a.unchanged("refused calls: " + what)
    assert not VIOLATIONS, "\n".join(VIOLATIONS)


def main():
    """Every case, and per kind the worst ratio to tolerance (a report; the tests above are the check)."""
    bad = []
    for name, args in tc.CASES:
        bad += check(name, args)
    print("compared %d cases" % len(tc.CASES))
    for kind, (w, where) in sorted(REPORT.items()):
        print("WORST ratio to tolerance, %-10s %.4f  (K = %d) at %s" % (kind, w, R.K[kind], where))
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

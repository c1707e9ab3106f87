"""The pooling, resize and ResNet spatial kernels (csrc/gz_infer.hip, first half of csrc/gz_resnet.hip) against the fp64
reference of spatial_reference.py, through the C ABI, at every boundary of their launch geometry (spatial_cases.py says
which size is which boundary, and for every pooling row which kernel runs: gz_pool2d_plan is asked again before each
launch).  Element by element:  |got - ref| <= K u scale with K derived in spatial_reference.py (measured on the CPU for
the bilinear kernels), never fitted to what the kernels give; max pooling, upsample2 forward, relu and the identity
resize bit for bit.

Every output lies in an arena with 64 sentinel words in front of and behind it, compared bit for bit afterwards, as are
the inputs; every arena slot is 16-byte aligned except the input of the one misaligned global average.

As a script (`python tests/test_spatial_fp64_gpu.py [--kinds pool]`) it runs every case (of the named kinds) and prints
the worst ratio to tolerance per kind; test_pooling_under_the_experiment_switches runs it that way in child processes
whose switches send the pooling table through the plane kernel and the flat kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import spatial_cases as sc  # noqa: E402
import spatial_reference as R  # noqa: E402
from spatial_cases import GZ_ERR_BAD_SHAPE  # noqa: E402
from test_tail_fp64_gpu import VIOLATIONS, Arena, _lib, _ok, _out, _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

REPORT = {}                 # {kind: (worst ratio to tolerance, where)}
SHARED_MEMORY = {}          # {"bytes": the device's shared memory per block, as read for the widest band}
CHUNK = 4 << 20             # input floats per piece of a reference (the large pooling cases: 17 M floats)


def _switches():
    """The name (spatial_cases.KNOBS) of the pooling switches this process runs under."""
    if os.environ.get("GZ_EXPERIMENTS", "0")[:1] in ("", "0"):
        return "default"
    group, plane = "GZ_NO_POOL_GROUP" in os.environ, "GZ_NO_POOL_PLANE" in os.environ
    assert group or not plane, "GZ_NO_POOL_PLANE alone is not a setting of the table"
    return "no_group_no_plane" if plane else "no_group" if group else "default"


def _held(got, out, what, bad):
    """One output against its reference: the mismatches into `bad`, the worst ratio into REPORT."""
    bad += R.compare(got, out, what)
    if out.tol is not None:
        w = R.worst(got, out)
        if w > REPORT.get(out.kind, (-1.0, ""))[0]:
            REPORT[out.kind] = (w, what)


# ---------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------
def _pool(c):
    bad, lib, knobs = [], _lib(), _switches()
    OH, OW = R.out_size(c.H, c.KS, c.S, c.P), R.out_size(c.W, c.KS, c.S, c.P)
    x = sc.pool_host(c)
    ax = Arena([x], [1 if c.misaligned else 0])
    assert (ax.ptr() % 16 != 0) == c.misaligned
    plan = sc.pool_plan(c, -1)                              # the launch THIS process makes
    if knobs == "default":
        assert plan == c.plan, (c, plan)
    assert plan.split()[0] == sc.pool_branch_under(c, knobs), (c, knobs, plan)
    if c.lds_check and plan.startswith("band"):
        import torch
        SHARED_MEMORY["bytes"] = torch.cuda.get_device_properties(0).shared_memory_per_block
        print("shared memory per block: %d bytes; the band kernel at W = %d asks for %d"
              % (SHARED_MEMORY["bytes"], c.W, 17 * c.W * 4))
        assert 17 * c.W * 4 <= SHARED_MEMORY["bytes"], "the dispatch accepts a width whose LDS request does not fit"
    step = max(1, CHUNK // (c.H * c.W))
    for mode in c.modes:
        ay = Arena([_out(c.planes * OH * OW)])
        _ok(lib.gz_pool2d(ax.ptr(), ay.ptr(), c.planes, c.H, c.W, OH, OW, c.KS, c.S, c.P, mode, None), "pool2d")
        got = ay.read("%s mode %d y" % (c.id, mode))[0].reshape(c.planes, OH, OW)
        for p0 in range(0, c.planes, step):
            _held(got[p0:p0 + step], R.pool2d_out(x[p0:p0 + step], c.KS, c.S, c.P, mode),
                  "%s mode %d planes %d.. [%s]" % (c.id, mode, p0, plan), bad)
    ax.unchanged(c.id + " x")
    return bad


# ---------------------------------------------------------------------------
# AvgPool2d(3, 2, 1), nearest 2x upsampling, forward and backward
# ---------------------------------------------------------------------------
def _spatial(c):
    bad, lib = [], _lib()
    a = sc.spatial_host(c)
    OH, OW = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
    ain = Arena([a])
    if c.kind == "avgpool3s2_fwd":
        out, ref = Arena([_out(c.planes, OH, OW)]), R.sum_out(*R.avgpool3s2_fwd(a), "spatial_sum")
        rc = lib.gz_avgpool3s2_fwd(ain.ptr(), out.ptr(), c.planes, c.H, c.W, OH, OW, None)
    elif c.kind == "avgpool3s2_bwd":
        out, ref = Arena([_out(c.planes, c.H, c.W)]), R.sum_out(*R.avgpool3s2_bwd(a, c.H, c.W), "spatial_sum")
        rc = lib.gz_avgpool3s2_bwd(ain.ptr(), out.ptr(), c.planes, c.H, c.W, OH, OW, None)
    elif c.kind == "upsample2_fwd":
        out, ref = Arena([_out(c.planes, 2 * c.H, 2 * c.W)]), R.Out(R.upsample2_fwd(a), None, "upsample2_fwd")
        rc = lib.gz_upsample2_fwd(ain.ptr(), out.ptr(), c.planes, c.H, c.W, None)
    else:
        out, ref = Arena([_out(c.planes, c.H, c.W)]), R.sum_out(*R.upsample2_bwd(a), 4, "spatial_sum")
        rc = lib.gz_upsample2_bwd(ain.ptr(), out.ptr(), c.planes, c.H, c.W, None)
    _ok(rc, c.kind)
    _held(out.read(c.id)[0], ref, c.id, bad)
    ain.unchanged(c.id + " input")
    return bad


# ---------------------------------------------------------------------------
# activation, residual tail
# ---------------------------------------------------------------------------
def _act32(o, act, slope):
    """act_fwd of float32 words in float32: what act_out must hold, bit for bit."""
    with np.errstate(under="ignore"):
        return np.where(o > 0, o, np.float32(0) if act == sc.ACT_RELU else o * np.float32(slope)).astype(np.float32)


def _act(c):
    bad, lib = [], _lib()
    a, _ = sc.ew_host(c)
    ain = Arena([a])
    for act, slope in sc.ACTS:
        y = Arena([_out(c.count)])
        _ok(lib.gz_act_fwd(ain.ptr(), y.ptr(), c.count, act, slope, None), "act_fwd")
        _held(y.read(c.id)[0], R.act_out(a, act, slope), "%s act %d slope %g" % (c.id, act, slope), bad)
    ain.unchanged(c.id + " x")
    return bad


def _axpby(c):
    bad, lib = [], _lib()
    a, b = sc.ew_host(c)
    act, slope = sc.AXPBY_ACT
    inp = Arena([a, b])
    for form in sc.AXPBY_FORMS:
        outs = Arena([_out(c.count), _out(c.count)])
        pb = None if form == "no_b" else inp.ptr(1)
        pact = None if form == "no_act_out" else outs.ptr(1)
        _ok(lib.gz_axpby(inp.ptr(0), sc.AXPBY_ALPHA, pb, sc.AXPBY_BETA, outs.ptr(0), pact, c.count, act, slope, None),
            "axpby")
        out, act_out = outs.read("%s %s" % (c.id, form))
        _held(out, R.axpby_out(a, sc.AXPBY_ALPHA, None if form == "no_b" else b, sc.AXPBY_BETA), "%s %s" % (c.id, form), bad)
        _same_bits(act_out, _out(c.count) if form == "no_act_out" else _act32(out, act, slope),
                   "%s %s: act_out against act_fwd of the out that was written" % (c.id, form))
    inp.unchanged(c.id + " inputs")
    return bad


# ---------------------------------------------------------------------------
# bilinear resize, generator output -> Inception input
# ---------------------------------------------------------------------------
def _resize(c):
    bad, lib = [], _lib()
    x = sc.resize_host(c)
    ax, ay = Arena([x]), Arena([_out(c.planes, c.OH, c.OW)])
    _ok(lib.gz_resize_bilinear(ax.ptr(), ay.ptr(), c.planes, c.H, c.W, c.OH, c.OW, c.mul, c.add, None), "resize_bilinear")
    got = ay.read(c.id)[0].reshape(c.planes, c.OH, c.OW)
    _held(got, R.resize_out(x, c.OH, c.OW, c.mul, c.add), c.id, bad)
    want, tol = sc.CONSTANT * c.mul + c.add, R.constant_plane_tol(sc.CONSTANT, c.mul, c.add)
    for p in sc.constant_planes(c):
        err = np.abs(got[p].astype(np.float64) - want).max()
        if not err <= tol:
            bad.append("%s: constant plane %d is off by %.3g, more than 4 u (|c mul| + |add|) = %.3g" % (c.id, p, err, tol))
    ax.unchanged(c.id + " x")
    return bad


def _samples(c):
    bad, lib = [], _lib()
    x = sc.samples_host(c)
    ax, ay = Arena([x]), Arena([_out(c.N, 3, c.OH, c.OW)])
    _ok(lib.gz_samples_to_inception_input(ax.ptr(), ay.ptr(), c.N, c.C, c.H, c.W, c.OH, c.OW, c.mul, c.add, None),
        "samples_to_inception_input")
    _held(ay.read(c.id)[0], R.samples_out(x, c.OH, c.OW, c.mul, c.add), c.id, bad)
    ax.unchanged(c.id + " x")
    return bad


DRIVERS = {"pool": _pool, "act": _act, "axpby": _axpby, "resize": _resize, "samples": _samples}
DRIVERS.update({op: _spatial for op in sc.SPATIAL_OPS})


def check(c):
    """One case: the mismatches, and what the arenas and the bit comparisons found."""
    del VIOLATIONS[:]
    bad = DRIVERS[c.kind](c)
    return bad + list(VIOLATIONS)


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------
def _cases(kinds, big=False):
    return [c for c in sc.CASES if c.kind in kinds and bool(getattr(c, "big", False)) == big]


def _param(kinds, big=False):
    cases = _cases(kinds, big)
    return pytest.mark.parametrize("c", cases, ids=[c.id for c in cases])


@_param(("pool",))
def test_pooling_agrees_with_the_fp64_reference(c):
    bad = check(c)
    assert not bad, "\n".join(bad)


@_param(("pool",), big=True)
def test_pooling_groups_beyond_the_grid_agree_with_the_fp64_reference(c):
    """8192 workgroups, more groups than that: a workgroup's second group lands on LDS images its first one filled."""
    bad = check(c)
    assert not bad, "\n".join(bad)


@_param(sc.SPATIAL_OPS)
def test_avgpool3s2_and_upsample2_agree_with_the_fp64_reference(c):
    bad = check(c)
    assert not bad, "\n".join(bad)


@_param(("act", "axpby"))
def test_activation_and_residual_tail_agree_with_the_fp64_reference(c):
    bad = check(c)
    assert not bad, "\n".join(bad)


@_param(("resize",))
def test_resize_agrees_with_the_fp64_reference(c):
    bad = check(c)
    assert not bad, "\n".join(bad)


@_param(("samples",))
def test_samples_to_inception_agrees_with_the_fp64_reference(c):
    bad = check(c)
    assert not bad, "\n".join(bad)


def test_counts_that_are_no_multiple_of_four_are_refused_and_write_nothing():
    del VIOLATIONS[:]
    lib = _lib()
    for n in sc.EW_BAD_COUNTS:
        a, b = (np.arange(n, dtype=np.float32) - 3 for _ in range(2))
        inp, outs = Arena([a, b]), Arena([_out(n), _out(n)])
        assert lib.gz_act_fwd(inp.ptr(0), outs.ptr(0), n, sc.ACT_RELU, 0.0, None) == GZ_ERR_BAD_SHAPE
        assert lib.gz_axpby(inp.ptr(0), 1.0, inp.ptr(1), 0.1, outs.ptr(0), outs.ptr(1), n, sc.ACT_LRELU, 0.2,
                            None) == GZ_ERR_BAD_SHAPE
        inp.unchanged("refused calls: inputs")
        outs.unchanged("refused calls: outputs")
    assert not VIOLATIONS, "\n".join(VIOLATIONS)


CHILD_TIMEOUT = 300


def test_pooling_under_the_experiment_switches():
    """The pooling table once without the group kernels (planes up to 8192 floats take the plane kernel, the others the
    flat kernel) and once without the plane kernel too (everything takes the flat kernel), against the same reference.
    The switches are read once per process: one child process per setting, one after the other, each under its own
    time limit; a child that ends on a signal or at its limit ends the test before another starts."""
    for knobs in ("no_group", "no_group_no_plane"):
        env = dict(os.environ, GZ_EXPERIMENTS="1", **sc.KNOB_ENV[knobs])
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kinds", "pool"], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.fail("%s: the child did not end within %d s: %s" % (knobs, CHILD_TIMEOUT, str(e.stdout)[-2000:]))
        print(knobs, r.stdout[-1500:])
        assert r.returncode >= 0, "%s: the child ended on signal %d: %s" % (knobs, -r.returncode, r.stdout[-3000:])
        assert r.returncode == 0 and "compared %d cases under %s" % (len(sc.POOL_ROWS), knobs) in r.stdout, (
            knobs, r.stdout[-3000:])


def main(argv):
    """Every case (of --kinds), and per kind the worst ratio to tolerance (a report; the tests above are the check)."""
    kinds = argv[argv.index("--kinds") + 1].split(",") if "--kinds" in argv else sorted(DRIVERS)
    cases = [c for c in sc.CASES if c.kind in kinds]
    bad = []
    for c in cases:
        bad += check(c)
    print("compared %d cases under %s" % (len(cases), _switches()))
    for kind, (w, where) in sorted(REPORT.items()):
        print("WORST ratio to tolerance, %-12s %.4f at %s" % (kind, w, where))
    if SHARED_MEMORY:
        print("shared memory per block read for the widest band: %d bytes" % SHARED_MEMORY["bytes"])
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

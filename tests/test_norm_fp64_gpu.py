"""The normalisation kernels (csrc/gz_norm.hip) against an fp64 reference, at every launch geometry that
test_norm_parent_bits_gpu.py pins.  That file says the bits have not moved; this one says they are right, and it is the
one that survives a change of summation order.

Same cases, same drivers, same seeded inputs; the raw outputs (not the digest form) are compared key by key and element
by element with the twin of the driver in norm_reference.py:  |got - ref| <= K u scale (+ what an activation mask that
may fall either way allows), untouched words and integers exactly.  K and the band are constants measured on the CPU
(`python tests/norm_reference.py --measure`), never fitted to what the kernels give.

The experiment settings are read once per process, so each runs in a fresh child (this file as a script) that exits
non-zero with the list of mismatches."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import norm_reference as R  # noqa: E402
import test_norm_parent_bits_gpu as bits  # noqa: E402

pytestmark = pytest.mark.gpu


def check(name, fn, args, report=None):
    """One case: the mismatches of every key (report: {kind: worst ratio to tolerance}, updated)."""
    got, ref = fn(*args), R.reference(fn.__name__.lstrip("_"), tuple(args))
    bad = [] if got.keys() == ref.keys() else ["%s: keys %s" % (name, sorted(set(got) ^ set(ref)))]
    for key in sorted(set(got) & set(ref)):
        bad += R.compare(got[key], ref[key], name + "/" + key)
        if report is not None and ref[key].kind != "int":
            w = R.worst(got[key], ref[key])
            if w > report.get(ref[key].kind, (-1.0, ""))[0]:
                report[ref[key].kind] = (w, name + "/" + key)
    return bad


@pytest.mark.parametrize("name,fn,args", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_agrees_with_the_fp64_reference(name, fn, args):
    bad = check(name, fn, args)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("setting", list(bits.SETTINGS))
def test_experiment_paths_agree_with_the_fp64_reference(setting):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), setting],
                       env=dict(os.environ, **bits.SETTINGS[setting][0]), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, (setting, r.stdout[-6000:])
    assert "compared %d cases" % len(bits.SETTINGS[setting][1]) in r.stdout, r.stdout[-2000:]


def main(setting):
    """The child: the cases of one setting (or, as `default`, the plain list -- a report, not a test)."""
    if setting == "default":
        cases = bits.CASES
    else:
        env, cases = bits.SETTINGS[setting]
        assert all(os.environ.get(k) == v for k, v in env.items()), "started without the environment"
    bad, report = [], {}
    for case in cases:
        bad += check(*case, report=report)
    print("compared %d cases" % len(cases))
    for kind, (w, where) in sorted(report.items()):
        print("worst ratio to tolerance, %-8s %.4f  (K = %d) at %s" % (kind, w, R.K[kind], where))
    print("\n".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))

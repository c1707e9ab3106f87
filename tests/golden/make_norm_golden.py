"""Writes tests/golden/norm_parent.npz: what the entry points of csrc/gz_norm.hip computed BEFORE the file's bodies were
written once (row walk, coefficient record, element terms, finalize, slice walk), on the cases of
tests/test_norm_parent_bits_gpu.py, which holds today's kernels to these bits.  Only the outputs (large ones as digest
plus every 257th element) and that library's ``gz_source_digest()`` are stored; the inputs are the seeded ones of the
test.  The experiment settings are recorded like the test runs them, one child process each; the parent read
GZ_BN_FINALIZE_LAUNCH without looking at GZ_EXPERIMENTS, so the test's spelling (both set) is also the parent's.

Needs an MI355X and the library of the commit before that refactor (its C ABI is today's):

    GZ_LIB=<that commit's libgz_hip.so> python tests/golden/make_norm_golden.py [out.npz]

Refuses to write a file that the guard test would reject (a clamped variance, an activation with one side only).

A file written again (after a change of summation order, or a kernel fix) is only acceptable together with a passing
tests/test_norm_fp64_gpu.py on the library that wrote it: recorded bits say what was computed, the fp64 reference that
it was right."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_norm_parent_bits_gpu as T  # noqa: E402


def main(out):
    from lightning_gan_zoo_amd._lib import lib
    assert os.environ.get("GZ_LIB"), "GZ_LIB must name the parent commit's library"
    blob = {"library_digest": np.array(lib.gz_source_digest().decode())}
    for case in T.CASES:
        blob.update(T.outputs(*case))
    with tempfile.TemporaryDirectory() as tmp:
        for setting in T.SETTINGS:
            blob.update(T.run_setting(setting, os.path.join(tmp, setting + ".npz")))
    np.savez_compressed(out, **T.pack(blob))
    T._golden.clear()
    T._golden.update(blob)
    T.test_the_golden_file_holds_exactly_the_cases()
    print("wrote", out, os.path.getsize(out), "bytes,", len(blob), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "norm_parent.npz"))

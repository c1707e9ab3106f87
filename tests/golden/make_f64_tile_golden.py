"""Writes tests/golden/f64_tile_parent.npz: what gz_kid_sums, gz_feature_moments, gz_sqrtm_product and
gz_sqrtm_trace_norm computed BEFORE their common 64 x 64 fp64 MFMA tile was factored into csrc/gz_f64_tile.h, on the
cases of tests/test_f64_tile_parent_bits_gpu.py, which holds today's kernels to these bits.  Only the outputs and that
library's ``gz_source_digest()`` are stored; the inputs are the seeded ones of the tests.

Needs an MI355X and the library of the commit before that refactor (its C ABI is today's):

    GZ_LIB=<that commit's libgz_hip.so> python tests/golden/make_f64_tile_golden.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from test_f64_tile_parent_bits_gpu import CASES, outputs  # noqa: E402


def main(out):
    from lightning_gan_zoo_amd._lib import lib
    blob = {"library_digest": np.array(lib.gz_source_digest().decode())}
    for case in CASES:
        blob.update(outputs(*case))
    np.savez_compressed(out, **blob)
    print("wrote", out, os.path.getsize(out), "bytes", {k: v.shape for k, v in blob.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "f64_tile_parent.npz"))

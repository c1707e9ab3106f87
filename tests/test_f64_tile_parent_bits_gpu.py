"""The fp64 MFMA kernels (csrc/gz_kid.hip, gz_moments.hip, gz_sqrtm.hip) against the bits they produced BEFORE their
common tile was factored into csrc/gz_f64_tile.h.  The other tests of these kernels hold them to forward bounds that any
order of summation satisfies; the tile core fixes the order (slot map, steps, chunks, the folds), and this is the test
that notices if it moves.  tests/golden/f64_tile_parent.npz was written by tests/golden/make_f64_tile_golden.py with the
library of the commit before that refactor; the inputs are the seeded ones of the kernels' own tests.

The shapes are the smallest that cross every boundary of the core: a tile tail (17), two tiles (65, 67, 70), three
bands (150), a chunk tail (7, 17, 33, 48 = 32 + 16) and several chunks (48, 65, 67)."""
import os

import numpy as np
import pytest

from fid_support import PRODUCT_COEFFS, product_operands
from helpers import GOLDEN_DIR
from kid_support import mixed_sign_codes, subset_rows
from moments_support import offset_activations

pytestmark = pytest.mark.gpu

KID_SHAPES = [(17, 7, 3), (65, 48, 2), (150, 48, 7)]                      # (m, d, S)
KID_KERNELS = [(3, None, 1.0), (2, 0.05, 1.0)]                            # (degree, gamma, coef0)
MOMENTS_SHAPES = [(33, 17), (67, 70)]                                     # (n, d)
PRODUCT_DIMS = [17, 65]


def _kid(m, d, S, degree, gamma, coef0):
    from lightning_gan_zoo_amd import eval as E
    from test_kid_gpu import _dev
    g, r = mixed_sign_codes(d)
    return {"sums": E.kid_sums_device(_dev(g), _dev(r), subset_rows(m, S, seed=m * 31 + d), degree=degree, gamma=gamma,
                                      coef0=coef0)}


def _moments(n, d):
    from test_moments_gpu import device_moments
    mean, cov = device_moments(offset_activations(n, d))
    return {"mean": mean, "cov": cov}


def _product(d, alpha, beta):
    from test_fid_device_gpu import _product as product
    return {"c": product(*product_operands(d), alpha, beta)}


def _trace_norm(d):
    from test_fid_device_gpu import _trace_norm as trace_norm
    return {"trace_norm": trace_norm(product_operands(d)[0])}


CASES = ([("kid_m%d_d%d_S%d_deg%d_g%s_c%g" % (s + k), _kid, s + k) for s in KID_SHAPES for k in KID_KERNELS]
         + [("moments_n%d_d%d" % s, _moments, s) for s in MOMENTS_SHAPES]
         + [("product_d%d_a%g_b%g" % ((d,) + c), _product, (d,) + c) for d in PRODUCT_DIMS for c in PRODUCT_COEFFS]
         + [("trace_norm_d%d" % d, _trace_norm, (d,)) for d in PRODUCT_DIMS])


def outputs(name, fn, args):
    """{golden key: fp64 array} of one case, from the library in use."""
    return {name + "/" + key: np.asarray(v, dtype=np.float64) for key, v in fn(*args).items()}


_golden = {}


def _parent():
    if not _golden:
        with np.load(os.path.join(GOLDEN_DIR, "f64_tile_parent.npz")) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def test_the_golden_file_holds_exactly_the_cases():
    keys = set(_parent()) - {"library_digest"}
    assert {k.split("/")[0] for k in keys} == {name for name, _, _ in CASES}
    assert all(_parent()[k].dtype == np.float64 and np.isfinite(_parent()[k]).all() for k in keys)


@pytest.mark.parametrize("name,fn,args", CASES, ids=[c[0] for c in CASES])
def test_bits_equal_the_parents(name, fn, args):
    got = outputs(name, fn, args)
    for key, value in got.items():
        want = _parent()[key]
        assert value.shape == want.shape, key
        differ = np.argwhere(value.view(np.uint64) != want.view(np.uint64))
        assert differ.size == 0, (key, len(differ), differ[:8], value[tuple(differ[:8].T)], want[tuple(differ[:8].T)])

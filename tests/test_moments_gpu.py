"""Mean and covariance on the device (csrc/gz_moments.hip, eval.feature_moments_device) against numpy's fp64 evaluation.

Every entry is held to the first-order forward bounds of moments_support.moments_bounds, which cover ANY order of fp64
summation: numpy and the kernel both lie within one bound of the exact value, so the test allows 2 x bound.  Observed
worst error / bound on an MI355X, per shape (n, d): see DESIGN.md 3.4.5."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR
from moments_support import SHAPES, activations, exact_case, moments_bounds, offset_activations

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_moments(x):
    from lightning_gan_zoo_amd import eval as E
    mean, cov = E.feature_moments_device(_dev(x))
    assert mean.is_cuda and cov.is_cuda and mean.dtype == cov.dtype == torch.float64
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize("n,d", SHAPES)
def test_moments_within_twice_the_forward_bound(n, d):
    x = offset_activations(n, d)
    want_mean, want_cov = np.mean(x, axis=0), np.atleast_2d(np.cov(x, rowvar=False))
    e_mean, e_cov = moments_bounds(x)
    scale = np.sqrt(np.outer(np.diagonal(want_cov), np.diagonal(want_cov)))
    assert (e_cov > 0).all() and (e_cov <= 1e-11 * scale).all(), float((e_cov / scale).max())      # not vacuous
    mean, cov = device_moments(x)
    assert mean.shape == (d,) and cov.shape == (d, d) and np.isfinite(cov).all()
    err_mean, err_cov = np.abs(mean - want_mean), np.abs(cov - want_cov)
    print("moments n=%d d=%d: worst error / bound: mean %.3g cov %.3g (bound / scale at most %.3g)"
          % (n, d, float((err_mean / e_mean).max()), float((err_cov / e_cov).max()), float((e_cov / scale).max())))
    assert (err_mean <= 2 * e_mean).all()
    bad = np.argwhere(err_cov > 2 * e_cov)
    assert bad.size == 0, (bad[:8], cov[tuple(bad[:8].T)], want_cov[tuple(bad[:8].T)])
    assert np.array_equal(cov, cov.T)


def test_exact_integers_reproduce_numpys_bits():
    x = exact_case()
    assert x.shape == (64, 70)
    mean, cov = device_moments(x)
    assert np.array_equal(mean, np.mean(x, axis=0))
    assert np.array_equal(cov, np.cov(x, rowvar=False))


def test_contract_bits_prefill_symmetry_and_refusals():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    n, d, tail = 130, 129, 64
    x = _dev(offset_activations(n, d))
    ws_bytes = lib.gz_feature_moments_workspace_bytes(n, d)
    assert ws_bytes > 0

    def run(fill, n_given=n, ws_given=ws_bytes):
        mean = torch.full((d + tail,), -7.25, dtype=torch.float64, device="cuda")
        cov = torch.full((d * d + tail,), -7.25, dtype=torch.float64, device="cuda")
        mean[:d].view(torch.uint8).fill_(fill)
        cov[:d * d].view(torch.uint8).fill_(fill)
        ws = torch.full((ws_bytes + 64,), fill, dtype=torch.uint8, device="cuda")
        rc = lib.gz_feature_moments(F._p(x), n_given, d, F._p(mean), F._p(cov), F._p(ws), ws_given, F._stream())
        torch.cuda.synchronize()
        return rc, mean.cpu().numpy(), cov.cpu().numpy(), ws.cpu().numpy()

    rc, mean_a, cov_a, ws_a = run(0x00)
    assert rc == 0
    rc, mean_b, cov_b, _ = run(0x00)
    assert rc == 0 and np.array_equal(mean_a, mean_b) and np.array_equal(cov_a, cov_b)          # two calls, equal bits
    rc, mean_c, cov_c, ws_c = run(0xFF)                                                         # NaN-prefilled outputs
    assert rc == 0
    assert np.array_equal(mean_a.view(np.uint64), mean_c.view(np.uint64))
    assert np.array_equal(cov_a.view(np.uint64), cov_c.view(np.uint64))
    assert np.isfinite(mean_a[:d]).all() and np.isfinite(cov_a[:d * d]).all()
    square = cov_a[:d * d].reshape(d, d)
    assert np.array_equal(square.view(np.uint64), square.T.view(np.uint64))                     # bitwise symmetric
    for a in (mean_a, mean_c, cov_a, cov_c):                                                    # nothing behind the outputs
        assert (a[-tail:] == -7.25).all()
    assert (ws_a[ws_bytes:] == 0x00).all() and (ws_c[ws_bytes:] == 0xFF).all()                  # or behind the workspace
    for kwargs, code in ((dict(ws_given=ws_bytes - 1), -3), (dict(n_given=1), -1)):
        rc, mean_e, cov_e, ws_e = run(0xFF, **kwargs)
        assert rc == code
        assert (mean_e[:d].view(np.uint8) == 0xFF).all() and (cov_e[:d * d].view(np.uint8) == 0xFF).all()
        assert (ws_e == 0xFF).all()                                                             # nothing was launched


def test_frechet_distance_from_device_moments_matches_the_reference_value():
    from lightning_gan_zoo_amd import eval as E
    gold = float(np.load(os.path.join(GOLDEN_DIR, "eval_metrics.npz"))["fid"])
    real, fake = activations(1, 400, 48, 0.0), activations(2, 360, 48, 0.3)
    fid = E.frechet_distance(*device_moments(real), *device_moments(fake))
    print("fid from device moments %.15g, reference %.15g, relative difference %.3g" % (fid, gold, abs(fid - gold) / gold))
    assert abs(fid - gold) <= 1e-9 * abs(gold)

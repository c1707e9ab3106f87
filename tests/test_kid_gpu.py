"""KID on the device (csrc/gz_kid.hip, eval.polynomial_mmd_averages_device) against numpy's fp64 evaluation.

The sums are held to first-order forward error bounds (kid_support.sums_bounds) that cover ANY order of fp64
summation, so numpy and the kernel both lie within one bound of the exact value and the tests allow 2 x bound; the
end-to-end values are held to the tolerances tests/test_eval.py uses against tests/golden/eval_metrics.npz."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR
from kid_support import N_G, N_R, U, activations, mixed_sign_codes, numpy_sums, subset_rows, sums_bounds

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 1), (16, 4, 2), (17, 7, 3), (65, 48, 2), (150, 48, 7), (130, 2048, 2)]          # (m, d, S)
KERNELS = [(3, None, 1.0), (1, 0.05, 0.0), (2, 0.05, 1.0), (3, None, 0.0)]                      # (degree, gamma, coef0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("degree,gamma,coef0", KERNELS)
@pytest.mark.parametrize("m,d,S", SHAPES)
def test_sums_within_twice_the_forward_bound(m, d, S, degree, gamma, coef0):
    from lightning_gan_zoo_amd import eval as E
    g, r = mixed_sign_codes(d)
    idx = subset_rows(m, S, seed=m * 31 + d)
    assert (idx == 0).any(axis=2).all() and (idx[:, 0] == N_G - 1).any(axis=1).all() and (idx[:, 1] == N_R - 1).any(axis=1).all()
    out = E.kid_sums_device(_dev(g), _dev(r), idx, degree=degree, gamma=gamma, coef0=coef0)
    assert out.shape == (S, 6 * m + 3) and np.isfinite(out).all()
    worst = 0.0
    for s in range(S):
        gs, rs = g[idx[s, 0]], r[idx[s, 1]]
        want = numpy_sums(gs, rs, degree, gamma, coef0)
        bound = sums_bounds(gs, rs, degree, gamma, coef0)
        err = np.abs(out[s] - want)
        assert (bound > 0).all()
        worst = max(worst, float((err / bound).max()))
        bad = np.nonzero(err > 2 * bound)[0]
        assert bad.size == 0, (s, bad[:8], out[s][bad[:8]], want[bad[:8]], bound[bad[:8]])
    print("kid sums m=%d d=%d S=%d degree=%d gamma=%s coef0=%g: worst error / bound %.3g" % (m, d, S, degree, gamma, coef0, worst))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_end_to_end_matches_the_reference_values():
    from lightning_gan_zoo_amd import eval as E
    gold = np.load(os.path.join(GOLDEN_DIR, "eval_metrics.npz"))
    real, fake = activations(1, 400, 48, 0.0), activations(2, 360, 48, 0.3)
    np.random.seed(123)
    E.polynomial_mmd_averages(real, fake, n_subsets=7, subset_size=150)
    want_state = np.random.get_state()
    np.random.seed(123)
    mmds, variances = E.polynomial_mmd_averages_device(real, fake, n_subsets=7, subset_size=150)
    assert _same_state(np.random.get_state(), want_state)
    assert np.allclose(mmds, gold["kid_mmds"], rtol=1e-10, atol=0)
    assert np.allclose(variances, gold["kid_vars"], rtol=1e-8, atol=0)
    np.random.seed(123)
    only = E.polynomial_mmd_averages_device(torch.from_numpy(real), torch.from_numpy(fake).cuda(), n_subsets=7,
                                            subset_size=150, ret_var=False)
    assert np.array_equal(only, mmds)


def test_hard_cancellation():
    """One distribution on both sides: mmd^2 is ~1e-5 of the terms it is the difference of."""
    from lightning_gan_zoo_amd import eval as E
    m, d, S, n = 256, 2048, 2, 300
    rng = np.random.RandomState(7)
    g32, r32 = (np.abs(rng.randn(n, d)).astype(np.float32) * 0.5 for _ in range(2))
    g, r = g32.astype(np.float64), r32.astype(np.float64)
    np.random.seed(5)
    idx = E.draw_kid_subsets(n, n, S, m)
    np.random.seed(5)
    host = E.polynomial_mmd_averages(g, r, n_subsets=S, subset_size=m, ret_var=False)
    np.random.seed(5)
    dev = E.polynomial_mmd_averages_device(g32, r32, n_subsets=S, subset_size=m, ret_var=False)
    for s in range(S):
        kgg, krr, kgr = (E._poly_kernel(a, b, 3, None, 1) for a, b in ((g[idx[s, 0]], g[idx[s, 0]]),
                                                                      (r[idx[s, 1]], r[idx[s, 1]]),
                                                                      (g[idx[s, 0]], r[idx[s, 1]])))
        scale = ((abs(kgg.sum() - np.trace(kgg)) + abs(krr.sum() - np.trace(krr))) / (m * (m - 1))
                 + 2 * abs(kgr.sum()) / (m * m))
        print("kid cancellation subset %d: mmd2 host %.6e device %.6e diff %.3e scale %.3f bound %.3e"
              % (s, host[s], dev[s], abs(dev[s] - host[s]), scale, 2 * 3 * (d + 4) * U * scale))
        assert abs(host[s]) < 1e-3 * scale
        assert abs(dev[s] - host[s]) <= 2 * 3 * (d + 4) * U * scale


def test_subset_size_is_clamped_like_the_host():
    from lightning_gan_zoo_amd import eval as E
    g, r = activations(3, 40, 48, 0.0), activations(4, 30, 48, 0.3)
    np.random.seed(9)
    hm, hv = E.polynomial_mmd_averages(g, r, n_subsets=4, subset_size=1000)
    want_state = np.random.get_state()
    np.random.seed(9)
    dm, dv = E.polynomial_mmd_averages_device(g, r, n_subsets=4, subset_size=1000)
    assert _same_state(np.random.get_state(), want_state)
    assert np.allclose(dm, hm, rtol=1e-10, atol=0)
    assert np.allclose(dv, hv, rtol=1e-8, atol=0)


def test_contract_bits_prefill_sentinel_and_short_workspace():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    m, d, S = 70, 13, 3
    g, r = mixed_sign_codes(48)
    g, r = _dev(g[:, :d]), _dev(r[:, :d])
    idx = _dev(subset_rows(m, S, seed=3))
    n_out, tail = S * (6 * m + 3), 64
    ws_bytes = lib.gz_kid_workspace_bytes(S, m, d)
    assert ws_bytes > 0

    def run(fill, ws_given=ws_bytes):
        out = torch.full((n_out + tail,), -7.25, dtype=torch.float64, device="cuda")
        out[:n_out].view(torch.uint8).fill_(fill)
        ws = torch.full((ws_bytes + 64,), fill, dtype=torch.uint8, device="cuda")
        rc = lib.gz_kid_sums(F._p(g), N_G, F._p(r), N_R, d, F._p(idx), S, m, 1.0 / d, 1.0, 3, F._p(out), F._p(ws),
                             ws_given, F._stream())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), ws.cpu().numpy()

    rc, a, ws_a = run(0x00)
    assert rc == 0
    rc, b, _ = run(0x00)
    assert rc == 0 and np.array_equal(a, b)
    rc, c, ws_c = run(0xFF)
    assert rc == 0 and np.array_equal(a.view(np.uint64), c.view(np.uint64))
    assert np.isfinite(a[:n_out]).all()
    assert (a[n_out:] == -7.25).all() and (c[n_out:] == -7.25).all()
    assert (ws_a[ws_bytes:] == 0x00).all() and (ws_c[ws_bytes:] == 0xFF).all()      # nothing behind the workspace either
    rc, e, ws_e = run(0xFF, ws_given=ws_bytes - 1)
    assert rc == -3
    assert (e[:n_out].view(np.uint8) == 0xFF).all() and (ws_e == 0xFF).all()        # nothing was launched


def test_evaluate_with_kid_on_device():
    """The tiny dc_gan scenario of test_eval.test_sample_dump_matches_oracle_generator, a fixed linear feature map."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg("dc_gan", batch_size=8, features=8, noise_dim=16)
    torch.manual_seed(42)
    module = locate(cfg.model.lm["_target_"])(cfg, None).to("cuda")
    torch.manual_seed(5)
    dump = E.SampleDump(module, n_samples=20, batch_size=8)
    rng = np.random.RandomState(11)
    proj = {}

    def features(img):
        x = np.asarray(img, dtype=np.float64).reshape(len(img), -1) / 255.0
        if "w" not in proj:
            proj["w"] = rng.randn(x.shape[1], 8) / np.sqrt(x.shape[1])
        return x.dot(proj["w"])

    real_act = np.random.RandomState(12).randn(30, 8) * 0.5 + 0.25
    np.random.seed(21)
    host = E.evaluate(module, dump, features, real_act, n_subsets=5)
    want_state = np.random.get_state()
    np.random.seed(21)
    dev = E.evaluate(module, dump, features, real_act, n_subsets=5, kid_on_device=True)
    assert _same_state(np.random.get_state(), want_state)
    assert np.isfinite([host["fid"], host["kid"], host["kid_std"]]).all()
    assert dev["fid"] == host["fid"]
    assert np.isclose(dev["kid"], host["kid"], rtol=1e-10, atol=0)
    assert np.isclose(dev["kid_std"], host["kid_std"], rtol=1e-10, atol=0)
    # a caller that evaluates every epoch uploads the real codes once and hands them in: same bits
    real_dev = E.device_codes(real_act, module.device)
    assert real_dev.is_cuda and real_dev.dtype == torch.float64
    np.random.seed(21)
    again = E.evaluate(module, dump, features, real_act, n_subsets=5, kid_on_device=True, real_codes_device=real_dev)
    assert again == dev

"""The Frechet distance on the device (csrc/gz_sqrtm.hip, eval.frechet_distance_device): the fp64 MFMA product and the
trace / norm reduction against numpy within their forward bounds (fid_support), the Newton-Schulz loop against scipy's
value on every input set, and evaluate_device with and without ``fid_on_device`` on bit-identical activations.
Observed worst error / tolerance per group on an MI355X: see DESIGN.md 3.4.6."""
import os

import numpy as np
import pytest
import torch

from fid_support import (FULL_RANK, GOLDEN_SET, PRODUCT_COEFFS, PRODUCT_DIMS, REAL_SIZE, SAME_SET, SETS, TOL_DEFICIENT,
                         exact_operands, host_fid, product_bound, product_operands, statistics, tolerance,
                         trace_norm_bounds)
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()          # (a copy: the shared statistics are read-only)


def _product(a, b, alpha, beta):
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    d = a.shape[0]
    a, b = _dev(a), _dev(b)
    c = torch.full((d, d), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.gz_sqrtm_product(F._p(a), F._p(b), F._p(c), d, alpha, beta, F._stream()), "sqrtm_product")
    return c.cpu().numpy()


def _trace_norm(a):
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    d = a.shape[0]
    a = _dev(a)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    ws_bytes = lib.gz_sqrtm_trace_norm_workspace_bytes(d)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")
    check(lib.gz_sqrtm_trace_norm(F._p(a), d, F._p(out), F._p(ws), ws_bytes, F._stream()), "sqrtm_trace_norm")
    return out.cpu().numpy()


@pytest.mark.parametrize("alpha,beta", PRODUCT_COEFFS)
@pytest.mark.parametrize("d", PRODUCT_DIMS)
def test_product_within_twice_the_forward_bound(d, alpha, beta):
    a, b = product_operands(d)
    assert d == 1 or (not np.array_equal(a, a.T) and (a < 0).any() and (a > 0).any() and (b < 0).any() and (b > 0).any())
    want = alpha * a.dot(b) + beta * np.eye(d)
    bound = product_bound(a, b, alpha, beta)
    assert (bound > 0).all() and (bound <= 1e-11 * np.abs(a).dot(np.abs(b)) + 1e-15).all()      # not vacuous
    got = _product(a, b, alpha, beta)
    assert got.shape == (d, d) and np.isfinite(got).all()
    err = np.abs(got - want)
    print("product d=%d alpha=%g beta=%g: worst error / bound %.3g" % (d, alpha, beta, float((err / bound).max())))
    bad = np.argwhere(err > 2 * bound)
    assert bad.size == 0, (bad[:8], got[tuple(bad[:8].T)], want[tuple(bad[:8].T)])
    # a transposed operand or a dropped row is far outside: the bound separates them
    assert (np.abs(alpha * a.T.dot(b) + beta * np.eye(d) - want) > 2 * bound).any() or d == 1


@pytest.mark.parametrize("alpha,beta", PRODUCT_COEFFS)
def test_product_of_exact_integers_reproduces_numpys_bits(alpha, beta):
    a, b = exact_operands()
    assert a.shape == (70, 70)
    want = alpha * a.dot(b) + beta * np.eye(70)
    assert np.array_equal(want * 2, np.round(want * 2))
    assert np.array_equal(_product(a, b, alpha, beta), want)


def test_product_pair_equals_two_products():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    d = 65
    a, b = product_operands(d)
    a_dev, b_dev = _dev(a), _dev(b)
    c0 = torch.full((d, d), float("nan"), dtype=torch.float64, device="cuda")
    c1 = torch.full((d, d), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.gz_sqrtm_product_pair(F._p(a_dev), F._p(b_dev), F._p(c0), 1.0, 0.0, F._p(b_dev), F._p(a_dev), F._p(c1), -0.5,
                                    1.5, d, F._stream()), "sqrtm_product_pair")
    assert np.array_equal(c0.cpu().numpy().view(np.uint64), _product(a, b, 1.0, 0.0).view(np.uint64))
    assert np.array_equal(c1.cpu().numpy().view(np.uint64), _product(b, a, -0.5, 1.5).view(np.uint64))


def test_product_contract_bits_prefill_and_refusals():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    d, tail = 130, 64
    a, b = product_operands(d)
    a_dev, b_dev = _dev(a), _dev(b)

    def run(fill, d_given=d, out=None, pair=False):
        c = torch.full((d * d + tail,), -7.25, dtype=torch.float64, device="cuda")
        c[:d * d].view(torch.uint8).fill_(fill)
        c2 = c.clone()
        if pair:
            rc = lib.gz_sqrtm_product_pair(F._p(a_dev), F._p(b_dev), F._p(c), -0.5, 1.5, F._p(b_dev), F._p(a_dev),
                                           F._p(c2 if out is None else out), 1.0, 0.0, d_given, F._stream())
        else:
            rc = lib.gz_sqrtm_product(F._p(a_dev), F._p(b_dev), F._p(c if out is None else out), d_given, -0.5, 1.5,
                                      F._stream())
        torch.cuda.synchronize()
        return rc, c.cpu().numpy(), c2.cpu().numpy()

    rc, c_a, _ = run(0x00)
    assert rc == 0
    rc, c_b, _ = run(0x00)
    assert rc == 0 and np.array_equal(c_a.view(np.uint64), c_b.view(np.uint64))                 # two calls, equal bits
    rc, c_c, _ = run(0xFF)                                                                      # NaN-prefilled output
    assert rc == 0 and np.array_equal(c_a.view(np.uint64), c_c.view(np.uint64))
    assert np.isfinite(c_a[:d * d]).all() and (c_a[-tail:] == -7.25).all() and (c_c[-tail:] == -7.25).all()
    before = (a_dev.clone(), b_dev.clone())
    for kwargs in (dict(d_given=0), dict(out=a_dev), dict(out=b_dev), dict(out=a_dev.view(-1)[d:]),
                   dict(pair=True, d_given=0), dict(pair=True, out=a_dev), dict(pair=True, out=b_dev.view(-1)[1:])):
        rc, c_e, c2_e = run(0xFF, **kwargs)
        assert rc == -1, kwargs
        assert (c_e[:d * d].view(np.uint8) == 0xFF).all() and (c2_e[:d * d].view(np.uint8) == 0xFF).all()   # no launch
    assert torch.equal(a_dev, before[0]) and torch.equal(b_dev, before[1])


@pytest.mark.parametrize("d", PRODUCT_DIMS)
def test_trace_and_norm_within_twice_the_forward_bound(d):
    a = product_operands(d)[0] + 3.0 * np.eye(d)
    e_tr, e_f2 = trace_norm_bounds(a)
    tr, f2 = _trace_norm(a)
    want_tr, want_f2 = float(np.trace(a)), float((a * a).sum())
    print("trace / norm d=%d: errors %.3g %.3g, bounds %.3g %.3g" % (d, abs(tr - want_tr), abs(f2 - want_f2), e_tr, e_f2))
    assert abs(tr - want_tr) <= 2 * e_tr and abs(f2 - want_f2) <= 2 * e_f2
    assert e_f2 <= 1e-11 * want_f2


def test_trace_and_norm_contract():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    d = 130
    a = product_operands(d)[0]
    a_dev = _dev(a)
    ws_bytes = lib.gz_sqrtm_trace_norm_workspace_bytes(d)
    assert ws_bytes > 0

    def run(fill, d_given=d, ws_given=ws_bytes):
        out = torch.full((2 + 8,), -7.25, dtype=torch.float64, device="cuda")
        out[:2].view(torch.uint8).fill_(fill)
        ws = torch.full((ws_bytes + 64,), fill, dtype=torch.uint8, device="cuda")
        rc = lib.gz_sqrtm_trace_norm(F._p(a_dev), d_given, F._p(out), F._p(ws), ws_given, F._stream())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), ws.cpu().numpy()

    rc, out_a, ws_a = run(0x00)
    assert rc == 0
    rc, out_b, _ = run(0x00)
    assert rc == 0 and np.array_equal(out_a.view(np.uint64), out_b.view(np.uint64))             # two calls, equal bits
    rc, out_c, ws_c = run(0xFF)                                                                 # NaN-prefilled
    assert rc == 0 and np.array_equal(out_a.view(np.uint64), out_c.view(np.uint64))
    assert np.isfinite(out_a[:2]).all() and (out_a[2:] == -7.25).all() and (out_c[2:] == -7.25).all()
    assert (ws_a[ws_bytes:] == 0x00).all() and (ws_c[ws_bytes:] == 0xFF).all()                  # nothing behind the workspace
    for kwargs, code in ((dict(ws_given=ws_bytes - 1), -3), (dict(d_given=0), -1)):
        rc, out_e, ws_e = run(0xFF, **kwargs)
        assert rc == code
        assert (out_e[:2].view(np.uint8) == 0xFF).all() and (ws_e == 0xFF).all()                # nothing was launched


def _device_fid(case, **kwargs):
    from lightning_gan_zoo_amd import eval as E
    return E.frechet_distance_device(*[_dev(v) for v in statistics(case)], **kwargs)


@pytest.mark.parametrize("case", SETS, ids=str)
def test_device_distance_matches_scipy(case):
    from lightning_gan_zoo_amd import eval as E
    fid, (k1, k2), ok = _device_fid(case)
    want, tol = host_fid(case), tolerance(case)
    _, (h1, h2), host_ok = E.frechet_distance_newton_schulz(*statistics(case))
    print("%s: device %.15g scipy %.15g, error / tolerance %.3g, iterations %d + %d (numpy restatement %d + %d)"
          % (case, fid, want, abs(fid - want) / tol, k1, k2, h1, h2))
    assert ok and host_ok and 1 <= k1 <= E.NS_MAXIT and 1 <= k2 <= E.NS_MAXIT
    assert abs(fid - want) <= tol
    if case in FULL_RANK:
        assert abs(k1 - h1) <= 2 and abs(k2 - h2) <= 2


def test_device_distance_reproduces_the_golden_values_and_takes_a_cached_root():
    from lightning_gan_zoo_amd import eval as E
    gold = float(np.load(os.path.join(GOLDEN_DIR, "eval_metrics.npz"))["fid"])
    fid, its, ok = _device_fid(GOLDEN_SET)
    print("device fid %.15g, reference %.15g, relative difference %.3g" % (fid, gold, abs(fid - gold) / gold))
    assert ok and abs(fid - gold) <= 1e-9 * abs(gold)
    root, k, ok = E.sqrtm_psd_device(_dev(statistics(GOLDEN_SET)[1]))
    assert ok and k == its[0] and root.is_cuda and root.dtype == torch.float64
    sigma = statistics(GOLDEN_SET)[1]
    r = root.cpu().numpy()
    assert np.abs(r.dot(r) - sigma).max() <= 1e-12 * np.abs(sigma).max()
    again, its2, ok = _device_fid(GOLDEN_SET, root1=root)
    assert ok and its2 == (0, its[1]) and again == fid
    same, _, ok = _device_fid(SAME_SET)
    assert ok and abs(same) <= 1e-9 * 2 * np.trace(statistics(SAME_SET)[1])


def test_zero_covariance_and_too_few_iterations():
    from lightning_gan_zoo_amd import eval as E
    mu1, mu2 = _dev(np.array([1.0, -2.0, 0.5])), _dev(np.array([0.0, 1.0, 0.5]))
    zero = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
    assert E.frechet_distance_device(mu1, zero, mu2, zero) == (10.0, (0, 0), True)
    root, k, ok = E.sqrtm_psd_device(zero)
    assert ok and k == 0 and torch.equal(root, zero)
    fid, its, ok = E.frechet_distance_device(*[_dev(v) for v in statistics(GOLDEN_SET)], maxit=2)
    assert ok is False and its == (2, 2)


def test_evaluate_device_with_the_distance_on_the_device(monkeypatch):
    """fid_on_device=True against fid_on_device=False on bit-identical activations (a stand-in feature net): the FID
    within the tolerance of its statistics' rank, the KID equal, the real root made once over two evaluations."""
    from lightning_gan_zoo_amd import eval as E
    from test_eval_device_gpu import PixelStatistics, _native_dump, _tiny
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=200)
    net = PixelStatistics()
    host_act = np.concatenate([net(img) for img in dump.images(module)])
    rng = np.random.RandomState(12)
    real_act = host_act[rng.randint(0, 200, 260)] * 0.9 + rng.randn(260, 24) * host_act.std(axis=0) * 0.5
    real = E.RealStatistics(real_act, module.device)
    np.random.seed(21)
    off = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5)
    roots = []
    sqrtm = E.sqrtm_psd_device
    monkeypatch.setattr(E, "sqrtm_psd_device", lambda a, *args: roots.append(tuple(a.shape)) or sqrtm(a, *args))
    np.random.seed(21)
    on = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5, fid_on_device=True)
    np.random.seed(21)
    again = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5, fid_on_device=True)
    assert roots == [(24, 24)]                                     # the real set's root: once per run
    assert on == again and set(on) == {"fid", "kid", "kid_std"}
    assert on["kid"] == off["kid"] and on["kid_std"] == off["kid_std"]
    scale = float(np.trace(np.cov(real_act, rowvar=False)) + np.trace(np.cov(host_act, rowvar=False)))
    print("fid on the device %.15g, on the host %.15g, difference / (tr S1 + tr S2) %.3g"
          % (on["fid"], off["fid"], abs(on["fid"] - off["fid"]) / scale))
    assert np.isfinite(off["fid"]) and off["fid"] > 0
    assert abs(on["fid"] - off["fid"]) <= 1e-9 * scale             # 260 and 200 rows of 24 features: full rank


def test_real_size_once():
    """d = 2048, 2100 rows per side, ReLU-like features with dead columns.  The numpy restatement converges there in
    27 + 43 iterations, 4.6e-13 (tr S1 + tr S2) from scipy."""
    from lightning_gan_zoo_amd import eval as E
    st = statistics(REAL_SIZE)
    fid, (k1, k2), ok = E.frechet_distance_device(*[_dev(v) for v in st])
    want = host_fid(REAL_SIZE)
    scale = float(np.trace(st[1]) + np.trace(st[3]))
    print("d = 2048: device %.15g scipy %.15g, difference / (tr S1 + tr S2) %.3g, iterations %d + %d"
          % (fid, want, abs(fid - want) / scale, k1, k2))
    assert ok and abs(fid - want) <= TOL_DEFICIENT * scale

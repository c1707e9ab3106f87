"""The Frechet distance on the device, the parts that need no GPU: the numpy restatement of the Newton-Schulz recurrence
(eval.frechet_distance_newton_schulz) against scipy's value on every input set of fid_support, its stop rules, the
runner key, the untouched default call, the refusal to run anywhere but on the HIP kernels, the C ABI.

Measured: the restatement lies at most 3.2e-13 (tr S1 + tr S2) from eval.frechet_distance on the full-rank sets (bar 1e-9)
and at most 1.5e-8 on the rank-deficient ones (bar 1e-7); 1 to 65 iterations per root."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fid_support import GOLDEN_SET, SAME_SET, SETS, host_fid, statistics, tolerance
from helpers import GOLDEN_DIR


@pytest.mark.parametrize("case", SETS, ids=str)
def test_restatement_matches_scipy_and_converges(case):
    from lightning_gan_zoo_amd import eval as E
    fid, (k1, k2), ok = E.frechet_distance_newton_schulz(*statistics(case))
    want, tol = host_fid(case), tolerance(case)
    print("%s: restatement %.15g scipy %.15g, error / tolerance %.3g, iterations %d + %d"
          % (case, fid, want, abs(fid - want) / tol, k1, k2))
    assert ok and 1 <= k1 <= E.NS_MAXIT and 1 <= k2 <= E.NS_MAXIT
    assert np.isfinite(want) and abs(fid - want) <= tol


def test_restatement_reproduces_the_golden_values():
    from lightning_gan_zoo_amd import eval as E
    gold = np.load(os.path.join(GOLDEN_DIR, "eval_metrics.npz"))
    fid, _, ok = E.frechet_distance_newton_schulz(*statistics(GOLDEN_SET))
    assert ok and abs(fid - float(gold["fid"])) <= 1e-9 * abs(float(gold["fid"]))
    mu, sigma, mu2, sigma2 = statistics(SAME_SET)
    assert np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2)
    same, _, ok = E.frechet_distance_newton_schulz(mu, sigma, mu2, sigma2)
    assert ok and abs(same) <= 1e-9 * 2 * np.trace(sigma)
    assert abs(float(gold["fid_same"])) <= 1e-9 * 2 * np.trace(sigma)          # (the reference's own, for scale)


def test_zero_covariance_takes_no_iteration():
    from lightning_gan_zoo_amd import eval as E
    mu1, mu2 = np.array([1.0, -2.0, 0.5]), np.array([0.0, 1.0, 0.5])
    zero = np.zeros((3, 3))
    root, k, ok = E.sqrtm_psd_newton_schulz(zero)
    assert ok and k == 0 and np.array_equal(root, zero)
    fid, its, ok = E.frechet_distance_newton_schulz(mu1, zero, mu2, zero)
    assert ok and its == (0, 0) and fid == 10.0
    sigma2 = statistics(GOLDEN_SET)[3][:3, :3]
    fid, its, ok = E.frechet_distance_newton_schulz(mu1, zero, mu2, sigma2)     # R = 0: the inner matrix is zero too
    assert ok and its == (0, 0) and np.isclose(fid, 10.0 + np.trace(sigma2), rtol=1e-15)


def test_root_squares_to_its_argument():
    from lightning_gan_zoo_amd import eval as E
    sigma = statistics(GOLDEN_SET)[1]
    root, k, ok = E.sqrtm_psd_newton_schulz(sigma)
    assert ok and k > 1
    assert np.abs(root.dot(root) - sigma).max() <= 1e-12 * np.abs(sigma).max()


def test_too_few_iterations_report_not_converged():
    from lightning_gan_zoo_amd import eval as E
    st = statistics(GOLDEN_SET)
    fid, its, ok = E.frechet_distance_newton_schulz(*st, maxit=2)
    assert ok is False and its == (2, 2) and np.isfinite(fid)
    assert E.sqrtm_psd_newton_schulz(st[1], maxit=2)[1:] == (2, False)
    assert E.sqrtm_psd_newton_schulz(np.full((2, 2), np.inf))[2] is False       # a trace that is not finite


def test_stop_rules():
    from lightning_gan_zoo_amd import eval as E
    inf = float("inf")
    assert E._ns_verdict(1.0, float("nan"), inf)[0] == "fail"
    assert E._ns_verdict(1.0, 1.0 + 2.0 ** -50, inf)[0] == "new"                  # within 1e-14
    assert E._ns_verdict(1.0, 1.0 + 1e-12, 1e-13) == ("old", abs(1.0 + 1e-12 - 1.0))    # stopped shrinking under the floor
    assert E._ns_verdict(1.0, 1.0 + 1e-12, 1e-11)[0] == "go"                      # still shrinking
    assert E._ns_verdict(1.0, 1.0 + 1e-8, 1e-9)[0] == "go"                        # grew, but above the floor of 1e-10


def test_runner_key_parses_defaults_to_false_and_needs_the_device_pass():
    from lightning_gan_zoo_amd.run_network import RUNNER_KEYS, parse_overrides
    assert RUNNER_KEYS["fid_on_device"] is False
    assert parse_overrides(["+expt=dc_gan"])[3]["fid_on_device"] is False
    for plus in ("", "+"):
        run = parse_overrides(["+expt=dc_gan", plus + "eval_on_device=true", plus + "fid_on_device=true"])[3]
        assert run["fid_on_device"] is True and run["eval_on_device"] is True
    with pytest.raises(SystemExit, match="eval_on_device"):
        parse_overrides(["+expt=dc_gan", "fid_on_device=true"])
    with pytest.raises(SystemExit, match="eval_on_device"):
        parse_overrides(["+expt=dc_gan", "+fid_on_device=true", "kid_on_device=true"])


def _evaluator(monkeypatch, tmp_path, **keys):
    """make_fid_evaluator on stand-ins (tests/test_eval_device_cpu.py's arrangement) -> the recorded calls."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import inception as I
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.config import to_cfg
    real_act = np.random.RandomState(0).randn(12, 4)
    mu, sigma = E.activation_statistics(real_act)
    np.savez(tmp_path / "inception_cache.npz", mu=mu, sigma=sigma, act=real_act)
    calls = {"host": [], "device": []}

    class Features:
        def __init__(self, net, batch_size=16):
            pass

        def device(self, x):
            raise AssertionError("not reached")

    class Dump:
        def __init__(self, module, n_samples, batch_size):
            self.n_samples, self.batch_size = n_samples, batch_size

    class Real:
        def __init__(self, act, device, mu=None, sigma=None):
            pass

    result = {"fid": 1.0, "kid": 2.0, "kid_std": 3.0}
    monkeypatch.setattr(I, "load_fid_weights", lambda path, device, check_hash=True: "net")
    monkeypatch.setattr(I, "InceptionFeatures", Features)
    monkeypatch.setattr(E, "SampleDump", Dump)
    monkeypatch.setattr(E, "RealStatistics", Real)
    monkeypatch.setattr(E, "device_codes", lambda act, device: "codes")
    monkeypatch.setattr(E, "evaluate", lambda *a, **k: calls["host"].append((a, k)) or result)
    monkeypatch.setattr(E, "evaluate_device", lambda *a, **k: calls["device"].append((a, k)) or result)
    cfg = to_cfg({"calc_fid": True, "val": {"fid_n_samples": 32},
                  "dataset": {"_target_": "torchvision.datasets.ImageFolder", "val": {"root": str(tmp_path)}}})
    run = dict(R.RUNNER_KEYS, inception_weights="weights.pth", eval_batch_size=100, **keys)
    evaluate = R.make_fid_evaluator(cfg, run, "module", "cuda:0")
    assert evaluate("module", 3) == result
    return calls


@pytest.mark.parametrize("on", [False, True])
def test_make_fid_evaluator_passes_fid_on_device_only_when_asked(monkeypatch, tmp_path, on):
    calls = _evaluator(monkeypatch, tmp_path, eval_on_device=True, fid_on_device=on)
    assert calls["host"] == [] and len(calls["device"]) == 1
    kwargs = calls["device"][0][1]
    assert kwargs == ({"batch": 100, "fid_on_device": True} if on else {"batch": 100})


def test_make_fid_evaluator_refuses_the_key_without_the_device_pass(monkeypatch, tmp_path):
    with pytest.raises(SystemExit, match="eval_on_device"):
        _evaluator(monkeypatch, tmp_path, eval_on_device=False, fid_on_device=True)


def test_evaluate_device_keeps_todays_call_with_the_key_off(monkeypatch):
    """Key off: frechet_distance on the host moments, no device root.  Key on: the device distance with the real set's
    cached root; a root that did not converge sends the evaluation to the host, with one warning."""
    from lightning_gan_zoo_amd import eval as E
    mean, cov = torch.zeros(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    seen = {"host": 0, "device": 0, "roots": 0}

    class Real:
        mu, sigma, codes = np.zeros(3), np.eye(3), "codes"
        converged = True

        def device_root(self):
            seen["roots"] += 1
            return "mu", "sigma", "root", 5, self.converged

    def device(mu1, sigma1, mu2, sigma2, root1=None):
        assert (mu1, sigma1, root1) == ("mu", "sigma", "root") and mu2 is mean and sigma2 is cov
        seen["device"] += 1
        return 7.0, (0, 9), seen["device"] != 2                  # the second call reports no convergence

    monkeypatch.setattr(E, "device_activations", lambda module, dump, net, batch: mean)
    monkeypatch.setattr(E, "feature_moments_device", lambda codes: (mean, cov))
    monkeypatch.setattr(E, "frechet_distance", lambda *a: seen.__setitem__("host", seen["host"] + 1) or 3.0)
    monkeypatch.setattr(E, "frechet_distance_device", device)
    monkeypatch.setattr(E, "polynomial_mmd_averages_device", lambda *a, **k: (np.array([1.0, 3.0]), None))
    monkeypatch.setattr(E, "_fid_fallback_warned", False)
    real = Real()
    assert E.evaluate_device("m", "dump", "net", real)["fid"] == 3.0
    assert seen == {"host": 1, "device": 0, "roots": 0}
    assert E.evaluate_device("m", "dump", "net", real, fid_on_device=True) == {"fid": 7.0, "kid": 2.0, "kid_std": 1.0}
    assert seen == {"host": 1, "device": 1, "roots": 1}
    with pytest.warns(UserWarning, match="did not converge"):
        assert E.evaluate_device("m", "dump", "net", real, fid_on_device=True)["fid"] == 3.0
    assert seen == {"host": 2, "device": 2, "roots": 2}
    real.converged = False                                       # the real root itself: no device distance at all
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # once per run: no second warning
        assert E.evaluate_device("m", "dump", "net", real, fid_on_device=True)["fid"] == 3.0
    assert seen == {"host": 3, "device": 2, "roots": 3}


def test_device_functions_refuse_a_cpu_tensor():
    from lightning_gan_zoo_amd import eval as E
    mu, sigma = torch.zeros(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="there is no fallback"):
        E.sqrtm_psd_device(sigma)
    with pytest.raises(RuntimeError, match="there is no fallback"):
        E.frechet_distance_device(mu, sigma, mu, sigma)
    with pytest.raises(ValueError):
        E.sqrtm_psd_device(sigma.float())
    with pytest.raises(ValueError):
        E.sqrtm_psd_device(torch.zeros(3, 4, dtype=torch.float64))


def test_real_statistics_keeps_its_constructor():
    import inspect
    from lightning_gan_zoo_amd import eval as E
    assert list(inspect.signature(E.RealStatistics.__init__).parameters) == ["self", "real_act", "device", "mu", "sigma"]
    assert inspect.signature(E.evaluate_device).parameters["fid_on_device"].default is False


def test_header_declares_the_new_entry_points_and_they_check_their_arguments():
    from lightning_gan_zoo_amd._lib import lib, parse_header
    protos = parse_header()
    dbl, ptr, i32 = ctypes.c_double, ctypes.c_void_p, ctypes.c_int
    assert protos["gz_sqrtm_product"] == (i32, [ptr, ptr, ptr, i32, dbl, dbl, ptr])
    assert protos["gz_sqrtm_product_pair"] == (i32, [ptr, ptr, ptr, dbl, dbl, ptr, ptr, ptr, dbl, dbl, i32, ptr])
    assert protos["gz_sqrtm_trace_norm_workspace_bytes"] == (ctypes.c_size_t, [i32])
    assert protos["gz_sqrtm_trace_norm"] == (i32, [ptr, i32, ptr, ptr, ctypes.c_size_t, ptr])
    assert lib.gz_sqrtm_trace_norm_workspace_bytes(0) == 0 and lib.gz_sqrtm_trace_norm_workspace_bytes(1) >= 16
    assert lib.gz_sqrtm_trace_norm_workspace_bytes(2048) % 8 == 0 and lib.gz_sqrtm_trace_norm_workspace_bytes(2048) < (1 << 16)
    d = 4                                    # never dereferenced: every call below is refused before a launch
    a, b, c, e = (ctypes.c_void_p(0x10000 + 0x1000 * i) for i in range(4))
    inside = ctypes.c_void_p(0x10000 + 8 * (d * d - 1))          # the last double of a

    def product(a=a, b=b, c=c, d=d):
        return lib.gz_sqrtm_product(a, b, c, d, 1.0, 0.0, None)

    for bad in (dict(d=0), dict(d=-3), dict(a=None), dict(b=None), dict(c=None), dict(c=a), dict(c=b), dict(c=inside)):
        assert product(**bad) == -1, bad

    def pair(a0=a, b0=b, c0=c, a1=b, b1=a, c1=e, d=d):
        return lib.gz_sqrtm_product_pair(a0, b0, c0, 1.0, 0.0, a1, b1, c1, 1.0, 0.0, d, None)

    for bad in (dict(d=0), dict(a0=None), dict(b1=None), dict(c1=None), dict(c1=c), dict(c0=a), dict(c1=b), dict(c0=inside)):
        assert pair(**bad) == -1, bad

    def trace_norm(a=a, d=d, out=b, ws=c, ws_bytes=1 << 10):
        return lib.gz_sqrtm_trace_norm(a, d, out, ws, ws_bytes, None)

    for bad in (dict(d=0), dict(a=None), dict(out=None), dict(ws=None)):
        assert trace_norm(**bad) == -1, bad
    assert trace_norm(ws_bytes=lib.gz_sqrtm_trace_norm_workspace_bytes(d) - 1) == -3

"""The Inception Score on the device, the parts that need no GPU: the runner keys, the forwarding of the classifier head
only when asked, the untouched default call, the C ABI and its refusals, the host yardstick
(eval.inception_score_from_logits) against known values and against a long-double evaluation within the bound the GPU
test uses, the refusal to run anywhere but on the HIP kernels.

Measured on the CPU: the yardstick lies at most 2.6e-16 (relative, per split score) from the long-double evaluation on
the seven cases and 4.9e-16 on the +-800 logits; the bounds lie between 9.2e-13 and 4.0e-9."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from inception_score_support import (CASES, EXTREME_SPLITS, extreme_logits, host_logits, inputs, logit_delta,
                                     long_double_scores, score_bound)


def test_runner_keys_parse_default_off_and_need_the_device_pass():
    from lightning_gan_zoo_amd.run_network import RUNNER_KEYS, parse_overrides
    assert RUNNER_KEYS["inception_score"] is False and RUNNER_KEYS["inception_score_splits"] == 10
    run = parse_overrides(["+expt=dc_gan"])[3]
    assert run["inception_score"] is False and run["inception_score_splits"] == 10
    for plus in ("", "+"):
        run = parse_overrides(["+expt=gan_stability_r1", plus + "eval_on_device=true", plus + "inception_score=true",
                               plus + "inception_score_splits=4"])[3]
        assert run["inception_score"] is True and run["inception_score_splits"] == 4 and run["eval_on_device"] is True
    with pytest.raises(SystemExit, match="eval_on_device"):
        parse_overrides(["+expt=dc_gan", "inception_score=true"])
    with pytest.raises(SystemExit, match="eval_on_device"):
        parse_overrides(["+expt=dc_gan", "+inception_score=true", "kid_on_device=true"])


class _Tensor:
    """Stands in for a parameter of the classifier head: records the conversions it is put through."""

    def __init__(self, name, log, steps=()):
        self.name, self.log, self.steps = name, log, steps

    def _next(self, step):
        self.log.append((self.name, step))
        return _Tensor(self.name, self.log, self.steps + (step,))

    def detach(self):
        return self._next("detach")

    def to(self, what):
        return self._next(what)

    def contiguous(self):
        return self._next("contiguous")


def _evaluator(monkeypatch, tmp_path, capsys, **keys):
    """make_fid_evaluator on stand-ins (tests/test_fid_device_cpu.py's arrangement) -> (the recorded evaluate_device
    calls, the conversions of the head's parameters, the line printed per epoch)."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import inception as I
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.config import to_cfg
    real_act = np.random.RandomState(0).randn(12, 4)
    mu, sigma = E.activation_statistics(real_act)
    np.savez(tmp_path / "inception_cache.npz", mu=mu, sigma=sigma, act=real_act)
    calls, conversions = [], []

    class Net:
        @property
        def fc(self):                        # touched only with the key on
            conversions.append("fc")
            return type("Fc", (), {"weight": _Tensor("weight", conversions), "bias": _Tensor("bias", conversions)})

    class Features:
        def __init__(self, net, batch_size=16):
            self.net = net

        def device(self, x):
            raise AssertionError("not reached")

    class Dump:
        def __init__(self, module, n_samples, batch_size):
            self.n_samples, self.batch_size = n_samples, batch_size

    class Real:
        def __init__(self, act, device, mu=None, sigma=None):
            pass

    result = {"fid": 1.0, "kid": 2.0, "kid_std": 3.0}
    if keys.get("inception_score"):
        result = dict(result, **{"is": 4.25, "is_std": 0.5})
    monkeypatch.setattr(I, "load_fid_weights", lambda path, device, check_hash=True: Net())
    monkeypatch.setattr(I, "InceptionFeatures", Features)
    monkeypatch.setattr(E, "SampleDump", Dump)
    monkeypatch.setattr(E, "RealStatistics", Real)
    monkeypatch.setattr(E, "evaluate_device", lambda *a, **k: calls.append((a, k)) or result)
    cfg = to_cfg({"calc_fid": True, "val": {"fid_n_samples": 32},
                  "dataset": {"_target_": "torchvision.datasets.ImageFolder", "val": {"root": str(tmp_path)}}})
    run = dict(R.RUNNER_KEYS, inception_weights="weights.pth", eval_batch_size=100, **keys)
    evaluate = R.make_fid_evaluator(cfg, run, "module", "cuda:0")
    assert evaluate("module", 3) == result and evaluate("module", 4) == result
    return calls, conversions, capsys.readouterr().out


def test_make_fid_evaluator_keeps_todays_call_with_the_key_off(monkeypatch, tmp_path, capsys):
    calls, conversions, out = _evaluator(monkeypatch, tmp_path, capsys, eval_on_device=True)
    assert [k for _, k in calls] == [{"batch": 100}, {"batch": 100}]
    assert conversions == []                                         # the head is not even looked at
    assert out.splitlines() == ["epoch 3 FID: 1.0000 KID mean: 2.000000 KID stddev: 3.000000",
                                "epoch 4 FID: 1.0000 KID mean: 2.000000 KID stddev: 3.000000"]
    calls, _, _ = _evaluator(monkeypatch, tmp_path, capsys, eval_on_device=True, fid_on_device=True,
                             inception_score_splits=3)              # the splits alone ask for nothing
    assert calls[0][1] == {"batch": 100, "fid_on_device": True}


def test_make_fid_evaluator_forwards_the_classifier_head_when_asked(monkeypatch, tmp_path, capsys):
    calls, conversions, out = _evaluator(monkeypatch, tmp_path, capsys, eval_on_device=True, inception_score=True,
                                         inception_score_splits=4)
    assert len(calls) == 2
    for _, kwargs in calls:
        assert set(kwargs) == {"batch", "classifier", "inception_splits"}
        assert kwargs["batch"] == 100 and kwargs["inception_splits"] == 4
    weight, bias = calls[0][1]["classifier"]
    assert (weight.name, bias.name) == ("weight", "bias")
    assert weight.steps == bias.steps == ("detach", "cuda:0", torch.float64, "contiguous")
    assert calls[1][1]["classifier"][0] is weight                    # converted once per run, not per epoch
    assert conversions.count("fc") == 1 and len(conversions) == 1 + 2 * 4
    assert out.splitlines()[0] == "epoch 3 FID: 1.0000 KID mean: 2.000000 KID stddev: 3.000000 IS: 4.2500 +- 0.5000"


def test_make_fid_evaluator_refuses_the_key_without_the_device_pass(monkeypatch, tmp_path, capsys):
    with pytest.raises(SystemExit, match="eval_on_device"):
        _evaluator(monkeypatch, tmp_path, capsys, eval_on_device=False, inception_score=True)


def test_evaluate_device_scores_only_with_a_classifier(monkeypatch):
    from lightning_gan_zoo_amd import eval as E
    par = inspect.signature(E.evaluate_device).parameters
    assert par["classifier"].default is None and par["inception_splits"].default == 10
    par = inspect.signature(E.inception_score_device).parameters
    assert list(par) == ["codes", "weight", "bias", "splits"] and par["bias"].default is None and par["splits"].default == 10
    assert inspect.signature(E.inception_score_from_logits).parameters["splits"].default == 10
    mean, cov = torch.zeros(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    seen = []

    class Real:
        mu, sigma, codes = np.zeros(3), np.eye(3), "codes"

    def score(codes, weight, bias=None, splits=10):
        seen.append((codes, weight, bias, splits))
        return 5.0, 0.25, np.array([4.75, 5.25])

    fake = torch.zeros(2, 3, dtype=torch.float64)
    monkeypatch.setattr(E, "device_activations", lambda module, dump, net, batch: fake)
    monkeypatch.setattr(E, "feature_moments_device", lambda codes: (mean, cov))
    monkeypatch.setattr(E, "frechet_distance", lambda *a: 3.0)
    monkeypatch.setattr(E, "polynomial_mmd_averages_device", lambda *a, **k: (np.array([1.0, 3.0]), None))
    monkeypatch.setattr(E, "inception_score_device", score)
    assert E.evaluate_device("m", "dump", "net", Real()) == {"fid": 3.0, "kid": 2.0, "kid_std": 1.0}
    assert seen == []
    out = E.evaluate_device("m", "dump", "net", Real(), classifier=("w", "b"), inception_splits=2)
    assert out == {"fid": 3.0, "kid": 2.0, "kid_std": 1.0, "is": 5.0, "is_std": 0.25}
    assert len(seen) == 1 and seen[0][0] is fake and seen[0][1:] == ("w", "b", 2)     # the same resident generated codes


def test_header_declares_the_entry_points_and_they_check_their_arguments():
    from lightning_gan_zoo_amd._lib import lib, parse_header
    protos = parse_header()
    ptr, i32, i64, size = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert protos["gz_classifier_logits"] == (i32, [ptr, i64, i32, ptr, ptr, i32, ptr, ptr])
    assert protos["gz_inception_score_workspace_bytes"] == (size, [i64, i32, i32])
    assert protos["gz_inception_score"] == (i32, [ptr, i64, i32, i32, ptr, ptr, size, ptr])
    BAD, WORKSPACE, TOO_LARGE = -1, -3, -5
    n, d, classes = 6, 4, 5                   # never dereferenced: every call below is refused before a launch
    codes, weight, bias, logits = (ctypes.c_void_p(0x10000 + 0x1000 * i) for i in range(4))
    in_codes = ctypes.c_void_p(0x10000 + 8 * (n * d - 1))                       # the last double of codes
    in_weight = ctypes.c_void_p(0x11000 + 8 * (classes * d - 1))
    before_codes = ctypes.c_void_p(0x10000 - 8 * (n * classes - 1))             # logits' last double is codes' first

    def product(codes=codes, n=n, d=d, weight=weight, bias=bias, classes=classes, logits=logits):
        return lib.gz_classifier_logits(codes, n, d, weight, bias, classes, logits, None)

    for bad in (dict(n=0), dict(n=-2), dict(d=0), dict(classes=0), dict(classes=-1), dict(codes=None), dict(weight=None),
                dict(logits=None), dict(logits=codes), dict(logits=weight), dict(logits=in_codes),
                dict(logits=in_weight), dict(logits=before_codes)):
        assert product(**bad) == BAD, bad
    assert product(n=1 << 40, classes=64) == TOO_LARGE                           # 2^34 row tiles
    assert product(n=1 << 50, d=1 << 20) == TOO_LARGE                            # no such array

    ws_bytes = lib.gz_inception_score_workspace_bytes
    assert ws_bytes(0, 5, 1) == 0 and ws_bytes(6, 0, 1) == 0 and ws_bytes(6, 5, 0) == 0 and ws_bytes(6, 5, 7) == 0
    assert ws_bytes(6, 5, 2) >= 8 and ws_bytes(6, 5, 2) % 8 == 0
    # partial column sums per block of rows, never per row: below an eighth of the logits themselves
    assert 0 < ws_bytes(50000, 1008, 10) < 50000 * 1008 * 8 // 8
    assert ws_bytes(64, 4096, 1) > 0 and ws_bytes(64, 100000, 1) > 0             # classes has no cap
    scores, ws = bias, weight

    def score(logits=logits, n=n, classes=classes, splits=2, scores=scores, ws=ws, nbytes=1 << 62):
        return lib.gz_inception_score(logits, n, classes, splits, scores, ws, nbytes, None)

    for bad in (dict(n=0), dict(classes=0), dict(splits=0), dict(splits=-1), dict(splits=n + 1), dict(logits=None),
                dict(scores=None), dict(ws=None)):
        assert score(**bad) == BAD, bad
    assert score(nbytes=ws_bytes(n, classes, 2) - 1) == WORKSPACE
    assert score(nbytes=0) == WORKSPACE
    assert score(n=1 << 40, classes=1, splits=1) == TOO_LARGE                     # 2^34 blocks of rows
    assert score(n=1 << 37, classes=1, splits=1 << 30) == TOO_LARGE               # 2^31 (split, block) pairs
    assert score(n=1 << 36, classes=1028, splits=1 << 30) == TOO_LARGE            # 2^30 pairs x 5 blocks of classes
    assert ws_bytes(1 << 37, 1, 1 << 30) == 0


@pytest.mark.parametrize("case", CASES, ids=str)
def test_yardstick_lies_within_the_bound_of_a_long_double_evaluation(case):
    from lightning_gan_zoo_amd import eval as E
    if np.finfo(np.longdouble).nmant <= 52:
        pytest.skip("numpy's long double is no wider than fp64 on this platform")
    n, d, classes, splits = case
    codes, weight, bias = inputs(case)
    logits = host_logits(codes, weight, bias)
    bound = score_bound(logit_delta(codes, weight, bias).max(), classes, n // splits)
    mean, std, scores = E.inception_score_from_logits(logits, splits)
    exact = long_double_scores(logits, splits)
    err = float(np.abs(scores / exact - 1).max())
    print("%s: scores %.4f .. %.4f, relative error %.3g, bound %.3g" % (case, scores.min(), scores.max(), err, bound))
    assert scores.shape == (splits,) and err <= bound
    assert bound < 1e-8                                              # the bound the GPU test uses is not vacuous
    assert mean == float(np.mean(scores)) and std == float(np.std(scores))
    if n // splits > 1:
        assert scores.min() > 1.2                                    # well away from the score of no information


def test_yardstick_known_values():
    from lightning_gan_zoo_amd import eval as E
    rng = np.random.RandomState(3)
    same = np.tile(rng.randn(1, 9), (20, 1))                        # every row the same distribution: KL = 0
    mean, std, scores = E.inception_score_from_logits(same, 4)
    assert np.allclose(scores, 1.0, rtol=1e-14, atol=0) and abs(mean - 1) < 1e-14 and std < 1e-14
    k = 6                                                            # confident rows spread evenly over k classes
    sharp = np.full((5 * k, 11), -50.0)
    sharp[np.arange(5 * k), np.arange(5 * k) % k] = 50.0
    mean, std, scores = E.inception_score_from_logits(sharp, 1)
    assert scores.shape == (1,) and abs(mean - k) < 1e-12 * k and std == 0.0
    mean, std, scores = E.inception_score_from_logits(sharp, 5)      # splits of k rows: one row per class each
    assert np.allclose(scores, k, rtol=1e-12, atol=0)
    assert np.array_equal(E.inception_score_from_logits(sharp[:-1], 2)[2],
                          E.inception_score_from_logits(sharp[:-2], 2)[2])      # 29 rows: the trailing one is ignored
    with pytest.raises(ValueError):
        E.inception_score_from_logits(sharp, 0)
    with pytest.raises(ValueError):
        E.inception_score_from_logits(sharp[:3], 4)


def test_yardstick_takes_logits_of_plus_and_minus_800():
    from lightning_gan_zoo_amd import eval as E
    logits = extreme_logits()
    assert (logits == 800.0).sum() > 100 and (logits == -800.0).sum() > 100
    assert ((logits == 800.0).sum(axis=1) == 0).sum() > 5            # rows of both kinds
    mean, std, scores = E.inception_score_from_logits(logits, EXTREME_SPLITS)
    assert np.isfinite(scores).all() and np.isfinite(mean) and np.isfinite(std) and scores.min() > 2
    if np.finfo(np.longdouble).nmant > 52:
        bound = score_bound(0.0, logits.shape[1], logits.shape[0] // EXTREME_SPLITS)
        assert float(np.abs(scores / long_double_scores(logits, EXTREME_SPLITS) - 1).max()) <= bound


def test_device_functions_refuse_a_cpu_tensor():
    from lightning_gan_zoo_amd import eval as E
    codes, weight = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(5, 3)
    for fn in (E.classifier_logits_device, E.inception_score_device):
        with pytest.raises(RuntimeError, match="there is no fallback"):
            fn(codes, weight)
        with pytest.raises(ValueError):
            fn(codes.float(), weight)
        with pytest.raises(ValueError):
            fn(codes[0], weight)

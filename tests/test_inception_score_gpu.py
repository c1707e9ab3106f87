"""The Inception Score on the device (csrc/gz_inception_score.hip): gz_classifier_logits entry by entry and
gz_inception_score split by split against the host yardstick (numpy's logits, eval.inception_score_from_logits) within
the derived bounds of tests/inception_score_support.py; exact integers against numpy's bits; equal bits of two calls
with NaN-prefilled outputs and workspace; logits of +-800; the ignored trailing rows; eval.evaluate_device with and
without a classifier.

Measured on the MI355X: see each test's docstring; the seven cases and the +-800 logits take 3.5 s in all."""
import numpy as np
import pytest
import torch

from inception_score_support import (CASES, EXTREME_SPLITS, ONE_ROW_CASE, TRAILING_CASE, exact_inputs, extreme_logits,
                                     host_logits, inputs, logit_delta, score_bound)

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def _logits(codes, weight, bias):
    """gz_classifier_logits into a NaN-prefilled buffer -> numpy [n, classes]."""
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    (n, d), classes = codes.shape, weight.shape[0]
    c, w = _dev(codes), _dev(weight)
    b = None if bias is None else _dev(bias)
    out = torch.full((n, classes), NAN, dtype=torch.float64, device="cuda")
    check(lib.gz_classifier_logits(F._p(c), n, d, F._p(w), None if b is None else F._p(b), classes, F._p(out),
                                   F._stream()), "classifier_logits")
    return out.cpu().numpy()


def _scores(logits, splits):
    """gz_inception_score with NaN-prefilled scores and workspace, twice -> the two numpy [splits] results."""
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    n, classes = logits.shape
    l = _dev(logits)
    ws_bytes = lib.gz_inception_score_workspace_bytes(n, classes, splits)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    out = []
    for _ in range(2):
        scores = torch.full((splits,), NAN, dtype=torch.float64, device="cuda")
        ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
        check(lib.gz_inception_score(F._p(l), n, classes, splits, F._p(scores), F._p(ws), ws_bytes, F._stream()),
              "inception_score")
        out.append(scores.cpu().numpy())
    return out


_host = {}


def _host_side(case):
    """(numpy's logits, delta, the yardstick's split scores) of a case, computed once."""
    if case not in _host:
        from lightning_gan_zoo_amd import eval as E
        codes, weight, bias = inputs(case)
        logits = host_logits(codes, weight, bias)
        _host[case] = (logits, logit_delta(codes, weight, bias), E.inception_score_from_logits(logits, case[3])[2])
    return _host[case]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_logits_lie_within_the_bound_of_numpy(case):
    """Measured: the largest |device - numpy| / (2 delta) over the seven cases is 0.046, at (200, 40, 5, 10); 0.0011 at
    d = 2048; the other five cases have numpy's bits at every entry."""
    codes, weight, bias = inputs(case)
    want, delta, _ = _host_side(case)
    got = _logits(codes, weight, bias)
    assert got.shape == want.shape and np.isfinite(got).all()        # every row and class was stored
    ratio = float((np.abs(got - want) / (2 * delta)).max())
    print("%s: logits, largest error / (2 delta) %.3g, equal bits at %d of %d" % (case, ratio, (got == want).sum(), got.size))
    assert (np.abs(got - want) <= 2 * delta).all()


def test_logits_without_a_bias():
    case = (130, 70, 67, 2)
    codes, weight, _ = inputs(case)
    want, delta = host_logits(codes, weight), logit_delta(codes, weight)
    got = _logits(codes, weight, None)
    assert np.isfinite(got).all() and (np.abs(got - want) <= 2 * delta).all()
    assert np.abs(got - _host_side(case)[0]).max() > 1e-3            # (the bias is not a rounding error)


def test_logits_of_exact_integers_are_numpys_bits():
    codes, weight, bias = exact_inputs()
    assert np.array_equal(_logits(codes, weight, bias), host_logits(codes, weight, bias))
    assert np.array_equal(_logits(codes, weight, None), host_logits(codes, weight))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_scores_lie_within_the_bound_of_the_yardstick(case):
    """Device scores of the DEVICE's logits against the yardstick on numpy's logits, split by split.  Measured: the
    largest relative difference over the seven cases is 2.2e-15, at (65, 2048, 1008, 5) with a bound of 4.0e-9; the others
    lie at or below 4.4e-16 with bounds of 9.2e-13 .. 6.3e-11."""
    n, d, classes, splits = case
    codes, weight, bias = inputs(case)
    _, delta, want = _host_side(case)
    first, second = _scores(_logits(codes, weight, bias), splits)
    bound = score_bound(float(delta.max()), classes, n // splits)
    rel = np.abs(first / want - 1)
    print("%s: scores %.4f .. %.4f, largest relative difference %.3g, bound %.3g"
          % (case, want.min(), want.max(), float(rel.max()), bound))
    assert first.shape == (splits,) and np.isfinite(first).all()
    assert np.array_equal(first, second)                             # two calls, equal bits
    assert (rel <= bound).all()
    if case == ONE_ROW_CASE:
        assert np.array_equal(first, np.ones(splits))                # py = p: exactly 1


def test_scores_of_logits_of_plus_and_minus_800():
    """Measured: the yardstick's bits on both splits (relative difference 0), bound 4.4e-14."""
    from lightning_gan_zoo_amd import eval as E
    logits = extreme_logits()
    want = E.inception_score_from_logits(logits, EXTREME_SPLITS)[2]
    first, second = _scores(logits, EXTREME_SPLITS)
    bound = score_bound(0.0, logits.shape[1], logits.shape[0] // EXTREME_SPLITS)
    rel = np.abs(first / want - 1)
    print("+-800: scores %s, largest relative difference %.3g, bound %.3g" % (want, float(rel.max()), bound))
    assert np.isfinite(first).all() and np.array_equal(first, second)
    assert (rel <= bound).all()


def test_trailing_rows_are_ignored_bit_for_bit():
    n, d, classes, splits = TRAILING_CASE
    logits = _host_side(TRAILING_CASE)[0]
    used = (n // splits) * splits
    assert used == 255 and n - used == 2
    assert np.array_equal(_scores(logits, splits)[0], _scores(logits[:used], splits)[0])


def test_python_entry_points():
    from lightning_gan_zoo_amd import eval as E
    case = (130, 70, 67, 2)
    codes, weight, bias = inputs(case)
    want_logits, delta, want = _host_side(case)
    dev = _dev(codes)
    # the head as the weight file holds it: float32 on the host (widened exactly), and as the runner hands it over
    w32, b32 = torch.from_numpy(weight.astype(np.float32)), torch.from_numpy(bias.astype(np.float32))
    got32 = E.classifier_logits_device(dev, w32, b32).cpu().numpy()
    assert np.array_equal(got32, _logits(codes, w32.double().numpy(), b32.double().numpy()))
    got = E.classifier_logits_device(dev, _dev(weight), _dev(bias))
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (130, 67)
    assert np.array_equal(got.cpu().numpy(), _logits(codes, weight, bias))
    mean, std, scores = E.inception_score_device(dev, weight, bias, splits=2)
    assert np.array_equal(scores, _scores(got.cpu().numpy(), 2)[0])
    assert mean == float(np.mean(scores)) and std == float(np.std(scores))
    assert (np.abs(scores / want - 1) <= score_bound(float(delta.max()), 67, 65)).all()
    with pytest.raises(ValueError):
        E.inception_score_device(dev, weight, bias, splits=131)
    with pytest.raises(ValueError):
        E.classifier_logits_device(dev, weight[:, :-1], bias)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_evaluate_device_with_and_without_a_classifier():
    """Measured: ``is`` 2.699480 +- 0.047438; the yardstick's bits for ``is`` and 6.8e-17 (of the largest split score) from
    its ``is_std`` on the codes copied back, bound 8.1e-11."""
    from lightning_gan_zoo_amd import eval as E
    from test_eval_device_gpu import PixelStatistics, _native_dump, _tiny
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=200)
    net = PixelStatistics()
    rng = np.random.RandomState(12)
    codes = E.device_activations(module, dump, net.device, batch=16).cpu().numpy()
    real = E.RealStatistics(codes[rng.randint(0, 200, 260)] * 0.9 + rng.randn(260, 24) * codes.std(axis=0) * 0.5,
                            module.device)
    # a random head over the 24 stand-in features, scaled so that the logits differ by a few units from row to row and
    # centred by its bias (the features sit at ~1 with a spread of 0.1: uncentred, one class would take every row and
    # every score would be 1.00)
    weight = rng.randn(37, 24)
    weight *= 2.5 / (codes - codes.mean(axis=0)).dot(weight.T).std()
    bias = 0.1 * rng.randn(37) - codes.mean(axis=0).dot(weight.T)
    np.random.seed(21)
    plain = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5)
    state = np.random.get_state()
    np.random.seed(21)
    scored = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5,
                               classifier=(torch.from_numpy(weight), torch.from_numpy(bias)), inception_splits=4)
    assert _same_state(np.random.get_state(), state)                 # the score draws nothing
    assert set(plain) == {"fid", "kid", "kid_std"}
    assert set(scored) == {"fid", "kid", "kid_std", "is", "is_std"}
    assert {k: scored[k] for k in plain} == plain                    # today's dict, bit for bit
    want_mean, want_std, want = E.inception_score_from_logits(host_logits(codes, weight, bias), 4)
    bound = score_bound(float(logit_delta(codes, weight, bias).max()), 37, 50)
    print("evaluate_device: is %.6f +- %.6f, yardstick %.6f +- %.6f, relative differences %.3g and %.3g, bound %.3g"
          % (scored["is"], scored["is_std"], want_mean, want_std, abs(scored["is"] / want_mean - 1),
             abs(scored["is_std"] - want_std) / want.max(), bound))
    assert want.min() > 1.05 and want_std > 0
    assert abs(scored["is"] - want_mean) <= bound * want_mean
    assert abs(scored["is_std"] - want_std) <= bound * want.max()    # a std of values that each move by <= bound * value


def test_runner_evaluator_scores_with_the_heads_own_parameters(capsys):
    """run_network.device_fid_evaluator(inception_score=True) on a stand-in feature net whose ``net.fc`` is a float32
    nn.Linear on the device: the head is widened by the runner, the epoch line carries the score, and the score is the
    yardstick's on the float32 head's values."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import run_network as R
    from test_eval_device_gpu import PixelStatistics, _native_dump, _tiny
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=40)
    codes = E.device_activations(module, dump, PixelStatistics().device, batch=16).cpu().numpy()
    rng = np.random.RandomState(8)
    weight = rng.randn(11, 24)
    weight *= 2.5 / (codes - codes.mean(axis=0)).dot(weight.T).std()
    bias = 0.1 * rng.randn(11) - codes.mean(axis=0).dot(weight.T)

    class Features(PixelStatistics):
        class net:
            fc = torch.nn.Linear(24, 11).cuda()

    with torch.no_grad():
        Features.net.fc.weight.copy_(torch.from_numpy(weight))
        Features.net.fc.bias.copy_(torch.from_numpy(bias))
    w32, b32 = weight.astype(np.float32).astype(np.float64), bias.astype(np.float32).astype(np.float64)
    real_act = np.random.RandomState(3).rand(50, 24) * 2
    evaluate = R.device_fid_evaluator(dump, Features(), real_act, module.device, batch=16, inception_score=True,
                                      inception_splits=4)
    np.random.seed(1)
    m = evaluate(module, 2)
    assert set(m) == {"fid", "kid", "kid_std", "is", "is_std"}
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("epoch 2 FID: ") and line.endswith(" IS: %.4f +- %.4f" % (m["is"], m["is_std"]))
    want_mean, want_std, want = E.inception_score_from_logits(host_logits(codes, w32, b32), 4)
    bound = score_bound(float(logit_delta(codes, w32, b32).max()), 11, 10)
    assert want.min() > 1.05
    assert abs(m["is"] - want_mean) <= bound * want_mean and abs(m["is_std"] - want_std) <= bound * want.max()
    np.random.seed(1)
    plain = R.device_fid_evaluator(dump, PixelStatistics(), real_act, module.device, batch=16)(module, 2)
    assert plain == {k: m[k] for k in ("fid", "kid", "kid_std")}     # key off: no ``net`` is asked for
    assert " IS: " not in capsys.readouterr().out

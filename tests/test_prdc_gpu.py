"""Precision / recall / density / coverage on the device (csrc/gz_prdc.hip) against the host yardstick (eval.prdc: numpy
fp64 on direct differences) on the cases of tests/prdc_support.py: radii and nearest distances within the derived bound,
every count, total and quotient exactly the yardstick's (tests/test_prdc_cpu.py shows that no decision of any case lies
within 1000 bounds of its threshold); small-integer codes against the yardstick's bits; equal bits of two calls with
NaN-prefilled outputs and workspace and of two slicings; refusals that touch nothing; the Python wiring.

Measured on the MI355X: see each test's docstring; the 25 tests take 4.2 s in all."""
import ctypes

import numpy as np
import pytest
import torch

from prdc_support import (ALL_CASES, EXACT_CASE, REDUCED_BUDGET, SLICED_CASE, SLICED_PLAN_FULL, SLICED_PLAN_REDUCED,
                          dist_bound, duplicate_inputs, exact_inputs, host, inputs, near_bound, radii_bound, sqnorms)

pytestmark = pytest.mark.gpu
NAN = float("nan")
METRICS = ("precision", "recall", "density", "coverage")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # (a copy: the shared inputs are read-only)


def _radii(codes, k, calls=2):
    """gz_knn_radii into NaN-prefilled radii with a NaN-prefilled workspace, ``calls`` times -> numpy [n] each."""
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    n, d = codes.shape
    x = _dev(codes)
    ws_bytes = lib.gz_knn_radii_workspace_bytes(n, d, k)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    out = []
    for _ in range(calls):
        radii = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
        ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
        check(lib.gz_knn_radii(F._p(x), n, d, k, F._p(radii), F._p(ws), ws_bytes, F._stream()), "knn_radii")
        out.append(radii.cpu().numpy())
    return out


def _counts(g, rad_g, r, rad_r, calls=2):
    """gz_prdc_counts into prefilled outputs (NaN, -7) with a NaN-prefilled workspace, ``calls`` times
    -> (in_real, in_fake, near, totals) as numpy arrays each."""
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    (n_g, d), n_r = g.shape, r.shape[0]
    xg, xr, dg, dr = _dev(g), _dev(r), _dev(rad_g), _dev(rad_r)
    ws_bytes = lib.gz_prdc_counts_workspace_bytes(n_g, n_r, d)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    out = []
    for _ in range(calls):
        in_real = torch.full((n_g,), -7, dtype=torch.int32, device="cuda")
        in_fake = torch.full((n_r,), -7, dtype=torch.int32, device="cuda")
        near = torch.full((n_r,), NAN, dtype=torch.float64, device="cuda")
        totals = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")
        check(lib.gz_prdc_counts(F._p(xg), n_g, F._p(dg), F._p(xr), n_r, F._p(dr), d, F._p(in_real), F._p(in_fake),
                                 F._p(near), F._p(totals), F._p(ws), ws_bytes, F._stream()), "prdc_counts")
        out.append(tuple(t.cpu().numpy() for t in (in_real, in_fake, near, totals)))
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _plan(n_rows, n_cols):
    from lightning_gan_zoo_amd._lib import lib
    groups, slices = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.gz_prdc_plan(n_rows, n_cols, ctypes.byref(groups), ctypes.byref(slices)) == 0
    return groups.value, slices.value


def _host_totals(h):
    return [int((h["in_real"] > 0).sum()), int((h["in_fake"] > 0).sum()), int(h["in_real"].sum()),
            int((h["near"] <= h["rad_r"]).sum())]


@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_radii_lie_within_the_bound_of_the_yardstick(case):
    """Measured: the largest |device - yardstick| / bound per case, both sets: 0.032, 0.056, 0.051, 0.034, 0.0071 at
    d = 2048 and 0.114 on the sliced case."""
    h = host(case)
    worst = 0.0
    for codes, want in zip(inputs(case), (h["rad_g"], h["rad_r"])):
        first, second = _radii(codes, case[3])
        assert _same_bits(first, second)
        assert np.isfinite(first).all() and (first >= 0).all()
        ratio = np.abs(first - want) / radii_bound(codes, want)
        worst = max(worst, float(ratio.max()))
    print("radii %s: largest |device - yardstick| / bound %.3g" % (case, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("source", ["device_radii", "yardstick_radii"])
@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_counts_totals_and_quotients_are_the_yardsticks(case, source):
    """With the device's own radii, and with the yardstick's radii passed in so that a radius error cannot hide a count
    error.  Measured: the largest |near - yardstick| / bound per case, the same with either radii: 0.030, 0.018, 0.024,
    0.013, 0.0027 at d = 2048 and 0.048 on the sliced case."""
    from lightning_gan_zoo_amd import eval as E
    g, r = inputs(case)
    k, h = case[3], host(case)
    if source == "device_radii":
        rad_g, rad_r = _radii(g, k, calls=1)[0], _radii(r, k, calls=1)[0]
    else:
        rad_g, rad_r = h["rad_g"], h["rad_r"]
    first, second = _counts(g, rad_g, r, rad_r)
    for a, b in zip(first, second):
        assert _same_bits(a, b)
    in_real, in_fake, near, totals = first
    assert in_real.dtype == np.int32 and in_fake.dtype == np.int32 and totals.dtype == np.int64
    assert np.array_equal(in_real, h["in_real"]) and np.array_equal(in_fake, h["in_fake"])
    ratio = float((np.abs(near - h["near"]) / near_bound(g, r, h["near"])).max())
    print("counts %s %s: largest |near - yardstick| / bound %.3g" % (case, source, ratio))
    assert ratio <= 1.0 and (near >= 0).all()
    assert totals.tolist() == _host_totals(h)
    given = {} if source == "device_radii" else {"rad_g": _dev(rad_g), "rad_r": _dev(rad_r)}
    m = E.prdc_device(_dev(g), _dev(r), k=k, **given)
    assert set(m) == set(h)
    for key in METRICS:
        assert isinstance(m[key], float) and m[key] == h[key], key
    assert m["in_real"].dtype == torch.int32 and m["near"].is_cuda and m["rad_r"].dtype == torch.float64
    assert _same_bits(m["in_real"].cpu().numpy(), in_real) and _same_bits(m["in_fake"].cpu().numpy(), in_fake)
    assert _same_bits(m["near"].cpu().numpy(), near)
    assert _same_bits(m["rad_g"].cpu().numpy(), rad_g) and _same_bits(m["rad_r"].cpu().numpy(), rad_r)


def test_small_integer_codes_give_the_yardsticks_bits():
    """Every product, sum and difference is exact on either side, so radii and nearest distances are the yardstick's bits
    and the many exact ties (tests/test_prdc_cpu.py counts them) go through the <= as they do there."""
    g, r = exact_inputs()
    k, h = EXACT_CASE[3], host(EXACT_CASE)
    rad_g, rad_r = _radii(g, k, calls=1)[0], _radii(r, k, calls=1)[0]
    assert _same_bits(rad_g, h["rad_g"]) and _same_bits(rad_r, h["rad_r"])
    in_real, in_fake, near, totals = _counts(g, rad_g, r, rad_r, calls=1)[0]
    assert _same_bits(near, h["near"])
    assert np.array_equal(in_real, h["in_real"]) and np.array_equal(in_fake, h["in_fake"])
    assert totals.tolist() == _host_totals(h)


def test_exact_duplicates_come_out_at_zero_or_within_the_bound_never_negative():
    """Rows 5 and 68 are one row with |x|^2 ~ 400: the Gram form cancels to rounding noise of either sign, the clamp
    keeps it at 0 or above.  Measured: exactly 0.0 on both rows, bound 7.7e-12."""
    x = duplicate_inputs()
    rad = _radii(x, 1, calls=1)[0]
    s = sqnorms(x)
    bound = dist_bound(x.shape[1], 2 * s[5], 0.0)
    print("duplicates: squared distance %.3g and %.3g, bound %.3g" % (rad[5], rad[68], bound))
    assert rad[5] == rad[68] and 0.0 <= rad[5] <= bound
    assert (rad >= 0).all() and (np.delete(rad, [5, 68]) > 1.0).all()
    # as the real set of a counts walk: the generated copy of the row is inside both balls of radius ~0 only by <=
    g = np.ascontiguousarray(x[[5, 20]])
    in_real, in_fake, near, _ = _counts(g, np.array([rad[5], 0.0]), x, rad, calls=1)[0]
    assert near[5] == near[68] == rad[5] and (near >= 0).all()      # (the same expression on the same operands)
    assert in_real[0] >= 2 and in_fake[5] >= 1 and in_fake[68] >= 1


def test_two_slicings_give_identical_bits():
    """The sliced case at the full CU budget (65 row groups of two row tiles x 3 column slices; gz_knn_radii of the
    generated set in 7 slices) and at a budget of 64 CUs (one column slice; one slice): radii, counts, nearest distances and totals are the
    same bits, and the yardstick's integers."""
    from lightning_gan_zoo_amd._lib import lib
    g, r = inputs(SLICED_CASE)
    k, h = SLICED_CASE[3], host(SLICED_CASE)
    budget = lib.gz_get_cu_budget()
    results = []
    try:
        for cus, plan in ((256, SLICED_PLAN_FULL), (REDUCED_BUDGET, SLICED_PLAN_REDUCED)):
            assert lib.gz_set_cu_budget(cus) == cus
            assert _plan(g.shape[0], r.shape[0]) == plan
            rad_g, rad_r = _radii(g, k, calls=1)[0], _radii(r, k, calls=1)[0]
            results.append((rad_g, rad_r) + _counts(g, rad_g, r, rad_r, calls=1)[0])
    finally:
        lib.gz_set_cu_budget(budget)
    assert SLICED_PLAN_FULL[0] > 1 and SLICED_PLAN_FULL[1] > 1 and SLICED_PLAN_REDUCED[1] == 1
    ws = lib.gz_knn_radii_workspace_bytes
    lib.gz_set_cu_budget(REDUCED_BUDGET)
    try:
        one = ws(g.shape[0], g.shape[1], k)
    finally:
        lib.gz_set_cu_budget(budget)
    assert ws(g.shape[0], g.shape[1], k) > one == 8 * g.shape[0] * (1 + k)      # (more than one slice, exactly one)
    for a, b in zip(*results):
        assert _same_bits(a, b)
    assert np.array_equal(results[0][2], h["in_real"]) and np.array_equal(results[0][3], h["in_fake"])
    assert results[0][5].tolist() == _host_totals(h)


def test_refused_calls_return_their_code_and_touch_nothing():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    BAD, WORKSPACE = -1, -3
    n, d = 70, 9
    x = _dev(np.random.RandomState(0).randn(n, d))
    radii = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
    ws_bytes = lib.gz_knn_radii_workspace_bytes(n, d, 8)
    ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device="cuda")

    def knn(n=n, d=d, k=3, nbytes=ws_bytes, codes=x):
        return lib.gz_knn_radii(None if codes is None else F._p(codes), n, d, k, F._p(radii), F._p(ws), nbytes,
                                F._stream())

    for bad in (dict(k=0), dict(k=9), dict(k=n), dict(n=3, k=3), dict(d=0), dict(codes=None)):
        assert knn(**bad) == BAD, bad
    assert knn(k=8, nbytes=ws_bytes - 8) == WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(radii).all() and torch.isnan(ws).all()

    in_real = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    in_fake = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    near = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
    totals = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    rad = torch.ones((n,), dtype=torch.float64, device="cuda")
    cbytes = lib.gz_prdc_counts_workspace_bytes(n, n, d)
    cws = torch.full((cbytes // 8,), NAN, dtype=torch.float64, device="cuda")

    def counts(n_g=n, n_r=n, d=d, nbytes=cbytes, rad_g=rad):
        return lib.gz_prdc_counts(F._p(x), n_g, None if rad_g is None else F._p(rad_g), F._p(x), n_r, F._p(rad), d,
                                  F._p(in_real), F._p(in_fake), F._p(near), F._p(totals), F._p(cws), nbytes, F._stream())

    for bad in (dict(n_g=0), dict(n_r=0), dict(d=0), dict(rad_g=None)):
        assert counts(**bad) == BAD, bad
    assert counts(nbytes=cbytes - 8) == WORKSPACE
    torch.cuda.synchronize()
    assert (in_real == -7).all() and (in_fake == -7).all() and (totals == -7).all()
    assert torch.isnan(near).all() and torch.isnan(cws).all()
    assert counts() == 0 and knn() == 0                            # the same buffers are fine for an accepted call
    torch.cuda.synchronize()
    assert not torch.isnan(near).any() and not torch.isnan(radii).any() and int(in_real.min()) >= 0


def test_python_entries_take_fp64_device_tensors_only():
    from lightning_gan_zoo_amd import eval as E
    g, r = inputs(ALL_CASES[1])
    with pytest.raises(RuntimeError, match=r"no fallback \(use eval\.prdc\)"):
        E.prdc_device(torch.from_numpy(np.array(g)), torch.from_numpy(np.array(r)))
    with pytest.raises(RuntimeError, match=r"use eval\.prdc"):
        E.prdc_device(_dev(g), torch.from_numpy(np.array(r)))
    with pytest.raises(ValueError):
        E.prdc_device(_dev(g).float(), _dev(r))
    with pytest.raises(ValueError):
        E.prdc_device(_dev(g), _dev(r), k=9)
    with pytest.raises(ValueError):
        E.prdc_device(_dev(g), _dev(r), rad_r=torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        E.knn_radii_device(_dev(g), 64)
    strided = _dev(np.concatenate([g, g], axis=1))[:, :g.shape[1]]           # not contiguous: copied, not misread
    assert _same_bits(E.knn_radii_device(strided, 5).cpu().numpy(), E.knn_radii_device(_dev(g), 5).cpu().numpy())


def test_real_statistics_keep_their_radii_per_k(monkeypatch):
    from lightning_gan_zoo_amd import eval as E
    _, r = inputs(ALL_CASES[2])
    real = E.RealStatistics(np.array(r), "cuda")                   # (a copy: the shared inputs are read-only)
    calls = []
    device = E.knn_radii_device
    monkeypatch.setattr(E, "knn_radii_device", lambda codes, k: calls.append(k) or device(codes, k))
    first = real.radii(3)
    assert real.radii(3) is first and real.radii(5) is not first and real.radii(5) is real.radii(5)
    assert calls == [3, 5]
    assert _same_bits(first.cpu().numpy(), _radii(r, 3, calls=1)[0])


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_evaluate_device_with_and_without_a_k():
    """eval.evaluate_device on a tiny stand-in net: with ``prdc_k`` the dict gains the four metrics, which are
    ``prdc_device``'s on the resident codes; everything else, and numpy's generator afterwards, is what it is without."""
    from lightning_gan_zoo_amd import eval as E
    from test_eval_device_gpu import PixelStatistics, _native_dump, _tiny
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=200)
    net = PixelStatistics()
    rng = np.random.RandomState(12)
    fake = E.device_activations(module, dump, net.device, batch=16)
    codes = fake.cpu().numpy()
    real = E.RealStatistics(codes[rng.randint(0, 200, 260)] * 0.9 + rng.randn(260, 24) * codes.std(axis=0) * 0.5,
                            module.device)
    np.random.seed(21)
    plain = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5)
    state = np.random.get_state()
    np.random.seed(21)
    scored = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5, prdc_k=3)
    assert _same_state(np.random.get_state(), state)                 # the metrics draw nothing
    assert set(plain) == {"fid", "kid", "kid_std"}
    assert set(scored) == {"fid", "kid", "kid_std"} | set(METRICS)
    assert {key: scored[key] for key in plain} == plain              # today's dict, bit for bit
    direct = E.prdc_device(fake, real.codes, k=3)
    want = E.prdc(codes, real.codes.cpu().numpy(), k=3)
    print("evaluate_device:", {key: scored[key] for key in METRICS}, "yardstick", {key: want[key] for key in METRICS})
    for key in METRICS:
        # (the direct call is what the cases above hold to the yardstick; these stand-in codes have no arranged margins)
        assert scored[key] == direct[key] and 0.0 <= scored[key]
    assert 3 in real._radii and len(real._radii) == 1

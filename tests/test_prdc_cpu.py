"""Precision / recall / density / coverage without a GPU: the host yardstick (eval.prdc, eval.knn_radii) on hand cases
with known answers and against an unblocked brute force, its refusals, the runner keys, the C ABI's argument checks and
grid plan, and the conditions the GPU tests' inputs must meet (tests/prdc_support.py): no decision within 1000 bounds of
its threshold, all four metrics strictly inside (0, 1)."""
import ctypes

import numpy as np
import pytest

from prdc_support import (ALL_CASES, EXACT_CASE, MARGIN, REDUCED_BUDGET, SLICED_CASE, SLICED_PLAN_FULL,
                          SLICED_PLAN_REDUCED, duplicate_inputs, exact_inputs, host, inputs, smallest_margin)

METRICS = ("precision", "recall", "density", "coverage")


def _brute(g, r, k):
    """The definitions, one pair at a time."""
    def dist(x, y):
        return float(((x - y) ** 2).sum())

    def radii(x):
        return np.array([sorted(dist(x[i], x[j]) for j in range(len(x)) if j != i)[k - 1] for i in range(len(x))])

    rad_g, rad_r = radii(g), radii(r)
    cross = np.array([[dist(gj, ri) for ri in r] for gj in g])
    in_real = (cross <= rad_r[None, :]).sum(axis=1)
    in_fake = (cross <= rad_g[:, None]).sum(axis=0)
    near = cross.min(axis=0)
    return {"precision": (in_real > 0).sum() / len(g), "recall": (in_fake > 0).sum() / len(r),
            "density": in_real.sum() / (k * len(g)), "coverage": (near <= rad_r).sum() / len(r),
            "in_real": in_real, "in_fake": in_fake, "near": near, "rad_g": rad_g, "rad_r": rad_r}


def test_a_copy_of_the_real_set_scores_one():
    from lightning_gan_zoo_amd import eval as E
    r = np.random.RandomState(0).randn(40, 6)
    m = E.prdc(r.copy(), r, k=3)
    assert m["precision"] == 1.0 and m["recall"] == 1.0 and m["coverage"] == 1.0
    assert np.array_equal(m["near"], np.zeros(40))
    assert np.array_equal(m["rad_g"], m["rad_r"]) and (m["rad_r"] > 0).all()
    assert m["in_real"].min() >= 1 and m["in_real"].dtype.kind == "i"


def test_two_far_clusters_score_zero():
    from lightning_gan_zoo_amd import eval as E
    rng = np.random.RandomState(1)
    m = E.prdc(rng.randn(30, 5) + 100.0, rng.randn(35, 5) - 100.0, k=5)
    assert [m[key] for key in METRICS] == [0.0, 0.0, 0.0, 0.0]
    assert not m["in_real"].any() and not m["in_fake"].any() and m["near"].min() > 1e4


def test_a_block_of_duplicates_has_radius_zero_and_still_counts():
    """k + 1 equal real rows: each has k others at distance 0, so its radius is 0 (self is skipped by index, not by
    value), and a generated row that equals them lies in all k + 1 balls because the comparison is <=."""
    from lightning_gan_zoo_amd import eval as E
    rng = np.random.RandomState(2)
    k = 3
    r = rng.randn(20, 4)
    r[:k + 1] = r[0]
    g = rng.randn(12, 4) + 50.0
    g[7] = r[0]
    m = E.prdc(g, r, k=k)
    assert np.array_equal(m["rad_r"][:k + 1], np.zeros(k + 1)) and (m["rad_r"][k + 1:] > 0).all()
    assert np.array_equal(E.knn_radii(r, k), m["rad_r"])
    assert m["in_real"][7] >= k + 1 and m["in_real"].sum() == m["in_real"][7]
    assert m["precision"] == 1 / 12 and m["near"][0] == 0.0
    assert E.knn_radii(r, k + 1)[0] > 0                         # one neighbour more leaves the block


def test_the_blocked_yardstick_is_the_brute_force(monkeypatch):
    from lightning_gan_zoo_amd import eval as E
    rng = np.random.RandomState(3)
    g, r = rng.randn(37, 7), 0.8 * rng.randn(29, 7) + 0.3
    blocks = E._row_blocks
    assert blocks(10, 7, 3, budget=50) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10)]
    assert blocks(5, 100, 100, budget=50) == [(i, i + 1) for i in range(5)]
    assert blocks(5, 2, 2) == [(0, 5)]
    monkeypatch.setattr(E, "_row_blocks", lambda n, m, d: blocks(n, m, d, budget=7 * 7 * 5))    # 5, then 6 rows a block
    for k in (1, 4):
        got, want = E.prdc(g, r, k=k), _brute(g, r, k)
        assert set(got) == set(want)
        for key in want:
            assert np.array_equal(got[key], want[key]), (k, key)
        assert all(isinstance(got[key], float) for key in METRICS)


def test_bad_k_and_bad_shapes_are_refused():
    from lightning_gan_zoo_amd import eval as E
    g, r = np.zeros((12, 3)), np.zeros((10, 3))
    for k in (0, -1, 9, 10, 11):
        with pytest.raises(ValueError):
            E.prdc(g, r, k=k)
    with pytest.raises(ValueError):
        E.knn_radii(r, 10)
    with pytest.raises(ValueError):
        E.prdc(g, np.zeros((10, 4)))
    with pytest.raises(ValueError):
        E.prdc(g, np.zeros(10))
    with pytest.raises(ValueError):
        E.knn_radii(np.zeros((10, 0)), 2)
    assert E.prdc(g, r, k=8)["precision"] == 1.0 and E.knn_radii(r, 9 - 1).shape == (10,)


def test_the_device_path_refuses_cpu_tensors_and_names_the_yardstick():
    import torch
    from lightning_gan_zoo_amd import eval as E
    g, r = torch.zeros((12, 3), dtype=torch.float64), torch.zeros((10, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r"no fallback \(use eval\.prdc\)"):
        E.prdc_device(g, r)
    with pytest.raises(RuntimeError, match=r"no fallback \(use eval\.knn_radii\)"):
        E.knn_radii_device(r, 2)
    with pytest.raises(ValueError):
        E.prdc_device(g.float(), r)


def test_runner_keys_parse_default_off_and_need_the_device_pass():
    from lightning_gan_zoo_amd.run_network import RUNNER_KEYS, check_eval_keys, parse_overrides
    assert RUNNER_KEYS["precision_recall"] is False and RUNNER_KEYS["precision_recall_k"] == 5
    run = parse_overrides(["+expt=dc_gan"])[3]
    assert run["precision_recall"] is False and run["precision_recall_k"] == 5
    for plus in ("", "+"):
        run = parse_overrides(["+expt=dc_gan", plus + "eval_on_device=true", plus + "precision_recall=true",
                               plus + "precision_recall_k=3"])[3]
        assert run["precision_recall"] is True and run["precision_recall_k"] == 3
    with pytest.raises(SystemExit, match="precision_recall=true is honoured only together with eval_on_device=true"):
        parse_overrides(["+expt=dc_gan", "precision_recall=true"])
    with pytest.raises(SystemExit, match="eval_on_device"):
        check_eval_keys({"precision_recall": True, "kid_on_device": True})
    check_eval_keys({"precision_recall": True, "eval_on_device": True})
    check_eval_keys({"precision_recall_k": 3})


def test_evaluate_device_reports_the_metrics_only_with_a_k(monkeypatch):
    """After KID, on the same resident generated tensor, with the real set's kept radii; without ``prdc_k`` the call and
    the dict are today's."""
    import inspect
    from lightning_gan_zoo_amd import eval as E
    assert inspect.signature(E.evaluate_device).parameters["prdc_k"].default is None
    order = []

    class Fake:
        device = "gpu"

    fake = Fake()

    class Real:
        mu, sigma, codes = "mu", "sigma", "codes"

        def radii(self, k):
            order.append(("radii", k))
            return "rad%d" % k

    class Moment:
        def cpu(self):
            return self

        def numpy(self):
            return "m"

    def kid(*a, **k):
        order.append("kid")
        return (np.array([1.0, 3.0]),)

    def device(g, r, k=5, rad_r=None):
        order.append(("prdc", g, r, k, rad_r))
        return {"precision": 0.5, "recall": 0.25, "density": 1.5, "coverage": 0.75, "in_real": "x", "near": "y"}

    monkeypatch.setattr(E, "device_activations", lambda *a: fake)
    monkeypatch.setattr(E, "feature_moments_device", lambda codes: (Moment(), Moment()))
    monkeypatch.setattr(E, "frechet_distance", lambda *a: 3.0)
    monkeypatch.setattr(E, "polynomial_mmd_averages_device", kid)
    monkeypatch.setattr(E, "prdc_device", device)
    assert E.evaluate_device("m", "dump", "net", Real()) == {"fid": 3.0, "kid": 2.0, "kid_std": 1.0}
    assert order == ["kid"]
    out = E.evaluate_device("m", "dump", "net", Real(), prdc_k=3)
    assert out == {"fid": 3.0, "kid": 2.0, "kid_std": 1.0, "precision": 0.5, "recall": 0.25, "density": 1.5,
                   "coverage": 0.75}
    assert order[1:] == ["kid", ("radii", 3), ("prdc", fake, "codes", 3, "rad3")]


def test_runner_passes_k_and_prints_the_four_values(monkeypatch, capsys):
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import run_network as R
    calls = []
    result = {"fid": 1.0, "kid": 2.0, "kid_std": 0.5, "precision": 0.5, "recall": 0.25, "density": 1.5, "coverage": 0.75}
    monkeypatch.setattr(E, "RealStatistics", lambda *a, **k: "real")
    monkeypatch.setattr(E, "evaluate_device", lambda *a, **k: calls.append(k) or result)

    class Features:
        device = "net"

    class Module:
        training = False

    plain = R.device_fid_evaluator("dump", Features(), "act", "cuda")
    scored = R.device_fid_evaluator("dump", Features(), "act", "cuda", prdc_k=3)
    assert plain(Module(), 4) is result and scored(Module(), 4) is result
    assert calls == [{"batch": 250}, {"batch": 250, "prdc_k": 3}]
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "epoch 4 FID: 1.0000 KID mean: 2.000000 KID stddev: 0.500000"
    assert lines[1] == lines[0] + " P: 0.5000 R: 0.2500 D: 1.5000 C: 0.7500"


def test_header_declares_the_entry_points_and_they_check_their_arguments():
    from lightning_gan_zoo_amd._lib import lib, parse_header
    protos = parse_header()
    ptr, i32, i64, size = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
    assert protos["gz_knn_radii_workspace_bytes"] == (size, [i64, i32, i32])
    assert protos["gz_knn_radii"] == (i32, [ptr, i64, i32, i32, ptr, ptr, size, ptr])
    assert protos["gz_prdc_counts_workspace_bytes"] == (size, [i64, i64, i32])
    assert protos["gz_prdc_counts"] == (i32, [ptr, i64, ptr, ptr, i64, ptr, i32, ptr, ptr, ptr, ptr, ptr, size, ptr])
    assert protos["gz_prdc_plan"] == (i32, [i64, i64, ptr, ptr])
    BAD, WORKSPACE, TOO_LARGE = -1, -3, -5
    p = [ctypes.c_void_p(0x10000 + 0x1000 * i) for i in range(9)]      # never dereferenced: every call is refused

    def radii(codes=p[0], n=20, d=4, k=5, out=p[1], ws=p[2], nbytes=1 << 62):
        return lib.gz_knn_radii(codes, n, d, k, out, ws, nbytes, None)

    for bad in (dict(k=0), dict(k=-1), dict(k=9), dict(k=5, n=5), dict(k=5, n=4), dict(d=0), dict(n=0), dict(codes=None),
                dict(out=None), dict(ws=None)):
        assert radii(**bad) == BAD, bad
    need = lib.gz_knn_radii_workspace_bytes(20, 4, 5)
    assert need >= 8 * (20 + 20 * 5) and need % 8 == 0
    assert radii(nbytes=need - 1) == WORKSPACE and radii(nbytes=0) == WORKSPACE
    assert radii(n=1 << 50, d=1 << 20) == TOO_LARGE                     # no such array
    assert radii(n=1 << 40, d=1) == TOO_LARGE                           # 2^38 workgroups of the norms' pre-pass
    q = lib.gz_knn_radii_workspace_bytes
    assert q(20, 4, 0) == 0 and q(20, 4, 9) == 0 and q(5, 4, 5) == 0 and q(20, 0, 5) == 0 and q(1 << 50, 1 << 20, 5) == 0

    def counts(g=p[0], n_g=20, rad_g=p[1], r=p[2], n_r=30, rad_r=p[3], d=4, in_real=p[4], in_fake=p[5], near=p[6],
               totals=p[7], ws=p[8], nbytes=1 << 62):
        return lib.gz_prdc_counts(g, n_g, rad_g, r, n_r, rad_r, d, in_real, in_fake, near, totals, ws, nbytes, None)

    for bad in (dict(n_g=0), dict(n_r=0), dict(n_r=-3), dict(d=0), dict(g=None), dict(rad_g=None), dict(r=None),
                dict(rad_r=None), dict(in_real=None), dict(in_fake=None), dict(near=None), dict(totals=None),
                dict(ws=None)):
        assert counts(**bad) == BAD, bad
    need = lib.gz_prdc_counts_workspace_bytes(20, 30, 4)
    assert need >= 8 * (20 + 30) + 12 * 30 + 4 * 20 and need % 8 == 0
    assert counts(nbytes=need - 1) == WORKSPACE
    assert counts(n_g=1 << 50, d=1 << 20) == TOO_LARGE
    q = lib.gz_prdc_counts_workspace_bytes
    assert q(0, 30, 4) == 0 and q(20, 0, 4) == 0 and q(20, 30, 0) == 0
    # partials per row group and per column slice, never per block of 64 rows: 50 000 rows a side stay below 100 MB
    assert 0 < q(50000, 50000, 2048) < 100 << 20


def _plan(n_rows, n_cols):
    from lightning_gan_zoo_amd._lib import lib
    groups, slices = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.gz_prdc_plan(n_rows, n_cols, ctypes.byref(groups), ctypes.byref(slices)) == 0
    return groups.value, slices.value


def test_the_plan_depends_on_the_shapes_and_the_cu_budget_alone():
    from lightning_gan_zoo_amd._lib import lib
    budget = lib.gz_get_cu_budget()
    try:
        assert lib.gz_set_cu_budget(256) == 256
        assert _plan(65, 63) == (2, 1) and _plan(64, 64) == (1, 1) and _plan(130, 200) == (3, 4)
        assert _plan(*SLICED_CASE[:2]) == SLICED_PLAN_FULL
        assert _plan(5000, 5000) == (79, 6)
        groups, slices = _plan(50000, 50000)            # 782 row tiles in groups of 7, the last one shorter
        assert (groups, slices) == (112, 4) and groups * slices <= 2 * 256       # one round of two per CU
        assert lib.gz_set_cu_budget(REDUCED_BUDGET) == REDUCED_BUDGET
        assert _plan(*SLICED_CASE[:2]) == SLICED_PLAN_REDUCED
        assert _plan(130, 200) == (3, 4)                # (one slice per column tile at most)
        assert _plan(50000, 50000) == (112, 1)
        assert lib.gz_prdc_plan(0, 5, None, None) == -1 and lib.gz_prdc_plan(5, 5, None, None) == -1
    finally:
        lib.gz_set_cu_budget(budget)


@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_inputs_leave_no_decision_near_its_threshold_and_every_metric_interior(case):
    """The device may legitimately differ from the yardstick only where a distance lies within the two bounds of the
    radius it is compared with.  No decision of any case lies within 1000 times that, so the set of decisions the device
    may flip is empty and the GPU tests demand equal integers.  Smallest margins, in bounds: 1.0e10, 7.5e9, 6.4e8, 9.6e8,
    6.8e6 (d = 2048) and 2.0e7 (the sliced case)."""
    h = host(case)
    for key in METRICS:
        assert 0.0 < h[key] < 1.0, (key, h[key])
    assert h["in_real"].max() > 1 and h["in_fake"].max() > 1
    margin = smallest_margin(case)
    print(case, {key: round(h[key], 4) for key in METRICS}, "smallest margin %.3g bounds" % margin)
    assert margin > MARGIN


def test_the_exact_and_duplicate_inputs_are_what_they_claim():
    g, r = exact_inputs()
    assert np.array_equal(g, np.round(g)) and np.array_equal(r, np.round(r))
    assert np.abs(g).max() == 1 and r.min() == -1 and r.max() == 2
    h = host(EXACT_CASE)
    # ties: far fewer distinct values than rows, and radii that cross distances hit exactly
    assert len(np.unique(h["rad_r"])) < len(h["rad_r"]) // 2
    cross = ((g[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)
    assert (cross == h["rad_r"][None, :]).sum() > 50 and (cross == h["rad_g"][:, None]).sum() > 50
    assert 0 < h["precision"] < 1 and 0 < h["recall"] < 1 and 0 < h["coverage"] < 1
    x = duplicate_inputs()
    assert np.array_equal(x[5], x[68]) and len(np.unique(x, axis=0)) == len(x) - 1
    assert inputs(ALL_CASES[0])[0].flags.writeable is False

"""Shared by tests/test_kid_cpu.py, tests/test_kid_gpu.py and tests/test_f64_tile_parent_bits_gpu.py: the fixture
construction, numpy's version of the kernel's output and the forward error bounds of the sums."""
import numpy as np

U = 2.0 ** -53
N_G, N_R = 400, 360
_codes = {}


def activations(seed, n, d, shift):          # same construction as tests/golden/make_eval_golden.py
    rng = np.random.RandomState(seed)
    basis = rng.randn(d, d) / np.sqrt(d)
    return rng.randn(n, d).dot(basis) + shift * rng.rand(d)


def mixed_sign_codes(d):
    if d not in _codes:
        rng = np.random.RandomState(1000 + d)
        _codes[d] = (rng.randn(N_G, d) * 1.5 + 0.2, rng.randn(N_R, d) - 0.1)
    return _codes[d]


def subset_rows(m, S, seed):
    """[S, 2, m] rows without repetition inside a subset; every subset holds rows 0 and n-1 of both sets (so row 0 is
    shared by any two subsets)."""
    rng = np.random.RandomState(seed)
    idx = np.empty((S, 2, m), dtype=np.int32)
    for s in range(S):
        for slot, n in ((0, N_G), (1, N_R)):
            rows = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)])[:m]
            idx[s, slot] = rng.permutation(rows)
    return idx


def host_rows(n_g, n_r, n_subsets, subset_size):
    """What ``polynomial_mmd_averages``'s loop draws (its lines, without the arithmetic)."""
    subset_size = min(n_g, n_r, subset_size)
    return np.array([[np.random.choice(n_g, subset_size, replace=False),
                      np.random.choice(n_r, subset_size, replace=False)] for _ in range(n_subsets)])


def numpy_sums(g, r, degree=3, gamma=None, coef0=1):
    """The 6m+3 numbers of include/gz_ops.h (gz_kid_sums) from numpy's own kernel matrices."""
    from lightning_gan_zoo_amd import eval as E
    kgg, krr, kgr = (E._poly_kernel(a, b, degree, gamma, coef0) for a, b in ((g, g), (r, r), (g, r)))
    return np.concatenate([kgg.sum(axis=1), np.diagonal(kgg), krr.sum(axis=1), np.diagonal(krr), kgr.sum(axis=1),
                           kgr.sum(axis=0), [E._sq(kgg), E._sq(krr), E._sq(kgr)]])


def _entry_bounds(x, y, degree, gamma, coef0):
    """(|K|, e_K) per entry of (gamma x y^T + coef0)^degree: first-order forward bound of any fp64 evaluation."""
    d = x.shape[1]
    a = np.abs(x).dot(np.abs(y).T)
    s = x.dot(y.T)
    t = gamma * s + coef0
    e_t = gamma * (d + 1) * U * a + 2 * U * (gamma * np.abs(s) + abs(coef0))
    p = degree
    e_k = p * (np.abs(t) + e_t) ** (p - 1) * e_t + (p - 1) * U * (np.abs(t) + e_t) ** p
    return np.abs(t ** p), e_k


def _sum_bound(k_abs, e_k, axis):
    n = k_abs.size if axis is None else k_abs.shape[axis]
    return e_k.sum(axis=axis) + (n - 1) * U * (k_abs + e_k).sum(axis=axis)


def sums_bounds(g, r, degree=3, gamma=None, coef0=1):
    """Bound of every one of the 6m+3 sums, in the order of ``numpy_sums``: a sum of n entries carries
    sum e_K + (n-1) u sum(|K| + e_K); an entry of a Frobenius sum carries 2|K| e_K + e_K^2 + u K^2 first."""
    if gamma is None:
        gamma = 1.0 / g.shape[1]
    parts, frob = [], []
    for (x, y), kinds in (((g, g), ("row", "diag")), ((r, r), ("row", "diag")), ((g, r), ("row", "col"))):
        k_abs, e_k = _entry_bounds(x, y, degree, gamma, coef0)
        for kind in kinds:
            if kind == "diag":
                parts.append(np.diagonal(e_k))
            else:
                parts.append(_sum_bound(k_abs, e_k, 1 if kind == "row" else 0))
        e_sq = 2 * k_abs * e_k + e_k ** 2 + U * k_abs ** 2
        frob.append(_sum_bound(k_abs ** 2, e_sq, None))
    return np.concatenate(parts + [frob])

"""Shared by tests/test_fid_device_cpu.py and tests/test_fid_device_gpu.py: the input sets of the device Frechet distance
(eval.frechet_distance_device, csrc/gz_sqrtm.hip), their tolerances and the forward bounds of its two kernels.

Input sets (n1, n2, d, kind), made with make_eval_golden.py's ``activations(seed, n, d, shift)`` (seed 1, shift 0 for the
first set; seed 2, shift 0.3 for the second, the golden file's own):
  kind 0  plain;
  kind 1  abs(x) * exp(-j / (d / 12)): non-negative features whose scale falls by e^12 over the columns;
  kind 2  relu(x - 0.5) * exp(-j / (d / 6)) with every 7th column zero: ReLU-like features with dead columns;
  kind 3  x + 100: every column four hundred standard deviations from zero.

Tolerances, in units of tr S1 + tr S2, against scipy's ``Tr sqrtm(S1 S2)`` (eval.frechet_distance):
  * FULL_RANK sets (n > d on both sides, no dead column): 1e-9, the bar tests/test_moments_gpu.py holds the Frechet
    distance to;
  * RANK_DEFICIENT sets: 1e-7 = ten times sqrt(u), the size of a square root's response to the rounding of a zero
    eigenvalue (scipy itself lies up to 6.3e-9 from a symmetric-eigenvalue evaluation of the same trace on these sets).

Forward bounds, first order in u = 2^-53, valid for ANY order of summation, fused or unfused:
  * product C = alpha (A B) + beta I: d products, d - 1 additions, the scaling and the addition of beta:
        |C^_ij - C_ij| <= (d + 2) u |alpha| sum_k |a_ik| |b_kj| + u |beta| [i == j];
  * trace: d - 1 additions: (d - 1) u sum_i |a_ii|;  squared norm: d^2 products and d^2 - 1 additions of non-negative
    terms: d^2 u sum a_ij^2.
numpy and the kernel both lie within one bound of the exact value, so the tests allow 2 x bound.
"""
import numpy as np

U = 2.0 ** -53
FULL_RANK = [(400, 360, 48, 0), (400, 400, 48, 0), (9, 7, 1, 3), (300, 280, 130, 1), (500, 450, 200, 3)]
RANK_DEFICIENT = [(3, 3, 5, 0), (40, 2, 17, 0), (30, 25, 48, 0), (200, 190, 65, 2), (100, 90, 130, 2), (64, 64, 200, 1),
                  (20, 300, 200, 1)]
SETS = FULL_RANK + RANK_DEFICIENT
GOLDEN_SET, SAME_SET = FULL_RANK[0], FULL_RANK[1]
REAL_SIZE = (2100, 2100, 2048, 2)                # the size of real Inception statistics, once
TOL_FULL, TOL_DEFICIENT = 1e-9, 1e-7

PRODUCT_DIMS = (1, 5, 17, 48, 65, 130, 200)
PRODUCT_COEFFS = ((1.0, 0.0), (-0.5, 1.5))


def activations(seed, n, d, shift):          # same construction as tests/test_eval.py / make_eval_golden.py
    rng = np.random.RandomState(seed)
    basis = rng.randn(d, d) / np.sqrt(d)
    return rng.randn(n, d).dot(basis) + shift * rng.rand(d)


def shaped(x, kind):
    d = x.shape[1]
    j = np.arange(d)
    if kind == 0:
        return x
    if kind == 1:
        return np.abs(x) * np.exp(-j / (d / 12.0))
    if kind == 2:
        y = np.maximum(x - 0.5, 0.0) * np.exp(-j / (d / 6.0))
        y[:, ::7] = 0.0
        return y
    if kind == 3:
        return x + 100.0
    raise ValueError(kind)


def input_set(case):
    """-> (first activations [n1, d], second activations [n2, d]); SAME_SET has one set on both sides."""
    n1, n2, d, kind = case
    first = shaped(activations(1, n1, d, 0.0), kind)
    if case == SAME_SET:
        return first, first.copy()
    return first, shaped(activations(2, n2, d, 0.3), kind)


_cache = {}


def statistics(case):
    """(mu1, sigma1, mu2, sigma2) of a set, numpy's; made once and shared (read-only)."""
    if case not in _cache:
        a, b = input_set(case)
        out = (np.mean(a, axis=0), np.atleast_2d(np.cov(a, rowvar=False)),
               np.mean(b, axis=0), np.atleast_2d(np.cov(b, rowvar=False)))
        for v in out:
            v.setflags(write=False)
        _cache[case] = out
    return _cache[case]


_host = {}


def host_fid(case):
    """eval.frechet_distance (scipy's sqrtm) of a set, once."""
    if case not in _host:
        from lightning_gan_zoo_amd import eval as E
        _host[case] = E.frechet_distance(*statistics(case))
    return _host[case]


def tolerance(case):
    _, s1, _, s2 = statistics(case)
    return (TOL_FULL if case in FULL_RANK else TOL_DEFICIENT) * float(np.trace(s1) + np.trace(s2))


def product_operands(d):
    """Non-symmetric, mixed-sign d x d operands."""
    rng = np.random.RandomState(9000 + d)
    return rng.randn(d, d) * (1.0 + rng.rand(d)), rng.randn(d, d) - 0.25


def product_bound(a, b, alpha, beta):
    d = a.shape[0]
    return (d + 2) * U * abs(alpha) * np.abs(a).dot(np.abs(b)) + U * abs(beta) * np.eye(d)


def exact_operands(d=70):
    """Integers in [-8, 8]: every product, every partial sum (below 2^13) and the halves of alpha = -0.5 are exact in
    fp64 whatever the order, so the kernel must reproduce numpy's bits."""
    rng = np.random.RandomState(7000 + d)
    return (rng.randint(-8, 9, size=(d, d)).astype(np.float64), rng.randint(-8, 9, size=(d, d)).astype(np.float64))


def trace_norm_bounds(a):
    d = a.shape[0]
    return (d - 1) * U * float(np.abs(np.diagonal(a)).sum()), d * d * U * float((a * a).sum())

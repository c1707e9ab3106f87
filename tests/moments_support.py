"""Shared by tests/test_moments_gpu.py and tests/test_eval_device_cpu.py: the fixtures of the device moments
(gz_feature_moments, csrc/gz_moments.hip) and the forward error bounds of a two-pass mean / covariance.

The bounds are first order in u = 2^-53 and hold for ANY order of fp64 summation, fused or unfused products, so numpy
and the kernel both lie within one bound of the exact value.  With x [n, d], mu the exact column means, c = x - mu:

* mean.  n - 1 additions and one division: |mean^ - mu_j| <= e_m[j] = u * sum_k |x_kj|    (= n u mean|x_j|).
* centred values.  c^_kj = (x_kj - mean^_j)(1 + delta) = (c_kj - eps_j)(1 + delta), |eps_j| <= e_m[j], |delta| <= u.
* products.  sum_k c^_ki c^_kj = S_ij - eps_j sum_k c_ki - eps_i sum_k c_kj + n eps_i eps_j + roundings.  The exact
  centred columns sum to zero, so the mean's error enters through n eps_i eps_j only (this is why the two-pass form is
  the one to use); the roundings are the two subtractions (2u), the product and the n - 1 additions (n u) on terms of
  magnitude at most (|c_ki| + e_m[i]) (|c_kj| + e_m[j]):
      e_S[i, j] = n e_m[i] e_m[j] + (n + 2) u sum_k (|c_ki| + e_m[i]) (|c_kj| + e_m[j]).
* scaling.  1 / (n - 1) is rounded once and the product once: e_cov = r e_S + 2 u r (|S| + e_S), r = 1 / (n - 1).
"""
import numpy as np

U = 2.0 ** -53
SHAPES = [(2, 1), (5, 3), (33, 17), (67, 70), (130, 129), (300, 200)]          # (n, d)
OFFSET = 100.0


def activations(seed, n, d, shift):          # same construction as tests/test_eval.py / make_eval_golden.py
    rng = np.random.RandomState(seed)
    basis = rng.randn(d, d) / np.sqrt(d)
    return rng.randn(n, d).dot(basis) + shift * rng.rand(d)


def offset_activations(n, d):
    """The bound test's input: every column sits at ~100, four hundred standard deviations from zero, so a one-pass
    E[xy] - E[x]E[y] would lose five digits and the centring is what is being tested."""
    return activations(1000 + 7 * n + d, n, d, 0.3) + OFFSET


def exact_case():
    """n = 64, d = 70, integers in [-8, 8]: the column sums are integers, the means multiples of 1/64, the centred
    values multiples of 1/64 below 2^5, their products multiples of 2^-12 below 2^10 and every partial sum below 2^16:
    all exact in fp64 whatever the order, so the kernel must reproduce numpy's bits."""
    return np.random.RandomState(64070).randint(-8, 9, size=(64, 70)).astype(np.float64)


def long_double_moments(x):
    """Mean and covariance in numpy's extended precision (64-bit mantissa on x86): the 'exact' value of the CPU check."""
    xl = np.asarray(x, dtype=np.longdouble)
    n = xl.shape[0]
    mu = xl.sum(axis=0) / np.longdouble(n)
    c = xl - mu
    cov = np.zeros((xl.shape[1], xl.shape[1]), dtype=np.longdouble)
    for k in range(n):                       # (np.dot has no long-double BLAS; outer products keep the precision)
        cov += np.outer(c[k], c[k])
    return mu, cov / np.longdouble(n - 1)


def moments_bounds(x):
    """(e_mean [d], e_cov [d, d]) of the module docstring for the fp64 array x [n, d]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mu = x.mean(axis=0)
    e_m = U * np.abs(x).sum(axis=0)
    c = np.abs(x - mu) + e_m                 # |c_kj| + e_m[j]  (mu's own error is second order here)
    s_abs = c.T.dot(c)
    e_s = n * np.outer(e_m, e_m) + (n + 2) * U * s_abs
    r = 1.0 / (n - 1)
    s = np.abs((x - mu).T.dot(x - mu))
    return e_m, r * e_s + 2 * U * r * (s + e_s)

"""Shared by tests/test_inception_score_cpu.py and tests/test_inception_score_gpu.py: the cases of the device Inception
Score (gz_classifier_logits, gz_inception_score; csrc/gz_inception_score.hip) and the forward error bounds the device is
held to against the host yardstick (eval.inception_score_from_logits on numpy's logits).

The bounds are first order in u = 2^-53, hold for any order of fp64 summation, and are derived, not tuned:

* logits.  l_ic = sum_k codes_ik weight_ck + bias_c is d products, d - 1 additions and the bias addition:
      |l^_ic - l_ic| <= delta_ic = (d + 2) u (|codes| |weight|^T + |bias|)_ic
  for the device and for numpy alike, so the two differ by at most 2 delta_ic.
* split score.  A perturbation of every logit of a split by at most eps moves log p_ic by at most 2 eps (eps in the
  logit, eps in the log of the partition sum) and log py_c, a mean of such p, by at most 2 eps; so log(p_ic / py_c) moves
  by at most 4 eps and the weights p_ic by a factor within exp(+-2 eps).  The mean KL divergence is
  mean_i sum_c p_ic log(p_ic / py_c) with sum_c p_ic |log(p_ic / py_c)| <= 2 ln classes <= 16 for classes < 2981: moving
  the weights costs at most 2 eps * 16, moving the logarithms 4 eps -- below 64 eps in all.  With eps = 2 max delta the
  logarithm of a split score moves by at most 128 max delta, and so does the score, relatively.  The evaluation of the
  formula itself (a row's classes sums, the split's n // splits rows, exp and log within a few u each) adds
  (classes + n // splits + 64) 2^-52:
      |score^ - score| / score <= 128 max delta + (classes + n // splits + 64) 2^-52.
"""
import numpy as np

U = 2.0 ** -53

# (n, d, classes, splits): the smallest shapes on which each tail can go wrong
CASES = [(64, 32, 64, 1),          # no tails
         (130, 70, 67, 2),         # every tail: rows, classes, reduction index
         (257, 100, 130, 3),       # two trailing rows dropped
         (96, 33, 1008, 1),
         (200, 40, 5, 10),         # classes below 16
         (65, 2048, 1008, 5),      # the real d and classes
         (7, 5, 3, 7)]             # one row per split: every score exactly 1.0
TRAILING_CASE = (257, 100, 130, 3)
ONE_ROW_CASE = (7, 5, 3, 7)
# the weights' standard deviation per case: logits with a spread of a few units, scores well away from 1
SCALE = {(64, 32, 64, 1): 0.5, (130, 70, 67, 2): 0.3, (257, 100, 130, 3): 0.25, (96, 33, 1008, 1): 0.5,
         (200, 40, 5, 10): 1.0, (65, 2048, 1008, 5): 0.05, (7, 5, 3, 7): 1.0}

_made = {}


def inputs(case):
    """(codes [n, d], weight [classes, d], bias [classes]) of a case: codes non-negative like pool features.  Made once
    per process and shared; read-only."""
    if case not in _made:
        n, d, classes, _ = case
        rng = np.random.RandomState(1000 * n + 10 * d + classes)
        codes = np.abs(rng.randn(n, d)) * rng.rand(n, 1) * 2
        weight = rng.randn(classes, d) * SCALE[case]
        bias = 0.1 * rng.randn(classes)
        for a in (codes, weight, bias):
            a.setflags(write=False)
        _made[case] = (codes, weight, bias)
    return _made[case]


def host_logits(codes, weight, bias=None):
    out = codes.dot(weight.T)
    return out if bias is None else out + bias


def logit_delta(codes, weight, bias=None):
    """delta [n, classes] of the module docstring."""
    mag = np.abs(codes).dot(np.abs(weight).T)
    if bias is not None:
        mag = mag + np.abs(bias)
    return (codes.shape[1] + 2) * U * mag


def score_bound(max_delta, classes, rows_per_split):
    """The relative bound on a split score of the module docstring."""
    return 128.0 * max_delta + (classes + rows_per_split + 64) * 2.0 ** -52


def exact_inputs():
    """n = 70, d = 45, classes = 66 (every tail), integers in [-8, 8]: products below 2^6, every partial sum below 2^12,
    all exact in fp64 whatever the order, so the kernel must reproduce numpy's bits."""
    rng = np.random.RandomState(704566)
    return (rng.randint(-8, 9, size=(70, 45)).astype(np.float64), rng.randint(-8, 9, size=(66, 45)).astype(np.float64),
            rng.randint(-8, 9, size=(66,)).astype(np.float64))


EXTREME_SPLITS = 2


def extreme_logits():
    """[130, 67] logits of a few units with a fifth of the entries replaced by exactly +800 or -800: a row that holds
    j entries of +800 is the uniform distribution over them, every other entry of it underflows to p = 0 (exp(-795) is
    below the smallest denormal); a row that holds none is an ordinary softmax with some classes at p = 0."""
    rng = np.random.RandomState(800)
    logits = rng.randn(130, 67) * 2
    pick = rng.rand(130, 67)
    logits[pick < 0.1] = -800.0
    logits[pick > 0.97] = 800.0
    return logits


def long_double_scores(logits, splits):
    """The split scores by the same formula in numpy's extended precision (64-bit mantissa on x86), classes with p = 0
    contributing 0: the 'exact' value of the CPU check."""
    l = np.asarray(logits, dtype=np.longdouble)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    m = l.shape[0] // splits
    out = []
    for k in range(splits):
        part = p[k * m:(k + 1) * m]
        py = part.sum(axis=0) / np.longdouble(m)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = np.where(part > 0, part * (np.log(part) - np.log(py)), np.longdouble(0))
        out.append(np.exp(terms.sum() / np.longdouble(m)))
    return np.asarray(out, dtype=np.longdouble)

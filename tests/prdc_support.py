"""Shared by tests/test_prdc_cpu.py and tests/test_prdc_gpu.py: the cases, their seeded inputs, the host yardstick's
results (computed once per process, read-only) and the error bound of a device distance.

The device takes squared distances in the Gram form, D = max(0, s_i + s_j - 2 <x_i, x_j>), the yardstick from direct
differences.  With u = 2^-53 and gamma_m = m u / (1 - m u),

    |D_dev - D_host| <= 2 gamma_{d+3} (s_i + s_j) + gamma_{d+2} D_host

The first term: s_i, s_j and the dot product are sums of d products in some order, each within gamma_d of its exact value,
|<x_i, x_j>| <= (s_i + s_j) / 2, and three more roundings combine them (the clamp at 0 only moves a value towards the
exact one, which is >= 0).  The second term is the yardstick's own error: d subtractions, squares and additions.  A k-th
smallest value or a minimum over j is monotone in every D_ij, so it inherits the bound with the row's largest s_i + s_j
in the first term and its own host value in the second.
"""
import functools

import numpy as np

U = 2.0 ** -53
MARGIN = 1000.0           # no decision of a case may lie within MARGIN bounds of its threshold

# (n_g, n_r, d, k)
CASES = [(65, 63, 33, 1),           # one row past a tile, one short of a tile, d one past a chunk, k = 1
         (64, 64, 32, 5),           # exact tiles
         (130, 200, 40, 3),
         (257, 129, 70, 8),         # k at its cap
         (200, 130, 2048, 5)]       # the real d, low intrinsic dimension
# gz_prdc_plan: 129 row tiles in 65 groups of two (the last of one), so that a workgroup adds a second row tile to the
# column-wise partials it wrote, and 3 column slices at the full CU budget, one column slice at a budget of 64 CUs (where
# gz_knn_radii of the generated set, on the plan of (n_g, n_g), takes one slice instead of seven); d is small so that the
# yardstick stays quick
SLICED_CASE = (8200, 150, 4, 3)
SLICED_PLAN_FULL, SLICED_PLAN_REDUCED, REDUCED_BUDGET = (65, 3), (65, 1), 64
ALL_CASES = CASES + [SLICED_CASE]
EXACT_CASE = (130, 100, 33, 3)      # small-integer codes: every distance is exact in fp64 on either side
SEEDS = {(65, 63, 33, 1): 1, (64, 64, 32, 5): 2, (130, 200, 40, 3): 3, (257, 129, 70, 8): 4, (200, 130, 2048, 5): 5,
         SLICED_CASE: 6}


def gamma(m):
    return m * U / (1.0 - m * U)


def dist_bound(d, s_sum, d_host):
    return 2.0 * gamma(d + 3) * s_sum + gamma(d + 2) * d_host


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(codes_g, codes_r): both sets are a mixture of a cluster they share and a cluster of their own in a latent space of
    at most 4 dimensions, mixed into d features, plus small full-rank noise -- so that some generated rows lie off the
    real manifold (precision < 1), some real rows are not reached (recall, coverage < 1) and most of either are."""
    n_g, n_r, d, _ = case
    rng = np.random.RandomState(SEEDS[case])
    q = min(d, 4)
    mix = rng.randn(q, d) / np.sqrt(q)

    def draw(n, own):
        z = rng.randn(n, q)
        away = rng.rand(n) < 0.3
        z[away] = 0.6 * z[away] + own
        return z.dot(mix) + 0.01 * rng.randn(n, d)

    shift = np.zeros(q)
    shift[0] = 4.0
    return _frozen(draw(n_g, shift)), _frozen(draw(n_r, -shift))


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """Integers in -1 .. 2 (every third real row is shifted by one): d * 9 is far below 2^53, so sums of products and
    direct differences are both exact; the distances take few distinct values, so radii and counts sit on exact ties."""
    n_g, n_r, d, _ = EXACT_CASE
    rng = np.random.RandomState(11)
    g = rng.randint(-1, 2, (n_g, d)).astype(np.float64)
    r = rng.randint(-1, 2, (n_r, d)).astype(np.float64)
    r[::3] += 1.0
    return _frozen(g), _frozen(r)


@functools.lru_cache(maxsize=None)
def duplicate_inputs():
    """[70, 40] codes whose rows 5 and 68 (two tiles) are one row, scaled so that the Gram form cancels ~1e3 to 0."""
    rng = np.random.RandomState(12)
    x = 3.0 + rng.randn(70, 40)
    x[68] = x[5]
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def host(case):
    """eval.prdc of a case's inputs (the exact case included), arrays read-only."""
    from lightning_gan_zoo_amd import eval as E
    g, r = exact_inputs() if case == EXACT_CASE else inputs(case)
    out = E.prdc(g, r, k=case[3])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def sqnorms(x):
    return (x * x).sum(axis=1)


def radii_bound(codes, rad_host):
    """Per row: the bound a device radius inherits."""
    s = sqnorms(codes)
    return dist_bound(codes.shape[1], s + s.max(), rad_host)


def near_bound(codes_g, codes_r, near_host):
    return dist_bound(codes_g.shape[1], sqnorms(codes_r) + sqnorms(codes_g).max(), near_host)


def smallest_margin(case):
    """The smallest |value - threshold| / (bound of the value + bound of the threshold) over every decision of a case:
    D(G_j, R_i) against rad_r[i] and against rad_g[j], near[i] against rad_r[i]."""
    g, r = inputs(case)
    h = host(case)
    d = g.shape[1]
    sg, sr = sqnorms(g), sqnorms(r)
    bg, br = radii_bound(g, h["rad_g"]), radii_bound(r, h["rad_r"])
    worst = np.inf
    step = max(1, (1 << 21) // (r.shape[0] * d))
    for a in range(0, g.shape[0], step):
        dist = ((g[a:a + step, None, :] - r[None, :, :]) ** 2).sum(axis=2)
        b = dist_bound(d, sg[a:a + step, None] + sr[None, :], dist)
        worst = min(worst, (np.abs(dist - h["rad_r"][None, :]) / (b + br[None, :])).min(),
                    (np.abs(dist - h["rad_g"][a:a + step, None]) / (b + bg[a:a + step, None])).min())
    nb = near_bound(g, r, h["near"])
    return min(worst, (np.abs(h["near"] - h["rad_r"]) / (nb + br)).min())

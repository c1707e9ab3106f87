"""Shared by tests/test_swd_cpu.py and tests/test_swd_gpu.py: the cases, their seeded inputs and draws, the numpy yardstick's
results (computed once per process, read-only) and the error bounds of the device kernels (csrc/gz_swd.hip), all in fp64.

u = 2^-24 is fp32's unit roundoff and gamma_k = k u / (1 - k u).

Pyramid.  Every stage of the device is one 5-tap sum s = sum_t w_t x_t, w_t > 0, as ONE chain of fused multiply-adds from
0 with t ascending (csrc/gz_swd.hip says so).  The first link, 2^-4 x_0 + 0, is exact; a down stage therefore rounds k = 4
times.  An up stage filters a zero-inserted signal: the links of the inserted zeros add nothing, exactly, which leaves three
samples (the first exact again) at an even position and two at an odd one: k = 2.  So |fl(s) - s| <= gamma_k sum_t w_t |x_t|.
An input that already carries an error |e| <= E adds the same taps applied to E, and its own rounding acts on |x| + E:

    E_out = taps(E_in) + gamma_k taps(|x| + E_in)                       (``_stage``; zero-inserted samples carry 0)

and a level L = G - up(G') adds one rounding: E_L = E_G + E_up + u (|G| + |up| + E_G + E_up).  ``bounds_of`` runs this
recurrence beside the fp64 pyramid, so the bound is composed over the levels exactly as the values are.

Projection.  The device normalises in fp32, x^ = fl(fl(d - fl(m)) fl(1 / s)): fl(m) = m (1 + d0), three more roundings,
so |x^ - x| <= gamma_3 |x| + (1 + gamma_3) u |m| / s =: e_x.  The order of the dot product is stated in include/gz_ops.h:
the 7 products of a patch row (c, dy) in one chain of fused multiply-adds from 0, then the 7 C chain results added to one
total in order.  A product passes at most 7 roundings inside its chain and at most 7 C - 1 additions after it, so with
K = 7 + 7 C (28 for C = 3, not D = 147): |p^ - sum_k x^_k w_k| <= gamma_K sum_k |x^_k| |w_k|.  Hence

    |p^ - p| <= sum_k e_xk |w_k| + gamma_K sum_k (|x_k| + e_xk) |w_k| + gamma64_D sum_k |x_k| |w_k|

the last term being the yardstick's own fp64 dot product (``projection_bound``).

End to end the device's levels carry the pyramid's error E (``bounds_of``, elementwise, gathered at the patch positions: e_d
per descriptor value) and its statistics come from fp64 sums of N = rows * 49 < 2^13 shifted values v - v0 per channel
(relative error of each sum at most N 2^-53 <= 2^-40; the variance s2 / N - (s1 / N)^2 then errs by at most 3 * 2^-40
max|v - v0|^2 and the deviation by half of that over s: with max|v - v0| / s below 2^5 that is under 2^-34 max|v - v0|;
SLACK = 2^-30 max|v - v0| covers mean and deviation).  Values perturbed by e_d move the channel mean by at most
e_m = mean(e_d) + SLACK and the population deviation by at most e_s = rms(e_d) + SLACK (|std(v + e) - std(v)| <= std(e)
<= rms(e)), so with rho = e_s / s

    |x' - x| <= ((e_d + e_m) / s + |x| rho) / (1 - rho) =: dx

and the fp32 terms above act on |x| + dx, with |m| + e_m and s - e_s in e_x.  A sorted sequence moves by at most the
largest change of any of its keys (the k-th smallest of a set is monotone in every key and moves by at most their largest
change), so the mean of |a_sorted - b_sorted| moves by at most the sum of both sets' worst projection errors:
``end_to_end_bound``.
"""
import functools

import numpy as np

from lightning_gan_zoo_amd import eval as E

U = 2.0 ** -24
U64 = 2.0 ** -53

# (N, C, S)
PYRAMID_CASES = [(1, 1, 16), (3, 3, 32), (2, 3, 64), (2, 1, 128)]
# (n, C, H, P, ndirs): row counts around the projection's 128-row tile, 1, 5 and 128 directions (and one past a chunk of 128)
PROJECT_CASES = [(2, 1, 16, 5, 1), (3, 3, 16, 43, 5), (2, 3, 32, 64, 128), (5, 1, 32, 77, 130)]
# (n, C, S, P, dirs, repeats)
END_TO_END_CASES = [(8, 3, 32, 16, 8, 2), (8, 3, 64, 16, 8, 2)]


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ternary_images(case):
    n, c, s = case
    return _frozen(np.random.RandomState(100 + s).randint(-1, 2, (n, c, s, s)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def random_images(case):
    n, c, s = case
    return _frozen(np.random.RandomState(200 + s).randn(n, c, s, s).astype(np.float32))


@functools.lru_cache(maxsize=None)
def host_pyramid(kind, case):
    images = ternary_images(case) if kind == "ternary" else random_images(case)
    return tuple(_frozen(l) for l in E.laplacian_pyramid(images))


def _stage(x, err, axis, taps, k):
    return (E._swd_filter(x, axis, taps),
            E._swd_filter(err, axis, taps) + gamma(k) * E._swd_filter(np.abs(x) + err, axis, taps))


def _zero_insert(a, axis):
    shape = list(a.shape)
    shape[axis] *= 2
    out = np.zeros(shape)
    index = [slice(None)] * a.ndim
    index[axis] = slice(None, None, 2)
    out[tuple(index)] = a
    return out


def bounds_of(images):
    """Per level: the bound of |device - yardstick| for the fp32 device pyramid of fp32 ``images``, elementwise."""
    g, eg, bounds = np.asarray(images, dtype=np.float64), np.zeros(images.shape), []
    for _ in E.swd_level_sizes(images.shape[2])[:-1]:
        t, et = _stage(g, eg, -1, E.SWD_TAPS, 4)
        gn, en = _stage(t[..., ::2], et[..., ::2], -2, E.SWD_TAPS, 4)
        gn, en = gn[..., ::2, :], en[..., ::2, :]
        v, ev = _stage(_zero_insert(gn, -2), _zero_insert(en, -2), -2, 2.0 * E.SWD_TAPS, 2)
        up, eu = _stage(_zero_insert(v, -1), _zero_insert(ev, -1), -1, 2.0 * E.SWD_TAPS, 2)
        bounds.append(eg + eu + U * (np.abs(g) + np.abs(up) + eg + eu))
        g, eg = gn, en
    return bounds + [eg]


@functools.lru_cache(maxsize=None)
def pyramid_bounds(case):
    return tuple(_frozen(b) for b in bounds_of(random_images(case)))


def pyramid_fp32(images, reverse=False):
    """The pyramid with every operation rounded to fp32, taps summed in order t = 0 .. 4 or 4 .. 0 -> fp32 levels."""
    f = np.float32
    order = range(4, -1, -1) if reverse else range(5)

    def filt(x, axis, scale):
        n = x.shape[axis]
        out = np.zeros_like(x)
        for t in order:
            out = (out + f(scale * E.SWD_TAPS[t]) * np.take(x, E._swd_mirror(np.arange(n) + t - 2, n), axis=axis)).astype(f)
        return out

    g, levels = np.asarray(images, dtype=f), []
    for _ in E.swd_level_sizes(g.shape[2])[:-1]:
        gn = filt(filt(g, -1, 1.0)[..., ::2], -2, 1.0)[..., ::2, :]
        up = filt(_zero_insert(filt(_zero_insert(gn, -2).astype(f), -2, 2.0), -1).astype(f), -1, 2.0)
        levels.append((g - up).astype(f))
        g = gn
    return levels + [g]


# ---- projection ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def project_inputs(case):
    """(level fp32 [n, C, H, H], centres int32 [n, P, 2], directions fp32 [ndirs, 49 C]).  The first four patches of image 0
    sit in the four corners (centres 3 and H - 4 on either axis); with C = 3 the last channel is constant: its standard
    deviation is exactly 0 and the rule "divide by 1" applies; channel 0 is shifted off zero so that the mean matters."""
    n, c, h, p, ndirs = case
    rng = np.random.RandomState(300 + 7 * h + ndirs)
    level = rng.randn(n, c, h, h).astype(np.float32)
    level[:, 0] += np.float32(0.75)
    if c == 3:
        level[:, 2] = np.float32(0.3)
    pos = rng.randint(3, h - 3, (n, p, 2)).astype(np.int32)
    pos[0, :4] = [[3, 3], [3, h - 4], [h - 4, 3], [h - 4, h - 4]]
    d = rng.randn(ndirs, 49 * c)
    dirs = (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32)
    return _frozen(level), _frozen(pos), _frozen(dirs)


@functools.lru_cache(maxsize=None)
def host_projection(case):
    """(projections [rows, ndirs], their bound, (mean, std) per channel) of the yardstick, fp64."""
    level, pos, dirs = project_inputs(case)
    c = level.shape[1]
    desc = E.swd_descriptors(level, pos)
    mean, std = E.swd_channel_statistics(desc, c)
    x = E.swd_normalise(desc, c)
    return _frozen(x.dot(dirs.astype(np.float64).T)), _frozen(projection_bound(x, mean, std, dirs)), (mean, std)


def _per_element(per_channel, d):
    return np.repeat(np.asarray(per_channel, dtype=np.float64), d // len(per_channel))[None, :]


def projection_bound(x, mean, std, dirs, dx=None):
    """|device - yardstick| per projection [rows, ndirs] for normalised descriptors x (fp64) that the device knows up to
    ``dx`` (elementwise; None: exactly)."""
    d = x.shape[1]
    w = np.abs(np.asarray(dirs, dtype=np.float64)).T
    s = np.where(std == 0.0, 1.0, std)
    dx = np.zeros_like(x) if dx is None else dx
    xa = np.abs(x) + dx
    ex = gamma(3) * xa + (1.0 + gamma(3)) * U * _per_element(np.abs(mean) / s, d)
    return (dx + ex + gamma(7 + d // 7) * (xa + ex)).dot(w) + gamma(d, U64) * np.abs(x).dot(w)


# ---- end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def end_to_end_inputs(case):
    """(images_a, images_b, plan).  a is white noise: every projection of its patches is close to a standard normal.  b is
    low-rank at every level: per level above the coarsest a stripe pattern of that level's Nyquist width (along x and y in
    turn, scaled to unit deviation on its level) times one normal factor per image and channel, plus one normal offset per
    image and channel for the coarsest level -- its projections are normal factors times a direction-dependent scale, so
    the distance is 0.2 .. 0.5 (200 .. 500 in the result's unit) at every level, far above the error bound."""
    n, c, s, p, dirs, repeats = case
    rng = np.random.RandomState(400 + s)
    plan = E.SwdPlan(s, c, n, patches=p, dirs=dirs, repeats=repeats, seed=5)
    a = rng.randn(n, c, s, s).astype(np.float32)
    yy, xx = np.mgrid[0:s, 0:s]
    b = np.zeros((n, c, s, s))
    for l in range(len(plan.sizes) - 1):
        stripes = ((((xx if l % 2 == 0 else yy) >> l) & 1) * 2 - 1).astype(np.float64)
        own = E.laplacian_pyramid(stripes[None, None])[l].std()
        b = b + rng.randn(n, c, 1, 1) * stripes / own
    b = (b + rng.randn(n, c, 1, 1)).astype(np.float32)
    return _frozen(a), _frozen(b), plan


@functools.lru_cache(maxsize=None)
def host_end_to_end(case):
    a, b, plan = end_to_end_inputs(case)
    return E.swd(a, b, plan.positions, plan.directions, plan.repeats)


def _set_error(images, case, plan):
    """Per level: the worst projection error of one set, the device's pyramid and statistics errors included."""
    levels = E.laplacian_pyramid(images)
    bounds = bounds_of(images)
    worst = []
    c = images.shape[1]
    for level, bound, pos, dirs in zip(levels, bounds, plan.positions, plan.directions):
        desc = E.swd_descriptors(level, pos)
        mean, std = E.swd_channel_statistics(desc, c)
        assert (std > 0).all()
        x = E.swd_normalise(desc, c)
        d = x.shape[1]
        shaped = (len(desc), c, -1)
        spread = np.abs(desc - desc[0:1, :]).reshape(shaped).max(axis=(0, 2))              # >= max|v - v0| per channel
        ed = E.swd_descriptors(bound, pos)
        em = ed.reshape(shaped).mean(axis=(0, 2)) + 2.0 ** -30 * spread
        es = np.sqrt((ed.reshape(shaped) ** 2).mean(axis=(0, 2))) + 2.0 ** -30 * spread
        s = _per_element(std, d)
        rho = _per_element(es, d) / s
        dx = ((ed + _per_element(em, d)) / s + np.abs(x) * rho) / (1.0 - rho)
        worst.append(float(projection_bound(x, np.abs(mean) + em, std - es, dirs, dx=dx).max()))
    return worst


@functools.lru_cache(maxsize=None)
def end_to_end_bound(case):
    """{key: bound of |device - yardstick|} for every key of the result, in the result's unit (1000 x the distance)."""
    a, b, plan = end_to_end_inputs(case)
    per = [1000.0 * (ea + eb) * (1.0 + 2.0 ** -40) for ea, eb in zip(_set_error(a, case, plan), _set_error(b, case, plan))]
    out = {"swd_%d" % s: v for s, v in zip(plan.sizes, per)}
    out["swd"] = float(np.mean(per))
    return out


# ---- sort ---------------------------------------------------------------------------------------------------------------
SORT_CONTENTS = ("random", "equal", "sorted", "reversed", "duplicates", "special")


def sort_input(content, rows, cols, seed=0):
    """fp32 [cols, rows].  "special": +-inf, -0.0 and denormals among ordinary keys -- and no +0.0: the device orders -0.0
    below +0.0 by its bits while np.sort calls them equal and may leave them in either order."""
    rng = np.random.RandomState(500 + seed + rows % 1000 + cols)
    if content == "equal":
        return np.full((cols, rows), 1.5, dtype=np.float32)
    x = rng.randn(cols, rows).astype(np.float32)
    if content == "sorted":
        return np.sort(x, axis=1)
    if content == "reversed":
        return np.ascontiguousarray(np.sort(x, axis=1)[:, ::-1])
    if content == "duplicates":
        return np.round(x * 2).astype(np.float32) + np.float32(0.5)          # about nine distinct keys, none of them 0
    if content == "special":
        special = np.array([np.inf, -np.inf, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3.4e38, -3.4e38], dtype=np.float32)
        pick = rng.rand(cols, rows) < 0.3
        x[pick] = special[rng.randint(0, len(special), int(pick.sum()))]
        assert not ((x == 0) & ~np.signbit(x)).any()
    return x

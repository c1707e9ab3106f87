"""The cases of the step tails (csrc/gz_optim.hip, csrc/gz_loss.hip) as data: sizes, switch lists and the seeded float32
HOST inputs.  Nothing here touches a GPU or the library, so the fp64 reference and its float32 replay
(tail_reference.py, CPU only) and the GPU test (test_tail_fp64_gpu.py, which uploads these arrays and drives the C ABI)
see the same numbers.  Every size is the smallest at which a branch of the launch geometry exists; the comment next to
it says which."""
import itertools
import zlib

import numpy as np

SENTINEL = 123.0
GUARD = 64                      # sentinel words in front of and behind every output buffer
GZ_ERR_BAD_SHAPE, GZ_ERR_UNSUPPORTED = -1, -2


def rng(*tag):
    return np.random.RandomState(zlib.crc32(repr(tag).encode()) & 0x7FFFFFFF)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def c32(x):
    """A scalar as the C ABI receives it: rounded to float32, held as a Python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------
# optimizers: 4096 elements per workgroup, 256 threads, float4 when every pointer is 16-byte aligned
# ---------------------------------------------------------------------------
OPT_MAX_TENSORS = 24
OPT_NUMELS = [1, 3, 4, 5, 7,        # below, at and past one float4: the scalar tail inside the float4 path
              4095, 4096, 4097,     # around one workgroup's chunk
              8193]                 # a third chunk of one element
OPT_LAYOUTS = ("single", "table", "offset")
OPT_OFFSET_TENSOR = 3               # "offset": this tensor's four arrays start 4 bytes off -> the whole call goes scalar
ADAM_LR, ADAM_EPS = 2e-4, 1e-8
BETAS = [(0.5, 0.999), (0.0, 0.9)]
STEPS = [1, 2, 10, 1000, 100000]
RMSPROP_LR, RMSPROP_ALPHA, RMSPROP_EPS = 5e-5, 0.99, 1e-8


def opt_numels(layout):
    """The tensors of one call ("single": of the nine calls, one tensor each)."""
    if layout == "table":           # find_tensor walks the whole prefix table
        return (OPT_NUMELS * 3)[:OPT_MAX_TENSORS]
    return list(OPT_NUMELS)


def opt_offsets(layout):
    return [1 if layout == "offset" and k == OPT_OFFSET_TENSOR else 0 for k in range(len(opt_numels(layout)))]


def adam_switches():
    """(beta1, beta2, step, grad_scale, zero_grads)."""
    return [(b1, b2, t, gs, zg) for (b1, b2) in BETAS for t in STEPS for gs in (1.0, 0.5) for zg in (0, 1)]


def rmsprop_switches():
    return [(gs, zg) for gs in (1.0, 0.5) for zg in (0, 1)]


def adam_tag(b1, b2, t, gs, zg):
    return "b%g_%g_t%d_gs%g_zg%d" % (b1, b2, t, gs, zg)


def opt_tensor_host(layout, k, n):
    """p, g, m, v of tensor k (n elements).  Tensors 1 and 7 of each nine have p == 0: p' is the update itself.
    Tensors 4 and 8 have g == 0 and v == 0 in every third element: v' = 0, the quotient is m' / eps.  All normal."""
    r = rng("opt", layout, k, n)
    d = {"p": 0.05 * r.randn(n), "g": 1e-2 * r.randn(n), "m": 1e-3 * r.randn(n), "v": 1e-5 + 1e-4 * r.rand(n)}
    if k % 9 in (1, 7):
        d["p"][:] = 0.0
    if k % 9 in (4, 8):
        d["g"][::3] = 0.0
        d["v"][::3] = 0.0
    return {key: f32(a) for key, a in d.items()}


# Adam from slabs: 256 floats per workgroup
SLAB_MAX_TENSORS, SLAB_MAX_SRC = 12, 4
SLAB_NUMELS = [4, 252, 256, 260, 1028]      # one float4; one short of, at and past one workgroup; a fifth workgroup
SLAB_NZ = [1, 3, 4, 5, 17, 33]              # every remainder loop of reduce_sources (strides of 32, 16 and 4 slabs)
SLAB_PAD = 12                               # slab stride = numel + SLAB_PAD floats
SLAB_SHIFT = 2.0 ** -10


def slab_params():
    """[(numel, [nz of each source])] of the one call with twelve parameters."""
    nz = itertools.cycle(SLAB_NZ)
    return [(SLAB_NUMELS[k % len(SLAB_NUMELS)], [next(nz) for _ in range(1 + k % SLAB_MAX_SRC)])
            for k in range(SLAB_MAX_TENSORS)]


def slab_switches():
    return [(b1, b2, t, gs) for (b1, b2) in BETAS for t in (1, 1000) for gs in (1.0, 0.5)]


def slab_host(k, n, nzs):
    """p, m, v and per source a [nz][n + SLAB_PAD] slab array of small integers times 2^-10: any order of summation
    gives the same float32 gradient (|sum| <= 4 * 33 * 7 < 2^24)."""
    from exact_support import int_operands
    d = opt_tensor_host("slabs", k, n)
    slabs = []
    for q, nz in enumerate(nzs):
        s = int_operands((nz, n + SLAB_PAD), 7, 0.8, 100 * k + q + 1).numpy() * np.float32(SLAB_SHIFT)
        s[:, n:] = SENTINEL                 # the padding between slabs: never read
        slabs.append(f32(s))
    return {"p": d["p"], "m": d["m"], "v": d["v"], "slabs": slabs}


# ---------------------------------------------------------------------------
# loss tails: forward one workgroup of 256, backward grid-stride with at most 2048 workgroups
# ---------------------------------------------------------------------------
LOSS_N = [1, 255, 256, 257, 513, 70001]     # around one pass of the workgroup, a third pass, many passes
LOSS_BWD_N = LOSS_N + [2048 * 256 + 1]      # one thread of the capped grid takes a second pass
UPSTREAM = 0.37
LOGIT_EDGES = [30.0, -30.0, 90.0, -90.0]


def bce_host(n):
    x = 3.0 * rng("bce", n).randn(n)
    if n >= 255:
        x[:4] = LOGIT_EDGES
        x[-2:] = [90.0, -90.0]              # (the workgroup's last lanes too)
    return {"x": f32(x), "g": f32([UPSTREAM])}


def mse_host(n):
    r = rng("mse", n)
    return {"a": f32(r.randn(n)), "b": f32(r.randn(n)), "g": f32([UPSTREAM])}


def gp_host(n):
    """Per-sample sums of squares around 1; from 255 on rows with 0, exactly 1 and 1 +- 2^-20."""
    s = (1.0 + 0.3 * rng("gp", n).randn(n)) ** 2
    if n >= 255:
        s[:4] = [0.0, 1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20]
        s[-1] = 0.0
    return {"sumsq": f32(s), "g": f32([UPSTREAM])}


# ---------------------------------------------------------------------------
# vector operations and the element-wise spectral-norm kernels
# ---------------------------------------------------------------------------
SN_EPS = 1e-12
VEC_N = [1, 255, 256, 257, 3000]
VEC_MODES = ("plain", "inplace", "no_out2", "zero")
MAT_SHAPES = [(1, 4), (3, 8), (16, 200), (65, 1028),
              (2049, 1028)]     # 526593 float4: more than 2048 * 256


def vec_host(n, zero=False):
    r = rng("vec", n)
    x = r.randn(n)
    return {"x": f32(np.zeros(n) if zero else x), "b": f32(r.randn(n))}


def mat_host(R, L):
    r = rng("mat", R, L)
    return {"x": f32(r.randn(R, L)), "sigma": f32([1.7]), "rowdots": f32(r.randn(R)), "u": f32(r.randn(R)),
            "v": f32(r.randn(L))}


# power iteration
POWER_SHAPES = [
    (1, 4), (3, 8),     # one slice, one column block, one row workgroup
    (63, 1020),         # last row count without slicing; one column block short of full
    (64, 1024),         # 32 slices of 2 rows; exactly one full column block
    (65, 1028),         # rps = 3: slices 22..31 are empty; a second column block of one float4
    (100, 2052),        # rps = 4: slices 25..31 are empty; three column blocks
    (2049, 1028),       # row workgroups capped at 2048: workgroup 0 takes two rows; share = 1
]
POWER_TABLE = [(65, 1028), (3, 8), (64, 1024), (2049, 1028)]
POWER_ZERO = [(3, 8), (65, 1028)]


def power_host(R, L, zero=False):
    """W[r][l] = a_r b_l |n_rl| with n standard normal and a, b random signs (every entry is standard normal), and
    u_r = a_r |z_r| normalised: the terms of every sum of W^T u and of W v then have one sign, so the norms are no
    cancellations and the scale of u, v and sigma stays near their size.  (With independent signs a sum of R terms is
    sqrt(R) below its magnitudes, the first-order scale of a normalised vector grows by that factor per product, and
    the tolerance of the second iteration at R = 2049 would pass a v that is off by 0.2 %.)
    v holds what the launch has to overwrite."""
    r = rng("power", R, L)
    a, b = r.choice([-1.0, 1.0], R), r.choice([-1.0, 1.0], L)
    W, u = np.abs(r.randn(R, L)) * a[:, None] * b[None, :], np.abs(r.randn(R)) * a
    return {"W": f32(np.zeros((R, L)) if zero else W), "u": f32(u / np.linalg.norm(u)), "v": f32(np.full(L, SENTINEL))}


# sigma term: 16 coefficient slices per group
SIGMA_GROUPS = [1, 2, 8]
SIGMA_ROWS_PER_GROUP = [1, 15, 16, 17,  # slices of one row: all but one empty, one empty, none empty; of two rows
                        4097]           # 257 rows a slice: a second pass of the 256 threads
SIGMA_SHAPES = [(3, 8), (65, 1028)]
SIGMA_EPS = 1e-5
WRONG_HALF = 1e30                       # the first float of every rowsums pair


def sigma_host(groups, rpg, R, L):
    r = rng("sigma", groups, rpg, R, L)
    rows = groups * rpg
    rowsums = np.stack([np.full(rows, WRONG_HALF), r.randn(rows)], 1)
    return {"rowsums": f32(rowsums), "rstd": f32(0.5 + r.rand(rows)), "sigma": f32(1.0 + r.rand(groups)),
            "u": f32(r.randn(groups, R)), "v": f32(r.randn(groups, L))}


# ---------------------------------------------------------------------------
# the list of cases: (reference / driver name, arguments)
# ---------------------------------------------------------------------------
CASES = ([("adam", (entry, layout)) for entry in ("step", "step_dev") for layout in OPT_LAYOUTS]
         + [("rmsprop", (layout,)) for layout in OPT_LAYOUTS]
         + [("tick", betas) for betas in BETAS]
         + [("slabs", ())]
         + [("bce", (n,)) for n in LOSS_N] + [("mse", (n,)) for n in LOSS_N] + [("gp", (n,)) for n in LOSS_N]
         + [("loss_bwd", (n,)) for n in LOSS_BWD_N]
         + [("vec", (n,)) for n in VEC_N]
         + [("mat", shape) for shape in MAT_SHAPES]
         + [("power", shape) for shape in POWER_SHAPES]
         + [("power_zero", shape) for shape in POWER_ZERO]
         + [("sigma_term", (g, rpg, R, L)) for g in SIGMA_GROUPS for rpg in SIGMA_ROWS_PER_GROUP
            for (R, L) in SIGMA_SHAPES])

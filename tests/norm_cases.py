"""The cases of the normalisation kernels (csrc/gz_norm.hip) as data: shapes, switch lists and the seeded float32 HOST
inputs.  Nothing here touches a GPU or the library, so the bits test (test_norm_parent_bits_gpu.py, which uploads these
arrays and drives the entry points) and the fp64 reference (norm_reference.py, CPU only) see the same numbers.

The generator, the tags and the order of the draws are what tests/golden/norm_parent.npz was recorded with: changing any
of them moves every recorded bit."""
import zlib

import numpy as np

EPS, MOMENTUM = 1e-5, 0.1
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "lrelu": (2, 0.2)}
SENTINEL = 123.0            # what an output buffer holds before the launch
NBT0 = 7                    # num_batches_tracked before the launch
GZ_ERR_UNSUPPORTED = -2
SIGMAS = [1.3, 0.8]         # gz_rownorm_act_fwd_sigma: sigma[g] of group g

ROW_SHAPES = [                 # (N, C, inner)
    (3, 5, 4),                 # q4 = 1, 64 rows per wave, 15 rows: dead sub-waves
    (3, 5, 12),                # q4 = 3 under lpr = 4: a dead lane inside a live row
    (2, 3, 64),                # lpr = 16
    (2, 3, 256),               # lpr = 64
    (2, 3, 1024),              # CACHE = 4, full
    (2, 3, 1280),              # forward CACHE = 16 with a tail; backward CACHE = 0 under the default knob
    (1, 2, 4096),              # forward CACHE = 16, full
    (1, 2, 4352),              # forward CACHE = 0
    (4, 131080, 4),            # 524320 rows: second trip of the row loop and of the float4 loop of the apply kernels
]
ADAIN_SHAPES = [(5, 3, 16), (5, 3, 256), (3, 2, 1024)]      # lpr 4 and 64, and the largest row the backward accepts
BN_SHAPES = [                  # (N, C, H, W)
    (4, 32, 4, 4),             # CB = 16
    (4, 8, 8, 8),              # CB = 4
    (6, 5, 8, 8),              # odd C, CB = 1
    (16, 32, 16, 16),          # S = 2
    (6, 4, 64, 64),            # S = 4, P = 2: the last slice is empty
    (12, 4, 64, 64),           # as above, with groups = 2
]
BIG_CHANNELS = (4, 131080, 4)  # the per-channel apply index with FastDiv, past one trip of the grid
EW_COUNTS = [4, 2097156]       # one float4, and past one trip of the grid
FINALIZE_C, FINALIZE_PER = 5, 32

# switch lists: every combination on the small shapes, one on the large
FWD_FULL = [(apr, unb, act) for apr in (0, 1) for unb in (0, 1) for act in ACTS]
FWD_FEW = [(1, 1, "lrelu")]
STATS_FULL, STATS_FEW = [(0, 0), (0, 1), (1, 0), (1, 1)], [(1, 0)]
# (affine_per_row, unbiased, activation, with dx); affine_per_row 2 is the packed [N][2C] gradient of AdaIN
BWD_FULL = ([(apr, unb, act, 1) for apr in (0, 1) for unb in (0, 1) for act in ACTS]
            + [(2, 1, "relu", 1), (1, 0, "lrelu", 0)])
BWD_FEW = [(0, 1, "relu", 1)]


def switches(N, C, inner, full, few):
    return full if N * C * inner <= 65536 else few


def small(N, C, inner):
    return N * C * inner <= 65536


def bn_fused_switches():
    """(groups, partial rows, running buffers, activation, affine, with dx) of the eight runs of the fused BatchNorm."""
    acts = list(ACTS)
    return [(g, p, r, acts[(i + 1) % 3], i != 0, i != 7)
            for i, (g, p, r) in enumerate((g, p, r) for g in (1, 2) for p in (0, 1) for r in (0, 1))]


def rng(*tag):
    return np.random.RandomState(zlib.crc32(repr(tag).encode()) & 0x7FFFFFFF)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _all_f32(d):
    return {k: f32(v) for k, v in d.items()}


def rows_host(tag, N, C, inner):
    """x with per-row means of 1.5 +- 0.5 and sigma 0.7, mixed-sign gradients, affine parameters of each form."""
    r = rng("rows", tag, N, C, inner)
    x = 1.5 + 0.5 * r.randn(N, C, 1) + 0.7 * r.randn(N, C, inner)
    d = {"x": x, "g": r.randn(N, C, inner), "v": r.randn(N, C, inner),
         "gamma_c": 1 + 0.3 * r.randn(C), "beta_c": 0.3 * r.randn(C),
         "gamma_r": 1 + 0.3 * r.randn(N * C), "beta_r": 0.3 * r.randn(N * C),
         "acc_gamma": r.randn(N * C), "acc_beta": r.randn(N * C)}
    return _all_f32(d)


def adain_host(N, C, inner):
    """x: the [C][inner] constant every sample shares; sb: the packed per-sample [N][scale C | shift C]; g."""
    r = rng("adain", N, C, inner)
    x = f32(1.5 + 0.5 * r.randn(C, 1) + 0.7 * r.randn(C, inner))
    sb = f32(np.concatenate([1 + 0.3 * r.randn(N, C), 0.3 * r.randn(N, C)], axis=1))
    return {"x": x, "sb": sb, "g": f32(r.randn(N, C, inner))}


def bn_inputs_host(tag, N, C, inner):
    r = rng("bn", tag, N, C, inner)
    x = 1.5 + 0.5 * r.randn(1, C, 1) + 0.7 * r.randn(N, C, inner)
    halves = x.reshape(N, C, 2, inner // 2).transpose(0, 2, 1, 3)                       # [N][half][C][inner / 2]
    partials = np.stack([halves.sum(-1), (halves * halves).sum(-1)], -1).reshape(2 * N, C, 2)
    d = {"x": x, "g": r.randn(N, C, inner), "partials": partials, "gamma": 1 + 0.3 * r.randn(C),
         "beta": 0.3 * r.randn(C), "rm": 0.2 * r.randn(C), "rv": 0.5 + r.rand(C), "acc_gamma": r.randn(C),
         "acc_beta": r.randn(C)}
    return _all_f32(d)


def finalize_host(rows, groups):
    """Partial rows of FINALIZE_PER elements each, [rows][C][2], and the affine parameters and running buffers."""
    C, per = FINALIZE_C, FINALIZE_PER
    r = rng("finalize", rows, groups)
    x = 1.5 + 0.5 * r.randn(1, C, 1) + 0.7 * r.randn(rows, C, per)
    partials = f32(np.stack([x.sum(-1), (x * x).sum(-1)], -1))
    d = _all_f32({"gamma": 1 + 0.3 * r.randn(C), "beta": 0.3 * r.randn(C), "rm": 0.2 * r.randn(C),
                  "rv": 0.5 + r.rand(C)})
    d["partials"] = partials
    return d


def channel_sum_host(N, C, inner):
    return {"x": f32(rng("channel_sum").randn(N, C, inner))}


def elementwise_host(count):
    r = rng("ew", count)
    g, v, out = (f32(r.randn(count)) for _ in range(3))
    g[:4] = np.abs(g[:4]) * [1, -1, -1, 1]          # (the one-float4 case has both sides of the activation too)
    out[:4] = np.abs(out[:4]) * [1, -1, 1, -1]
    return {"g": g, "v": v, "out": out}


def elementwise_acts(count):
    return list(ACTS.items()) + [("tanh", (3, 0.0))] if count <= 65536 else [("lrelu", ACTS["lrelu"])]

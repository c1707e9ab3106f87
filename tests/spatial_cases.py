"""The cases of the pooling, resize and ResNet spatial kernels (csrc/gz_infer.hip, first half of csrc/gz_resnet.hip) as
data: sizes, the launch boundary each size sits on, and the seeded float32 HOST inputs.  Nothing here touches a GPU; the
library is asked for one thing only, the text of gz_pool2d_plan (host arithmetic), so that the fp64 reference
(spatial_reference.py, CPU only) and the GPU test (test_spatial_fp64_gpu.py) see the same numbers.

Every pool row carries the plan text it expects under the default switches: which of the five kernels runs, with the
group size, grid and LDS bytes that follow from the shape.  A threshold edit that moves a row off its kernel fails
test_spatial_reference_cpu.py before any launch.  `loop` names the loop that makes a second trip in that row."""
import ctypes

import numpy as np

from eval_device_support import MUL_ADD, edge_samples
from tail_cases import GUARD, GZ_ERR_BAD_SHAPE, SENTINEL, c32, f32, rng  # noqa: F401

ACT_RELU, ACT_LRELU = 1, 2


class Case:
    def __init__(self, kind, name, **kw):
        self.kind, self.name, self.loop, self.note = kind, name, None, ""
        self.__dict__.update(kw)

    @property
    def id(self):
        return "%s_%s" % (self.kind, self.name)

    def __repr__(self):
        return self.id


# ---------------------------------------------------------------------------
# pooling: gz_pool2d chooses between global_avg_kernel<16>, pool2d_band_kernel, pool2d_group_kernel<3,1,1> / <3,2,0>,
# pool2d_plane_kernel and the flat pool2d_kernel
# ---------------------------------------------------------------------------
KNOBS = {"default": 0, "no_group": 1, "no_group_no_plane": 3}      # the bits of gz_pool2d_plan's `knobs`
KNOB_ENV = {"default": {}, "no_group": {"GZ_NO_POOL_GROUP": "1"},
            "no_group_no_plane": {"GZ_NO_POOL_GROUP": "1", "GZ_NO_POOL_PLANE": "1"}}
ALL, AVG = (0, 1, 2), (1, 2)
G311, G320 = (3, 1, 1), (3, 2, 0)


def _pool(name, planes, H, W, window, modes, plan, note, loop=None, misaligned=False, big=False, lds_check=False):
    KS, S, P = window
    return Case("pool", name, planes=planes, H=H, W=W, KS=KS, S=S, P=P, modes=modes, plan=plan, note=note, loop=loop,
                misaligned=misaligned, big=big, lds_check=lds_check)


def _group_rows():
    rows = []
    for tag, win in (("s1p1", G311), ("s2p0", G320)):
        g = "group<3,%d,%d>" % win[1:]
        pad = 2 * win[2]

        def lds(G, H, W):
            return G * (H + pad) * (W + pad) * 4

        def row(planes, H, W, note):
            G = max(1, 2048 // (H * W))
            groups = -(-planes // G)
            rows.append(_pool("%dx%d_%s_p%d" % (H, W, tag, planes), planes, H, W, win, ALL,
                              "%s G=%d grid=%d lds=%d" % (g, G, min(groups, 8192), lds(G, H, W)), note))
        row(1, 3, 3, "hw = 9, G = 227: one plane of a group of 227")
        row(227, 3, 3, "exactly one full group")
        row(228, 3, 3, "a second group of one plane")
        row(500, 3, 3, "three groups, the last ragged")
        row(7, 17, 17, "hw = 289, G = 7: exactly one group")
        row(8, 17, 17, "a second group of one plane")
        row(3, 35, 35, "hw = 1225, G = 1")
        row(3, 45, 46, "hw = 2070 > 2048: G clamps to 1")
        row(2, 3, 2730, "hw = 8190, the widest plane of the group kernel")
        row(2, 2730, 3, "hw = 8190, the tallest")
        row(2, 64, 128, "hw = 8192 exactly: the last size before band / flat")
    return rows


POOL_ROWS = _group_rows() + [
    _pool("46x46_s2p0_p8195", 8195, 46, 46, G320, ALL, "group<3,2,0> G=1 grid=8192 lds=8464",
          "8192 + 3 groups: three workgroups take a second group", loop="group", big=True),
    _pool("3x3_s1p1_p1859684", 8192 * 227 + 100, 3, 3, G311, ALL, "group<3,1,1> G=227 grid=8192 lds=22700",
          "8192 full groups and a ragged ninth-thousandth: workgroup 0 stages 100 planes over 227 stale ones",
          loop="group_ragged", big=True),
    # band: 3x3 s2 p0 on planes above 8192 floats, W <= 1024; 8 output rows per workgroup, 17 W floats of LDS
    _pool("91x91_band", 2, 91, 91, G320, ALL, "band<3,2> grid=12 lds=6188",
          "8281 floats, just past 8192; OH = 45 = 5 bands of 8 + 5 rows"),
    _pool("147x147_band", 1, 147, 147, G320, ALL, "band<3,2> grid=10 lds=9996", "InceptionV3's first max-pool"),
    _pool("100x131_band", 2, 100, 131, G320, ALL, "band<3,2> grid=14 lds=8908", "H != W, OH = 49 = 6 bands + 1 row"),
    _pool("20x963_band", 1, 20, 963, G320, ALL, "band<3,2> grid=2 lds=65484", "the last width under 64 KiB of LDS"),
    _pool("20x1024_band", 1, 20, 1024, G320, ALL, "band<3,2> grid=2 lds=69632",
          "the widest plane the dispatch accepts: 17 * 1024 * 4 bytes of LDS, more than 64 KiB", lds_check=True),
    # plane: what a default process runs for every other window on a plane of up to 8192 floats
    _pool("9x11_k2s2p0", 3, 9, 11, (2, 2, 0), ALL, "plane grid=3 lds=396", "KS 2, the last row and column unread"),
    _pool("9x11_k2s1p1", 3, 9, 11, (2, 1, 1), ALL, "plane grid=3 lds=396", "KS 2 with the largest padding"),
    _pool("9x11_k5s1p2", 3, 9, 11, (5, 1, 2), ALL, "plane grid=3 lds=396", "KS 5, same size"),
    _pool("9x11_k5s3p0", 3, 9, 11, (5, 3, 0), ALL, "plane grid=3 lds=396", "KS 5, stride 3"),
    _pool("9x11_k7s2p3", 3, 9, 11, (7, 2, 3), ALL, "plane grid=3 lds=396", "KS 7: corner windows hold 16 of 49 taps"),
    _pool("9x11_k7s1p0", 3, 9, 11, (7, 1, 0), ALL, "plane grid=3 lds=396", "KS 7 unpadded"),
    _pool("2x9_k3s1p1", 3, 2, 9, G311, ALL, "plane grid=3 lds=72", "a plane lower than the window"),
    _pool("9x2_k3s1p1", 3, 9, 2, G311, ALL, "plane grid=3 lds=72", "a plane narrower than the window"),
    _pool("4x4_global", 5, 4, 4, (4, 1, 0), AVG, "plane grid=5 lds=64", "a global average that is not 8 x 8"),
    _pool("5x5_global", 5, 5, 5, (5, 1, 0), AVG, "plane grid=5 lds=100", "a global average of an odd size"),
    _pool("8x8_global_misaligned", 5, 8, 8, (8, 1, 0), AVG, "plane grid=5 lds=256",
          "the 8 x 8 global average with x 4 bytes off 16-byte alignment", misaligned=True),
    _pool("90x91_k5s2p2", 2, 90, 91, (5, 2, 2), ALL, "plane grid=2 lds=32760", "8190 floats: the largest LDS plane"),
    _pool("2x2_k2_p65541", 65536 + 5, 2, 2, (2, 2, 0), ALL, "plane grid=65536 lds=16",
          "65536 + 5 planes: five workgroups take a second plane", loop="plane"),
    # global average: 16 lanes per 8 x 8 plane, 16 planes per workgroup
    _pool("global_p1", 1, 8, 8, (8, 1, 0), AVG, "global_avg<16> grid=1", "one plane: 16 live lanes"),
    _pool("global_p15", 15, 8, 8, (8, 1, 0), AVG, "global_avg<16> grid=1", "one short of a workgroup"),
    _pool("global_p16", 16, 8, 8, (8, 1, 0), AVG, "global_avg<16> grid=1", "exactly one workgroup"),
    _pool("global_p17", 17, 8, 8, (8, 1, 0), AVG, "global_avg<16> grid=2", "a second workgroup of one plane"),
    _pool("global_p4099", 4099, 8, 8, (8, 1, 0), AVG, "global_avg<16> grid=257", "257 workgroups, the last of 3 planes"),
    # flat: the default above 8192 floats for everything but the band form, and for the band form when W > 1024
    _pool("91x91_flat", 2, 91, 91, G311, ALL, "flat grid=65", "3x3 s1 p1 just past 8192 floats"),
    _pool("9x1100_flat", 2, 9, 1100, G320, ALL, "flat grid=18", "the band window on a plane wider than 1024"),
    _pool("100x131_k5s3p2_flat", 2, 100, 131, (5, 3, 2), ALL, "flat grid=12", "a run-time window above 8192 floats"),
    _pool("730x730_flat", 2, 730, 730, G311, ALL, "flat grid=4096",
          "1,065,800 outputs on 4096 workgroups of 256: a second trip", loop="flat"),
]


def pool_plan(c, knobs="default"):
    """gz_pool2d_plan's text for the row under the named switches (host only)."""
    from lightning_gan_zoo_amd._lib import lib
    buf = ctypes.create_string_buffer(256)
    OH, OW = (c.H + 2 * c.P - c.KS) // c.S + 1, (c.W + 2 * c.P - c.KS) // c.S + 1
    rc = lib.gz_pool2d_plan(c.planes, c.H, c.W, OH, OW, c.KS, c.S, c.P, c.modes[-1], 0 if c.misaligned else 1,
                            KNOBS[knobs] if knobs in KNOBS else knobs, buf, 256)
    assert rc > 0, (c, rc)
    return buf.value.decode()


def pool_branch_under(c, knobs):
    """The kernel a row takes under the named switches: its own by default; without the group kernels the plane kernel
    up to 8192 floats and the flat kernel above; without both the flat kernel."""
    if knobs == "default":
        return c.plan.split()[0]
    return "plane" if knobs == "no_group" and c.H * c.W <= 8192 else "flat"


def plan_loops(c, text):
    """Whether the launch the text describes makes a second trip of its loop (band and global average have none)."""
    f = dict(kv.split("=") for kv in text.split()[1:])
    OH, OW = (c.H + 2 * c.P - c.KS) // c.S + 1, (c.W + 2 * c.P - c.KS) // c.S + 1
    if text.startswith("group"):
        return -(-c.planes // int(f["G"])) > int(f["grid"])
    if text.startswith("plane"):
        return c.planes > int(f["grid"])
    if text.startswith("flat"):
        return c.planes * OH * OW > int(f["grid"]) * 256
    return False


CORNER = 100.0


def pool_host(c):
    """[planes, H, W] standard normal; plane 0 and, of three or more, the last plane hold values in [-3, -1] only (a
    padded corner window whose every real tap is negative); plane 1 (of two or more) is a normal plane with one large
    value at its first corner; of three or more, the last plane has -100 at its last corner and the middle plane 100 at
    its top right corner."""
    r = rng("pool", c.name)
    x = r.standard_normal((c.planes, c.H, c.W)).astype(np.float32)
    for p in {0, c.planes - 1 if c.planes >= 3 else 0}:
        x[p] = r.uniform(-3.0, -1.0, (c.H, c.W))
    if c.planes >= 2:
        x[1, 0, 0] = CORNER
    if c.planes >= 3:
        x[-1, -1, -1] = -CORNER
        x[c.planes // 2, 0, -1] = CORNER
    return x


# ---------------------------------------------------------------------------
# AvgPool2d(3, 2, 1) and nearest 2x upsampling, forward and backward: one item per thread, grid capped at 4096 x 256
# ---------------------------------------------------------------------------
SPATIAL_HW = [(1, 1), (1, 7), (7, 1),       # a single row / column: every guard of the 3 x 3 window at once
              (2, 2), (3, 3),               # even: the last window's third row is outside; odd: it is the last row
              (5, 8), (8, 5), (7, 7), (16, 12), (33, 17)]
SPATIAL_PLANES = [1, 5, 64]
SPATIAL_OPS = ("avgpool3s2_fwd", "avgpool3s2_bwd", "upsample2_fwd", "upsample2_bwd")
# (planes, H, W) of the forward's INPUT at which the op's own item space is 17 * 256 * 256 = 1,114,112 > 2^20
SPATIAL_LOOP = {"avgpool3s2_fwd": (17, 512, 512), "avgpool3s2_bwd": (17, 256, 256), "upsample2_fwd": (17, 256, 256),
                "upsample2_bwd": (17, 256, 256)}
SPATIAL_CASES = [Case(op, "%dx%d_p%d" % (H, W, p), planes=p, H=H, W=W) for op in SPATIAL_OPS for (H, W) in SPATIAL_HW
                 for p in SPATIAL_PLANES]
SPATIAL_CASES += [Case(op, "%dx%d_p%d_loop" % (H, W, p), planes=p, H=H, W=W, loop="rn_grid")
                  for op, (p, H, W) in SPATIAL_LOOP.items()]


def spatial_host(c):
    """The one input of the op: x [planes, H, W] for the forwards, gy in the forward's output shape for the backwards."""
    shape = {"avgpool3s2_fwd": (c.H, c.W), "upsample2_fwd": (c.H, c.W),
             "avgpool3s2_bwd": ((c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1), "upsample2_bwd": (2 * c.H, 2 * c.W)}[c.kind]
    return rng("spatial", c.kind, c.name).standard_normal((c.planes,) + shape).astype(np.float32)


# ---------------------------------------------------------------------------
# act_fwd, axpby: four floats per thread, grid capped at 4096 x 256
# ---------------------------------------------------------------------------
EW_COUNTS = [4, 1020, 1024, 1028,           # one float4; one short of, at and past one workgroup
             4 * (1048576 + 3)]             # three threads make a second trip
EW_BAD_COUNTS = [6, 1022]
ACTS = [(ACT_RELU, 0.0), (ACT_LRELU, 0.2), (ACT_LRELU, 0.0)]
AXPBY_ALPHA, AXPBY_BETA = 1.0, 0.1          # the residual tail x_s + 0.1 dx
AXPBY_FORMS = ("no_b", "no_act_out", "both")
AXPBY_ACT = (ACT_LRELU, 0.2)
EDGES = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e38, -3e38]      # +-0, denormals, the ends of the range
ACT_CASES = [Case("act", "n%d" % n, count=n, loop="rn_grid" if n > 4 * 1048576 else None) for n in EW_COUNTS]
AXPBY_CASES = [Case("axpby", "n%d" % n, count=n, loop="rn_grid" if n > 4 * 1048576 else None) for n in EW_COUNTS]


def ew_host(c):
    """a and b; the edges stand at the front (where they fit) and at the very end.  b holds an edge wherever a does, so
    that 3e38 + 0.1 * 3e38 (finite) and sums of denormals occur."""
    r = rng("ew", c.kind, c.count)
    a, b = (r.standard_normal(c.count).astype(np.float32) for _ in range(2))
    e = f32(EDGES)
    k = min(len(e), c.count)
    a[:k], b[:k] = e[:k], e[:k]
    a[-4:], b[-4:] = e[[6, 1, 3, 7]], e[[6, 0, 2, 7]]
    return a, b


# ---------------------------------------------------------------------------
# bilinear resize: one output per thread, grid capped at 4096 x 256; the fused generator-output kernel: 4096 x-blocks,
# 65535 planes
# ---------------------------------------------------------------------------
RESIZE_SIZES = [((64, 64), (299, 299)), ((128, 96), (299, 299)), ((300, 400), (299, 299)), ((17, 13), (17, 13)),
                ((1, 1), (5, 5)), ((1, 9), (4, 30)), ((9, 1), (30, 4)), ((5, 5), (1, 1)), ((2, 2), (299, 299))]
CONSTANT = -0.625
RESIZE_CASES = [Case("resize", "%dx%d_to_%dx%d_p%d_m%g" % (H, W, OH, OW, p, mul), planes=p, H=H, W=W, OH=OH, OW=OW,
                     mul=mul, add=add)
                for ((H, W), (OH, OW)) in RESIZE_SIZES for p in (1, 6) for (mul, add) in MUL_ADD]
RESIZE_CASES.append(Case("resize", "64x64_to_299x299_p12_loop", planes=12, H=64, W=64, OH=299, OW=299, mul=2.0, add=-1.0,
                         loop="infer_grid"))       # 1,072,812 outputs > 2^20


def resize_host(c):
    """Plane p: random for p % 3 == 0, a checkerboard of +-1 (the largest spread) for 1, the constant for 2."""
    r = rng("resize", c.H, c.W, c.planes)
    x = r.standard_normal((c.planes, c.H, c.W)).astype(np.float32)
    yy, xx = np.mgrid[:c.H, :c.W]
    for p in range(c.planes):
        if p % 3 == 1:
            x[p] = 1.0 - 2.0 * ((yy + xx) % 2)
        if p % 3 == 2:
            x[p] = CONSTANT
    return x


def constant_planes(c):
    return [p for p in range(c.planes) if p % 3 == 2]


SAMPLES_CASES = [Case("samples", "n%d_c%d_%dx%d_to_%dx%d_m%g" % (N, C, H, W, OH, OW, mul), N=N, C=C, H=H, W=W, OH=OH,
                      OW=OW, mul=mul, add=add, loop=loop)
                 for (N, (H, W), (OH, OW), muladd, loop) in [
                     (2, (8, 8), (299, 299), MUL_ADD, None),
                     (2, (64, 64), (299, 299), MUL_ADD[:1], None),
                     (1, (8, 8), (1025, 1025), MUL_ADD[:1], "samples_x"),           # 4105 x-blocks > 4096
                     (21846, (1, 1), (1, 1), MUL_ADD[:1], "samples_planes")]        # 65538 planes > 65535
                 for C in (1, 3) for (mul, add) in muladd]


def samples_host(c):
    return edge_samples((c.N, c.C, c.H, c.W), 1 + c.C)


def bilinear_cases():
    return RESIZE_CASES + SAMPLES_CASES


CASES = POOL_ROWS + SPATIAL_CASES + ACT_CASES + AXPBY_CASES + RESIZE_CASES + SAMPLES_CASES
LOOPS = ("group", "group_ragged", "plane", "flat", "rn_grid", "infer_grid", "samples_x", "samples_planes")
BRANCHES = ("global_avg<16>", "band<3,2>", "group<3,1,1>", "group<3,2,0>", "plane", "flat")

"""The pad-skip forms of igemm2's k4 s2 p1 row loaders on 4x4 maps (csrc/gz_igemm2_loaders.h: ConvFwdA2<256, 4, true>,
ConvDgA2<256, true>): a wavefront's 32-row blocks are staged uniform in the map row, the (block, k-step)
pairs whose vertical tap is padding only are not multiplied, and the accumulators go back to pixel order through LDS
before the epilogue.

1. Exact-integer cases (tests/exact_support.py): forward at H = W = 8 and the transposed form onto 8x8 (all four output
   phases are one launch), N = 3 / 16 / 19 (a partly empty tile, exactly one tile, a second partly empty tile), 256x64
   and 256x128 tiles, one and two wave groups, even and odd chunk counts, unsplit and split, with and without the partial
   BatchNorm statistics.  A misplaced or dropped row is a wrong integer: the comparison is torch.equal.
2. The same launches on seeded non-integer operands in two child processes, GZ_NO_PADSKIP set (the padding rows go
   through the matrix pipe as before) and unset: outputs and raw statistics rows are the same bits (sha256 over the
   uint32 images) -- the new path against the old one, not against itself.
3. Shapes that must keep the old path: 4 columns with 8 rows, 8 columns with 4 rows, 8x8 maps; exact against the fp64
   operator.

The planner gives these tiles to such small shapes only under the experiment switches and a small gz_set_cu_budget, so
each child process runs all of its cases and writes a report (as tests/test_igemm2_ring_gpu.py does)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

import exact_support as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = {"GZ_EXPERIMENTS": "1", "GZ_KG2_MIN_CHUNKS": "1", "GZ_FWD2_MIN_TILES": "1", "GZ_DG2_MIN_TILES": "1"}

# (id, op, (N, C, H, K), CU budget, tile, two wave groups?, slabs, statistics too?)
# F: chunks = C; Dg: chunks = K / 4, columns = C.  An odd chunk count under two wave groups gives the second group a
# chunk of zeros; under a barrier interval of two chunks it leaves half of the last pair empty.
CASES = [
    ("F64-kg2-n3", "F", (3, 17, 8, 4096), 64, "256x64", True, 1, True),
    ("F64-kg2-n16", "F", (16, 16, 8, 4096), 64, "256x64", True, 1, False),
    ("F64-kg2-n19", "F", (19, 17, 8, 2048), 64, "256x64", True, 1, True),
    ("F64-kg1-n3", "F", (3, 17, 8, 4160), 64, "256x64", False, 1, False),
    ("F64-kg1-n16", "F", (16, 17, 8, 4160), 64, "256x64", False, 1, True),
    ("F64-kg1-n19", "F", (19, 16, 8, 2112), 64, "256x64", False, 1, False),
    ("F64-kg2-split-n16", "F", (16, 65, 8, 2048), 64, "256x64", True, 2, True),
    ("F64-kg2-split-n19", "F", (19, 64, 8, 1024), 64, "256x64", True, 2, False),
    ("F64-kg1-split-n3", "F", (3, 65, 8, 2112), 64, "256x64", False, 2, False),
    ("F64-kg1-split-n19", "F", (19, 65, 8, 1088), 64, "256x64", False, 2, True),
    ("F128-kg2-n19", "F", (19, 17, 8, 4096), 64, "256x128", True, 1, True),
    ("F128-kg1-n19", "F", (19, 16, 8, 4160), 64, "256x128", False, 1, False),
    ("F128-kg1-n16", "F", (16, 17, 8, 8448), 64, "256x128", False, 1, True),
    ("F128-kg2-split-n19", "F", (19, 513, 8, 132), 64, "256x128", True, 16, False),
    ("Dg64-kg2-n3", "Dg", (3, 1024, 8, 68), 64, "256x64", True, 1, True),
    ("Dg64-kg2-n16", "Dg", (16, 1024, 8, 64), 64, "256x64", True, 1, False),
    ("Dg64-kg2-n19", "Dg", (19, 512, 8, 68), 64, "256x64", True, 1, True),
    ("Dg64-kg1-n3", "Dg", (3, 1088, 8, 64), 64, "256x64", False, 1, False),
    ("Dg64-kg1-n16", "Dg", (16, 1088, 8, 68), 64, "256x64", False, 1, True),
    ("Dg64-kg1-n19", "Dg", (19, 2112, 8, 68), 256, "256x64", False, 1, False),
    ("Dg64-kg2-split-n16", "Dg", (16, 256, 8, 516), 64, "256x64", True, 4, True),
    ("Dg64-kg2-split-n19", "Dg", (19, 256, 8, 256), 64, "256x64", True, 2, False),
    ("Dg64-kg1-split-n16", "Dg", (16, 320, 8, 516), 64, "256x64", False, 4, False),
    ("Dg64-kg1-split-n3", "Dg", (3, 320, 8, 512), 64, "256x64", False, 4, True),
    ("Dg128-kg2-n19", "Dg", (19, 1024, 8, 68), 64, "256x128", True, 1, True),
    ("Dg128-kg2-n16", "Dg", (16, 2048, 8, 64), 64, "256x128", True, 1, False),
    ("Dg128-kg1-n16", "Dg", (16, 2112, 8, 68), 64, "256x128", False, 1, True),
    ("Dg128-kg1-n19", "Dg", (19, 1088, 8, 64), 64, "256x128", False, 1, False),
    ("Dg128-kg1-n3", "Dg", (3, 2112, 8, 68), 64, "256x128", False, 1, False),
    ("Dg128-kg2-split-n19", "Dg", (19, 132, 8, 516), 64, "256x128", True, 4, True),
]
# (id, op, (N, C, H, W, K), tile, two wave groups?): OW (AW) = 4 with OH (AH) = 8, the transpose of that, 8x8 maps
OTHER = [
    ("F-ow4-oh8", "F", (3, 17, 16, 8, 4096), "256x64", True),
    ("F-ow4-oh8-kg1", "F", (9, 17, 16, 8, 2112), "256x64", False),
    ("F-ow4-oh8-128", "F", (9, 17, 16, 8, 4096), "256x128", True),
    ("F-ow8-oh4", "F", (3, 17, 8, 16, 4096), "256x64", True),
    ("F-8x8", "F", (8, 17, 16, 16, 2048), "256x64", True),
    ("Dg-aw4-ah8", "Dg", (3, 1024, 16, 8, 68), "256x64", True),
    ("Dg-aw4-ah8-kg1", "Dg", (3, 1088, 16, 8, 68), "256x64", False),
    ("Dg-aw8-ah4", "Dg", (3, 1024, 8, 16, 68), "256x64", True),
    ("Dg-8x8", "Dg", (3, 1024, 16, 16, 68), "256x64", True),
]


def _plan(lib, op, N, C, H, W, K):
    buf = ctypes.create_string_buffer(512)
    rc = lib.gz_conv2d_plan(S.OPS.index(op), N, C, H, W, K, H // 2, W // 2, 4, 4, 2, 1, buf, 512)
    assert rc >= 0, (op, N, C, H, W, K, rc)
    return buf.value.decode()


def _check_plan(lib, op, shape5, budget, tile, kg2, slabs=None):
    assert lib.gz_set_cu_budget(budget) == budget
    text = _plan(lib, op, *shape5)
    assert "igemm2<%s>" % tile in text and ("ConvFwdA2" if op == "F" else "ConvDgA2") in text, text
    assert ("wave_groups=2" in text) == kg2, text
    if slabs is not None:
        assert (S.split_count(text) or 1) == slabs, text
    return text


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().view("uint32").tobytes()).hexdigest()


def _launches(F, op, c, a, b, stats):
    """The plain launch and, where asked for, the one that also carries the partial statistics."""
    g = F.Geom(4, 4, 2, 1)
    if op == "F":
        out = [F._conv_fwd_raw(a, b, None, g, F.ACT_NONE, 0.0)]
        if stats:
            out += list(F._conv_fwd_stats_raw(a, b, g))
    else:
        out = [F._conv_dgrad_raw(a, b, None, g, (c.H, c.H), F.ACT_NONE, 0.0)]
        if stats:
            out += list(F._conv_dgrad_stats_raw(a, b, g, (c.H, c.H)))
    return out


def _seeded(torch, c, op, seed):
    """Non-integer operands of the case (uniform in [-1, 1), seeded): rounding, hence the order of the sum, shows."""
    gen = torch.Generator().manual_seed(seed)
    OH = c.H // 2
    sa = (c.N, c.C, c.H, c.H) if op == "F" else (c.N, c.K, OH, OH)
    return (torch.rand(sa, generator=gen) * 2 - 1).cuda(), (torch.rand((c.K, c.C, 4, 4), generator=gen) * 2 - 1).cuda()


def _child(path, mode):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    import torch.nn.functional as TF
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    report = {}
    for i, (cid, op, shape, budget, tile, kg2, slabs, stats) in enumerate(CASES):
        res = report[cid] = {"ok": True}
        try:
            c = S.ConvCase(*shape, 4, 2, 1)
            text = _check_plan(lib, op, (c.N, c.C, c.H, c.H, c.K), budget, tile, kg2, slabs)
            # 2. seeded non-integer operands: digests of the uint32 images, compared across the two children
            a, b = _seeded(torch, c, op, 4000 + i)
            outs = _launches(F, op, c, a, b, stats)
            assert not stats or (len(outs) == 3 and outs[2] is not None), "%s carries no statistics [%s]" % (cid, text)
            res["digests"] = [_digest(t) for t in outs]
            if mode == "off":
                continue
            # 1. exact integers
            a, b, ref = S.conv_ref(c, op)
            S.assert_bits_equal(_launches(F, op, c, a.cuda(), b.cuda(), False)[0], ref, "%s  [%s]" % (cid, text))
            if stats:
                a, b, y64 = S.stats_reference(tuple(c), op)
                _, y, st = _launches(F, op, c, a.cuda(), b.cuda(), True)
                S.assert_bits_equal(y, y64, "%s with statistics  [%s]" % (cid, text))
                assert torch.equal(st, st.round()) and bool((st[:, :, 1] >= st[:, :, 0].abs()).all()), cid
                tot = st.double().sum(0).cpu()
                S.assert_bits_equal(tot[:, 0], y64.sum((0, 2, 3)), "%s sum y" % cid)
                S.assert_bits_equal(tot[:, 1], (y64 * y64).sum((0, 2, 3)), "%s sum y^2" % cid)
        except AssertionError as e:
            res.update(ok=False, why=str(e)[:2000])
    if mode == "on":
        # 3. shapes that keep the loaders as they were
        g = F.Geom(4, 4, 2, 1)
        for cid, op, (N, C, H, W, K), tile, kg2 in OTHER:
            res = report[cid] = {"ok": True}
            try:
                text = _check_plan(lib, op, (N, C, H, W, K), 64, tile, kg2)
                terms = C * 16 if op == "F" else K * 4
                sa = (N, C, H, W) if op == "F" else (N, K, H // 2, W // 2)
                a, b = S.pair(sa, (K, C, 4, 4), terms, 8000 + N + C + H + K)
                fn = (lambda x, w: TF.conv2d(x, w, None, 2, 1)) if op == "F" else \
                     (lambda x, w: TF.conv_transpose2d(x, w, None, 2, 1))
                S.assert_exact_precondition(fn(a.double().abs(), b.double().abs()), cid)
                out = F._conv_fwd_raw(a.cuda(), b.cuda(), None, g, F.ACT_NONE, 0.0) if op == "F" else \
                    F._conv_dgrad_raw(a.cuda(), b.cuda(), None, g, (H, W), F.ACT_NONE, 0.0)
                S.assert_bits_equal(out, fn(a.double(), b.double()), "%s  [%s]" % (cid, text))
            except AssertionError as e:
                res.update(ok=False, why=str(e)[:2000])
    lib.gz_set_cu_budget(256)
    with open(path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    """Both children at once: the new path with every check, the old path for the digests of part 2."""
    d = tmp_path_factory.mktemp("padskip")
    procs = {}
    for mode in ("on", "off"):
        env = dict(os.environ, **KNOBS)
        env.pop("GZ_NO_PADSKIP", None)
        if mode == "off":
            env["GZ_NO_PADSKIP"] = "1"
        path = str(d / ("report_%s.json" % mode))
        procs[mode] = (path, subprocess.Popen([sys.executable, os.path.abspath(__file__), path, mode], env=env,
                                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for mode, (path, p) in procs.items():
        text, _ = p.communicate(timeout=600)
        assert p.returncode == 0 and os.path.exists(path), text[-3000:]
        out[mode] = json.load(open(path))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exact_integers_on_4x4_maps(reports, case):
    res = reports["on"][case[0]]
    assert res["ok"], res.get("why")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_same_bits_as_the_path_that_multiplies_the_padding(reports, case):
    on, off = reports["on"][case[0]], reports["off"][case[0]]
    assert off["ok"], off.get("why")
    assert "digests" in on and len(on["digests"]) == (3 if case[7] else 1), on
    assert on["digests"] == off["digests"], (case[0], on["digests"], off["digests"])


@pytest.mark.parametrize("case", OTHER, ids=[c[0] for c in OTHER])
def test_other_map_shapes_keep_their_path(reports, case):
    res = reports["on"][case[0]]
    assert res["ok"], res.get("why")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])

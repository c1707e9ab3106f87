"""The LDS-DMA ring of igemm2_kernel at the depth each instantiation ships with (csrc/gz_igemm2.h igemm2_depth):
the 256x64 tiles of the k4 s2 p1 layers (ConvFwdA2 / ConvDgA2) at reduction lengths around the depth D -- a workgroup
or wave group with D-2, D-1, D and D+1 chunks, fewer chunks than the prologue issues, the two wave groups of a workgroup
with unequal halves (the second group's tail chunks arrive as zeros), split launches whose last slab is a few chunks
long, a partly empty pixel tile.  Exact-integer operands (tests/exact_support.py): a chunk that is lost, duplicated or
read before it landed is a wrong integer, so the comparison with the fp64 CPU operator is torch.equal.

The planner gives these tiles to small shapes only under the experiment switches (GZ_KG2_MIN_CHUNKS, GZ_FWD2_MIN_TILES,
GZ_DG2_MIN_TILES; read once per process) and a small gz_set_cu_budget, so ONE child process runs every case and the
tests read its report.  What the planner cannot be brought to at these sizes: fewer than 16 chunks in an UNSPLIT
workgroup (pick_tile2 wants a reduction of 256), which is why the short reductions are the last slabs of split
launches (forward only: the input gradient's tiles come in fours, its split counts stay at 8 and a last slab is never
shorter than 25 chunks), and a column count that is no multiple of 64 (such layers never get the 256x64 tile)."""
import json
import os
import subprocess
import sys

import pytest

import exact_support as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = {"GZ_EXPERIMENTS": "1", "GZ_KG2_MIN_CHUNKS": "1", "GZ_FWD2_MIN_TILES": "1", "GZ_DG2_MIN_TILES": "1"}


def _shipped(name):
    """The default of a GZ2_* constant, read from the header, so that the cases follow what ships."""
    import re
    text = open(os.path.join(os.path.dirname(HERE), "lightning_gan_zoo_amd", "csrc", "gz_igemm2.h")).read()
    m = re.search(r"#ifndef %s\n#define %s (\d+)\n#endif" % (name, name), text)
    assert m, name
    return int(m.group(1))


# ring depths (stages) and barrier intervals shipped for the 128x32 wave tile.  With interval 2 the ring is depth / 2
# PAIRS of stages, the prologue issues depth - 2 chunks, and an odd chunk count runs a pair whose second chunk arrives
# as zeros.
DEPTH_KG2, DEPTH_KG1 = _shipped("GZ2_DEPTH_TN1_KG2"), _shipped("GZ2_DEPTH_TN1_KG1")
INTERVAL_KG2, INTERVAL_KG1 = _shipped("GZ2_BARRIER_TN1_KG2"), _shipped("GZ2_BARRIER_TN1_KG1")
assert 3 <= DEPTH_KG2 <= 15 and 3 <= DEPTH_KG1 <= 30, "the last-slab lengths below are 2 .. 33 chunks"


def _cases():
    """(id, op, (N, C, H, K), CU budget, two wave groups?, slabs, chunks of the last slab)"""
    out = []
    d2, d1 = DEPTH_KG2, DEPTH_KG1
    # forward, two wave groups, 32 slabs of 33 chunks (17 + 16 per group) and a last slab of r: r / 2 chunks per group
    lasts = sorted({2 * (d2 - 2), 2 * (d2 - 1), 2 * d2, 2 * (d2 + 1), 2 * d2 - 1, 3})
    for r in lasts:
        out.append(("F-kg2-last%d" % r, "F", (2, 1023 + r, 8, 128), 64, True, 32, r))
    # forward, one wave group (86 slabs x 3 column tiles: more workgroups than CUs), last slab of D-2 .. D+1 chunks
    for r in (d1 - 2, d1 - 1, d1, d1 + 1):
        out.append(("F-kg1-last%d" % r, "F", (2, 2805 + r, 8, 192), 256, False, 86, r))
    # unsplit, two wave groups: 16 chunks (8 + 8), 17 (9 + 8: one zero chunk in the second group); OW = 4, 8, 16;
    # 192 of a tile's 256 pixels (N = 3), two pixel tiles (H = 32)
    out.append(("F-kg2-16", "F", (3, 16, 16, 4096), 64, True, 1, 16))
    out.append(("F-kg2-17", "F", (2, 17, 8, 4096), 64, True, 1, 17))
    out.append(("F-kg2-ow16", "F", (2, 17, 32, 2048), 64, True, 1, 17))
    out.append(("Dg-kg2-16", "Dg", (3, 1024, 16, 64), 64, True, 1, 16))
    out.append(("Dg-kg2-17", "Dg", (4, 1024, 8, 68), 64, True, 1, 17))
    out.append(("Dg-kg2-split", "Dg", (4, 128, 16, 1036), 64, True, 8, 28))
    out.append(("Dg-kg1-17", "Dg", (17, 64, 32, 68), 64, False, 1, 17))      # 68 workgroups on 64 CUs: one wave group
    return out


CASES = _cases()
REPEATED = ("F-kg2-last3", "F-kg2-17", "Dg-kg2-17", "Dg-kg1-17")


def _check_plan(case, lib):
    cid, op, shape, budget, kg2, slabs, last = case
    assert lib.gz_set_cu_budget(budget) == budget
    text = S.conv2d_plan(op, *shape, 4, 2, 1)
    N, C, H, K = shape
    chunks = C if op == "F" else K // 4
    have = S.split_count(text) or 1
    per = -(-chunks // have)
    assert "igemm2<256x64>" in text and ("ConvFwdA2" if op == "F" else "ConvDgA2") in text, text
    assert ("wave_groups=2" in text) == kg2, text
    assert have == slabs and chunks - (-(-chunks // per) - 1) * per == last, (text, chunks, per)
    return text


def _child(path, plan_only):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    report = {}
    for case in CASES:
        cid, op, shape = case[:3]
        try:
            text = _check_plan(case, lib)
            if plan_only:
                print(cid, text)
                report[cid] = {"ok": True}
                continue
            c = S.ConvCase(*shape, 4, 2, 1)
            a, b, ref = S.conv_ref(c, op)
            ad, bd = a.cuda(), b.cuda()
            g = F.Geom(4, 4, 2, 1)
            run = (lambda: F._conv_fwd_raw(ad, bd, None, g, F.ACT_NONE, 0.0)) if op == "F" else \
                  (lambda: F._conv_dgrad_raw(ad, bd, None, g, (c.H, c.H), F.ACT_NONE, 0.0))
            out = run()
            S.assert_bits_equal(out, ref, "%s  [%s]" % (cid, text))
            report[cid] = {"ok": True, "repeat": bool(torch.equal(out, run()))}
        except AssertionError as e:
            report[cid] = {"ok": False, "why": str(e)[:2000]}
    lib.gz_set_cu_budget(256)
    with open(path, "w") as f:
        json.dump(report, f)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ring") / "report.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **KNOBS),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and os.path.exists(path), r.stdout[-3000:]
    return json.load(open(path))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ring_at_reduction_lengths_around_its_depth(report, case):
    res = report[case[0]]
    assert res["ok"], res.get("why")


@pytest.mark.parametrize("cid", REPEATED)
def test_ring_launch_is_repeatable(report, cid):
    res = report[cid]
    assert res["ok"] and res["repeat"], res


if __name__ == "__main__":
    _child(sys.argv[1], "--plan" in sys.argv)

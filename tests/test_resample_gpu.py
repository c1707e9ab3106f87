"""HoloGAN's rigid resampling (csrc/gz_resample.hip): the kernels that run in a training step -- the LDS-staged forward,
the hit lists with the LDS-staged backward -- and their fallbacks, element by element against an fp64 reference.

Reference: the oracle's own pieces (view_matrices, resample_coords, trilinear_indices) for any S.  Coordinates and
weights stay fp32, as in the reference program (the clamped-corner interpolation is discontinuous at the volume faces);
the weights are cast to fp64, the eight products of the forward are accumulated in fp64, and the backward is the exact
transpose of that by index_add_.  Every case first asserts that the device's eight index tensors equal the reference's
bit for bit, so the device's fp32 weights are the reference's and only the summation differs.

Tolerance, with u = 2^-24, on EVERY element:
  forward   |got - ref| <= 16 u sum_k |w_k v_k|      over the element's eight corners (gamma_8 of an fp32 dot product,
                                                     doubled);
  backward  |got - ref| <= 2 t u sum |w g|           over the t corner terms that land on the source voxel (gamma_t,
                                                     doubled).  At face voxels the cancelling out-of-volume corner pairs
                                                     enter the absolute sum, so the bound is looser there.
Neither depends on the summation order, so the same bounds hold for the experiment forms (tools/resample_ab.sh).  Each
test prints its worst err / bound (DESIGN.md section 3.4 records the figures observed on the MI355X).

Which backward ran is read back from the two workspace words include/gz_ops.h documents: the overflow flag and the
plane of list lengths.  ``test_values_*`` compare numbers only and hold under every experiment setting (the last test
runs them so, a fresh process per setting); ``test_path_*`` assert the launch choice of the shipped defaults."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import hologan_cpu as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEG = np.pi / 180.0
UNTOUCHED = -1          # workspace prefill: NaN as a weight, and no flag or list length the launcher writes
GZ_ERR_BAD_SHAPE = -1


def _gpu():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    from lightning_gan_zoo_amd.functional._base import _p, _stream
    return F, lib, _p, _stream


# ---- views ----------------------------------------------------------------------------------------------------------
# rows of (azimuth, elevation, scale, shift x, shift y, shift z); the training range is azimuth 220-320, elevation
# 70-110 degrees, scale 1, no shift (at most 12 hits per source voxel)

def batch_views(S, zoom=None):
    """Six views: the identity (every coordinate lands on an integer), a right-angle view (coordinates on the faces, a
    rounding error to either side of them), two from the training range, one shifted by more than a cell (clamped
    corners), one shifted mostly out of the volume (large cancelling weights).  Scales <= 1.15 keep every hit list at
    20 entries or fewer; ``zoom`` replaces the scale of view 3 (2.0: 27 to 71 hits at every S >= 4)."""
    v = np.zeros((6, 6))
    v[:, 2] = 1.0
    v[1, :2] = (270 * DEG, 90 * DEG)
    v[2, :2] = (233 * DEG, 74 * DEG)
    v[3, :3] = (301 * DEG, 107 * DEG, 1.15 if zoom is None else zoom)
    v[4] = (258 * DEG, 95 * DEG, 1.0, 0.7, -1.2, 0.4)
    v[5] = (287 * DEG, 81 * DEG, 0.9, 0.6 * S + 0.3, -0.4 * S, 0.2)
    return v


def zoom_views(rows, scale):
    """Views of test_rigid_resample_matches_oracle_and_indices_are_bit_exact (RandomState(5)) at another scale."""
    az_el = [(319, 106), (298, 109), (281, 97), (236, 100), (293, 86), (228, 77)]
    v = np.zeros((len(rows), 6))
    for i, r in enumerate(rows):
        v[i, :3] = (az_el[r][0] * DEG, az_el[r][1] * DEG, scale)
    return v


BATCHES = {
    "plain": lambda S: batch_views(S),
    "zoom": lambda S: batch_views(S, 2.0),
}


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the fp64 reference ---------------------------------------------------------------------------------------------

class Ref:
    """Reference values and per-element error bounds of one (views, S, vox, gout); all on the CPU."""

    def __init__(self, view, S, vox, gout=None):
        N, C = vox.shape[:2]
        S3 = S ** 3
        self.N, self.C, self.S = N, C, S
        self.minv = H.view_matrices(view, S, S).reshape(N, 16).contiguous()
        x, y, z = H.resample_coords(self.minv.reshape(N, 4, 4), S)          # fp32
        idx, wts = H.trilinear_indices(vox.shape, x, y, z)
        assert wts[0].dtype == torch.float32
        self.idx = torch.stack(idx)                                         # [8, N*S^3], reference order a..h
        w32 = torch.stack(wts)
        w = w32.double().unsqueeze(2)
        terms = w * vox.double().permute(0, 2, 3, 4, 1).reshape(-1, C)[self.idx]        # [8, N*S^3, C]
        self.fwd = self._out2d(terms.sum(0))
        self.fwd_bound = self._out2d(terms.abs().sum(0)) * (16 * U)
        # hits as the backward counts them: per output voxel one entry per DISTINCT source voxel with a non-zero
        # weight; a corner pair that the clamp collapsed onto one index carries +a and -a and is no hit
        live = torch.ones(N * S3, dtype=torch.bool)
        for s in (x, y, z):
            lo = torch.floor(s).long()
            live &= torch.clamp(lo, 0, S - 1) != torch.clamp(lo + 1, 0, S - 1)
        hit = live.unsqueeze(0) & (w32 != 0)
        self.hits = torch.bincount(self.idx[hit], minlength=N * S3)
        if gout is None:
            return
        g = gout.double().reshape(N, C, S, S, S).flip(2).permute(0, 1, 3, 2, 4)         # [n, c, z, y, x]
        gterms = (w * g.permute(0, 2, 3, 4, 1).reshape(1, -1, C)).reshape(-1, C)
        flat = self.idx.reshape(-1)
        t = torch.bincount(flat, minlength=N * S3).double().unsqueeze(1)
        self.bwd = self._vox(torch.zeros(N * S3, C, dtype=torch.float64).index_add_(0, flat, gterms))
        self.bwd_bound = self._vox(torch.zeros(N * S3, C, dtype=torch.float64).index_add_(0, flat, gterms.abs())
                                   * t * (2 * U))

    def _vox(self, rows):            # [N*S^3 (z, y, x), C] -> [N, C, S, S, S]
        return rows.reshape(self.N, self.S, self.S, self.S, self.C).permute(0, 4, 1, 2, 3).contiguous()

    def _out2d(self, rows):          # -> out2d[n][c*S + (S-1-y)][z][x]
        S = self.S
        return self._vox(rows).permute(0, 1, 3, 2, 4).flip(2).reshape(self.N, self.C * S, S, S).contiguous()


def worst(got, ref, bound):
    """max err / bound over every element; 0 / 0 counts as 0, NaN or an error where the bound is 0 as inf."""
    err = (got.detach().double().cpu() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max())


def assert_indices(ref, vox_d, minv_d):
    """The device's eight corner-index tensors are the reference's, bit for bit -- before any value is compared."""
    F = _gpu()[0]
    _, idx = F.rigid_resample_indices(vox_d, minv_d)
    mism = int((idx.cpu() != ref.idx).sum())
    assert mism == 0, "%d of %d voxel indices differ from the reference's" % (mism, ref.idx.numel())


# ---- launches with buffers of the test's own --------------------------------------------------------------------------

def fwd_raw(vox_d, minv_d):
    """gz_rigid_resample_fwd into a NaN-filled buffer with a NaN tail of four channel volumes behind the output."""
    _, lib, _p, _stream = _gpu()
    N, C, S = vox_d.shape[:3]
    n = N * C * S ** 3
    buf = torch.full((n + 4 * S ** 3,), float("nan"), device="cuda")
    rc = lib.gz_rigid_resample_fwd(_p(vox_d), _p(minv_d), _p(buf), None, N, C, S, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool(torch.isnan(buf[n:]).all()), "gz_rigid_resample_fwd wrote behind its output"
    return buf[:n].view(N, C * S, S, S)


def bwd_raw(gout_d, minv_d, N, C, S, workspace=True):
    """gz_rigid_resample_bwd into a NaN-filled gvox (same tail) with a workspace of the test's own, prefilled with
    UNTOUCHED.  -> (gvox, flag word, list-length plane); the two words are None without a workspace."""
    _, lib, _p, _stream = _gpu()
    S3 = S ** 3
    n = N * C * S3
    buf = torch.full((n + 4 * S3,), float("nan"), device="cuda")
    ws, nbytes = None, 0
    if workspace:
        nbytes = lib.gz_rigid_resample_bwd_workspace_bytes(N, S)
        assert nbytes % 4 == 0
        ws = torch.full((nbytes // 4,), UNTOUCHED, dtype=torch.int32, device="cuda")
        assert ws.data_ptr() % 16 == 0
    rc = lib.gz_rigid_resample_bwd(_p(gout_d), _p(minv_d), _p(buf), _p(ws), nbytes, N, C, S, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool(torch.isnan(buf[n:]).all()), "gz_rigid_resample_bwd wrote behind gvox"
    flag = counts = None
    if workspace:
        cap = lib.gz_rigid_resample_bwd_list_capacity()
        flag = int(ws[(nbytes - 16) // 4])
        counts = ws[cap * N * S3:(cap + 1) * N * S3].cpu()
    return buf[:n].view(N, C, S, S, S), flag, counts


@functools.lru_cache(maxsize=None)
def case(batch, S, C):
    """One batch through the forward (autograd wrapper and C ABI) and the backward (C ABI, own workspace and none):
    the worst err / bound of each, and the workspace words."""
    F, lib, _, _ = _gpu()
    view = BATCHES[batch](S) if isinstance(batch, str) else zoom_views(*batch)
    N = len(view)
    vox = rnd(N, C, S, S, S, seed=1000 * S + C)
    gout = rnd(N, C * S, S, S, seed=2000 * S + C)
    ref = Ref(view, S, vox, gout)
    vox_d, minv_d, gout_d = vox.cuda(), ref.minv.cuda(), gout.cuda()
    assert_indices(ref, vox_d, minv_d)
    out_raw = fwd_raw(vox_d, minv_d)
    out = F.rigid_resample(vox_d, minv_d)
    assert torch.equal(out, out_raw)
    r = {"ref": ref, "minv_d": minv_d, "gout_d": gout_d, "vox_d": vox_d, "fwd": worst(out, ref.fwd, ref.fwd_bound),
         "cpu_hits": int(ref.hits.max()), "capacity": lib.gz_rigid_resample_bwd_list_capacity()}
    gv, r["flag"], r["counts"] = bwd_raw(gout_d, minv_d, N, C, S)
    r["bwd"] = worst(gv, ref.bwd, ref.bwd_bound)
    r["bwd_null"] = worst(bwd_raw(gout_d, minv_d, N, C, S, workspace=False)[0], ref.bwd, ref.bwd_bound)
    print("%s S=%d C=%d: worst err/bound forward %.3f backward %.3f null-workspace %.3f; flag %s, hits cpu %d device %s"
          % (batch, S, C, r["fwd"], r["bwd"], r["bwd_null"], r["flag"], r["cpu_hits"],
             None if r["counts"] is None else int(r["counts"].max())))
    return r


# S: 4 = 64 voxels < 256 threads; 6 = not a power of two; 8 = smallest swizzled size, 512 voxels = exactly one
# two-voxel pass of the staged backward; 12 = 3 * 512 + 192 voxels, the second voxel of the last pass is out of range;
# 16 = the workload, 64 KiB of LDS; 5 = S^3 % 4 != 0 and 20 = 4 * S^3 floats exceed 64 KiB: direct forward, gather
# backward.  C: 5 = a ragged group of four, 33 = a second 32-channel slice of the gather kernel.
STAGED = [(4, 1), (4, 5), (6, 4), (6, 5), (8, 5), (8, 33), (12, 1), (12, 5), (16, 4), (16, 5)]
DIRECT = [(5, 5), (5, 33), (20, 4), (20, 5)]
ids = lambda cases: ["S%d-C%d" % c for c in cases]        # noqa: E731


@pytest.mark.parametrize("S,C", STAGED + DIRECT, ids=ids(STAGED + DIRECT))
def test_values_match_fp64_reference(S, C):
    r = case("plain", S, C)
    assert r["fwd"] <= 1.0 and r["bwd"] <= 1.0 and r["bwd_null"] <= 1.0


@pytest.mark.parametrize("S,C", [(8, 33), (16, 5), (4, 5), (12, 4)], ids=ids([(8, 33), (16, 5), (4, 5), (12, 4)]))
def test_values_of_a_batch_with_one_overflowing_view(S, C):
    """One scale-2 view among six: every sample's gradient, the non-overflowing ones included, is within the bound."""
    r = case("zoom", S, C)
    assert r["fwd"] <= 1.0 and r["bwd"] <= 1.0 and r["bwd_null"] <= 1.0


@pytest.mark.parametrize("S,C", STAGED, ids=ids(STAGED))
def test_path_staged(S, C):
    r = case("plain", S, C)
    assert r["cpu_hits"] <= 20
    assert r["flag"] == 0
    assert torch.equal(r["counts"], r["ref"].hits.clamp(max=r["capacity"]).int())


@pytest.mark.parametrize("S,C", DIRECT, ids=ids(DIRECT))
def test_path_direct_gather_leaves_the_workspace_alone(S, C):
    r = case("plain", S, C)
    assert r["flag"] == UNTOUCHED and bool((r["counts"] == UNTOUCHED).all())


@pytest.mark.parametrize("S,C", [(8, 33), (16, 5), (4, 5), (12, 4)], ids=ids([(8, 33), (16, 5), (4, 5), (12, 4)]))
def test_path_fallback_sets_the_flag(S, C):
    r = case("zoom", S, C)
    assert 27 <= r["cpu_hits"] <= 71
    assert r["flag"] != 0 and r["flag"] != UNTOUCHED
    assert torch.equal(r["counts"], r["ref"].hits.clamp(max=r["capacity"]).int())


# ---- a list that is exactly full ---------------------------------------------------------------------------------------
# (rows of zoom_views, scale): longest lists of 24, 24, 24, 23 hits, and of 24, 24, 24, 25 (each count holds over
# scales 1.33 to 1.34 at least, and several voxels reach it)
FULL = ((0, 3, 5, 1), 1.34)
ONE_OVER = ((0, 3, 5, 4), 1.34)


def test_values_full_and_overfull_lists():
    for batch in (FULL, ONE_OVER):
        r = case(batch, 16, 5)
        assert r["fwd"] <= 1.0 and r["bwd"] <= 1.0 and r["bwd_null"] <= 1.0


def test_path_full_list_stays_staged_and_one_more_hit_falls_back():
    full, over = case(FULL, 16, 5), case(ONE_OVER, 16, 5)
    cap = full["capacity"]
    assert int(full["counts"].max()) == cap and int(full["ref"].hits.max()) == cap and full["flag"] == 0
    assert int(over["ref"].hits.max()) == cap + 1 and int(over["counts"].max()) == cap and over["flag"] == 1


# ---- the autograd wrapper's scratch, reused across launches ---------------------------------------------------------------

def test_scratch_reuse_overflow_staged_overflow():
    """The wrapper's scratch comes back from the allocator with the previous launch's flag and lists in it."""
    F = _gpu()[0]
    S, C = 8, 5
    seq = [case("zoom", S, C), case("plain", S, C), case("zoom", S, C)]
    assert seq[0]["flag"] == 1 and seq[1]["flag"] == 0
    grads = []
    for i, r in enumerate(seq + seq[1:2]):
        v = r["vox_d"].clone().requires_grad_()
        F.rigid_resample(v, r["minv_d"]).backward(r["gout_d"])
        ratio = worst(v.grad, r["ref"].bwd, r["ref"].bwd_bound)
        print("scratch reuse, launch %d: worst err/bound %.3f" % (i, ratio))
        assert ratio <= 1.0
        grads.append(v.grad)
    assert torch.equal(grads[0], grads[2])          # no atomics on either path
    assert torch.equal(grads[1], grads[3])


# ---- alignment contract ---------------------------------------------------------------------------------------------

def _offset_view(t):
    """The same values on the GPU, 4 bytes off a 16-byte boundary."""
    return torch.empty(t.numel() + 1, device="cuda")[1:].view_as(t).copy_(t)


def test_unaligned_operands_take_the_direct_kernels():
    _, lib, _p, _stream = _gpu()
    S, C = 8, 5
    r = case("plain", S, C)
    ref, N = r["ref"], r["ref"].N
    vs, gs = _offset_view(r["vox_d"]), _offset_view(r["gout_d"])
    assert vs.data_ptr() % 16 == 4 and gs.data_ptr() % 16 == 4
    fwd = worst(fwd_raw(vs, r["minv_d"]), ref.fwd, ref.fwd_bound)
    gv, flag, counts = bwd_raw(gs, r["minv_d"], N, C, S)
    bwd = worst(gv, ref.bwd, ref.bwd_bound)
    print("unaligned S=%d C=%d: worst err/bound forward %.3f backward %.3f" % (S, C, fwd, bwd))
    assert fwd <= 1.0 and bwd <= 1.0
    assert r["flag"] == 0 and flag == UNTOUCHED and bool((counts == UNTOUCHED).all())
    out = torch.full((N, C * S, S, S), float("nan"), device="cuda")
    assert lib.gz_rigid_resample_views_fwd(_p(vs), _p(r["minv_d"]), _p(out), N, 1, C, S, _stream()) == GZ_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- the multi-view kernel away from S = 16 --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def multi_view_case():
    F = _gpu()[0]
    B, V, C, S = 3, 5, 6, 8
    rng = np.random.RandomState(8)
    view = np.zeros((B * V, 6))           # any azimuth / elevation, zoom, shifts, as tests/test_figures_gpu.py draws them
    view[:, 0] = rng.uniform(0, 2 * np.pi, B * V)
    view[:, 1] = rng.uniform(-1.2, 1.2, B * V)
    view[:, 2] = rng.uniform(0.7, 1.3, B * V)
    view[:, 3:] = rng.uniform(-1.5, 1.5, (B * V, 3))
    view[0] = (0, 0, 1, 0, 0, 0)
    view[1, :2] = (270 * DEG, 90 * DEG)
    vox = rnd(B, C, S, S, S, seed=88)
    rep = vox.repeat_interleave(V, 0).contiguous()
    ref = Ref(view, S, rep)
    vox_d, rep_d, minv_d = vox.cuda(), rep.cuda(), ref.minv.cuda()
    assert_indices(ref, rep_d, minv_d)
    got = F.rigid_resample_views(vox_d, minv_d)
    assert got.shape == (B * V, C * S, S, S)
    return ref, got, F.rigid_resample(rep_d, minv_d)


def test_values_multi_view_kernel_at_s8():
    ref, got, _ = multi_view_case()
    ratio = worst(got, ref.fwd, ref.fwd_bound)
    print("multi-view B=3 V=5 C=6 S=8: worst err/bound %.3f" % ratio)
    assert ratio <= 1.0


def test_multi_view_kernel_is_bit_equal_to_the_staged_kernel_at_s8():
    _, got, single = multi_view_case()
    assert torch.equal(got, single)


# ---- the experiment forms, once --------------------------------------------------------------------------------------

EXPERIMENTS = [
    ({"GZ_NO_RESAMPLE_SWIZZLE": "1"}, "test_values"),
    ({"GZ_RESAMPLE_FWD_DIRECT": "1", "GZ_RESAMPLE_BWD": "2"}, "test_values"),
    ({"GZ_RESAMPLE_BWD": "1"}, "test_values and not S20"),
]


def test_experiment_forms_hold_the_same_bounds():
    """The value tests of this file under the forms tools/resample_ab.sh compares: plain LDS placement, the direct
    forward with the direct gather, the LDS-atomic scatter (two volumes in 64 KiB of LDS: it returns
    GZ_ERR_UNSUPPORTED above S = 16, so the S = 20 cases are deselected for it).  The switches are read once per
    process, hence one child process per setting, one after another; the first that does not pass ends the test."""
    for knobs, select in EXPERIMENTS:
        env = dict(os.environ, GZ_EXPERIMENTS="1", **knobs)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-s",
                            "-p", "no:cacheprovider", "-k", select], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        print(knobs, r.stdout[-1500:])
        assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, (knobs, r.stdout[-3000:])

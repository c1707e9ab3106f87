"""Precision / recall / density / coverage at the evaluation's real sizes: eval.knn_radii_device and eval.prdc_device
(csrc/gz_prdc.hip) against two things that are not the code under test -- the host yardstick eval.prdc (numpy fp64 on
direct differences) and the fp64 MFMA floor of each walk.

    python tools/prdc_bench.py [--n 5000 50000] [--d 2048] [--k 5] [--host-n 1000] [--reps 5] [--out prdc_bench.json]

Per ``n`` (rows per side), with the codes resident: ``radii_ms`` (one gz_knn_radii call: the n x n walk) and ``counts_ms``
(one gz_prdc_counts call: the n x n cross walk) by HIP events, median of ``--reps`` after two warm-up calls;
``prdc_device_s``: eval.prdc_device end to end with the real set's radii kept (what an epoch pays: one radii walk, the
cross walk, the 32-byte copy back).  The floor of a walk is ``2 n_rows n_cols d / PEAK`` with PEAK = 78.6 TFLOP/s, AMD's
published fp64 matrix rate of the MI355X (256 CUs x 4 SIMDs x 32 FLOP / clk x 2.4 GHz: half the fp32 matrix rate);
``*_of_floor`` is floor / measured.  gz_knn_radii walks all n x n tiles, not the upper triangle: its floor counts them
all.  ``--host-n``: the yardstick is timed once at that many rows per side (0: not at all; a size of its own unless
``--n`` lists it -- the yardstick's three n x n x d passes over direct differences take minutes at n = 5000 on one
core, which is why the default is 1000), the device's integers are compared with it, and the worst
|device - yardstick| / bound of radii and nearest distances is reported (tests/prdc_support.py has the bound).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lightning_gan_zoo_amd import eval as E               # noqa: E402
from lightning_gan_zoo_amd import functional as F         # noqa: E402
from lightning_gan_zoo_amd._lib import check, lib         # noqa: E402

PEAK_FP64_MFMA = 78.6e12


def codes(n, d, seed, shift):
    """Pool-feature-like codes of low intrinsic dimension: a rank-16 non-negative mix plus small noise, fp32-valued."""
    rng = np.random.RandomState(seed)
    z = np.abs(rng.randn(n, 16) + shift)
    mix = np.abs(np.random.RandomState(99).randn(16, d)) / 4
    return (z.dot(mix) + 0.02 * np.abs(rng.randn(n, d))).astype(np.float32).astype(np.float64)


def events(call, reps):
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def one(n, d, k, reps, host):
    g_host, r_host = codes(n, d, 1, 0.15), codes(n, d, 2, 0.0)
    g, r = E.device_codes(g_host, "cuda"), E.device_codes(r_host, "cuda")
    radii = torch.empty((n,), dtype=torch.float64, device="cuda")
    ws_bytes = lib.gz_knn_radii_workspace_bytes(n, d, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    radii_ms = events(lambda: check(lib.gz_knn_radii(F._p(r), n, d, k, F._p(radii), F._p(ws), ws_bytes, F._stream()),
                                    "knn_radii"), reps)
    rad_r, rad_g = E.knn_radii_device(r, k), E.knn_radii_device(g, k)
    in_real = torch.empty((n,), dtype=torch.int32, device="cuda")
    in_fake = torch.empty((n,), dtype=torch.int32, device="cuda")
    near = torch.empty((n,), dtype=torch.float64, device="cuda")
    totals = torch.empty((4,), dtype=torch.int64, device="cuda")
    cbytes = lib.gz_prdc_counts_workspace_bytes(n, n, d)
    cws = torch.empty(max(cbytes, 8), dtype=torch.uint8, device="cuda")
    counts_ms = events(lambda: check(lib.gz_prdc_counts(F._p(g), n, F._p(rad_g), F._p(r), n, F._p(rad_r), d, F._p(in_real),
                                                        F._p(in_fake), F._p(near), F._p(totals), F._p(cws), cbytes,
                                                        F._stream()), "prdc_counts"), reps)
    E.prdc_device(g, r, k=k, rad_r=rad_r), E.prdc_device(g, r, k=k, rad_r=rad_r)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev = E.prdc_device(g, r, k=k, rad_r=rad_r)           # (synchronised by the copy back of the totals)
        times.append(time.perf_counter() - t0)
    groups, slices = ctypes.c_int(), ctypes.c_int()
    lib.gz_prdc_plan(n, n, ctypes.byref(groups), ctypes.byref(slices))
    floor_ms = 2.0 * n * n * d / PEAK_FP64_MFMA * 1e3
    rec = {"n": n, "d": d, "k": k, "radii_ms": round(radii_ms, 3), "counts_ms": round(counts_ms, 3),
           "floor_ms": round(floor_ms, 3), "radii_of_floor": round(floor_ms / radii_ms, 3),
           "counts_of_floor": round(floor_ms / counts_ms, 3), "prdc_device_s": round(float(np.median(times)), 4),
           "row_groups": groups.value, "col_slices": slices.value,
           "radii_workspace_mb": round(ws_bytes / 2 ** 20, 2), "counts_workspace_mb": round(cbytes / 2 ** 20, 2)}
    rec.update((key, round(dev[key], 6)) for key in ("precision", "recall", "density", "coverage"))
    if host:
        from prdc_support import near_bound, radii_bound
        t0 = time.perf_counter()
        want = E.prdc(g_host, r_host, k=k)
        rec["host_s"] = round(time.perf_counter() - t0, 2)
        rec["host_over_device"] = round(rec["host_s"] / (rec["prdc_device_s"] + radii_ms * 1e-3), 1)
        rec["counts_equal"] = bool(np.array_equal(dev["in_real"].cpu().numpy(), want["in_real"])
                                   and np.array_equal(dev["in_fake"].cpu().numpy(), want["in_fake"]))
        rec["metrics_equal"] = all(dev[key] == want[key] for key in ("precision", "recall", "density", "coverage"))
        rec["radii_worst_over_bound"] = float(max(
            (np.abs(dev["rad_g"].cpu().numpy() - want["rad_g"]) / radii_bound(g_host, want["rad_g"])).max(),
            (np.abs(dev["rad_r"].cpu().numpy() - want["rad_r"]) / radii_bound(r_host, want["rad_r"])).max()))
        rec["near_worst_over_bound"] = float(
            (np.abs(dev["near"].cpu().numpy() - want["near"]) / near_bound(g_host, r_host, want["near"])).max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[5000, 50000])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for n in ([a.host_n] if a.host_n and a.host_n not in a.n else []) + a.n:
        lines.append(json.dumps(one(n, a.d, a.k, a.reps, host=(n == a.host_n))))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

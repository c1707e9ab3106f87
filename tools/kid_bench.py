"""KID at the evaluation's real size, host against device: eval.polynomial_mmd_averages (numpy fp64 GEMMs, 16 BLAS
threads) against eval.polynomial_mmd_averages_device (csrc/gz_kid.hip) on the same codes, the same subsets.

    python tools/kid_bench.py [--subsets 100] [--m 1000] [--d 2048] [--rows 5000] [--host-subsets 100] [--reps 5]
                              [--out kid_bench.json]

The device time is end to end -- subset draw, index upload, the two launches, the copy back of the sums, the estimator's
formula on the host -- with the codes already resident (the evaluator uploads the real codes once per run; the upload is
timed separately as ``upload_ms``): two warm-up calls, then the median of ``--reps`` calls, each device-synchronised by
its copy back.  The kernel's own time comes from HIP events around the launch sequence (median of ``--reps``); its
TFLOP/s counts the four products the kernel executes (GG, RR, GR and RG: 4/3 of the three the estimator needs).
``--host-subsets`` below ``--subsets`` times fewer subsets on the host and scales (the loop is linear in them).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")           # before numpy loads its BLAS
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")

import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightning_gan_zoo_amd import eval as E               # noqa: E402
from lightning_gan_zoo_amd import functional as F         # noqa: E402
from lightning_gan_zoo_amd._lib import check, lib         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--host-subsets", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    S, m, d, n = a.subsets, min(a.m, a.rows), a.d, a.rows
    rng = np.random.RandomState(0)
    # pool-feature-like codes: non-negative, fp32-valued
    real = np.abs(rng.randn(n, d)).astype(np.float32).astype(np.float64) * 0.5
    fake = np.abs(rng.randn(n, d) + 0.05).astype(np.float32).astype(np.float64) * 0.5

    t0 = time.perf_counter()
    g, r = E.device_codes(real, "cuda"), E.device_codes(fake, "cuda")
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3

    def device():
        np.random.seed(1)
        return E.polynomial_mmd_averages_device(g, r, n_subsets=S, subset_size=m)

    device(), device()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dev = device()
        times.append(time.perf_counter() - t0)
    device_s = float(np.median(times))

    # the launch sequence alone, by HIP events
    np.random.seed(1)
    idx = torch.from_numpy(E.draw_kid_subsets(n, n, S, m)).cuda()
    out = torch.empty((S, 6 * m + 3), dtype=torch.float64, device="cuda")
    ws_bytes = lib.gz_kid_workspace_bytes(S, m, d)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    kernel_ms = []
    for i in range(a.reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib.gz_kid_sums(F._p(g), n, F._p(r), n, d, F._p(idx), S, m, 1.0 / d, 1.0, 3, F._p(out), F._p(ws), ws_bytes,
                              F._stream()), "kid_sums")
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            kernel_ms.append(e0.elapsed_time(e1))
    kernel_ms = float(np.median(kernel_ms))
    flop = 2.0 * S * 4 * m * m * d

    hs = min(a.host_subsets or S, S)
    np.random.seed(1)
    t0 = time.perf_counter()
    host = E.polynomial_mmd_averages(real, fake, n_subsets=hs, subset_size=m)
    host_s = (time.perf_counter() - t0) * S / hs

    rec = {"S": S, "m": m, "d": d, "rows": n, "blas_threads": int(os.environ["OMP_NUM_THREADS"]),
           "host_s": round(host_s, 3), "host_subsets_timed": hs, "device_s": round(device_s, 4),
           "host_over_device": round(host_s / device_s, 1), "upload_ms": round(upload_ms, 2),
           "kernel_ms": round(kernel_ms, 3), "kernel_fp64_tflops": round(flop / kernel_ms / 1e9, 2),
           "max_rel_diff_mmd2": float(np.max(np.abs(dev[0][:hs] - host[0]) / np.abs(host[0]))),
           "max_rel_diff_var": float(np.max(np.abs(dev[1][:hs] - host[1]) / np.abs(host[1])))}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Time to draw each experiment's figure set (core/figures/types.py) on one GPU: the batched rendering against the
reference-shaped one (one generator call per frame / column, one grid per frame) built from the same kernels.

    python tools/figures_bench.py [--expts dc_gan,hologan] [--reps 3] [--out figures_bench.json]
    python tools/figures_bench.py --resample B V [--reps 20]     # kernel (a) vs V launches of the single-view one
                                                                 # (run under rocprofv3 --kernel-trace --stats)

Each figure is planned once (host draws, seeded) and rendered with both paths: one warm-up, then ``--reps`` timed
repetitions each, device-synchronised.  Reference widths (features 64), eval mode, no_grad; what is timed is render
(GPU work and the copies of the frames to the host), not the plan or the file writes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightning_gan_zoo_amd import functional as F                     # noqa: E402
from lightning_gan_zoo_amd.config import locate, make_cfg              # noqa: E402
from lightning_gan_zoo_amd.core.figures import types as T             # noqa: E402
from lightning_gan_zoo_amd.core.models.hologan_generator import view_inverse_matrices   # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def bench_expt(expt, reps, tmp):
    cfg = make_cfg(expt)
    torch.manual_seed(0)
    np.random.seed(0)
    module = locate(cfg.model.lm["_target_"])(cfg, logging_dir=tmp).cuda().eval()
    rec = {"figures": {}}
    with torch.no_grad():
        for fig in T.build_figures(cfg, module, tmp):
            plan = fig.plan(module)
            b = timed(lambda: fig.render(module, plan)[1].cpu(), reps)
            r = timed(lambda: fig.render_per_frame(module, plan)[1].cpu(), reps)
            rec["figures"][type(fig).__name__] = {"batched_ms": round(b, 2), "per_frame_ms": round(r, 2),
                                                  "speedup": round(r / b, 2)}
    rec["batched_ms"] = round(sum(f["batched_ms"] for f in rec["figures"].values()), 2)
    rec["per_frame_ms"] = round(sum(f["per_frame_ms"] for f in rec["figures"].values()), 2)
    rec["speedup"] = round(rec["per_frame_ms"] / rec["batched_ms"], 2)
    return rec


def bench_resample(B, V, reps):
    S, C = 16, 64
    vox = torch.randn(B, C, S, S, S, device="cuda")
    views = np.zeros((B * V, 6))
    views[:, 0] = np.repeat(np.linspace(220, 320, V)[None], B, 0).reshape(-1) * np.pi / 180
    views[:, 1], views[:, 2] = np.pi / 2, 1.0
    minv = view_inverse_matrices(views).reshape(B * V, 16).contiguous().cuda()
    per_view = [minv.reshape(B, V, 16)[:, v].contiguous() for v in range(V)]
    multi = timed(lambda: [F.rigid_resample_views(vox, minv) for _ in range(reps)], 1) / reps
    single = timed(lambda: [[F.rigid_resample(vox, m) for m in per_view] for _ in range(reps)], 1) / reps
    out_bytes = B * V * C * S ** 3 * 4
    return {"B": B, "V": V, "C": C, "S": S, "multi_view_ms": round(multi, 4), "single_view_x_V_ms": round(single, 4),
            "multi_view_write_TBps": round(out_bytes / multi / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expts", default="dc_gan,wgan,wgan_gp,gan_stability_r1,hologan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resample", nargs=2, type=int, metavar=("B", "V"))
    ap.add_argument("--out")
    ap.add_argument("--tmp", help="directory the figures' constructors create theirs in (default: a fresh temporary one)")
    a = ap.parse_args()
    if a.resample:
        rec = bench_resample(a.resample[0], a.resample[1], max(a.reps, 20))
    else:
        import tempfile
        tmp = a.tmp or tempfile.mkdtemp()
        rec = {e: bench_expt(e, a.reps, tmp) for e in a.expts.split(",")}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

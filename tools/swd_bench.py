"""What the sliced Wasserstein distance (eval.swd_device, csrc/gz_swd.hip) costs on one GPU.

    python tools/swd_bench.py [--out profiles/swd_bench.json] [--images 16384] [--sizes 64,128]

  kernels:<S>   at the runner's default size (swd_images x 3 x S x S, 128 patches, 4 x 128 directions): milliseconds between
                two HIP events around each launcher -- gz_swd_pyramid once, then per level gz_swd_channel_stats,
                gz_swd_project, gz_swd_sort_columns and gz_swd_distance -- median of ``--rounds`` calls after one warm-up.
                Beside the sort: its block and global passes, the bytes they move (every pass reads and writes every key
                of every column) per second, and a device-to-device copy of the projection buffer (as many bytes read and
                written as ONE pass) in the same process.
  whole:<S>     eval.swd_device on two such sets, wall clock around a device synchronise, three calls (``seconds``: their
                median; the first also pays for the allocator's first large blocks).
  yardstick     eval.swd in numpy and eval.swd_device at one REDUCED size (stated in the entry), wall clock; and the
                yardstick's time at the default size EXTRAPOLATED from it by the ratio of rows x directions x log2(rows)
                (its sort) -- labelled so, never measured.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median_ms(fn, rounds):
    import numpy as np
    fn()
    return round(float(np.median([event_ms(fn) for _ in range(rounds)])), 4)


def kernels(size, images, rounds, patches=128, dirs=128, repeats=4):
    import torch
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    plan = E.SwdPlan(size, 3, images, patches=patches, dirs=dirs, repeats=repeats, seed=0)
    x = torch.randn(images, 3, size, size, device="cuda")
    out = {"images": images, "patches": patches, "directions": repeats * dirs,
           "pyramid_ms": median_ms(lambda: E.laplacian_pyramid_device(x), rounds),
           "pyramid_bytes": int(x.numel() * 4 * (1 + sum(4.0 ** -l for l in range(len(plan.sizes))))), "levels": {}}
    out["pyramid_TBps"] = round(out["pyramid_bytes"] / out["pyramid_ms"] / 1e9, 3)
    levels = E.laplacian_pyramid_device(x)
    del x
    pos, directions = plan.on("cuda")
    rows = images * patches
    block, padded, block_passes, global_passes = E.swd_sort_plan(rows)
    pitch = max(padded, 4)
    ndirs = repeats * dirs
    for l, level in enumerate(levels):
        n, c, h, _ = level.shape
        stats = torch.empty((2 * c,), dtype=torch.float64, device="cuda")
        ws_bytes = lib.gz_swd_channel_stats_workspace_bytes(n, c, h, patches)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
        proj = torch.empty((ndirs, pitch), dtype=torch.float32, device="cuda")
        other = torch.empty_like(proj)

        def stats_call():
            check(lib.gz_swd_channel_stats(F._p(level), n, c, h, F._p(pos[l]), patches, F._p(stats), F._p(ws), ws_bytes,
                                           F._stream()), "stats")

        def project_call():
            check(lib.gz_swd_project(F._p(level), n, c, h, F._p(pos[l]), patches, F._p(stats), F._p(directions[l]), ndirs,
                                     F._p(proj), pitch, F._stream()), "project")

        def sort_call():
            check(lib.gz_swd_sort_columns(F._p(proj), rows, ndirs, pitch, F._stream()), "sort")

        entry = {"size": h, "stats_ms": median_ms(stats_call, rounds), "project_ms": median_ms(project_call, rounds)}
        # the sort is timed on fresh projections every time (a sorted input is not the evaluation's input)
        times = []
        for _ in range(rounds + 1):
            project_call()
            times.append(event_ms(sort_call))
        entry["sort_ms"] = round(sorted(times[1:])[len(times[1:]) // 2], 4)
        moved = 2 * 4 * ndirs * padded * (block_passes + global_passes)
        entry.update(sort_block_passes=block_passes, sort_global_passes=global_passes, sort_bytes=moved,
                     sort_TBps=round(moved / entry["sort_ms"] / 1e9, 3))
        entry["copy_ms"] = median_ms(lambda: other.copy_(proj), rounds)
        entry["copy_TBps"] = round(2 * 4 * ndirs * pitch / entry["copy_ms"] / 1e9, 3)
        entry["sort_over_one_copy_per_pass"] = round(entry["sort_ms"] / (entry["copy_ms"] * (block_passes + global_passes)), 3)
        dws_bytes = lib.gz_swd_distance_workspace_bytes(rows, dirs, repeats)
        dws = torch.empty(max(dws_bytes, 8), dtype=torch.uint8, device="cuda")
        dist = torch.empty((repeats,), dtype=torch.float64, device="cuda")
        other.copy_(proj)
        entry["distance_ms"] = median_ms(lambda: check(lib.gz_swd_distance(
            F._p(proj), rows, F._p(other), rows, dirs, repeats, pitch, F._p(dist), F._p(dws), dws_bytes, F._stream()),
            "distance"), rounds)
        out["levels"]["swd_%d" % h] = entry
        del proj, other
    return out


def whole(size, images, patches=128, dirs=128, repeats=4):
    import torch
    from lightning_gan_zoo_amd import eval as E
    plan = E.SwdPlan(size, 3, images, patches=patches, dirs=dirs, repeats=repeats, seed=0)
    a, b = torch.randn(images, 3, size, size, device="cuda"), torch.rand(images, 3, size, size, device="cuda")
    E.swd_device(a[:64], b[:64], [p[:64] for p in plan.positions], plan.directions, repeats)        # code objects loaded
    seconds = []
    for _ in range(3):           # the first call also pays for the allocator's first 4 GB blocks; every call is reported
        torch.cuda.synchronize()
        t0 = time.time()
        result = E.swd_device(a, b, plan.positions, plan.directions, repeats)
        torch.cuda.synchronize()
        seconds.append(round(time.time() - t0, 3))
    return {"images": images, "seconds_each_call": seconds, "seconds": sorted(seconds)[1],
            "result": {k: round(v, 3) for k, v in result.items()}}


def yardstick(full_images, size=64, images=512, patches=64, dirs=64, repeats=2):
    import numpy as np
    import torch
    from lightning_gan_zoo_amd import eval as E
    plan = E.SwdPlan(size, 3, images, patches=patches, dirs=dirs, repeats=repeats, seed=0)
    rng = np.random.RandomState(0)
    a, b = rng.randn(images, 3, size, size).astype(np.float32), rng.rand(images, 3, size, size).astype(np.float32)
    t0 = time.time()
    host = E.swd(a, b, plan.positions, plan.directions, repeats)
    host_s = time.time() - t0
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    E.swd_device(da, db, plan.positions, plan.directions, repeats)
    torch.cuda.synchronize()
    t0 = time.time()
    dev = E.swd_device(da, db, plan.positions, plan.directions, repeats)
    torch.cuda.synchronize()
    dev_s = time.time() - t0
    rows, full_rows = images * patches, full_images * 128
    factor = (full_rows * 512 * math.log2(full_rows)) / (rows * repeats * dirs * math.log2(rows))
    return {"reduced_size": {"S": size, "images": images, "patches": patches, "directions": repeats * dirs},
            "numpy_seconds": round(host_s, 3), "device_seconds": round(dev_s, 4),
            "largest_relative_difference": float(max(abs(dev[k] - host[k]) / host[k] for k in host)),
            "numpy_seconds_at_default_size": {"extrapolated": True, "not_measured": True, "S": size, "images": full_images,
                                              "by": "rows x directions x log2(rows)", "factor": round(factor, 1),
                                              "seconds": round(host_s * factor, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swd_bench.json"))
    ap.add_argument("--images", type=int, default=16384)
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/swd_bench.py measures on the GPU; there is none here (nothing is estimated instead)")
    result = {"device": torch.cuda.get_device_name(0)}
    for size in (int(s) for s in args.sizes.split(",")):
        result["kernels:%d" % size] = kernels(size, args.images, args.rounds)
        torch.cuda.empty_cache()
        result["whole:%d" % size] = whole(size, args.images)
        torch.cuda.empty_cache()
        print(json.dumps({k: result[k] for k in ("kernels:%d" % size, "whole:%d" % size)}), flush=True)
    result["yardstick"] = yardstick(args.images)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result["yardstick"]))


if __name__ == "__main__":
    main()

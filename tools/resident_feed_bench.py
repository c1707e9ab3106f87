"""Feed comparison for the resident training set (resident_data.py): ms per dc_gan optimizer cycle with the batches
coming from (a) SyntheticImages, (b) ResidentImages, (c) ImageFolderImages over one generated folder of CelebA-sized
(178x218) JPEGs, on ONE trainer, the feeds taking turns inside every repetition so that clock drift hits them alike.
Also: build time of the set with 1 worker and with the pool, cache write / load / upload times.

    python tools/resident_feed_bench.py [--images 4096] [--batch 128] [--size 64] [--steps 200] [--reps 3]
    python tools/resident_feed_bench.py --kernel-only      # the gather launches alone, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/resident_feed_bench.py --kernel-only
    python tools/resident_feed_bench.py --trace-csv <dir>/.../*_kernel_trace.csv     # gather time per launch shape

Prints one JSON line per result.
"""
import argparse
import csv
import gc
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_jpeg_folder(root, count, seed=0):
    """``count`` 178x218 JPEGs (CelebA's size) in two class folders: smooth random fields plus grain, so that the
    decoder has a picture's work to do."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for c in ("a", "b"):
        os.makedirs(os.path.join(root, c), exist_ok=True)
    for i in range(count):
        low = Image.fromarray(rng.randint(0, 256, size=(7, 6, 3), dtype=np.uint8)).resize((178, 218), Image.BICUBIC)
        img = np.asarray(low, dtype=np.int16) + rng.randint(-12, 13, size=(218, 178, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(
            os.path.join(root, "ab"[i % 2], "%06d.jpg" % i), quality=90)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def host_figures(root, size, cache, emit):
    from lightning_gan_zoo_amd import resident_data as RD
    source = RD.image_folder_source(root, size, 3)
    n = len(source["items"])
    one, t1 = timed(lambda: RD.build_set(source, size, 3, workers=1))
    pool, tp = timed(lambda: RD.build_set(source, size, 3))
    assert one.tobytes() == pool.tobytes()
    emit({"what": "build_set", "images": n, "size": size, "workers_pool": RD.pool_workers(),
          "seconds_1_worker": round(t1, 3), "seconds_pool": round(tp, 3),
          "images_per_s_1_worker": round(n / t1, 1), "images_per_s_pool": round(n / tp, 1),
          "scaling": round(t1 / tp, 2)})
    digest = RD.set_digest(source, size, 3)
    _, tw = timed(lambda: RD.save_cache(cache, digest, pool, source["labels"], source["classes"], source, size, 3))
    hit, tl = timed(lambda: RD.load_cache(cache, digest, pool.shape))
    emit({"what": "cache", "bytes": int(pool.nbytes), "write_seconds": round(tw, 4), "open_seconds": round(tl, 4)})
    return hit[0]


def feed_figures(args, root, cache, emit):
    import torch
    from bench import build_trainer
    from lightning_gan_zoo_amd.resident_data import ResidentImages, upload
    from lightning_gan_zoo_amd.run_network import ImageFolderImages, SyntheticImages
    device = torch.device("cuda", 0)
    mapped = host_figures(root, args.size, cache, emit)
    torch.cuda.synchronize()
    _, tu = timed(lambda: (upload(mapped, device), torch.cuda.synchronize()))
    emit({"what": "upload_from_cache_file", "bytes": int(mapped.size), "seconds": round(tu, 4)})
    module, trainer = build_trainer("dc_gan", args.batch, device, 1, img_size=args.size)
    feeds = {
        "synthetic": iter(SyntheticImages(args.batch, 3, args.size, device, 1234)),
        "resident": iter(ResidentImages(root, args.batch, args.size, 3, 0.5, 0.5, device, cache_dir=cache)),
        "image_folder": iter(ImageFolderImages(root, args.batch, args.size, 3, 0.5, 0.5, device)),
    }
    per_pair = len(trainer.order)
    full = lambda b: len(b[0]) == args.batch      # noqa: E731  (the partial last batch would change the step's shapes)

    def run(name, cycles):
        it, k = feeds[name], 0
        while k < cycles * per_pair:
            b = next(it)
            if full(b):
                trainer.step(b)
                k += 1
        trainer.finish()

    for name in feeds:
        run(name, args.warmup)
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    cycles = {"synthetic": args.steps, "resident": args.steps, "image_folder": max(4, args.steps // 10)}
    times = {name: [] for name in feeds}
    for _ in range(args.reps):
        for name in feeds:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, cycles[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / cycles[name] * 1e3)
    med = {name: sorted(v)[len(v) // 2] for name, v in times.items()}
    emit({"what": "ms_per_step", "expt": "dc_gan", "batch": args.batch, "size": args.size, "cycles": cycles,
          "ms_per_step": {k: round(v, 3) for k, v in med.items()},
          "each": {k: [round(x, 3) for x in v] for k, v in times.items()},
          "resident_vs_synthetic": round(med["resident"] / med["synthetic"], 4),
          "image_folder_vs_synthetic": round(med["image_folder"] / med["synthetic"], 2)})


KERNEL_SHAPES = ((128, 64), (64, 128))          # (batch, image side), 3 channels


def kernel_only(emit, launches=200, rows=4096):
    """The gather alone at the two launch shapes, back to back: for a kernel trace, and timed with events as a
    cross-check (launch gaps included)."""
    import torch
    from lightning_gan_zoo_amd import functional as F
    for batch, side in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(side)
        set_u8 = torch.randint(0, 256, (rows, side, side, 3), dtype=torch.uint8, generator=g).cuda()
        labels = torch.zeros(rows, dtype=torch.int64, device="cuda")
        order = torch.randperm(rows, generator=g).cuda()
        views = [order[(i * batch) % (rows - batch):][:batch] for i in range(launches)]
        for v in views[:10]:
            F.gather_normalize_u8(set_u8, v, 0.5, 0.5, labels)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for v in views:
            F.gather_normalize_u8(set_u8, v, 0.5, 0.5, labels)
        end.record()
        torch.cuda.synchronize()
        emit({"what": "gather_back_to_back", "batch": batch, "side": side, "launches": launches,
              "us_per_launch_with_gaps": round(start.elapsed_time(end) / launches * 1e3, 2),
              "bytes_in": batch * side * side * 3, "bytes_out": batch * side * side * 3 * 4})


def trace_figures(path, emit):
    """Per launch shape, the gather kernel's own duration from a rocprofv3 kernel-trace CSV."""
    by_grid = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if "u8hwc_gather" not in row["Kernel_Name"]:
                continue
            key = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
            by_grid.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for batch, side in KERNEL_SHAPES:
        threads = batch * side * side // 4
        ns = sorted(by_grid.get(threads, []))
        if not ns:
            emit({"what": "gather_kernel_trace", "batch": batch, "side": side, "error": "no launches with %d threads"
                  % threads, "grids_seen": sorted(by_grid)})
            continue
        moved = batch * side * side * 3 * 5
        emit({"what": "gather_kernel_trace", "batch": batch, "side": side, "launches": len(ns),
              "us_median": round(ns[len(ns) // 2] / 1e3, 2), "us_min": round(ns[0] / 1e3, 2),
              "us_mean": round(sum(ns) / len(ns) / 1e3, 2), "hbm_bytes": moved,
              "tb_per_s_at_median": round(moved / ns[len(ns) // 2] / 1e3, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace-csv")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.trace_csv:
        return trace_figures(args.trace_csv, emit)
    if args.kernel_only:
        return kernel_only(emit)
    work = tempfile.mkdtemp(prefix="resident_feed_")
    try:
        root, cache = os.path.join(work, "data"), os.path.join(work, "cache")
        _, tg = timed(lambda: make_jpeg_folder(root, args.images))
        emit({"what": "generated_folder", "images": args.images, "seconds": round(tg, 2)})
        feed_figures(args, root, cache, emit)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()

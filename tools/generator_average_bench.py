"""What generator weight averaging (averaging.GeneratorAverage, csrc/gz_ema.hip) costs on one GPU.

    python tools/generator_average_bench.py [--configs dc_gan:128,gan_stability_r1:64] [--pairs 40] [--rounds 5]
                                            [--out generator_average_bench.json]

Per configuration (reference widths, synthetic batch):
  * the update alone: ``--launches`` back-to-back launches between two HIP events, after a warm-up that also brings the
    clocks up; the achieved rate counts 12 bytes per parameter (read avg, read src, write avg).  Back-to-back updates of
    a generator that fits the 256 MiB Infinity Cache re-read what the previous launch left there: that figure is the
    cache-resident rate, named as such.  ``update_cold_us`` times the update behind a pass over a buffer larger than
    the cache, one launch per sample, which is what a training step sees;
  * harness.Trainer ms per D+G pair with the average off and on: two trainers built from the same seed, timed in
    alternating blocks of ``--pairs`` pairs (HIP events around a block, device-synchronised), ``--rounds`` blocks each;
    median and min..max over the blocks are reported, so the difference can be read against the spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightning_gan_zoo_amd.averaging import GeneratorAverage              # noqa: E402
from lightning_gan_zoo_amd.config import locate, make_cfg                  # noqa: E402
from lightning_gan_zoo_amd.harness import Trainer                          # noqa: E402


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


NATIVE_IMG_SIZE = {"gan_stability_r1": 128}      # conf/expt/gan_stability_r1.yaml; every other experiment: 64


def build(expt, bs, averaged):
    cfg = make_cfg(expt, batch_size=bs, img_size=NATIVE_IMG_SIZE.get(expt, 64))
    torch.manual_seed(0)
    np.random.seed(0)
    module = locate(cfg.model.lm["_target_"])(cfg, None).cuda()
    avg = GeneratorAverage(module.generator, beta=0.999) if averaged else None
    t = cfg.train
    g = torch.Generator().manual_seed(1)
    real = (torch.rand(bs, t.channels_img, t.img_size, t.img_size, generator=g) * 2 - 1).cuda()
    batch = (real, torch.zeros(bs, dtype=torch.int64, device="cuda"))
    return module, Trainer(module, generator_average=avg), avg, batch


def run_pairs(trainer, batch, pairs):
    for _ in range(pairs * len(trainer.order)):
        trainer.step(batch)


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4),
            "n": len(xs)}


def bench(expt, bs, pairs, rounds, launches):
    _, tr_off, _, batch = build(expt, bs, False)
    _, tr_on, avg, _ = build(expt, bs, True)
    for tr in (tr_off, tr_on):                       # warm-up: allocator, lazy optimizer state, pack tables, clocks
        run_pairs(tr, batch, max(10, pairs // 2))
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(rounds):                          # alternate, so that drift hits both alike
        off.append(event_ms(lambda: run_pairs(tr_off, batch, pairs)) / pairs)
        on.append(event_ms(lambda: run_pairs(tr_on, batch, pairs)) / pairs)
    nparams = sum(p.numel() for p in avg.shadow.parameters())
    nbytes = 12 * nparams
    for _ in range(20):
        avg.update()
    hot = [event_ms(lambda: [avg.update() for _ in range(launches)]) / launches * 1e3 for _ in range(rounds)]
    flush = torch.empty(320 << 20, dtype=torch.uint8, device="cuda")      # larger than the 256 MiB Infinity Cache
    cold = []
    for _ in range(max(rounds, 10)):
        flush.add_(1)
        cold.append(event_ms(avg.update) * 1e3)
    hot_us, cold_us = float(np.median(hot)), float(np.median(cold))
    return {"expt": expt, "batch_size": bs, "generator_parameters": nparams, "tensors": len(avg.names),
            "bytes_per_update": nbytes,
            "update_back_to_back_us": spread(hot), "update_back_to_back_TBps": round(nbytes / hot_us / 1e6, 3),
            "update_cold_us": spread(cold), "update_cold_TBps": round(nbytes / cold_us / 1e6, 3),
            "pair_ms_average_off": spread(off), "pair_ms_average_on": spread(on),
            "pair_ms_delta_of_medians": round(float(np.median(on) - np.median(off)), 4),
            "pairs_per_block": pairs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="dc_gan:128,gan_stability_r1:64")
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    rec = {}
    for item in a.configs.split(","):
        expt, bs = item.split(":")
        rec["%s_bs%s" % (expt, bs)] = bench(expt, int(bs), a.pairs, a.rounds, a.launches)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

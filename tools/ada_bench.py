"""What the gated DiffAugment launch and the ADA controller (augment.AdaptiveAugment, csrc/gz_ada.hip) cost on one GPU.

    python tools/ada_bench.py [--out profiles/ada_bench.json] [--limit 240]

The protocol is tools/diffaugment_bench.py's: every section in a child process of its own under its own time limit,
``hot`` (back-to-back launches between two HIP events) and ``cold`` (one launch behind a pass over a buffer larger than
the Infinity Cache) medians with their min / max, nothing more started after a child that fails or runs out of time.

  kernel:<C>x<H>x<W>   at R = 128 from one source and R = 256 stacked from two, full policy, modes 0 and 2:
                       (a) gz_diffaug (the yardstick: the kernel as it was) against gz_diffaug_gated on the same operands
                           with p = NULL and orientation 0 -- once with blit = 0 (the instantiation without the turning
                           route) and once with blit = 3 (the one that carries it, and its LDS allocation);
                       (b) gz_diffaug_gated, blit = 3, p = NULL, every sample at orientation 0 / 4 (flip only) / 1 (one
                           turn: the LDS route) / n mod 8 (the mixture a run draws).
  step:dc_gan:128      (c) harness.Trainer ms per D+G pair with diffaugment=color,translation,cutout, and with
                           augment_blit=xflip,rot90 ada_target=0.6 on top: two trainers from one seed in alternating
                           blocks, the delta of the medians, and the library launches of one pair counted on the host.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diffaugment_bench import FULL, count_pair, event_ms, hot_and_cold_us, spread      # noqa: E402

SECTIONS = ["kernel:3x64x64", "kernel:3x128x128", "step:dc_gan:128"]
CLASSES = (("o0", lambda n: 0), ("flip", lambda n: 4), ("turn", lambda n: 1), ("mixed", lambda n: n % 8))


def bench_kernel(shape, launches, rounds):
    import torch
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd.augment import DiffAugment
    C, H, W = shape
    aug = DiffAugment(FULL)
    cut = aug.cut(H, W)
    flush = torch.empty(320 << 20, dtype=torch.uint8, device="cuda")      # larger than the 256 MiB Infinity Cache
    rec = {}
    for label, R0, R1 in (("R128", 128, 0), ("R256_stacked", 128, 128)):
        torch.manual_seed(0)
        R = R0 + R1
        x0 = torch.randn(R0, C, H, W, device="cuda")
        x1 = torch.randn(R1, C, H, W, device="cuda") if R1 else None
        p8 = aug.draw(R, H, W)
        params8 = p8.cuda()

        def wide(code):
            p16 = torch.zeros((R, 16))
            p16[:, :8] = p8
            p16[:, 7] = torch.tensor([float(code(n)) for n in range(R)])
            return p16.cuda()

        out = {"bytes": 8 * R * C * H * W}
        for mode, name in ((0, "forward"), (2, "adjoint")):
            m = {}
            m["gz_diffaug"], base_hot, base_cold = hot_and_cold_us(
                lambda: F._diffaug_raw(x0, x1, params8, cut, mode), flush, launches, rounds)
            p16 = wide(lambda n: 0)
            for key, blit in (("gated_o0_blit0", 0), ("gated_o0_blit3", 3)):
                m[key], hot, cold = hot_and_cold_us(
                    lambda: F._diffaug_gated_raw(x0, x1, p16, cut, None, blit, mode), flush, launches, rounds)
                m[key].update({"hot_over_gz_diffaug": round(hot / base_hot, 3),
                               "cold_over_gz_diffaug": round(cold / base_cold, 3)})
            cls = {}
            for key, code in CLASSES:
                pk = wide(code)
                cls[key], hot, cold = hot_and_cold_us(
                    lambda: F._diffaug_gated_raw(x0, x1, pk, cut, None, 3, mode), flush, launches, rounds)
            ref = cls["o0"]
            for key in cls:
                cls[key].update({"hot_over_o0": round(cls[key]["hot_us"]["median"] / ref["hot_us"]["median"], 3),
                                 "cold_over_o0": round(cls[key]["cold_us"]["median"] / ref["cold_us"]["median"], 3)})
            m["classes_blit3"] = cls
            out[name] = m
        rec[label] = out
    return rec


def bench_step(expt, bs, pairs, rounds):
    import numpy as np
    import torch
    from lightning_gan_zoo_amd.augment import AdaptiveAugment, DiffAugment
    from lightning_gan_zoo_amd.config import locate, make_cfg
    from lightning_gan_zoo_amd.harness import Trainer

    def build(**keys):
        cfg = make_cfg(expt, batch_size=bs, img_size=64)
        cfg["diffaugment"] = FULL
        for k, v in keys.items():
            cfg[k] = v
        torch.manual_seed(0)
        np.random.seed(0)
        module = locate(cfg.model.lm["_target_"])(cfg, None).cuda()
        t = cfg.train
        g = torch.Generator().manual_seed(1)
        real = (torch.rand(bs, t.channels_img, t.img_size, t.img_size, generator=g) * 2 - 1).cuda()
        return Trainer(module), (real, torch.zeros(bs, dtype=torch.int64, device="cuda"))

    def run_pairs(trainer, batch, n):
        for _ in range(n * len(trainer.order)):
            trainer.step(batch)

    (tr_base, batch), (tr_ada, _) = build(), build(augment_blit="xflip,rot90", ada_target=0.6)
    assert type(tr_base.module.diffaugment) is DiffAugment and type(tr_ada.module.diffaugment) is AdaptiveAugment
    for tr in (tr_base, tr_ada):
        run_pairs(tr, batch, max(10, pairs // 2))
    torch.cuda.synchronize()
    base, ada = [], []
    for _ in range(rounds):
        base.append(event_ms(lambda: run_pairs(tr_base, batch, pairs)) / pairs)
        ada.append(event_ms(lambda: run_pairs(tr_ada, batch, pairs)) / pairs)
    calls_base, _ = count_pair(tr_base, batch)
    calls_ada, _ = count_pair(tr_ada, batch)
    n_base, n_ada = sum(calls_base.values()), sum(calls_ada.values())
    p, r = tr_ada.module.diffaugment.values()
    return {"expt": expt, "batch_size": bs, "steps_per_pair": len(tr_base.order), "pairs_per_block": pairs,
            "pair_ms_diffaugment": spread(base), "pair_ms_ada": spread(ada),
            "pair_us_delta_of_medians": round(float(np.median(ada) - np.median(base)) * 1e3, 1),
            "ada_over_diffaugment": round(float(np.median(ada) / np.median(base)), 4),
            "library_launches_per_pair": {"diffaugment": n_base, "ada": n_ada, "delta": n_ada - n_base,
                                          **{k: calls_ada.get(k, 0) for k in ("gz_diffaug_gated", "gz_ada_observe",
                                                                              "gz_ada_update")}},
            "p_after": round(p, 6), "r_last": round(r, 4)}


def run_section(name, a):
    kind, rest = name.split(":", 1)
    if kind == "kernel":
        return bench_kernel(tuple(int(v) for v in rest.split("x")), a.launches, a.rounds)
    expt, bs = rest.split(":")
    return bench_step(expt, int(bs), a.pairs, a.rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--section", help="run ONE section in this process and print its record (what the parent starts)")
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per section")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.section:
        print("RECORD " + json.dumps(run_section(a.section, a)))
        return 0
    rec = {}
    for name in a.sections.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--pairs", str(a.pairs), "--rounds",
               str(a.rounds), "--launches", str(a.launches)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("section %s ran out of its %g s: nothing more is started" % (name, a.limit), file=sys.stderr)
            return 3
        line = next((l for l in r.stdout.splitlines() if l.startswith("RECORD ")), None)
        if r.returncode != 0 or line is None:
            print("section %s failed (exit status %d): nothing more is started\n%s"
                  % (name, r.returncode, r.stderr[-3000:]), file=sys.stderr)
            return 2
        rec[name] = json.loads(line[len("RECORD "):])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

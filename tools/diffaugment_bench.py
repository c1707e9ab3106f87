"""What DiffAugment (augment.DiffAugment, csrc/gz_diffaug.hip) costs on one GPU.

    python tools/diffaugment_bench.py [--out profiles/diffaugment_bench.json] [--limit 240]

Every timed section runs in a child process of its own under its own time limit (``--limit`` seconds); after a child
that fails or runs out of time nothing more is started and the exit status is non-zero.

  kernel:<C>x<H>x<W>   gz_diffaug modes 0 (forward) and 2 (adjoint) at R = 128 from one source and at R = 256 stacked from
                       two sources of 128, full policy, against a device-to-device copy of the same bytes (R*C*H*W floats
                       read, as many written) in the same process.  ``hot``: back-to-back launches between two HIP events
                       (operands of <= 100 MB stay in the 256 MiB Infinity Cache, so this is the cache-resident time);
                       ``cold``: one launch behind a pass over a buffer larger than the cache, which is what a training
                       step sees.
  step:<expt>:<bs>     harness.Trainer ms per D+G pair with the policy off and on: two trainers built from the same
                       seed, timed in alternating blocks (generator_average_bench.py's scheme), the delta of the medians
                       in microseconds, and the launches of one pair counted on the host: calls into libgz_hip.so that
                       take a stream, and torch.cat calls (the stacked discriminator batch is a cat with the policy off
                       and a two-source gz_diffaug launch with it on).
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = "color,translation,cutout"
SECTIONS = ["kernel:3x64x64", "kernel:3x128x128", "step:dc_gan:128", "step:gan_stability_r1:64"]
NATIVE_IMG_SIZE = {"gan_stability_r1": 128}      # conf/expt/gan_stability_r1.yaml; every other experiment: 64


def event_ms(fn):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def spread(xs):
    import numpy as np
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4),
            "n": len(xs)}


def hot_and_cold_us(fn, flush, launches, rounds):
    import numpy as np
    for _ in range(20):
        fn()
    hot = [event_ms(lambda: [fn() for _ in range(launches)]) / launches * 1e3 for _ in range(rounds)]
    cold = []
    for _ in range(max(rounds, 10)):
        flush.add_(1)
        cold.append(event_ms(fn) * 1e3)
    return {"hot_us": spread(hot), "cold_us": spread(cold)}, float(np.median(hot)), float(np.median(cold))


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
        x0 = torch.randn(R0, C, H, W, device="cuda")
        x1 = torch.randn(R1, C, H, W, device="cuda") if R1 else None
        params = aug.draw(R0 + R1, H, W).cuda()
        src = torch.randn(R0 + R1, C, H, W, device="cuda")
        dst = torch.empty_like(src)
        nbytes = 8 * src.numel()
        out = {"bytes": nbytes}
        out["copy"], copy_hot, copy_cold = hot_and_cold_us(lambda: dst.copy_(src), flush, launches, rounds)
        for mode, name in ((0, "forward"), (2, "adjoint")):
            fn = (lambda mode=mode: F._diffaug_raw(x0, x1, params, cut, mode))
            out[name], hot, cold = hot_and_cold_us(fn, flush, launches, rounds)
            out[name].update({"hot_over_copy": round(hot / copy_hot, 3), "cold_over_copy": round(cold / copy_cold, 3),
                              "cold_TBps": round(nbytes / cold / 1e6, 3)})
        rec[label] = out
    return rec


def _stream_launchers():
    from lightning_gan_zoo_amd._lib import HEADER_PATH
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    return set(m.group(1) for m in re.finditer(r"\b(gz_\w+)\s*\(([^;{]*?hipStream_t[^;{]*?)\)\s*;", text))


class _CountingDll:
    def __init__(self, dll, names):
        self._dll, self._names, self.calls = dll, names, {}

    def __getattr__(self, name):
        fn = getattr(self._dll, name)
        if name not in self._names:
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def count_pair(trainer, batch):
    """{launcher name: calls} of one D+G pair, and the torch.cat calls in it."""
    import torch
    from lightning_gan_zoo_amd import _lib
    dll = _lib.lib.load()
    proxy = _CountingDll(dll, _stream_launchers())
    cats, plain_cat = [0], torch.cat

    def cat(*a, **k):
        cats[0] += 1
        return plain_cat(*a, **k)
    _lib.lib._dll, torch.cat = proxy, cat
    try:
        for _ in range(len(trainer.order)):
            trainer.step(batch)
        torch.cuda.synchronize()
    finally:
        _lib.lib._dll, torch.cat = dll, plain_cat
    return proxy.calls, cats[0]


def bench_step(expt, bs, pairs, rounds):
    import numpy as np
    import torch
    from lightning_gan_zoo_amd.config import locate, make_cfg
    from lightning_gan_zoo_amd.harness import Trainer

    def build(policy):
        cfg = make_cfg(expt, batch_size=bs, img_size=NATIVE_IMG_SIZE.get(expt, 64))
        cfg["diffaugment"] = policy
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

    (tr_off, batch), (tr_on, _) = build(""), build(FULL)
    assert tr_off.module.diffaugment is None and tr_on.module.diffaugment is not None
    for tr in (tr_off, tr_on):                       # warm-up: allocator, lazy optimizer state, pack tables, clocks
        run_pairs(tr, batch, max(10, pairs // 2))
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(rounds):                          # alternate, so that drift hits both alike
        off.append(event_ms(lambda: run_pairs(tr_off, batch, pairs)) / pairs)
        on.append(event_ms(lambda: run_pairs(tr_on, batch, pairs)) / pairs)
    calls_off, cat_off = count_pair(tr_off, batch)
    calls_on, cat_on = count_pair(tr_on, batch)
    n_off, n_on = sum(calls_off.values()), sum(calls_on.values())
    return {"expt": expt, "batch_size": bs, "steps_per_pair": len(tr_off.order), "pairs_per_block": pairs,
            "pair_ms_policy_off": spread(off), "pair_ms_policy_on": spread(on),
            "pair_us_delta_of_medians": round(float(np.median(on) - np.median(off)) * 1e3, 1),
            "on_over_off": round(float(np.median(on) / np.median(off)), 4),
            "library_launches_per_pair": {"off": n_off, "on": n_on, "delta": n_on - n_off,
                                          "gz_diffaug": calls_on.get("gz_diffaug", 0)},
            "torch_cat_per_pair": {"off": cat_off, "on": cat_on, "delta": cat_on - cat_off}}


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

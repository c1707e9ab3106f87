"""The runner's evaluation, host path against device path, in one process on one GPU: dc_gan at the reference's widths,
InceptionV3 with seeded random weights (the published file is not needed to time the work), a synthetic real set.

    python tools/eval_bench.py [--n 5000 50000] [--host-n 5000] [--batch 250] [--subsets 100] [--reps 5] [--host-kid]
                               [--out eval_bench.json]

Per sample count n the one JSON line holds
  * ``evaluate_s``         eval.evaluate, the path ``eval_on_device=false`` runs: generator and InceptionV3 at batch 16,
                           every batch through the host, np.cov on the host (only for the counts in ``--host-n``: the pass
                           is linear in n).  KID runs on the device in both paths unless ``--host-kid`` (eval_on_device
                           implies the device KID; the host KID's own minute is tools/kid_bench.py's subject);
  * ``evaluate_device_s``  eval.evaluate_device: batch ``--batch``, activations resident, gz_feature_moments, the same KID,
                           the same host sqrtm;
  * ``device_features_moments_s``  the part of it that bench.py's ``fid50k_features.seconds`` times, plus the moments;
  * ``sqrtm_s``            eval.frechet_distance alone on the two statistics (host; ``fid_on_device=false``);
  * ``fid_device_s``       eval.frechet_distance_device on the same statistics with the real set's cached root: what one
                           epoch pays with ``fid_on_device=true``; ``root_real_s`` the once-per-run root of the real
                           covariance; ``root_real_iterations`` / ``fid_device_iterations`` the Newton-Schulz iteration
                           counts, ``fid_rel_diff`` = |device - host| / |host| of the two distances,
                           ``sqrtm_over_fid_device`` = sqrtm_s / fid_device_s;
  * ``product_ms`` / ``product_fp64_tflops`` / ``product_pair_fp64_tflops``  gz_sqrtm_product and gz_sqrtm_product_pair at
                           d x d by HIP events (median of ``--reps`` after two warm-ups; FLOP = 2 d^3 per product);
  * ``moments_ms`` / ``moments_fp64_tflops`` / ``np_cov_s``  the moments launch sequence by HIP events (median of
                           ``--reps`` after two warm-ups; FLOP = 2 n d^2 / 2 * (1 + 1/tiles): the upper-triangle tiles the
                           kernel executes) beside numpy's np.cov of the same array;
  * ``inception_score_s`` / ``inception_score_host_s``  eval.inception_score_device on the resident [n, 2048] codes with a
                           seeded 1008-class head (median wall time of ``--reps`` calls after a warm-up) beside the host's
                           way to the same score: ``codes.cpu()``, a numpy product, eval.inception_score_from_logits
                           (once); ``inception_score_rel_diff`` the largest relative difference of a split score,
                           ``logits_ms`` / ``logits_fp64_tflops`` gz_classifier_logits alone by HIP events (FLOP =
                           2 n 2048 1008);
and once: ``input_fused_us`` beside ``input_resize_us``: gz_samples_to_inception_input against gz_resize_bilinear alone on
the same [250, 3, 64, 64] -> 299 x 299 shape (events, median of 20 after 5 warm-ups).
All wall times follow a warm-up pass (clocks, allocator, folded weights) and end with a device synchronisation.
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


def seeded_inception(seed=0):
    """He-scaled convolutions, BatchNorm statistics away from their defaults: finite, well-spread features."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    net = FIDInceptionV3()
    g = torch.Generator().manual_seed(seed)
    sd = net.state_dict()
    for k, v in sd.items():
        if k.endswith("conv.weight"):
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5
        elif k.endswith("bn.weight"):
            sd[k] = 1 + 0.2 * (torch.rand(v.shape, generator=g) - 0.5)
        elif k.endswith("bn.bias"):
            sd[k] = 0.2 * (torch.rand(v.shape, generator=g) - 0.5)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
    net.load_state_dict(sd)
    return net.cuda()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def events_ms(fn, reps, warm):
    times = []
    for i in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def moments_record(codes, reps):
    n, d = codes.shape
    mean = torch.empty((d,), dtype=torch.float64, device="cuda")
    cov = torch.empty((d, d), dtype=torch.float64, device="cuda")
    ws_bytes = lib.gz_feature_moments_workspace_bytes(n, d)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device="cuda")
    ms = events_ms(lambda: check(lib.gz_feature_moments(F._p(codes), n, d, F._p(mean), F._p(cov), F._p(ws), ws_bytes,
                                                        F._stream()), "feature_moments"), reps, 2)
    tiles = (d + 63) // 64
    flop = 2.0 * n * 64 * 64 * (tiles * (tiles + 1) // 2)
    host = codes.cpu().numpy()
    t0 = time.perf_counter()
    want = np.cov(host, rowvar=False)
    np_cov_s = time.perf_counter() - t0
    scale = np.sqrt(np.outer(np.diagonal(want), np.diagonal(want)))
    live = scale > 0                         # (a seeded random network leaves some features constant: variance 0)
    return {"moments_ms": round(ms, 3), "moments_fp64_tflops": round(flop / ms / 1e9, 2), "np_cov_s": round(np_cov_s, 3),
            "moments_max_err_over_scale": float((np.abs(cov.cpu().numpy() - want)[live] / scale[live]).max()) if live.any()
            else None}


def product_record(d, reps):
    a, b = torch.randn(d, d, dtype=torch.float64, device="cuda"), torch.randn(d, d, dtype=torch.float64, device="cuda")
    c, c2 = torch.empty_like(a), torch.empty_like(a)
    one = events_ms(lambda: check(lib.gz_sqrtm_product(F._p(a), F._p(b), F._p(c), d, -0.5, 1.5, F._stream()),
                                  "sqrtm_product"), reps, 2)
    two = events_ms(lambda: check(lib.gz_sqrtm_product_pair(F._p(a), F._p(b), F._p(c), 1.0, 0.0, F._p(b), F._p(a), F._p(c2),
                                                            1.0, 0.0, d, F._stream()), "sqrtm_product_pair"), reps, 2)
    flop = 2.0 * d ** 3
    return {"product_ms": round(one, 3), "product_fp64_tflops": round(flop / one / 1e9, 2),
            "product_pair_ms": round(two, 3), "product_pair_fp64_tflops": round(2 * flop / two / 1e9, 2)}


def inception_score_record(codes, reps, classes=1008, splits=10):
    """``inception_score_s``: eval.inception_score_device on the resident codes (a warm-up call, then the median wall
    time of ``reps`` calls, each ending in its own copy-back of the split scores); ``inception_score_host_s``: what the
    same score costs without the kernels -- ``codes.cpu()``, numpy's product with the head and
    eval.inception_score_from_logits, once.  A seeded classifier head, scaled so that the logits differ by a few units
    from row to row and centred by its bias (uncentred, the features' common mean hands every row to one class and the
    score is 1.00 whatever the rows are); converted once per run, as the runner does."""
    n, d = codes.shape
    g = torch.Generator().manual_seed(7)
    w64 = torch.randn(classes, d, generator=g, dtype=torch.float64).cuda()
    mean = codes.mean(dim=0)
    w64 *= 2.5 / float(((codes[:2000] - mean) @ w64.T).std())
    b64 = 0.1 * torch.randn(classes, generator=g, dtype=torch.float64).cuda() - w64 @ mean
    E.inception_score_device(codes, w64, b64, splits)
    times = []
    for _ in range(reps):
        t, dev = wall(lambda: E.inception_score_device(codes, w64, b64, splits))
        times.append(t)
    logits_ms = events_ms(lambda: E.classifier_logits_device(codes, w64, b64), reps, 1)

    def host():
        x = codes.cpu().numpy()
        return E.inception_score_from_logits(x.dot(w64.cpu().numpy().T) + b64.cpu().numpy(), splits)

    t_host, want = wall(host)
    return {"inception_score_s": round(float(np.median(times)), 4), "inception_score_host_s": round(t_host, 3),
            "inception_score": dev[0], "inception_score_std": dev[1],
            "inception_score_rel_diff": float(np.abs(dev[2] / want[2] - 1).max()),
            "logits_ms": round(logits_ms, 3), "logits_fp64_tflops": round(2.0 * n * d * classes / logits_ms / 1e9, 2)}


def input_record():
    N, C, H, W, OH, OW = 250, 3, 64, 64, 299, 299
    x = torch.rand(N, C, H, W, device="cuda") * 1.4 - 0.2
    x01 = torch.clamp(x, 0, 1)
    y = torch.empty((N, 3, OH, OW), device="cuda", dtype=torch.float32)
    fused = events_ms(lambda: check(lib.gz_samples_to_inception_input(F._p(x), F._p(y), N, C, H, W, OH, OW, 2.0, -1.0,
                                                                      F._stream()), "fused"), 20, 5)
    plain = events_ms(lambda: check(lib.gz_resize_bilinear(F._p(x01), F._p(y), N * C, H, W, OH, OW, 2.0, -1.0,
                                                           F._stream()), "resize"), 20, 5)
    return {"input_fused_us": round(fused * 1e3, 1), "input_resize_us": round(plain * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[5000, 50000])
    ap.add_argument("--host-n", type=int, nargs="*", default=[5000])
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-kid", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from lightning_gan_zoo_amd.config import locate, make_cfg
    from lightning_gan_zoo_amd.inception import InceptionFeatures
    cfg = make_cfg("dc_gan", batch_size=a.batch)
    torch.manual_seed(42)
    module = locate(cfg.model.lm["_target_"])(cfg, None).to("cuda")
    # an untrained generator's tanh output stays below 1 / 255: every image would be black and every feature constant.
    # The last layer's weights are scaled until the output in front of the tanh has a spread of 1.5 (the work is the same)
    with torch.no_grad():
        module.eval()
        spread = float(module.generator(torch.randn(64, cfg.model.noise_dim, device="cuda")).std())
        module.generator.net.transpose_conv_out.weight.mul_(1.5 / max(spread, 1e-6))
        module.train()
    features = InceptionFeatures(seeded_inception(), batch_size=16)
    rec = {"batch": a.batch, "subsets": a.subsets, "blas_threads": int(os.environ["OMP_NUM_THREADS"]),
           "host_kid": bool(a.host_kid), "runs": []}

    # warm-up: clocks, allocator, folded weights, both paths' kernel choices
    torch.manual_seed(1)
    warm = E.SampleDump(module, n_samples=2 * a.batch, batch_size=16)
    E.device_activations(module, warm, features.device, a.batch)
    for img in list(warm.images(module))[:4]:
        features(img)
    torch.cuda.synchronize()

    for n in a.n:
        torch.manual_seed(5)
        dump = E.SampleDump(module, n_samples=n, batch_size=16)
        rng = np.random.RandomState(n)
        real_act = np.abs(rng.randn(n, 2048)).astype(np.float32).astype(np.float64) * 0.5
        real = E.RealStatistics(real_act, "cuda")                 # once per run: outside the per-epoch times
        run = {"n": n}
        t_fm, fake = wall(lambda: (lambda act: (act, E.feature_moments_device(act)))(
            E.device_activations(module, dump, features.device, a.batch)))
        run["device_features_moments_s"] = round(t_fm, 3)
        np.random.seed(1)
        t_dev, dev = wall(lambda: E.evaluate_device(module, dump, features.device, real, batch=a.batch,
                                                    n_subsets=a.subsets))
        run["evaluate_device_s"] = round(t_dev, 3)
        mean, cov = fake[1]
        t_sq, fid_host = wall(lambda: E.frechet_distance(real.mu, real.sigma, mean.cpu().numpy(), cov.cpu().numpy()))
        run["sqrtm_s"] = round(t_sq, 3)
        t_root, (mu1, sigma1, root1, k_real, ok_real) = wall(real.device_root)      # once per run
        t_fd, (fid_dev, (_, k_fake), ok_fake) = wall(lambda: E.frechet_distance_device(mu1, sigma1, mean, cov, root1=root1))
        run.update({"root_real_s": round(t_root, 3), "fid_device_s": round(t_fd, 3), "root_real_iterations": k_real,
                    "fid_device_iterations": k_fake, "fid_device_converged": bool(ok_real and ok_fake),
                    "fid_rel_diff": abs(fid_dev - fid_host) / abs(fid_host),
                    "sqrtm_over_fid_device": round(t_sq / t_fd, 2)})
        run.update(product_record(mean.shape[0], a.reps))
        del mu1, sigma1, root1
        run.update(moments_record(fake[0], a.reps))
        run.update(inception_score_record(fake[0], a.reps))
        del fake
        if n in a.host_n:
            np.random.seed(1)
            t_host, host = wall(lambda: E.evaluate(module, dump, features, real_act, n_subsets=a.subsets,
                                                   kid_on_device=not a.host_kid, real_codes_device=real.codes))
            run["evaluate_s"] = round(t_host, 3)
            run["host_over_device"] = round(t_host / t_dev, 2)
            run["fid_host"], run["fid_device"] = host["fid"], dev["fid"]
            run["kid_host"], run["kid_device"] = host["kid"], dev["kid"]
        rec["runs"].append(run)
        del real, real_act
        torch.cuda.empty_cache()
    rec.update(input_record())
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

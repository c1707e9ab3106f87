"""Writes tests/golden/eval_input_parent.npz: what ``functional.normalize_u8_images`` and ``gz_resize_bilinear`` computed
BEFORE their expressions were factored into shared device functions (csrc/gz_common.h u8_norm, csrc/gz_infer.hip
bilinear_sample) for the fused Inception-input kernel.  tests/test_eval_device_gpu.py holds today's kernels to these bits.

Needs an MI355X and the library of the commit before that refactor, whose header lacks today's entry points:

    GZ_LIB=<that commit's libgz_hip.so> GZ_OPS_H=<that commit's include/gz_ops.h> \\
        python tests/golden/make_eval_input_golden.py [out.npz]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from eval_device_support import GOLDEN_CASES, MUL_ADD, golden_u8  # noqa: E402
from lightning_gan_zoo_amd import _lib  # noqa: E402


def main(out):
    header = os.environ.get("GZ_OPS_H")
    if header:
        parse = _lib.parse_header
        _lib.parse_header = lambda path=header: parse(path)
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    blob = {"library_digest": np.array(lib.gz_source_digest().decode())}
    for seed, (name, shape, (OH, OW)) in enumerate(GOLDEN_CASES):
        u8 = golden_u8(shape, seed + 1)
        dev = torch.from_numpy(u8).cuda()
        x01 = F.normalize_u8_images(dev, 0.0, 1.0)
        blob[name + "/u8"] = u8
        blob[name + "/norm_0_1"] = x01.cpu().numpy()
        blob[name + "/norm_0.5_0.5"] = F.normalize_u8_images(dev, 0.5, 0.5).cpu().numpy()
        N, C, H, W = x01.shape
        for mul, add in (MUL_ADD if OH * OW < 50000 else MUL_ADD[:1]):
            y = torch.empty((N, C, OH, OW), device="cuda", dtype=torch.float32)
            check(lib.gz_resize_bilinear(F._p(x01), F._p(y), N * C, H, W, OH, OW, mul, add, F._stream()), "resize")
            blob[name + "/resize_%g_%g" % (mul, add)] = y.cpu().numpy()
    torch.cuda.synchronize()
    np.savez_compressed(out, **blob)
    print("wrote", out, {k: v.shape for k, v in blob.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eval_input_parent.npz"))

"""Shared by tests/test_eval_device_gpu.py and tests/golden/make_eval_input_golden.py: generator-output stand-ins that
sit on every edge of the sample dump's quantiser, the host's version of that quantiser, and the golden cases."""
import numpy as np

NEIGHBOURS = (0, 1, 2, 3, 64, 85, 127, 128, 170, 200, 253, 254, 255)      # levels whose float neighbours are planted
# (input shape [N, C, H, W], output size) of the fused-kernel test
FUSED_CASES = [((3, 3, 64, 64), (299, 299)), ((2, 1, 28, 28), (299, 299)), ((2, 3, 5, 7), (11, 13)),
               ((1, 3, 40, 24), (9, 10))]
MUL_ADD = [(2.0, -1.0), (1.0, 0.0)]
# (name, u8 shape [N, H, W, C], output size) of tests/golden/eval_input_parent.npz: small enough to commit
GOLDEN_CASES = [("a", (2, 5, 7, 3), (11, 13)), ("b", (1, 40, 24, 3), (9, 10)), ("c", (2, 28, 28, 1), (37, 41)),
                ("d", (1, 64, 64, 1), (299, 299))]


def planted_values():
    """Every k / 255 in fp32, the floats on either side of several of them, both ends of the clamp, values outside."""
    f32 = np.float32
    levels = np.arange(256, dtype=f32) / f32(255)
    near = levels[list(NEIGHBOURS)]
    return np.concatenate([levels, np.nextafter(near, f32(-np.inf)), np.nextafter(near, f32(np.inf)),
                           np.array([0.0, -0.0, 1.0, -0.25, -1.0, -1e-30, 1.25, 2.0, 0.5, 0.999999], dtype=f32)])


def edge_samples(shape, seed):
    """float32 [N, C, H, W] in [-0.3, 1.3] with ``planted_values`` scattered over it (all of them where they fit; a
    window that starts at a seed-dependent place and always holds the clamp's ends and the outside values otherwise)."""
    n = int(np.prod(shape))
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.3, 1.3, n).astype(np.float32)
    special = planted_values()
    if special.size > n // 2:
        special = np.concatenate([special[-10:], np.roll(special[:-10], -61 * seed)])[:n // 2]
    x[rng.permutation(n)[:special.size]] = special
    return x.reshape(shape)


def host_quantise(x):
    """``SampleDump.images``' host arithmetic on a float32 [N, C, H, W] array -> uint8 [N, H, W, 3 or C]."""
    import torch
    s = torch.clamp(torch.from_numpy(np.ascontiguousarray(x)), 0, 1).permute(0, 2, 3, 1).numpy()
    return (s * 255).astype(int).astype(np.uint8)


def golden_u8(shape, seed):
    return host_quantise(edge_samples((shape[0], shape[3], shape[1], shape[2]), seed))

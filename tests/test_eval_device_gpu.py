"""The evaluation pass on the device (eval.evaluate_device): the fused generator-output -> Inception-input kernel
against the composition it replaces, bit for bit; the refactored kernels against the bits they produced before
(tests/golden/eval_input_parent.npz, tests/golden/make_eval_input_golden.py); the sample dump's device sweep against
its host sweep; the metrics against the host path's on bit-identical activations."""
import os

import numpy as np
import pytest
import torch

from eval_device_support import FUSED_CASES, GOLDEN_CASES, MUL_ADD, edge_samples, host_quantise, planted_values
from helpers import GOLDEN_DIR, seeded_inception_state

pytestmark = pytest.mark.gpu
TOL = 1e-3                                   # tests/test_inception_gpu.py's


def _resize(x, OH, OW, mul, add):
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    N, C, H, W = x.shape
    y = torch.empty((N, C, OH, OW), device="cuda", dtype=torch.float32)
    check(lib.gz_resize_bilinear(F._p(x), F._p(y), N * C, H, W, OH, OW, mul, add, F._stream()), "resize")
    return y


def _fused(x, OH, OW, mul, add):
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    N, C, H, W = x.shape
    y = torch.full((N, 3, OH, OW), float("nan"), device="cuda", dtype=torch.float32)
    check(lib.gz_samples_to_inception_input(F._p(x), F._p(y), N, C, H, W, OH, OW, mul, add, F._stream()), "fused")
    return y


@pytest.mark.parametrize("mul,add", MUL_ADD)
@pytest.mark.parametrize("shape,size", FUSED_CASES)
def test_fused_input_kernel_equals_the_composition_bit_for_bit(shape, size, mul, add):
    from lightning_gan_zoo_amd import functional as F
    x = edge_samples(shape, seed=sum(shape))
    have = set(x.ravel().tolist())
    assert x.min() < 0 and x.max() > 1 and 0.0 in have and 1.0 in have
    if x.size >= 2 * planted_values().size:
        assert have.issuperset(planted_values().tolist())        # every k / 255 and the planted neighbours
    u8 = host_quantise(x)                                          # SampleDump.images' arithmetic, on the host
    if shape[1] == 1:
        u8 = np.concatenate(3 * [u8], axis=3)                      # greyscale -> RGB, as images() does
    want = _resize(F.normalize_u8_images(torch.from_numpy(u8).cuda(), 0.0, 1.0), size[0], size[1], mul, add)
    got = _fused(torch.from_numpy(x).cuda(), size[0], size[1], mul, add)
    assert got.shape == want.shape == (shape[0], 3, size[0], size[1])
    assert torch.equal(got, want), int((got != want).sum())


def test_fused_input_kernel_refuses_what_it_does_not_run():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    x = torch.zeros(1, 2, 4, 4, device="cuda")
    y = torch.zeros(1, 3, 4, 4, device="cuda")
    assert lib.gz_samples_to_inception_input(F._p(x), F._p(y), 1, 2, 4, 4, 4, 4, 1.0, 0.0, F._stream()) == -1
    assert lib.gz_samples_to_inception_input(F._p(x), F._p(y), 0, 1, 4, 4, 4, 4, 1.0, 0.0, F._stream()) == -1
    assert lib.gz_samples_to_inception_input(None, F._p(y), 1, 1, 4, 4, 4, 4, 1.0, 0.0, F._stream()) == -1


@pytest.mark.parametrize("name,shape,size", GOLDEN_CASES)
def test_refactored_kernels_keep_the_bits_of_the_commit_before(name, shape, size):
    from lightning_gan_zoo_amd import functional as F
    gold = np.load(os.path.join(GOLDEN_DIR, "eval_input_parent.npz"))
    u8 = torch.from_numpy(gold[name + "/u8"]).cuda()
    assert tuple(u8.shape) == shape
    x01 = F.normalize_u8_images(u8, 0.0, 1.0)
    assert torch.equal(x01.cpu(), torch.from_numpy(gold[name + "/norm_0_1"]))
    assert torch.equal(F.normalize_u8_images(u8, 0.5, 0.5).cpu(), torch.from_numpy(gold[name + "/norm_0.5_0.5"]))
    seen = 0
    for mul, add in MUL_ADD:
        key = name + "/resize_%g_%g" % (mul, add)
        if key in gold:
            seen += 1
            assert torch.equal(_resize(x01, size[0], size[1], mul, add).cpu(), torch.from_numpy(gold[key])), key
    assert seen >= 1


# ---- the sample dump's device sweep -------------------------------------------------------------------------------------
def _tiny(expt, seed=42):
    """A tiny module on the GPU.  An untrained tiny dc_gan generator's tanh output stays below 1 / 255 -- every image of
    its dump is black, and every comparison of dumps would hold trivially -- so the weights of its last layer are
    scaled until the output in front of the tanh has a spread of 1.5: images with all 256 grey levels in reach."""
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg(expt, batch_size=8, features=8, noise_dim=16)
    torch.manual_seed(seed)
    module = locate(cfg.model.lm["_target_"])(cfg, None).to("cuda")
    if expt == "dc_gan":
        last = module.generator.net.transpose_conv_out.weight
        z = torch.randn(16, 16, generator=torch.Generator().manual_seed(9)).cuda()
        module.eval()
        with torch.no_grad():
            spread = float(module.generator(z).std())
            assert 0 < spread < 0.05                                # tanh still linear: the scale below is what it says
            last.mul_(1.5 / spread)
        module.train()
    return module


def _native_dump(module, n_samples, batch_size=16):
    """A SampleDump whose device sweep yields the quantised image itself (native size, x 1 + 0) instead of the
    299 x 299 Inception input (the tiny generators draw 64 x 64): then ``round(y * 255)`` is the grey level."""
    from lightning_gan_zoo_amd import eval as E

    class NativeDump(E.SampleDump):
        def device_batches(self, module, batch=250, size=(64, 64), mul=1.0, add=0.0):
            return super().device_batches(module, batch, size=size, mul=mul, add=add)

    return NativeDump(module, n_samples=n_samples, batch_size=batch_size)


def _levels(y):
    """Inputs made with mul 1, add 0 at native size -> the uint8 NHWC images they were made from."""
    return torch.round(y * 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def test_device_batches_reproduce_images():
    from lightning_gan_zoo_amd import eval as E
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = E.SampleDump(module, n_samples=40, batch_size=16)
    assert module.training
    want = np.concatenate(list(dump.images(module)))
    assert want.shape == (40, 64, 64, 3) and module.training
    got = [y for y in dump.device_batches(module, batch=16, size=(64, 64), mul=1.0, add=0.0)]
    assert module.training                                          # mode restored
    assert [tuple(y.shape) for y in got] == [(16, 3, 64, 64), (16, 3, 64, 64), (8, 3, 64, 64)]
    assert all(y.is_cuda and y.dtype == torch.float32 for y in got)
    assert np.array_equal(np.concatenate([_levels(y) for y in got]), want)
    assert len(np.unique(want)) > 8                                 # not a blank image
    module.eval()
    shapes = [tuple(y.shape) for y in dump.device_batches(module, batch=250)]
    assert shapes == [(40, 3, 299, 299)] and not module.training


class PixelStatistics:
    """Stand-in for InceptionFeatures: 24 integer statistics per image (8 bands of rows x 3 channels, sums of grey
    levels: at most 8 * 64 * 255, exact in fp32) times 2^-15 (exact as well; it keeps the cubic kernel of KID near 1,
    where its estimator is not a difference of 1e30s), from uint8 NHWC images on the host (``__call__``) and from the
    quantised [b, 3, H, W] float image on the device (``device``).  Identical numbers either way."""
    SCALE = 2.0 ** -15

    def __call__(self, images_u8):
        a = np.asarray(images_u8).astype(np.int64)
        n, H, W, C = a.shape
        return a.reshape(n, 8, H // 8, W, C).sum(axis=(2, 3)).reshape(n, 8 * C).astype(np.float64) * self.SCALE

    def device(self, x):
        u = torch.round(x * 255)
        n, C, H, W = u.shape
        return u.reshape(n, C, 8, H // 8, W).sum(dim=(3, 4)).permute(0, 2, 1).reshape(n, 8 * C) * self.SCALE


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_evaluate_device_matches_the_host_path_on_identical_activations():
    from lightning_gan_zoo_amd import eval as E
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=200)
    net = PixelStatistics()
    host_act = np.concatenate([net(img) for img in dump.images(module)])
    # batch 16, the host sweep's: the generator's bits at another batch size are not promised to be the same
    dev_act = E.device_activations(module, dump, net.device, batch=16)
    assert dev_act.shape == (200, 24) and dev_act.dtype == torch.float64 and dev_act.is_cuda
    assert np.array_equal(dev_act.cpu().numpy(), host_act)
    # 260 real rows against 200 generated ones: KID's subsets of 200 then differ from one another on the real side (with
    # 200 and 200 every subset is the whole of both sets and kid_std is the rounding noise of one number)
    rng = np.random.RandomState(12)
    real_act = host_act[rng.randint(0, 200, 260)] * 0.9 + rng.randn(260, 24) * host_act.std(axis=0) * 0.5
    conds = [np.linalg.cond(np.cov(a, rowvar=False)) for a in (host_act, real_act)]
    print("covariance condition numbers: generated %.3g, real %.3g" % tuple(conds))
    assert max(conds) < 1e6
    np.random.seed(21)
    host = E.evaluate(module, dump, net, real_act, n_subsets=5)
    want_state = np.random.get_state()
    real = E.RealStatistics(real_act, module.device)
    np.random.seed(21)
    dev = E.evaluate_device(module, dump, net.device, real, batch=16, n_subsets=5)
    assert _same_state(np.random.get_state(), want_state)
    assert set(dev) == set(host) == {"fid", "kid", "kid_std"}
    print("kid device %.15g host %.15g, kid_std device %.15g host %.15g" % (dev["kid"], host["kid"], dev["kid_std"], host["kid_std"]))
    assert host["kid_std"] > 1e-6 * abs(host["kid"])               # subsets that differ: a standard deviation to compare
    assert np.isclose(dev["kid"], host["kid"], rtol=1e-10, atol=0)
    assert np.isclose(dev["kid_std"], host["kid_std"], rtol=1e-10, atol=0)
    want_fid = E.frechet_distance(*E.activation_statistics(real_act), *E.activation_statistics(host_act))
    print("fid device %.15g host %.15g" % (dev["fid"], want_fid))
    assert np.isfinite(want_fid) and want_fid > 0
    assert abs(dev["fid"] - want_fid) <= 1e-9 * abs(want_fid)


def test_hologan_host_draws_are_left_as_the_host_path_leaves_them():
    from lightning_gan_zoo_amd import eval as E
    module = _tiny("hologan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=40)
    net = PixelStatistics()
    real_act = np.random.RandomState(3).rand(50, 24) * 2
    np.random.seed(77)
    E.evaluate(module, dump, net, real_act, n_subsets=3)
    want_state = np.random.get_state()
    real = E.RealStatistics(real_act, module.device)
    np.random.seed(77)
    out = E.evaluate_device(module, dump, net.device, real, batch=250, n_subsets=3)
    assert _same_state(np.random.get_state(), want_state)
    assert np.isfinite(out["kid"])


def test_real_inception_features_at_two_batch_sizes():
    """The device pass at one batch of 48 against InceptionFeatures' host sweep at 16: other convolution kernels, one
    launch instead of three for the input, the same features (1e-3, test_inception_gpu.py's tolerance)."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd.inception import FIDInceptionV3, InceptionFeatures
    net = FIDInceptionV3()
    net.load_state_dict(seeded_inception_state(net, 3))
    features = InceptionFeatures(net.cuda(), batch_size=16)
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = E.SampleDump(module, n_samples=48, batch_size=16)
    want = np.concatenate([features(img) for img in dump.images(module)])
    got = E.device_activations(module, dump, features.device, batch=48)
    assert got.shape == (48, 2048) and got.dtype == torch.float64 and got.is_cuda
    err = float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max())
    print("inception features, device pass at 48 against host sweep at 16: rel err %.2e" % err)
    assert err < TOL and float(np.abs(want).max()) > 1e-3


def test_real_statistics_are_computed_once_per_run(monkeypatch, capsys):
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd import run_network as R
    module = _tiny("dc_gan")
    torch.manual_seed(5)
    dump = _native_dump(module, n_samples=40)
    net = PixelStatistics()
    real_act = np.random.RandomState(3).rand(50, 24) * 2
    calls = []
    moments = E.feature_moments_device
    monkeypatch.setattr(E, "feature_moments_device", lambda codes: calls.append(tuple(codes.shape)) or moments(codes))
    evaluate = R.device_fid_evaluator(dump, net, real_act, module.device, batch=16)
    assert calls == [(50, 24)]                                      # the real set, when the evaluator is built
    np.random.seed(1)
    first = evaluate(module, 1)
    np.random.seed(1)
    second = evaluate(module, 2)
    assert calls == [(50, 24), (40, 24), (40, 24)]                  # per epoch: the generated set alone
    assert first == second and "epoch 2 FID: " in capsys.readouterr().out
    # statistics a cache file already holds are taken as they are
    mu, sigma = E.activation_statistics(real_act)
    del calls[:]
    R.device_fid_evaluator(dump, net, real_act, module.device, batch=16, mu=mu, sigma=sigma)
    assert calls == []

"""the FID / KID feature extractor (InceptionV3 with the FID patches) on the HIP convolution family.

Round 5: pinned to the REFERENCE'S OWN network code.  tests/golden/inception_ref.npz holds the 2048-d pool features (and
logits) that ``InceptionV3([3])`` of /root/reference/core/submodules/gan_stability/metrics/inception.py -- run unmodified
by tests/golden/make_inception_golden.py over torchvision's layer definitions (restated in
oracle/torchvision_inception.py: torchvision is absent) -- produces for seeded weights and seeded inputs;
inception_state_keys.json is the state_dict listing of the network that code builds.  The CPU oracle
(oracle/inception_cpu.py) and the HIP network are both held to those numbers.  The real weight FILE comes from a URL (no
network here): what is pinned is the architecture and the arithmetic; ``load_fid_weights`` verifies the file's sha256
prefix (the ``6726825d`` of its published name) when a user supplies it."""
import json
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

TOL = 1e-3


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


from helpers import seeded_inception_state as seeded_state  # noqa: E402


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((64, 2), (299, 2), (32, 3), (128, 1))       # tests/golden/make_inception_golden.py


def reference_features():
    blob = np.load(os.path.join(GOLDEN, "inception_ref.npz"))
    return int(blob["seed"]), {size: torch.from_numpy(blob["pool3/%d" % size]) for size, _ in CASES}


def test_state_dict_listing_is_the_one_the_reference_code_builds():
    """Key order, shapes and dtypes of the product network and of the CPU oracle == the state_dict of
    ``fid_inception_v3()`` as the reference's code builds it (inception_state_keys.json): the weight file the reference
    downloads loads into either without renaming."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    with open(os.path.join(GOLDEN, "inception_state_keys.json")) as f:
        ref = json.load(f)
    assert ref["weights_url"].endswith("pt_inception-2015-12-05-6726825d.pth")
    want = [(k, tuple(shape), dt) for k, shape, dt in ref["keys"]]
    for net in (FIDInceptionV3(), Oracle()):
        got = [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in net.state_dict().items()]
        assert got == want


def test_oracle_inception_matches_the_reference_fixture():
    """oracle/inception_cpu.py (the flat restatement the GPU box uses as its checker) against the features the
    reference's own InceptionV3 produced: same seeded weights, same seeded inputs, 1e-5."""
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    torch.set_num_threads(4)
    seed, feats = reference_features()
    oracle = Oracle().eval()
    oracle.load_state_dict(seeded_state(oracle, seed))
    for size, n in CASES:
        x = torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(size))
        with torch.no_grad():
            out = oracle(x)
        assert out.shape == feats[size].shape and rel(out, feats[size]) < 1e-5, (size, rel(out, feats[size]))


def published_shapes():
    with open(os.path.join(GOLDEN, "inception_shapes.json")) as f:
        t = json.load(f)
    return tuple(t["input"]), [(name, tuple(shape)) for name, shape in t["shapes"]]


def test_torchvision_stand_in_reproduces_the_published_shape_table():
    """VERDICT r5 item 6a.  torchvision is absent, so tests/golden/make_inception_golden.py runs the reference's FID code
    over oracle/torchvision_inception.py -- layer definitions typed in by the builder.  Its state-dict listing was
    already held to the published one; here its GEOMETRY is held to something the builder did not produce: the
    per-layer output shapes at 299 x 299 that torchvision's own source lists beside every call of Inception3._forward
    (tests/golden/inception_shapes.json; = Table 1 of the Inception-v3 paper).  A wrong kernel size, stride, padding or
    branch width in BasicConv2d / InceptionA..E changes a shape somewhere down the chain.  The same table for the CPU
    oracle the GPU box checks against (oracle/inception_cpu.py), through its module outputs."""
    from oracle import torchvision_inception as TV
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    torch.set_num_threads(4)
    shape_in, table = published_shapes()
    x = torch.rand(1, *shape_in, generator=torch.Generator().manual_seed(3))
    net = TV.Inception3(aux_logits=False).eval()
    got = []
    with torch.no_grad():
        h = x
        for name, mod in net.named_children():          # registration order == Inception3._forward's call order
            if name in ("dropout", "fc"):
                continue
            h = mod(h)
            got.append((name, tuple(h.shape[1:])))
    assert got == table, [(a, b) for a, b in zip(got, table) if a != b]
    oracle = Oracle().eval()
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: seen.__setitem__(n, tuple(o.shape[1:])))
             for n, m in oracle.named_children() if n != "fc"]
    with torch.no_grad():
        feats = oracle(x, resize_input=False, normalize_input=False)
    for h_ in hooks:
        h_.remove()
    want = dict(table)
    assert seen and all(seen[n] == want[n] for n in seen), {n: (seen[n], want[n]) for n in seen if seen[n] != want[n]}
    assert {n for n, _ in table if n.startswith(("Conv2d", "Mixed"))} <= set(seen)
    assert tuple(feats.shape) == (1, 2048)


def test_fid_weight_file_hash_is_checked(tmp_path):
    """``load_fid_weights``: a file that is not the published one (sha256 prefix 6726825d, the suffix of its name in
    the reference's URL, inception.py:13) is refused unless the caller opts out."""
    from lightning_gan_zoo_amd import inception as I
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    path = str(tmp_path / "pt_inception-2015-12-05-6726825d.pth")
    torch.save(seeded_state(Oracle(), 1), path)
    with pytest.raises(RuntimeError, match="sha256"):
        I.fid_weights_state(path)
    sd = I.fid_weights_state(path, check_hash=False)
    assert "Mixed_7c.branch_pool.bn.running_var" in sd
    assert I.FID_WEIGHTS_SHA256_PREFIX == "6726825d"


def test_state_dict_layout_is_torchvisions():
    """The keys of the weight file the reference downloads (pytorch-fid's pt_inception-2015-12-05): torchvision's
    inception_v3(num_classes=1008, aux_logits=False)."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    sd = FIDInceptionV3().state_dict()
    assert list(sd) == list(Oracle().state_dict())
    assert sd["Conv2d_1a_3x3.conv.weight"].shape == (32, 3, 3, 3)
    assert sd["Mixed_5b.branch5x5_2.conv.weight"].shape == (64, 48, 5, 5)
    assert sd["Mixed_6b.branch7x7_2.conv.weight"].shape == (128, 128, 1, 7)
    assert sd["Mixed_6e.branch7x7dbl_4.conv.weight"].shape == (192, 192, 7, 1)
    assert sd["Mixed_7a.branch3x3_2.conv.weight"].shape == (320, 192, 3, 3)
    assert sd["Mixed_7c.branch3x3dbl_3b.conv.weight"].shape == (384, 384, 3, 1)
    assert sd["Mixed_7c.branch_pool.bn.running_var"].shape == (192,)
    assert sd["fc.weight"].shape == (1008, 2048)
    assert sum(v.numel() for k, v in sd.items() if not k.endswith("num_batches_tracked")) == 23_885_392


@pytest.mark.gpu
@pytest.mark.parametrize("case", [
    # N, C, H, W, K, KH, KW, SH, SW, PH, PW  (the layer types of InceptionV3 + ragged ones)
    (2, 3, 75, 75, 32, 3, 3, 2, 2, 0, 0), (2, 32, 37, 37, 32, 3, 3, 1, 1, 0, 0), (2, 48, 35, 35, 64, 5, 5, 1, 1, 2, 2),
    (2, 128, 17, 17, 128, 1, 7, 1, 1, 0, 3), (2, 160, 17, 17, 192, 7, 1, 1, 1, 3, 0),
    (3, 384, 8, 8, 384, 1, 3, 1, 1, 0, 1), (3, 384, 8, 8, 384, 3, 1, 1, 1, 1, 0), (2, 288, 35, 35, 384, 3, 3, 2, 2, 0, 0),
    (1, 2048, 8, 8, 320, 1, 1, 1, 1, 0, 0), (2, 20, 13, 9, 7, 2, 4, 2, 1, 1, 2), (16, 192, 17, 17, 192, 3, 3, 2, 2, 0, 0),
    # round 6: launches that fill the chip with 256x64 tiles take the igemm2 skeleton (ConvTapAnyA2 + EpiNCHWBiasAct):
    # 1x7 / 7x1 with asymmetric padding, 5x5 p2 on 48 channels (three channel blocks), 3x3 stride 2, 1x1; ragged last tiles
    (72, 128, 17, 17, 192, 1, 7, 1, 1, 0, 3), (72, 160, 17, 17, 192, 7, 1, 1, 1, 3, 0), (48, 48, 35, 35, 64, 5, 5, 1, 1, 2, 2),
    (64, 288, 35, 35, 384, 3, 3, 2, 2, 0, 0), (96, 256, 17, 17, 192, 1, 1, 1, 1, 0, 0), (40, 64, 33, 37, 128, 3, 3, 1, 1, 1, 1),
    # ... 72 channels (the last channel block of a tap half empty) under a ragged last pixel tile (11560 pixels = 45.2 tiles)
    (40, 72, 17, 17, 320, 1, 7, 1, 1, 0, 3)])
def test_conv2d_fwd_any(case):
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import check, lib
    N, C, H, W, K, KH, KW, SH, SW, PH, PW = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, KH, KW, generator=g) * (2.0 / (C * KH * KW)) ** 0.5
    b = torch.randn(K, generator=g)
    ref = TF.relu(TF.conv2d(x, w, b, (SH, SW), (PH, PW)))
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    wp = torch.empty(lib.gz_conv2d_pack_fwd_any_elems(K, C, KH, KW), device="cuda")
    check(lib.gz_conv2d_pack_fwd_any(F._p(wd), F._p(wp), K, C, KH, KW, F._stream()), "pack")
    OH, OW = ref.shape[2:]
    y = torch.empty(N, K, OH, OW, device="cuda")
    nb = lib.gz_conv2d_fwd_any_workspace_bytes(N, C, H, W, K, OH, OW, KH, KW, SH, SW, PH, PW)
    ws = torch.empty(max(nb // 4, 1), device="cuda")
    check(lib.gz_conv2d_fwd_any(F._p(xd), F._p(wp), F._p(bd), F._p(y), F._p(ws), nb, N, C, H, W, K, OH, OW, KH, KW, SH, SW,
                                PH, PW, F.ACT_RELU, 0.0, F._stream()), "fwd_any")
    assert rel(y, ref) < TOL
    if N >= 40:          # (the igemm2 cases) also without the activation, and repeatable bit for bit
        y2 = torch.empty_like(y)
        check(lib.gz_conv2d_fwd_any(F._p(xd), F._p(wp), F._p(bd), F._p(y2), F._p(ws), nb, N, C, H, W, K, OH, OW, KH, KW, SH,
                                    SW, PH, PW, F.ACT_RELU, 0.0, F._stream()), "fwd_any")
        assert torch.equal(y, y2)
        check(lib.gz_conv2d_fwd_any(F._p(xd), F._p(wp), F._p(bd), F._p(y2), F._p(ws), nb, N, C, H, W, K, OH, OW, KH, KW, SH,
                                    SW, PH, PW, F.ACT_NONE, 0.0, F._stream()), "fwd_any")
        assert rel(y2, TF.conv2d(x, w, b, (SH, SW), (PH, PW))) < TOL
        # ... and into a channel slice of a wider tensor (a block's concatenation): the same bits, neighbours untouched
        import ctypes
        before, after = 24, 40
        wide = torch.full((N, before + K + after, OH, OW), 7.0, device="cuda")
        dst = wide[:, before:before + K]
        rc = lib.gz_conv2d_fwd_any_into(F._p(xd), F._p(wp), F._p(bd), ctypes.c_void_p(dst.data_ptr()), before + K + after,
                                        N, C, H, W, K, OH, OW, KH, KW, SH, SW, PH, PW, F.ACT_RELU, 0.0, F._stream())
        assert rc == 0, rc
        assert torch.equal(dst, y)
        assert bool((wide[:, :before] == 7.0).all()) and bool((wide[:, before + K:] == 7.0).all())
    else:                # launches without a destination stride say so instead of writing a dense tensor into the slice
        import ctypes
        rc = lib.gz_conv2d_fwd_any_into(F._p(xd), F._p(wp), F._p(bd), ctypes.c_void_p(y.data_ptr()), K + 8, N, C, H, W, K,
                                        OH, OW, KH, KW, SH, SW, PH, PW, F.ACT_RELU, 0.0, F._stream())
        assert rc == -2, rc


@pytest.mark.gpu
def test_pool_and_resize():
    from lightning_gan_zoo_amd import inception as I
    x = torch.randn(3, 5, 17, 13, generator=torch.Generator().manual_seed(1))
    xd = x.cuda()
    assert rel(I._pool(xd, 3, 2, 0, I.MAX), TF.max_pool2d(x, 3, 2)) < 1e-6
    assert rel(I._pool(xd, 3, 1, 1, I.MAX), TF.max_pool2d(x, 3, 1, 1)) < 1e-6
    assert rel(I._pool(xd, 3, 1, 1, I.AVG_NOPAD), TF.avg_pool2d(x, 3, 1, 1, count_include_pad=False)) < 1e-6
    assert rel(I._pool(xd, 3, 1, 1, I.AVG), TF.avg_pool2d(x, 3, 1, 1)) < 1e-6
    # the compile-time 3 x 3 windows on groups of whole planes (round 6): InceptionV3's plane sizes, plane counts that
    # leave a ragged last group, bit-equal to torch (same summation order; max is exact)
    for (n, c, h, w) in ((2, 5, 35, 35), (3, 11, 17, 17), (2, 37, 8, 8), (1, 3, 71, 71), (5, 1, 3, 3), (2, 3, 9, 40)):
        t = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h))
        td = t.cuda()
        assert torch.equal(I._pool(td, 3, 2, 0, I.MAX).cpu(), TF.max_pool2d(t, 3, 2))
        assert torch.equal(I._pool(td, 3, 1, 1, I.MAX).cpu(), TF.max_pool2d(t, 3, 1, 1))
        assert rel(I._pool(td, 3, 1, 1, I.AVG_NOPAD), TF.avg_pool2d(t, 3, 1, 1, count_include_pad=False)) < 1e-6
        assert rel(I._pool(td, 3, 1, 1, I.AVG), TF.avg_pool2d(t, 3, 1, 1)) < 1e-6
        assert rel(I._pool(td, 3, 2, 0, I.AVG), TF.avg_pool2d(t, 3, 2)) < 1e-6
    # planes beyond one LDS image go by bands of eight output rows (147 x 147 and a ragged 100 x 131)
    for (n, c, h, w) in ((1, 3, 147, 147), (2, 2, 100, 131)):
        t = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h))
        assert torch.equal(I._pool(t.cuda(), 3, 2, 0, I.MAX).cpu(), TF.max_pool2d(t, 3, 2))
        assert rel(I._pool(t.cuda(), 3, 2, 0, I.AVG), TF.avg_pool2d(t, 3, 2)) < 1e-6
    big = torch.randn(3, 41, 8, 8, generator=torch.Generator().manual_seed(3))          # 16 lanes per 8 x 8 plane
    assert rel(I._pool(big.cuda(), 8, 1, 0, I.AVG), TF.adaptive_avg_pool2d(big, 1)) < 1e-6
    sq = torch.randn(2, 7, 8, 8, generator=torch.Generator().manual_seed(2))
    assert rel(I._pool(sq.cuda(), 8, 1, 0, I.AVG), TF.adaptive_avg_pool2d(sq, 1)) < 1e-6
    from lightning_gan_zoo_amd._lib import check, lib
    from lightning_gan_zoo_amd import functional as F
    for (H, W, OH, OW) in ((64, 64, 299, 299), (128, 96, 299, 299), (300, 400, 299, 299), (17, 13, 17, 13)):
        img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H))
        ref = 2 * TF.interpolate(img, size=(OH, OW), mode="bilinear", align_corners=False) - 1
        out = torch.empty(2, 3, OH, OW, device="cuda")
        check(lib.gz_resize_bilinear(F._p(img.cuda()), F._p(out), 6, H, W, OH, OW, 2.0, -1.0, F._stream()), "resize")
        assert rel(out, ref) < 1e-5


@pytest.mark.gpu
def test_inception_pool_features_match_the_reference_fixture():
    """The HIP network against the features the reference's own InceptionV3 code produced (inception_ref.npz): 64x64,
    299x299, 32x32 and 128x128 inputs, seeded weights, 1e-3."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    seed, feats = reference_features()
    net = FIDInceptionV3()
    net.load_state_dict(seeded_state(net, seed))
    net.cuda()
    for size, n in CASES:
        x = torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(size))
        out = net(x.cuda())
        err = rel(out, feats[size])
        print(f"inception features at {size}x{size} vs the reference fixture: rel err {err:.1e}")
        assert out.shape == feats[size].shape and err < TOL


@pytest.mark.gpu
def test_inception_pool_features_match_oracle():
    """2048-d pool features of two 64x64 and two 299x299 images, seeded weights, HIP vs CPU oracle at 1e-3."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3, InceptionFeatures
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    torch.set_num_threads(min(16, torch.get_num_threads()))
    oracle = Oracle().eval()
    sd = seeded_state(oracle, 3)
    oracle.load_state_dict(sd)
    net = FIDInceptionV3()
    net.load_state_dict(sd)                       # the same keys: how the reference's weight file would load
    net.cuda()
    for size in (64, 299):
        x = torch.rand(2, 3, size, size, generator=torch.Generator().manual_seed(size))
        with torch.no_grad():
            ref = oracle(x)
        out = net(x.cuda())
        assert out.shape == (2, 2048)
        err = rel(out, ref)
        print(f"inception features at {size}x{size}: rel err {err:.1e}, |ref| max {float(ref.abs().max()):.2f}, "
              f"mean {float(ref.mean()):.3f}")
        assert err < TOL and float(ref.abs().max()) > 1e-3
    # the evaluate() plumbing: uint8 NHWC images -> float64 activations, batches of 16
    u8 = np.random.RandomState(0).randint(0, 256, size=(5, 32, 32, 3)).astype(np.uint8)
    act = InceptionFeatures(net, batch_size=2)(u8)
    with torch.no_grad():
        ref = oracle(torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255)
    assert act.shape == (5, 2048) and act.dtype == np.float64 and rel(torch.from_numpy(act), ref) < TOL
    # a parameter change invalidates the folded weights
    with torch.no_grad():
        net.Conv2d_1a_3x3.bn.weight.mul_(1.5)
        oracle.Conv2d_1a_3x3.bn.weight.mul_(1.5)
        assert rel(net(x.cuda()), oracle(x)) < TOL


@pytest.mark.gpu
def test_hip_inception_reproduces_the_published_shape_table():
    """The product network's module outputs at 299 x 299 against torchvision's published per-layer shapes."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    shape_in, table = published_shapes()
    net = FIDInceptionV3().cuda()
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, i, o, n=n: seen.__setitem__(n, tuple(o.shape[1:])))
             for n, m in net.named_children() if n != "fc"]
    x = torch.rand(2, *shape_in, generator=torch.Generator().manual_seed(3)).cuda()
    feats = net(x, resize_input=False, normalize_input=False)
    for h in hooks:
        h.remove()
    want = dict(table)
    assert {n for n, _ in table if n.startswith(("Conv2d", "Mixed"))} == set(seen)
    assert all(seen[n] == want[n] for n in seen), {n: (seen[n], want[n]) for n in seen if seen[n] != want[n]}
    assert tuple(feats.shape) == (2, 2048)


@pytest.mark.gpu
@pytest.mark.skipif(not os.environ.get("GZ_FID_WEIGHTS"), reason="set GZ_FID_WEIGHTS=<pt_inception-2015-12-05-6726825d.pth> "
                    "(the reference fetches it from a URL, metrics/inception.py:13; no network here)")
def test_fid_end_to_end_with_the_published_weight_file():
    """the first box that HAS the weight file closes the loop -- sha256 gate, the HIP feature
    extractor on the real weights against the CPU oracle on the same file (1e-3), and eval.fid_from_weight_file on a
    DCGAN generator: FID of a sample set against itself ~ 0, against a perturbed set > 0, finite KID."""
    from helpers import synthetic_real
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd.config import locate, make_cfg
    from lightning_gan_zoo_amd.inception import fid_weights_state, load_fid_weights
    from oracle.inception_cpu import FIDInceptionV3 as Oracle
    path = os.environ["GZ_FID_WEIGHTS"]
    net = load_fid_weights(path)                       # raises unless the file is the published one
    oracle = Oracle().eval()
    oracle.load_state_dict(fid_weights_state(path))
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        assert rel(net(x.cuda()), oracle(x)) < TOL
    cfg = make_cfg("dc_gan", batch_size=16)
    torch.manual_seed(42)
    module = locate(cfg.model.lm["_target_"])(cfg, None).cuda()
    real = ((synthetic_real(64, seed=1) * 0.5 + 0.5).clamp(0, 1) * 255).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    np.random.seed(0)
    out = E.fid_from_weight_file(module, real, weights=path, n_samples=64, n_subsets=4)
    assert np.isfinite(out["fid"]) and out["fid"] > 0 and np.isfinite(out["kid"])
    same = E.fid_from_weight_file(module, None, weights=path, n_samples=64, n_subsets=4)      # generated vs generated
    assert abs(same["fid"]) < 1e-3 * max(1.0, out["fid"])


@pytest.mark.gpu
def test_inception_features_do_not_depend_on_the_batch_size():
    """Round 6: at the evaluation batch most convolutions take the igemm2 skeleton (ConvTapAnyA2 + EpiNCHWBiasAct) and the
    pooling takes the plane-per-workgroup kernel; at batch 2 -- the size of the reference-fixture test above -- they take
    the round-5 kernels.  Same seeded weights, same images: the 2048-d pool features of a batch of 96 must equal those of
    the same images pushed through two at a time (1e-3; observed ~1e-6)."""
    from lightning_gan_zoo_amd.inception import FIDInceptionV3
    seed, _ = reference_features()
    net = FIDInceptionV3()
    net.load_state_dict(seeded_state(net, seed))
    net = net.cuda()
    x = torch.rand(96, 3, 64, 64, generator=torch.Generator().manual_seed(11)).cuda()
    big = net(x)
    small = torch.cat([net(x[i:i + 2]) for i in range(0, 96, 2)])
    assert big.shape == (96, 2048) and rel(big, small) < TOL, rel(big, small)

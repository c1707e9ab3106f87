"""Resident training set, device half: gz_u8hwc_gather_to_nchw against the streaming kernel over the gathered rows
(bit-equal), 64-bit row offsets, the guarded index, error codes, ResidentImages' batch sequence against
ImageFolderImages', one launch per batch, and the runner end to end."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from test_resident_data import make_folder, write_mnist

pytestmark = pytest.mark.gpu


def reference(set_u8, idx, mean, std):
    """What the issue compares with: the streaming kernel over the rows set[idx]."""
    from lightning_gan_zoo_amd import functional as F
    return F.normalize_u8_images(set_u8[idx], mean, std)


@pytest.mark.parametrize("shape", [(3, 5, 7, 3), (4, 1, 1, 1), (6, 12, 20, 1), (9, 16, 16, 3), (5, 8, 8, 4)])
def test_gather_equals_streaming_kernel(shape):
    from lightning_gan_zoo_amd import functional as F
    M, H, W, C = shape
    g = torch.Generator().manual_seed(M * 1000 + H * W * C)
    set_u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
    labels = torch.randint(0, 1000, (M,), dtype=torch.int64, generator=g).cuda()
    for n in (1, 5, 257):                                        # n > M and repeated indices; 257 rows: several blocks
        idx = torch.randint(0, M, (n,), dtype=torch.int64, generator=g).cuda()
        for mean, std in ((0.4, 0.25), (0.5, 0.5)):
            want = reference(set_u8, idx, mean, std)
            x, lab = F.gather_normalize_u8(set_u8, idx, mean, std, labels)
            assert x.shape == (n, C, H, W) and x.dtype == torch.float32
            assert torch.equal(x, want)
            assert torch.equal(lab, labels[idx])
            x2, none = F.gather_normalize_u8(set_u8, idx, mean, std)          # labels = NULL
            assert none is None and torch.equal(x2, want)
            formula = (set_u8[idx].permute(0, 3, 1, 2).float() / 255 - mean) / std
            err = float((x - formula).abs().max())
            print("shape %s n %d mean %.2f std %.2f: max |kernel - torch formula| = %.3e" % (shape, n, mean, std, err))
            assert err < 1e-6


def test_argument_checks():
    from lightning_gan_zoo_amd import functional as F
    set_u8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8, device="cuda")
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="uint8 NHWC"):
        F.gather_normalize_u8(set_u8.float(), idx, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="uint8 NHWC"):
        F.gather_normalize_u8(set_u8.cpu(), idx, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="contiguous"):
        F.gather_normalize_u8(set_u8.permute(0, 2, 1, 3), idx, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="int64"):
        F.gather_normalize_u8(set_u8, idx.int(), 0.5, 0.5)
    with pytest.raises(RuntimeError, match="int64"):
        F.gather_normalize_u8(set_u8, idx.cpu(), 0.5, 0.5)


def test_row_offsets_are_64_bit():
    from lightning_gan_zoo_amd import functional as F
    M, row = 349_600, 64 * 64 * 3
    assert M * row > 2 ** 32
    set_u8 = torch.empty((M, 64, 64, 3), dtype=torch.uint8, device="cuda")     # 4.30 GB, allocated and not filled
    rows = [0, (2 ** 31) // row + 1, (2 ** 32) // row + 1, M - 1]
    assert rows[1] * row > 2 ** 31 and rows[2] * row > 2 ** 32
    g = torch.Generator().manual_seed(7)
    fill = torch.randint(0, 256, (4, 64, 64, 3), dtype=torch.uint8, generator=g).cuda()
    for k, r in enumerate(rows):
        set_u8[r].copy_(fill[k])
    labels = torch.arange(M, dtype=torch.int64, device="cuda")
    x, lab = F.gather_normalize_u8(set_u8, torch.tensor(rows, dtype=torch.int64, device="cuda"), 0.5, 0.5, labels)
    assert torch.equal(x, F.normalize_u8_images(fill, 0.5, 0.5))
    assert lab.tolist() == rows
    del set_u8
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(3, 5, 7, 3), (4, 16, 16, 3)])
def test_index_outside_the_set_is_guarded(shape):
    """idx = [0, -1, M, 2]: rows 1 and 2 are NaN with label -1 and nothing is read for them (the kernel compares the
    index with [0, M) before it forms an address); rows 0 and 3 are exact; the call succeeds."""
    from lightning_gan_zoo_amd import functional as F
    M = shape[0]
    g = torch.Generator().manual_seed(9)
    set_u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
    labels = torch.tensor([10, 11, 12, 13][:M], dtype=torch.int64, device="cuda")
    idx = torch.tensor([0, -1, M, 2], dtype=torch.int64, device="cuda")
    x, lab = F.gather_normalize_u8(set_u8, idx, 0.4, 0.25, labels)
    torch.cuda.synchronize()
    good = torch.tensor([0, 2], dtype=torch.int64, device="cuda")
    assert torch.equal(x[[0, 3]], reference(set_u8, good, 0.4, 0.25))
    assert bool(torch.isnan(x[1:3]).all()) and lab.tolist() == [10, -1, -1, 12]
    x2, lab2 = F.gather_normalize_u8(set_u8, good, 0.4, 0.25, labels)      # a following ordinary call is exact
    assert torch.equal(x2, reference(set_u8, good, 0.4, 0.25)) and lab2.tolist() == [10, 12]


def test_error_codes():
    from lightning_gan_zoo_amd._lib import lib
    set_u8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8, device="cuda")
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = torch.full((2, 5, 8, 8), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def call(M=4, n=2, H=8, W=8, C=3, std=0.5):
        return lib.gz_u8hwc_gather_to_nchw(p(set_u8), M, p(idx), None, p(out), None, n, H, W, C, 0.5, std, None)

    BAD_SHAPE, TOO_LARGE = -1, -5
    assert call(std=0.0) == BAD_SHAPE and call(C=5) == BAD_SHAPE and call(n=0) == BAD_SHAPE
    assert call(C=0) == BAD_SHAPE and call(M=0) == BAD_SHAPE and call(H=0) == BAD_SHAPE and call(W=-1) == BAD_SHAPE
    assert call(n=2 ** 20, H=2 ** 6, W=2 ** 5) == TOO_LARGE                 # n*H*W = 2^31: refused before any launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                        # nothing was launched
    assert call() == 0


def batches(it, k):
    return [next(it) for _ in range(k)]


def test_batch_sequence_equals_the_streaming_path(tmp_path):
    from cpu_harness import HostNormalisedFolder
    from lightning_gan_zoo_amd.resident_data import ResidentImages
    from lightning_gan_zoo_amd.run_network import ImageFolderImages
    root = str(tmp_path / "data")
    make_folder(root)
    res = batches(iter(ResidentImages(root, 4, 16, 3, 0.5, 0.5, "cuda")), 10)
    ref = batches(iter(ImageFolderImages(root, 4, 16, 3, 0.5, 0.5, "cuda")), 10)
    assert [len(x) for x, _ in res] == [4, 2] * 5                 # epochs follow each other, the partial batch is kept
    for (x, l), (xr, lr) in zip(res, ref):
        assert torch.equal(x, xr) and torch.equal(l, lr) and l.dtype == torch.int64
    cache = str(tmp_path / "cache")
    ResidentImages(root, 4, 16, 3, 0.5, 0.5, "cuda", rank=0, world=2, cache_dir=cache)      # rank 0 writes the file
    shard = ResidentImages(root, 2, 16, 3, 0.5, 0.5, "cuda", rank=1, world=2, cache_dir=cache)
    shard.set_epoch(3)
    host = HostNormalisedFolder(ImageFolderImages(root, 2, 16, 3, 0.5, 0.5, "cpu", rank=1, world=2))
    host.set_epoch(3)
    seen = []
    for (x, l), (xh, lh) in zip(batches(iter(shard), 5), batches(iter(host), 5)):      # epochs 3, 4 and half of 5
        err = float((x.cpu() - xh).abs().max())
        print("rank 1 of 2: max |resident - host| = %.3e" % err)
        assert x.shape == xh.shape and torch.equal(l.cpu(), lh) and err < 1e-6
        seen.append(l.tolist())
    assert [len(s) for s in seen] == [2, 1, 2, 1, 2]


class CountingLib:
    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("gz_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)

        return counted


def test_one_launch_per_batch(tmp_path, monkeypatch):
    """After the first batch of an epoch, next() is ONE gz_ launch and no framework kernel: every aten operator it
    dispatches is an allocation or a view."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from lightning_gan_zoo_amd.functional import _misc
    from lightning_gan_zoo_amd.resident_data import ResidentImages
    root = str(tmp_path / "data")
    make_folder(root)
    proxy = CountingLib(_misc.lib)
    monkeypatch.setattr(_misc, "lib", proxy)
    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))

    it = iter(ResidentImages(root, 2, 16, 3, 0.5, 0.5, "cuda"))
    next(it)                                                       # upload, the epoch's order
    for _ in range(4):                                             # batches 2, 3 of epoch 0 and 1, 2 of epoch 1
        del proxy.calls[:], seen[:]
        with Record():
            x, l = next(it)
        assert proxy.calls == ["gz_u8hwc_gather_to_nchw"]
        assert set(seen) <= {"empty", "slice"}, seen
        assert x.shape == (2, 3, 16, 16) and l.shape == (2,)


def logged_losses(text):
    rows = re.findall(r"^step (\d+) epoch \d+ (.*?) \(", text, flags=re.M)
    return [(int(s), [float(v) for v in re.findall(r"_loss=(\S+)", body)]) for s, body in rows]


SMALL = ["+expt=dc_gan", "resident_data=true", "train.batch_size=4", "train.img_size=64", "train.features_gen=8",
         "train.features_disc=8", "+max_steps=6", "log_every=1"]


def test_runner_end_to_end_image_folder(tmp_path, monkeypatch, capsys):
    from lightning_gan_zoo_amd import run_network as R
    root = str(tmp_path / "data")
    make_folder(root)                                              # 6 images
    monkeypatch.chdir(tmp_path)
    module, trainer, step = R.main(SMALL + ["dataset=image_folder", "dataset_path=" + root])
    rows = logged_losses(capsys.readouterr().out)
    assert step == 6 and [s for s, _ in rows] == [1, 2, 3, 4, 5, 6]
    assert all(v and all(math.isfinite(x) for x in v) for _, v in rows)
    assert module.cfg.train.channels_img == 3


def test_runner_end_to_end_mnist(tmp_path, monkeypatch, capsys):
    from lightning_gan_zoo_amd import run_network as R
    rng = np.random.RandomState(5)
    write_mnist(str(tmp_path), rng.randint(0, 256, size=(7, 28, 28), dtype=np.uint8), rng.randint(0, 10, size=7))
    monkeypatch.chdir(tmp_path)
    module, trainer, step = R.main(SMALL + ["dataset=mnist", "dataset_path=" + str(tmp_path)])
    rows = logged_losses(capsys.readouterr().out)
    assert step == 6 and len(rows) == 6 and all(v and all(math.isfinite(x) for x in v) for _, v in rows)
    assert module.cfg.train.channels_img == 1

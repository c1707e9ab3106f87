"""Resident training set, host half (resident_data.py): the decoded uint8 set is the streaming path's bytes, the
decode pool cannot change it, the cache file is keyed by content, the guards end in a SystemExit, MNIST raw files are read
as torchvision reads them."""
import glob
import gzip
import os
import struct

import numpy as np
import pytest


def make_folder(root):
    """Built like test_input_step.make_folder: mixed sizes, png and jpg, a non-image file, a nested class directory."""
    from PIL import Image
    rng = np.random.RandomState(3)
    spec = {"b_class": ["z.png", "a.png", "m.jpg"], "a_class": ["2.png", "10.png", "notes.txt"], "c_class/sub": ["k.png"]}
    for d, names in spec.items():
        os.makedirs(os.path.join(root, d), exist_ok=True)
        for n in names:
            path = os.path.join(root, d, n)
            if n.endswith(".txt"):
                open(path, "w").write("not an image")
                continue
            h, w = rng.randint(20, 50, size=2)
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8)).save(path)


def write_mnist(parent, planes, labels, gz=False, train=True, image_magic=2051, label_magic=2049):
    raw = os.path.join(parent, "MNIST", "raw")
    os.makedirs(raw, exist_ok=True)
    stem = "train" if train else "t10k"
    opener = gzip.open if gz else open
    ext = ".gz" if gz else ""
    with opener(os.path.join(raw, stem + "-images-idx3-ubyte" + ext), "wb") as f:
        f.write(struct.pack(">iiii", image_magic, len(planes), planes.shape[1], planes.shape[2]) + planes.tobytes())
    with opener(os.path.join(raw, stem + "-labels-idx1-ubyte" + ext), "wb") as f:
        f.write(struct.pack(">ii", label_magic, len(labels)) + bytes(bytearray(int(x) for x in labels)))
    return raw


def resident(root, channels=3, size=16, **kw):
    from lightning_gan_zoo_amd.resident_data import ResidentImages
    return ResidentImages(root, 4, size, channels, 0.5, 0.5, "cpu", **kw)


@pytest.mark.parametrize("channels", [3, 1])
def test_set_is_the_streaming_paths_bytes(tmp_path, channels):
    from lightning_gan_zoo_amd.run_network import ImageFolderImages, image_folder_samples
    root = str(tmp_path)
    make_folder(root)
    samples, classes = image_folder_samples(root)
    stream = ImageFolderImages(root, 4, 16, channels, 0.5, 0.5, "cpu")
    want = np.stack([stream.decode(p) for p, _ in samples])
    data = resident(root, channels)
    u8, labels = data.host_set()
    assert u8.dtype == np.uint8 and u8.shape == (6, 16, 16, channels) and u8.tobytes() == want.tobytes()
    assert labels.dtype == np.int64 and labels.tolist() == [c for _, c in samples] and data.classes == classes
    assert len(data) == len(stream) == 6
    one = resident(root, channels, workers=1).host_set()[0]
    assert one.tobytes() == u8.tobytes()                         # 1 worker == the pool
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # the device half needs the GPU
        next(iter(data))
    halves = [resident(root, channels, rank=r, world=2, cache_dir=str(tmp_path / "cache")) for r in range(2)]
    assert [h.order for h in halves] == [[0, 2, 4], [1, 3, 5]]


def test_pool_is_sized_by_affinity_not_cpu_count(monkeypatch):
    from lightning_gan_zoo_amd import resident_data as RD
    monkeypatch.setattr(os, "cpu_count", lambda: 4096)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(3)))
    assert RD.pool_workers() == 3
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(200)))
    assert RD.pool_workers() == 16


def test_cache_round_trip_and_rebuild(tmp_path, monkeypatch):
    from PIL import Image
    from lightning_gan_zoo_amd.run_network import ImageFolderImages
    root, cache = str(tmp_path / "data"), str(tmp_path / "cache")
    make_folder(root)
    before = sorted(glob.glob(str(tmp_path / "**" / "*"), recursive=True))
    first = resident(root).host_set()[0]
    assert sorted(glob.glob(str(tmp_path / "**" / "*"), recursive=True)) == before     # no data_cache: nothing written
    first_c = resident(root, cache_dir=cache)
    assert first_c.host_set()[0].tobytes() == first.tobytes()
    entries = sorted(os.listdir(cache))
    assert len(entries) == 2 and entries[0].endswith(".json") and entries[1].endswith(".u8.npy")
    assert entries[0][:-len(".json")] == entries[1][:-len(".u8.npy")]
    assert not [f for f in os.listdir(cache) if f.endswith(".tmp")]

    real_decode = ImageFolderImages.decode
    calls = []

    def refuse(self, path):
        calls.append(path)
        raise AssertionError("decode called although the cache holds this set")

    monkeypatch.setattr(ImageFolderImages, "decode", refuse)
    again = resident(root, cache_dir=cache)
    u8, labels = again.host_set()
    assert u8.tobytes() == first.tobytes() and labels.tolist() == first_c.host_set()[1].tolist()
    assert again.classes == first_c.classes and not calls
    other = resident(root, cache_dir=cache, rank=1, world=2)              # a rank other than 0 never decodes
    assert other.host_set()[0].tobytes() == first.tobytes() and not calls
    with pytest.raises(AssertionError):                                   # another resolution is another cache entry
        resident(root, size=8, cache_dir=cache)
    calls.clear()

    # one image rewritten with other pixels: another digest, the stale entry is not used, the set is rebuilt
    rng = np.random.RandomState(11)
    Image.fromarray(rng.randint(0, 256, size=(33, 47, 3), dtype=np.uint8)).save(os.path.join(root, "b_class", "a.png"))
    with pytest.raises(AssertionError):
        resident(root, cache_dir=cache)
    assert calls
    monkeypatch.setattr(ImageFolderImages, "decode", real_decode)
    rebuilt = resident(root, cache_dir=cache).host_set()[0]
    assert rebuilt[[0, 1, 3, 4, 5]].tobytes() == first[[0, 1, 3, 4, 5]].tobytes()
    assert rebuilt[2].tobytes() != first[2].tobytes()
    assert len(os.listdir(cache)) == 4 and not [f for f in os.listdir(cache) if f.endswith(".tmp")]


def test_guards(tmp_path):
    root = str(tmp_path / "data")
    make_folder(root)
    with pytest.raises(SystemExit, match="GB"):                  # 6 x 16x16x3 bytes = 4608 B > 1e-6 GB
        resident(root, max_gb=1e-6)
    with pytest.raises(SystemExit, match="data_cache"):
        resident(root, rank=0, world=2)
    with pytest.raises(SystemExit, match="no cache entry"):      # rank 1 does not decode, with or without a cache dir
        resident(root, rank=1, world=2, cache_dir=str(tmp_path / "empty"))
    assert not os.path.exists(str(tmp_path / "empty")) or not os.listdir(str(tmp_path / "empty"))


@pytest.mark.parametrize("gz", [False, True])
def test_mnist_raw_files(tmp_path, gz):
    from PIL import Image
    parent = str(tmp_path)
    rng = np.random.RandomState(5)
    planes = rng.randint(0, 256, size=(7, 28, 28), dtype=np.uint8)
    digits = rng.randint(0, 10, size=7)
    write_mnist(parent, planes, digits, gz=gz)
    data = resident(parent, channels=1, source="mnist")
    u8, labels = data.host_set()
    want = np.stack([np.asarray(Image.fromarray(p, mode="L").resize((16, 16), Image.BILINEAR), dtype=np.uint8)
                     for p in planes])[..., None]
    assert u8.shape == (7, 16, 16, 1) and u8.tobytes() == want.tobytes()
    assert labels.dtype == np.int64 and labels.tolist() == digits.tolist()
    cache = str(tmp_path / "cache")
    a = resident(parent, channels=1, source="mnist", cache_dir=cache).host_set()
    b = resident(parent, channels=1, source="mnist", cache_dir=cache, rank=1, world=2).host_set()
    assert a[0].tobytes() == b[0].tobytes() == want.tobytes() and b[1].tolist() == digits.tolist()


def test_mnist_errors(tmp_path):
    planes = np.zeros((2, 28, 28), dtype=np.uint8)
    with pytest.raises(SystemExit, match="train-images-idx3-ubyte"):      # names the paths it expects
        resident(str(tmp_path / "nowhere"), channels=1, source="mnist")
    bad = str(tmp_path / "bad")
    write_mnist(bad, planes, [1, 2], image_magic=2052)
    with pytest.raises(SystemExit, match="2051"):
        resident(bad, channels=1, source="mnist")
    bad2 = str(tmp_path / "bad2")
    write_mnist(bad2, planes, [1, 2], label_magic=2050)
    with pytest.raises(SystemExit, match="2049"):
        resident(bad2, channels=1, source="mnist")
    only_test = str(tmp_path / "only_test")
    write_mnist(only_test, planes, [1, 2], train=False)
    with pytest.raises(SystemExit, match="not found"):
        resident(only_test, channels=1, source="mnist")
    assert resident(only_test, channels=1, source="mnist", train=False).host_set()[1].tolist() == [1, 2]


def test_runner_keys_and_mnist_config(tmp_path):
    from lightning_gan_zoo_amd import run_network as R
    conf_dir, expt, rest, run = R.parse_overrides(["+expt=dc_gan", "dataset=mnist", "resident_data=true",
                                                   "data_cache=/tmp/c", "+resident_max_gb=4"])
    assert run["resident_data"] is True and run["data_cache"] == "/tmp/c" and run["resident_max_gb"] == 4
    assert R.RUNNER_KEYS["resident_data"] is False and R.RUNNER_KEYS["data_cache"] is None
    assert R.RUNNER_KEYS["resident_max_gb"] == 32
    cfg = R.compose(conf_dir, expt, rest, run)
    assert cfg.train.channels_img == 1 and cfg.dataset["_target_"] == "torchvision.datasets.MNIST"
    _, expt, rest, run = R.parse_overrides(["+expt=dc_gan", "dataset=mnist", "resident_data=true",
                                            "filepaths.mnist_parent_directory=/data/mnist"])
    cfg = R.compose(None, expt, rest, run)
    assert cfg.dataset.root == "/data/mnist/MNIST" and cfg.dataset.train.root == "/data/mnist"
    assert cfg.dataset.train.train is True and cfg.dataset.val.train is False and cfg.dataset.n_channels == 1
    # the MNIST target is served by the resident path only, and says so
    run["resident_data"] = False
    with pytest.raises(SystemExit, match="resident_data=true"):
        R.build_data(cfg, run, "cpu")
    # build_data dispatch: ImageFolder stays the streaming class unless the key is given
    root = str(tmp_path / "data")
    make_folder(root)
    _, expt, rest, run = R.parse_overrides(["+expt=dc_gan", "dataset=image_folder", "dataset_path=" + root,
                                            "train.img_size=16"])
    cfg = R.compose(None, expt, rest, run)
    assert type(R.build_data(cfg, run, "cpu")).__name__ == "ImageFolderImages"
    run["resident_data"] = True
    data = R.build_data(cfg, run, "cpu")
    assert type(data).__name__ == "ResidentImages" and data.host_set()[0].shape == (6, 16, 16, 3)
    run["resident_max_gb"] = 1e-6
    with pytest.raises(SystemExit, match="resident_max_gb"):
        R.build_data(cfg, run, "cpu")

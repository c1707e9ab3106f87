"""Resident training set (runner key ``resident_data=true``): the reference's input step has no augmentation and no
randomness (Resize -> ToTensor -> Normalize, core/lightning_module.py:42-47), so the bytes a decode produces in epoch
7 are the bytes of epoch 0.  Decode and resize every file ONCE into one uint8 [M, S, S, C] array (a bounded thread
pool; optionally kept as a cache file), upload it once, and serve every batch with one launch that gathers the
batch's rows by a device-side index vector, normalises and transposes (functional.gather_normalize_u8).

Host half (testable anywhere): ``image_folder_source`` / ``mnist_source`` / ``build_set`` / the cache.  Device half:
``ResidentImages``, the drop-in for run_network.ImageFolderImages.
"""
import gzip
import hashlib
import json
import os
import struct
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

UPLOAD_CHUNK_BYTES = 64 << 20          # the one pinned staging buffer of the upload
MNIST_FILES = {True: ("train-images-idx3-ubyte", "train-labels-idx1-ubyte"),
               False: ("t10k-images-idx3-ubyte", "t10k-labels-idx1-ubyte")}


def pool_workers():
    """Decode threads: the CPUs this process may run on, 16 at the most (never the machine's CPU count)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


# ---------------------------------------------------------------------------------------------------------
# sample sources: (items, decode(item) -> uint8 [S, S, C], labels, class names, files the digest covers)
# ---------------------------------------------------------------------------------------------------------
def image_folder_source(root, size, channels):
    """ImageFolder ordering (run_network.image_folder_samples) and exactly ImageFolderImages.decode: the bytes are the
    streaming path's bytes by construction."""
    from .run_network import ImageFolderImages, image_folder_samples
    samples, classes = image_folder_samples(root)
    if not samples:
        raise FileNotFoundError("no images under %r" % root)
    holder = types.SimpleNamespace(size=size, channels=channels)      # what decode() reads of its object

    def decode(path):
        return ImageFolderImages.decode(holder, path)

    paths = [p for p, _ in samples]
    return {"kind": "image_folder", "root": root, "items": paths, "decode": decode,
            "labels": np.array([c for _, c in samples], dtype=np.int64), "classes": classes, "files": paths}


def _open_raw(path):
    return gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")


def _find_raw(raw_dir, name):
    for cand in (os.path.join(raw_dir, name), os.path.join(raw_dir, name + ".gz")):
        if os.path.isfile(cand):
            return cand
    return None


def read_mnist_raw(root, train=True):
    """torchvision.datasets.MNIST's files under ``<root>/MNIST/raw`` (plain or .gz) -> (uint8 [M, 28, 28], int64 [M],
    [images path, labels path]).  Nothing is ever downloaded."""
    raw_dir = os.path.join(root, "MNIST", "raw")
    names = MNIST_FILES[bool(train)]
    found = [_find_raw(raw_dir, n) for n in names]
    if None in found:
        raise SystemExit("MNIST files not found (nothing is downloaded; `download: true` is not acted on): expected %s "
                         "(or the same with .gz)" % " and ".join(os.path.join(raw_dir, n) for n in names))
    with _open_raw(found[0]) as f:
        blob = f.read()
    if len(blob) < 16 or struct.unpack(">i", blob[:4])[0] != 2051:
        raise SystemExit("%s is not an idx3 image file (magic number %s, expected 2051)"
                         % (found[0], struct.unpack(">i", blob[:4])[0] if len(blob) >= 4 else "missing"))
    m, h, w = struct.unpack(">iii", blob[4:16])
    if len(blob) != 16 + m * h * w:
        raise SystemExit("%s: header says %d images of %dx%d, the file holds %d bytes" % (found[0], m, h, w, len(blob)))
    planes = np.frombuffer(blob, dtype=np.uint8, offset=16).reshape(m, h, w)
    with _open_raw(found[1]) as f:
        blob = f.read()
    if len(blob) < 8 or struct.unpack(">i", blob[:4])[0] != 2049:
        raise SystemExit("%s is not an idx1 label file (magic number %s, expected 2049)"
                         % (found[1], struct.unpack(">i", blob[:4])[0] if len(blob) >= 4 else "missing"))
    if struct.unpack(">i", blob[4:8])[0] != m or len(blob) != 8 + m:
        raise SystemExit("%s does not hold %d labels, one per image of %s" % (found[1], m, found[0]))
    return planes, np.frombuffer(blob, dtype=np.uint8, offset=8).astype(np.int64), found


def mnist_source(root, size, channels, train=True):
    """``torchvision.datasets.MNIST.__getitem__`` (``Image.fromarray(plane, mode="L")``) followed by
    ``transforms.Resize((S, S))`` (PIL bilinear)."""
    if channels != 1:
        raise SystemExit("MNIST has 1 channel; train.channels_img is %d" % channels)
    planes, labels, files = read_mnist_raw(root, train)

    def decode(i):
        from PIL import Image
        img = Image.fromarray(planes[i], mode="L").resize((size, size), Image.BILINEAR)
        return np.asarray(img, dtype=np.uint8)[:, :, None]

    return {"kind": "mnist_train" if train else "mnist_test", "root": os.path.join(root, "MNIST", "raw"),
            "items": list(range(len(planes))), "decode": decode, "labels": labels,
            "classes": [str(d) for d in range(10)], "files": files}


def build_set(source, size, channels, workers=None):
    """uint8 [M, S, S, C]: every item decoded once; each worker writes its sample's own row of a preallocated array, so
    the worker count cannot change the result."""
    items, decode = source["items"], source["decode"]
    out = np.empty((len(items), size, size, channels), dtype=np.uint8)

    def one(i):
        out[i] = decode(items[i])

    workers = pool_workers() if workers is None else int(workers)
    if workers <= 1:
        for i in range(len(items)):
            one(i)
    else:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            for _ in ex.map(one, range(len(items)), chunksize=1):
                pass
    return out


# ---------------------------------------------------------------------------------------------------------
# cache file: <dir>/<digest>.u8.npy + <digest>.json
# ---------------------------------------------------------------------------------------------------------
def set_digest(source, size, channels):
    """Covers the ordered relative paths, each file's size and mtime, S, C, the source kind and PIL's version: a changed,
    added, removed or reordered file, another resolution or another resampler implementation is another cache."""
    import PIL
    h = hashlib.sha256()
    h.update(json.dumps([source["kind"], int(size), int(channels), PIL.__version__]).encode())
    for path in source["files"]:
        st = os.stat(path)
        h.update(json.dumps([os.path.relpath(path, source["root"]), st.st_size, st.st_mtime_ns]).encode())
    return h.hexdigest()[:32]


def cache_paths(cache_dir, digest):
    return os.path.join(cache_dir, digest + ".u8.npy"), os.path.join(cache_dir, digest + ".json")


def load_cache(cache_dir, digest, shape):
    """(memory-mapped uint8 array, labels, classes), or None when ``cache_dir`` holds no complete entry for this
    digest and shape.  An entry under another digest is simply not looked at."""
    npy, meta_path = cache_paths(cache_dir, digest)
    if not (os.path.isfile(npy) and os.path.isfile(meta_path)):
        return None
    with open(meta_path) as f:
        meta = json.load(f)
    if meta.get("digest") != digest or list(meta.get("shape", [])) != list(shape):
        return None
    arr = np.load(npy, mmap_mode="r")
    if arr.dtype != np.uint8 or list(arr.shape) != list(shape):
        return None
    return arr, np.asarray(meta["labels"], dtype=np.int64), list(meta["classes"])


def _replace_into(path, write):
    tmp = "%s.%d.tmp" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_cache(cache_dir, digest, arr, labels, classes, source, size, channels):
    import PIL
    os.makedirs(cache_dir, exist_ok=True)
    npy, meta_path = cache_paths(cache_dir, digest)
    meta = {"digest": digest, "kind": source["kind"], "root": source["root"], "size": int(size),
            "channels": int(channels), "pil": PIL.__version__, "shape": list(arr.shape),
            "labels": [int(x) for x in labels], "classes": list(classes)}
    _replace_into(npy, lambda f: np.save(f, arr))                      # the array first: the json marks it complete
    _replace_into(meta_path, lambda f: f.write(json.dumps(meta).encode()))


def upload(host, device, chunk_bytes=UPLOAD_CHUNK_BYTES):
    """The whole array to the device through ONE pinned staging buffer of ``chunk_bytes`` (a 10 GB set does not need
    10 GB of pinned memory; ``host`` may be a memory-mapped cache file)."""
    dev = torch.empty(host.shape, dtype=torch.uint8, device=device)
    flat = dev.view(-1)
    row = int(np.prod(host.shape[1:]))
    rows = max(1, chunk_bytes // row)
    stage = torch.empty(rows * row, dtype=torch.uint8).pin_memory()
    stage_np = stage.numpy()
    for a in range(0, host.shape[0], rows):
        b = min(a + rows, host.shape[0])
        k = (b - a) * row
        np.copyto(stage_np[:k].reshape((b - a,) + tuple(host.shape[1:])), host[a:b])     # file / array -> pinned
        flat[a * row:a * row + k].copy_(stage[:k], non_blocking=True)
        torch.cuda.current_stream(device).synchronize()               # the buffer is rewritten by the next chunk
    return dev


# ---------------------------------------------------------------------------------------------------------
# the data set
# ---------------------------------------------------------------------------------------------------------
class ResidentImages:
    """ImageFolderImages' batch sequence -- dataset order in one process, ``shard_indices(M, rank, world, epoch)`` per
    epoch under data parallelism, the incomplete last batch kept, epoch after epoch -- served from a uint8 set that
    lives in HBM.  Once per epoch the epoch's order goes to the device as one int64 tensor; each batch is one
    ``gz_u8hwc_gather_to_nchw`` launch over a view of it: no host decode, no pinned ring, no host->device copy, no host
    synchronisation per step.

    ``source``: "image_folder" (``root`` = the class folders' parent) or "mnist" (``root`` = the directory holding
    ``MNIST/raw``; ``train`` picks the split).  ``cache_dir``: where the decoded set is kept between runs (None: nowhere,
    nothing is written).  ``max_gb``: a larger set is refused -- there is no silent fallback to the streaming path.
    Data parallel: every rank holds the full set (the sampler permutes the whole set each epoch); rank 0 decodes and
    writes the cache, the others wait (``group``: a process group with a long timeout) and load the file."""

    def __init__(self, root, batch, img_size, channels, mean, std, device, rank=0, world=1, source="image_folder",
                 cache_dir=None, max_gb=32, workers=None, train=True, group=None):
        from .run_network import shard_indices
        self.batch, self.size, self.channels = int(batch), int(img_size), int(channels)
        self.mean, self.std, self.device = mean, std, torch.device(device)
        self.rank, self.world, self.epoch = rank, world, 0
        if world > 1 and not cache_dir:
            raise SystemExit("resident_data with %d data-parallel ranks needs data_cache=<dir>: rank 0 decodes the set "
                             "once and the other ranks load the file" % world)
        self._u8, self._labels, self.classes, err = None, None, None, None
        try:
            if rank == 0:
                self._u8, self._labels, self.classes = self._obtain(root, source, train, cache_dir, max_gb, workers, True)
        except BaseException as e:  # noqa: BLE001  (SystemExit included: the other ranks must hear of it)
            err = e
        if world > 1 and torch.distributed.is_available() and torch.distributed.is_initialized():
            # rank 0 says whether the file is there; the others leave with it instead of waiting out the long timeout
            flag = torch.tensor([0 if err is None else 1])
            torch.distributed.broadcast(flag, 0, group=group)
            if int(flag.item()) and err is None:
                raise SystemExit("resident_data: rank 0 could not build the training set")
        if err is not None:
            raise err
        if rank != 0:
            self._u8, self._labels, self.classes = self._obtain(root, source, train, cache_dir, max_gb, workers, False)
        self.order = shard_indices(len(self._u8), rank, world)             # (length / unshuffled view)
        self._dev = None

    def _obtain(self, root, kind, train, cache_dir, max_gb, workers, may_decode):
        if kind == "image_folder":
            source = image_folder_source(root, self.size, self.channels)
        elif kind == "mnist":
            source = mnist_source(root, self.size, self.channels, train)
        else:
            raise ValueError("unknown resident source %r" % kind)
        shape = (len(source["items"]), self.size, self.size, self.channels)
        gb = float(np.prod(shape, dtype=np.float64)) / 1e9
        if gb > float(max_gb):
            raise SystemExit("resident_data: the set is %d x %dx%dx%d uint8 = %.3f GB, above resident_max_gb=%s; raise "
                             "the key or train without resident_data (the streaming path is not chosen silently)"
                             % (shape + (gb, max_gb)))
        digest = set_digest(source, self.size, self.channels) if cache_dir else None
        hit = load_cache(cache_dir, digest, shape) if cache_dir else None
        if hit is not None:
            return hit
        if not may_decode:
            raise SystemExit("resident_data: rank %d found no cache entry %s under %r (rank 0 writes it; do all ranks "
                             "see the same directory and the same files?)" % (self.rank, digest, cache_dir))
        arr = build_set(source, self.size, self.channels, workers)
        if cache_dir:
            save_cache(cache_dir, digest, arr, source["labels"], source["classes"], source, self.size, self.channels)
        return arr, source["labels"], source["classes"]

    def __len__(self):
        return len(self.order)

    def set_epoch(self, epoch):
        """The epoch the next ``iter()`` starts with (see ImageFolderImages.set_epoch)."""
        self.epoch = int(epoch)

    def host_set(self):
        """(uint8 [M, S, S, C], int64 labels [M]) on the host."""
        return self._u8, self._labels

    def epoch_order(self, epoch):
        from .run_network import shard_indices
        return self.order if self.world <= 1 else shard_indices(len(self._u8), self.rank, self.world, epoch)

    def __iter__(self):
        from . import functional as F
        if self.device.type != "cuda":
            raise RuntimeError("lightning_gan_zoo_amd: the input step normalises on the GPU (no CPU fallback); "
                               "host_set() returns the decoded uint8 set")
        if self._dev is None:
            self._dev = (upload(self._u8, self.device), torch.from_numpy(np.ascontiguousarray(self._labels))
                         .to(self.device))
        set_dev, labels_dev = self._dev
        epoch, order_dev = self.epoch, None
        while True:
            # the epoch's order, one int64 tensor on the device (one process: every epoch has the same order, so the
            # first upload serves them all and no later epoch start waits for a copy)
            if order_dev is None or self.world > 1:
                order_dev = torch.tensor(self.epoch_order(epoch), dtype=torch.int64).to(self.device)
            epoch += 1
            for i in range(0, order_dev.numel(), self.batch):
                yield F.gather_normalize_u8(set_dev, order_dev[i:i + self.batch], self.mean, self.std, labels_dev)

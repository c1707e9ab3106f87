"""Thin runner with the reference's command-line grammar (run_network.py:25-75 + Hydra overrides):

    python -m lightning_gan_zoo_amd.run_network +expt=dc_gan train.batch_size=64 +max_steps=200 \\
           dataset=synthetic train.ckpt_dir=output/ckpt
    python -m lightning_gan_zoo_amd.run_network --config-dir /path/to/lightning_gan_zoo/conf \\
           +expt=dc_gan dataset=celeb_a filepaths=local

Without ``--config-dir`` the experiment is composed from the built-in restatement of the reference's tree
(config.make_cfg); with it, from the user's own ``conf/``-shaped directory (config.compose_tree: defaults lists,
``+expt=``, ``group=option``, ``${a.b}``), whose ``core.*`` ``_target_`` strings are served by this package
(dropin.install).  ``num_gpus`` > 1 expects a torch.distributed launch (one process per GPU).

What the reference delegates to pytorch_lightning is done by harness.Trainer: per-batch optimizer alternation, toggle,
backward, step, per-epoch LR scheduler, ``max_epochs=cfg.train.num_epochs``, checkpoint save / resume
(``find_ckpt``: the single ``*.ckpt`` under ``train.ckpt_dir``; ``ModelCheckpoint(monitor='fid',
filename='model_best-{fid:.2f}')`` keeps the best-scoring file when the metric is available, else the latest), the
DistributedSampler's per-rank sharding of the dataset.  Checkpoints are ``torch.save`` dicts in Lightning's envelope
(``epoch, global_step, pytorch-lightning_version, state_dict, optimizer_states, lr_schedulers, callbacks``) whose
``state_dict`` keys are ``generator.<...>`` / ``discriminator.<...>`` exactly as the reference's LightningModule
produces them.

The product runner only ever builds the HIP modules on a GPU; tests drive ``fit()`` with their own module / data.
"""
import contextlib
import glob
import math
import os
import random
import sys
import time

import numpy as np
import torch

from .config import ConfigError, compose_tree, locate, make_cfg, parse_value

# keys of this runner, not of the reference's config (accepted with or without Hydra's "+")
RUNNER_KEYS = {"max_steps": None, "log_every": 10, "dataset_path": None, "seed": 42, "steps_per_epoch": 100,
               "inception_weights": None, "inception_check_hash": True, "figures": False,
               # resident training set (resident_data.py): decode once, keep the uint8 set in HBM, one gather launch per
               # batch; data_cache = directory of the decoded-set cache file; a set above resident_max_gb is refused
               "resident_data": False, "data_cache": None, "resident_max_gb": 32,
               # exponential moving average of the generator's weights (averaging.py; gan_stability's update_average with
               # its model_average_beta default): evaluation, figures and checkpoints see the averaged generator
               "generator_average": False, "generator_average_beta": 0.999,
               # KID's kernel-matrix sums on the GPU (eval.polynomial_mmd_averages_device, csrc/gz_kid.hip) instead of
               # ~a minute of host fp64 GEMMs per evaluation; FID stays on the host
               "kid_on_device": False,
               # the whole evaluation pass on the device (eval.evaluate_device): generator and InceptionV3 at
               # eval_batch_size, activations resident in fp64, mean / covariance on csrc/gz_moments.hip, KID as with
               # kid_on_device (implied); only the matrix square root of the Frechet distance stays on the host
               "eval_on_device": False, "eval_batch_size": 250,
               # with eval_on_device: the Frechet distance's matrix square roots on the device too (Newton-Schulz on
               # csrc/gz_sqrtm.hip, eval.frechet_distance_device); within 1e-9 (rank-deficient statistics: 1e-7) of
               # tr S1 + tr S2 of the host value, which an evaluation whose iteration does not converge falls back to
               "fid_on_device": False,
               # with eval_on_device: the Inception Score (gan_stability's metrics/inception_score.py, splits as there) of
               # the generated codes the pass already holds, through the classifier head of the FID weight file
               # (eval.inception_score_device, csrc/gz_inception_score.hip) -- not torchvision's ImageNet network
               "inception_score": False, "inception_score_splits": 10,
               # with eval_on_device: improved precision / recall and density / coverage over precision_recall_k nearest
               # neighbours of the two code sets the pass already holds (eval.prdc_device, csrc/gz_prdc.hip)
               "precision_recall": False, "precision_recall_k": 5,
               # DiffAugment of the discriminator's input (augment.py, csrc/gz_diffaug.hip): a comma-separated subset of
               # color, translation, cutout; "" = off.  Travels into the module's cfg as cfg.diffaugment
               "diffaugment": "",
               # adaptive discriminator augmentation on top of it (augment.AdaptiveAugment, csrc/gz_ada.hip; Karras et
               # al. 2020): augment_blit = a subset of xflip,rot90; augment_p = a fixed probability per sample and group
               # (unset: 1.0, or the start value 0.0 when adapting); ada_target in (0, 1) = adapt p toward
               # E[sign(D(real))] = target (the paper: 0.6), every ada_interval discriminator steps, at a rate that moves
               # p from 0 to 1 over ada_kimg thousand real images.  All five travel into the module's cfg
               "augment_blit": "", "augment_p": None, "ada_target": None, "ada_interval": 4, "ada_kimg": 500,
               # sliced Wasserstein distance on Laplacian-pyramid patches (eval.evaluate_swd, csrc/gz_swd.hip): a quality
               # number per resolution level from pixels alone -- no network, no weight file.  swd_images real and as many
               # generated images (clamped to the real images there are), swd_patches 7x7 patches per image and level,
               # swd_repeats x swd_dirs directions, every draw from a private generator seeded with swd_seed; the real
               # set's sorted projections stay resident while they fit under swd_cache_gb
               "swd": False, "swd_images": 16384, "swd_patches": 128, "swd_dirs": 128, "swd_repeats": 4, "swd_seed": 0,
               "swd_cache_gb": 16}
BUILTIN_DATASETS = ("synthetic", "image_folder", "tensor_file", "celeb_a", "mnist")
AVERAGE_PREFIX = "generator_average."     # state_dict keys of the averaged generator's parameters, next to generator.*
LIGHTNING_VERSION_TAG = "1.2.0"       # envelope layout written below (Lightning 1.1 / 1.2 generation)


def parse_overrides(argv):
    """-> (conf_dir or None, expt, [override strings for the composer], runner keys)."""
    argv = list(argv)
    conf_dir, rest, runner = None, [], dict(RUNNER_KEYS)
    i = 0
    while i < len(argv):
        arg = argv[i]
        if arg in ("--config-dir", "-cd", "--config-path", "-cp"):
            conf_dir = argv[i + 1]
            i += 2
            continue
        if arg.startswith(("--config-dir=", "--config-path=")):
            conf_dir = arg.split("=", 1)[1]
            i += 1
            continue
        i += 1
        if "=" not in arg and not arg.startswith("~"):
            raise SystemExit("cannot parse %r (expected key=value or +expt=name)" % arg)
        key = arg.split("=", 1)[0].lstrip("+")
        if key in runner:
            runner[key] = parse_value(arg.split("=", 1)[1])
        else:
            rest.append(arg)
    expt = next((parse_value(a.split("=", 1)[1]) for a in rest if a.split("=", 1)[0] in ("+expt", "expt")), None)
    if expt is None:
        raise SystemExit("missing +expt=<dc_gan|wgan|wgan_gp|hologan|gan_stability_r1>")
    check_eval_keys(runner)
    check_diffaugment(runner)
    check_ada_keys(runner, expt)
    return conf_dir, expt, rest, runner


def check_diffaugment(run):
    """The policy as the canonical comma-separated string ('' = off); a bad one ends the run with the parser's message."""
    from .augment import parse_policy
    try:
        run["diffaugment"] = ",".join(parse_policy(run.get("diffaugment", "")))
    except ValueError as e:
        raise SystemExit(str(e)) from e


ADA_KEYS = ("augment_blit", "augment_p", "ada_target", "ada_interval", "ada_kimg")


def check_ada_keys(run, expt=None):
    """The five keys of the adaptive augmentation: canonical augment_blit, ranges, and the combinations that make no
    sense end the run with the reason."""
    from .augment import parse_blit
    try:
        run["augment_blit"] = ",".join(parse_blit(run.get("augment_blit", "")))
    except ValueError as e:
        raise SystemExit(str(e)) from e

    def number(key):
        v = run.get(key)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise SystemExit("%s must be a number, got %r" % (key, v))
        return float(v)

    if run.get("augment_p") is not None and not 0.0 <= number("augment_p") <= 1.0:
        raise SystemExit("augment_p must lie in [0, 1], got %r" % (run["augment_p"],))
    if run.get("ada_target") is not None and not 0.0 < number("ada_target") < 1.0:
        raise SystemExit("ada_target must lie in (0, 1), got %r (the paper uses 0.6)" % (run["ada_target"],))
    interval = run.get("ada_interval", 4)
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise SystemExit("ada_interval must be a positive integer, got %r" % (interval,))
    if not number("ada_kimg") > 0:
        raise SystemExit("ada_kimg must be positive, got %r" % (run["ada_kimg"],))
    touched = [k for k in ADA_KEYS if run.get(k, RUNNER_KEYS[k]) != RUNNER_KEYS[k]]
    if touched and not run.get("diffaugment") and not run["augment_blit"]:
        raise SystemExit("%s set with nothing to apply: diffaugment and augment_blit are both empty; name at least one "
                         "group (diffaugment=color,translation,cutout and / or augment_blit=xflip,rot90)"
                         % ", ".join(touched))
    if run.get("ada_target") is not None and expt in ("wgan", "wgan_gp"):
        raise SystemExit("ada_target is not served for expt=%s: the controller reads the overfitting heuristic "
                         "r_t = E[sign(D(real))], and the sign of an unbounded Wasserstein critic's output says nothing "
                         "about overfitting; use a fixed augment_p (and augment_blit) instead" % expt)


def check_swd_keys(run):
    if not isinstance(run.get("swd", False), bool):
        raise SystemExit("swd must be true or false, got %r" % (run["swd"],))
    for key in ("swd_images", "swd_patches", "swd_dirs", "swd_repeats"):
        v = run.get(key, 1)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise SystemExit("%s must be a positive integer, got %r" % (key, v))
    seed = run.get("swd_seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
        raise SystemExit("swd_seed must be a non-negative integer, got %r" % (seed,))
    if run.get("swd", False) and run.get("resident_data", False):
        raise SystemExit("swd=true is not served together with resident_data=true: the metric's real images come from "
                         "the streaming loader's input step (or a synthetic set / tensor file), not from the resident "
                         "set's gather; train without resident_data to score a run with swd")
    gb = run.get("swd_cache_gb", 16)
    if isinstance(gb, bool) or not isinstance(gb, (int, float)) or gb < 0:
        raise SystemExit("swd_cache_gb must be a non-negative number, got %r" % (gb,))


def check_eval_keys(run):
    check_swd_keys(run)
    if run.get("fid_on_device", False) and not run.get("eval_on_device", False):
        raise SystemExit("fid_on_device=true is honoured only together with eval_on_device=true: the device Frechet "
                         "distance reads the moments the device evaluation pass leaves on the GPU")
    if run.get("inception_score", False) and not run.get("eval_on_device", False):
        raise SystemExit("inception_score=true is honoured only together with eval_on_device=true: the device Inception "
                         "Score reads the codes the device evaluation pass leaves on the GPU")
    if run.get("precision_recall", False) and not run.get("eval_on_device", False):
        raise SystemExit("precision_recall=true is honoured only together with eval_on_device=true: the device precision, "
                         "recall, density and coverage read the codes the device evaluation pass leaves on the GPU")


def _builtin_dataset(name, run, filepaths):
    if name == "synthetic":
        return {"_target_": "lightning_gan_zoo_amd.run_network.SyntheticImages", "n_channels": 3}
    if name == "tensor_file":
        return {"_target_": "lightning_gan_zoo_amd.run_network.TensorFileImages", "n_channels": 3,
                "root": run["dataset_path"], "train": {"root": run["dataset_path"]}}
    if name == "image_folder":
        root = run["dataset_path"]
        return {"_target_": "torchvision.datasets.ImageFolder", "n_channels": 3, "root": root, "train": {"root": root}}
    if name == "celeb_a":                 # conf/dataset/celeb_a.yaml:1-12
        root = filepaths.get("celeb_a_root")
        if not root:
            raise SystemExit("dataset=celeb_a needs filepaths.celeb_a_root=<dir> (conf/filepaths/example.yaml)")
        return {"_target_": "torchvision.datasets.ImageFolder", "n_channels": 3, "root": root,
                "train": {"root": root + "/train"}, "val": {"root": root + "/train"}, "test": {"root": root + "/train"}}
    if name == "mnist":                   # conf/dataset/mnist.yaml:1-20 (download is carried along, never acted on)
        parent = filepaths.get("mnist_parent_directory") or run["dataset_path"]     # checked where it is opened
        node = {"_target_": "torchvision.datasets.MNIST", "n_channels": 1, "parent_directory": parent,
                "root": parent + "/MNIST" if parent else None, "download": True}
        for split, train in (("train", True), ("val", False), ("test", False)):
            node[split] = {"root": parent, "_target_": node["_target_"], "download": True, "train": train}
        return node
    raise SystemExit("unknown dataset %r (built in: %s)" % (name, ", ".join(BUILTIN_DATASETS)))


def compose(conf_dir, expt, overrides, run=None):
    """The experiment's config: from ``conf_dir`` when given, else from the built-in tree."""
    run = run or dict(RUNNER_KEYS)
    check_diffaugment(run)
    for key in ADA_KEYS:
        run.setdefault(key, RUNNER_KEYS[key])
    check_ada_keys(run, expt)
    if conf_dir:
        from . import dropin
        dropin.install()
        try:
            cfg = compose_tree(conf_dir, overrides)
        except ConfigError as e:
            raise SystemExit("config error: %s" % e) from e
        cfg["diffaugment"] = run["diffaugment"]       # read by BaseGAN.__init__
        for key in ADA_KEYS:
            cfg[key] = run[key]
        return cfg
    dotted, dataset, filepaths = {}, "synthetic", {}
    for arg in overrides:
        key, text = arg.split("=", 1)
        key = key.lstrip("+")
        if key == "expt":
            continue
        if key == "dataset":
            dataset = parse_value(text)
        elif key.startswith("filepaths."):
            filepaths[key.split(".", 1)[1]] = parse_value(text)
        elif key == "filepaths":
            continue                      # a group choice of the yaml tree; the built-in tree has no file to pick
        else:
            dotted[key] = parse_value(text)
    probe = make_cfg(expt)
    for key in dotted:                    # Hydra refuses to override a key that does not exist
        node = probe
        parts = key.split(".")
        ok = True
        for k in parts[:-1]:
            if not isinstance(node, dict) or k not in node:
                ok = False
                break
            node = node[k]
        if not ok or (parts[-1] not in node and key not in ("train.weight_clip", "train.ckpt_dir", "save_ckpts")
                      and not key.startswith("loss_weight.")):
            raise SystemExit("unknown config key %r" % key)
    cfg = make_cfg(expt, dotted=dotted)
    cfg["dataset"] = _to_cfg(_builtin_dataset(dataset, run, filepaths))
    cfg["diffaugment"] = run["diffaugment"]           # read by BaseGAN.__init__
    for key in ADA_KEYS:                              # likewise (augment.build_augment)
        cfg[key] = run[key]
    cfg.train["channels_img"] = cfg.dataset.get("n_channels", 3) if "train.channels_img" not in dotted else \
        cfg.train["channels_img"]
    return cfg


def _to_cfg(obj):
    from .config import to_cfg
    return to_cfg(obj)


def seed_everything(seed):
    """pytorch_lightning.seed_everything (reference run_network.py:27): python, numpy and torch generators -- the
    SAME seed on every rank, as the reference does."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------
def shard_indices(n, rank, world, epoch=None, seed=0):
    """torch.utils.data.DistributedSampler(drop_last=False): pad to a multiple of ``world`` by wrapping around, then
    every ``world``-th index from ``rank``.  Under ``accelerator="ddp"`` (reference run_network.py:66) Lightning puts a
    DistributedSampler with shuffle=True in front of the train loader and calls ``set_epoch`` every epoch, so each
    epoch is a fresh permutation ``randperm(n, generator=manual_seed(seed + epoch))`` shared by all ranks (seed 0,
    the sampler's default): pass ``epoch`` to get that order; ``epoch=None`` is the unshuffled order (one process:
    the reference's loader has no shuffle, core/lightning_module.py:89-92)."""
    if world <= 1:
        return list(range(n))
    if epoch is None:
        idx = list(range(n))
    else:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    total = int(math.ceil(n / world)) * world
    idx += idx[:total - n]
    return idx[rank:total:world]


class SyntheticImages:
    """Endless batches of uniform[-1, 1] images (the range ToTensor+Normalize(0.5, 0.5) produces)."""

    def __init__(self, batch, channels, size, device, seed):
        g = torch.Generator().manual_seed(seed)
        self.real = (torch.rand(batch, channels, size, size, generator=g) * 2 - 1).to(device)
        self.labels = torch.zeros(batch, dtype=torch.int64, device=device)

    def __len__(self):
        return 0          # no epoch structure of its own: the runner's steps_per_epoch applies

    def __iter__(self):
        while True:
            yield self.real, self.labels


class TensorFileImages:
    """A ``.pt`` / ``.npy`` file holding [M, C, H, W] floats already normalised to [-1, 1]."""

    def __init__(self, path, batch, device, rank=0, world=1):
        data = torch.load(path) if path.endswith(".pt") else torch.from_numpy(np.load(path))
        self.data, self.batch, self.device = data.float(), batch, device
        self.rank, self.world, self.epoch = rank, world, 0
        self.order = shard_indices(len(self.data), rank, world)

    def set_epoch(self, epoch):
        """The epoch the next ``iter()`` starts with (Lightning: ``sampler.set_epoch(trainer.current_epoch)``)."""
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        epoch = self.epoch
        while True:
            # one process: no shuffling, as the reference's train_dataloader (:89-92); data parallel: the
            # DistributedSampler(shuffle=True) permutation of this epoch (shard_indices)
            order = torch.tensor(self.order if self.world <= 1
                                 else shard_indices(len(self.data), self.rank, self.world, epoch))
            epoch += 1
            for i in range(0, len(order), self.batch):
                real = self.data[order[i:i + self.batch]]
                if torch.device(self.device).type == "cuda":
                    real = real.pin_memory().to(self.device, non_blocking=True)
                yield real, torch.zeros(len(real), dtype=torch.int64, device=self.device)


IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def image_folder_samples(root):
    """(path, class_index) list with torchvision.datasets.ImageFolder's ordering: classes = sorted sub-directories,
    inside a class a sorted walk, file names sorted, image extensions only (reference lightning_module.py:89-91)."""
    classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
    if not classes:
        raise FileNotFoundError("no class folders under %r" % root)
    samples = []
    for idx, cls in enumerate(classes):
        for dirpath, _, fnames in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for fname in sorted(fnames):
                if fname.lower().endswith(IMG_EXTENSIONS):
                    samples.append((os.path.join(dirpath, fname), idx))
    return samples, classes


class ImageFolderImages:
    """The reference's real-data input step -- ImageFolder -> Resize((S, S)) -> ToTensor -> Normalize(mean, std),
    DataLoader without shuffling, incomplete last batch kept (core/lightning_module.py:42-47,89-92), sharded over the
    data-parallel ranks like DistributedSampler(shuffle=False) -- with the decode + resize on a background host thread
    and ToTensor / Normalize / HWC->CHW on the device (functional.normalize_u8_images): the host hands over 1 byte per
    element through a ring of pinned buffers.  ``host_batches()`` is the host half (uint8, testable anywhere);
    iterating the object is the device half and needs the GPU."""

    def __init__(self, root, batch, img_size, channels, mean, std, device, prefetch=3, rank=0, world=1):
        self.samples, self.classes = image_folder_samples(root)
        if not self.samples:
            raise FileNotFoundError("no images under %r" % root)
        self.rank, self.world, self.epoch = rank, world, 0
        self.order = shard_indices(len(self.samples), rank, world)          # (length / unshuffled view; see host_batches)
        self.batch, self.size, self.channels = batch, img_size, channels
        self.mean, self.std, self.device, self.prefetch = mean, std, torch.device(device), prefetch

    def __len__(self):
        return len(self.order)

    def set_epoch(self, epoch):
        """The epoch the next ``host_batches()`` / ``iter()`` starts with.  Lightning calls
        ``sampler.set_epoch(trainer.current_epoch)`` at every epoch start, so a run resumed from a checkpoint of epoch
        E continues with the permutation ``randperm(seed + E)``, not with ``seed + 0`` again (``fit`` passes the
        checkpoint's epoch here)."""
        self.epoch = int(epoch)

    def decode(self, path):
        from PIL import Image
        with open(path, "rb") as f:
            img = Image.open(f).convert("RGB" if self.channels == 3 else "L")    # ImageFolder's pil_loader gives RGB
        img = img.resize((self.size, self.size), Image.BILINEAR)                # transforms.Resize on a PIL image
        a = np.asarray(img, dtype=np.uint8)
        return a if a.ndim == 3 else a[:, :, None]

    def host_batches(self):
        """uint8 [b, S, S, C] arrays and int64 labels, epoch after epoch: dataset order in one process, a fresh
        DistributedSampler(shuffle=True) permutation per epoch under data parallelism (shard_indices)."""
        epoch = self.epoch
        while True:
            order = self.order if self.world <= 1 else shard_indices(len(self.samples), self.rank, self.world, epoch)
            epoch += 1
            for i in range(0, len(order), self.batch):
                chunk = [self.samples[j] for j in order[i:i + self.batch]]
                yield (np.stack([self.decode(p) for p, _ in chunk]), np.array([c for _, c in chunk], dtype=np.int64))

    def __iter__(self):
        import queue
        import threading
        from . import functional as F
        if self.device.type != "cuda":
            raise RuntimeError("lightning_gan_zoo_amd: the input step normalises on the GPU (no CPU fallback); "
                               "host_batches() yields the decoded uint8 batches")
        q = queue.Queue(maxsize=self.prefetch)

        def producer():
            for item in self.host_batches():
                q.put(item)

        threading.Thread(target=producer, daemon=True).start()
        ring, cursor = {}, 0
        while True:
            imgs, labels = q.get()
            key = imgs.shape
            slots = ring.setdefault(key, [[torch.empty(key, dtype=torch.uint8).pin_memory(), None]
                                          for _ in range(self.prefetch + 1)])
            buf, ev = slots[cursor % len(slots)]
            if ev is not None:
                ev.synchronize()
            buf.copy_(torch.from_numpy(imgs))
            u8 = buf.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            slots[cursor % len(slots)][1] = ev
            cursor += 1
            yield (F.normalize_u8_images(u8, self.mean, self.std),
                   torch.from_numpy(labels).to(self.device, non_blocking=True))


def build_data(cfg, run, device, rank=0, world=1, group=None):
    """The training set of ``cfg.dataset`` (reference ``instantiate(cfg.dataset.train, transform=...)``, :89-92).
    ``group``: the long-timeout process group the ranks of a resident set wait on while rank 0 decodes."""
    t = cfg.train
    node = cfg.get("dataset") or {}
    target = str(node.get("_target_", ""))
    if run.get("synthetic") or target.endswith("SyntheticImages") or not target:
        return SyntheticImages(t.batch_size, t.channels_img, t.img_size, device, 1234 + rank)
    train = node.get("train", node)
    if target.endswith("TensorFileImages"):
        return TensorFileImages(train["root"], t.batch_size, device, rank, world)
    resident = dict(cache_dir=run.get("data_cache"), max_gb=run.get("resident_max_gb", 32), rank=rank, world=world,
                    group=group)
    if target.endswith("datasets.MNIST"):
        if not run.get("resident_data"):
            raise SystemExit("dataset target %r is served by the resident training set only: pass resident_data=true "
                             "(60 000 x 64x64 bytes = 246 MB of HBM)" % target)
        if not train.get("root"):
            raise SystemExit("dataset=mnist needs filepaths.mnist_parent_directory=<dir holding MNIST/raw> "
                             "(conf/filepaths/example.yaml) or dataset_path=<that dir>")
        from .resident_data import ResidentImages
        return ResidentImages(train["root"], t.batch_size, t.img_size, t.channels_img, t.data_mean, t.data_std, device,
                              source="mnist", train=bool(train.get("train", True)), **resident)
    if target.endswith("ImageFolder") and run.get("resident_data"):
        from .resident_data import ResidentImages
        return ResidentImages(train["root"], t.batch_size, t.img_size, t.channels_img, t.data_mean, t.data_std, device,
                              source="image_folder", **resident)
    if target.endswith("ImageFolder"):
        return ImageFolderImages(train["root"], t.batch_size, t.img_size, t.channels_img, t.data_mean, t.data_std,
                                 device, rank=rank, world=world)
    raise SystemExit("dataset target %r is not supported by this runner (ImageFolder-shaped datasets, MNIST raw files, "
                     "tensor files and synthetic batches are)" % target)


# ---------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------
def find_ckpt(ckpt_dir):
    """reference run_network.py:19-23: every *.ckpt below the directory; more than one is an error."""
    if not ckpt_dir:
        return None
    hits = [y for x in os.walk(ckpt_dir) for y in glob.glob(os.path.join(x[0], "*.ckpt"))]
    assert len(hits) <= 1, "Multiple ckpts found!"
    return hits[0] if hits else None


def checkpoint_blob(module, trainer, step, epoch, keeper=None, average=None):
    """Lightning's checkpoint envelope (``trainer.checkpoint_connector.dump_checkpoint`` of the 1.1 / 1.2 generation).
    ``average`` (averaging.GeneratorAverage): its parameters join ``state_dict`` as ``generator_average.<name>``."""
    state = {k: v.detach().cpu() for k, v in module.state_dict().items()}       # generator.* / discriminator.*
    if average is not None:
        state.update({AVERAGE_PREFIX + k: v.cpu() for k, v in average.state_dict().items()})
    blob = {"epoch": epoch, "global_step": step, "pytorch-lightning_version": LIGHTNING_VERSION_TAG,
            "state_dict": state,
            "optimizer_states": [o["optimizer"].state_dict() for o in trainer.optim],
            "lr_schedulers": [o["lr_scheduler"].state_dict() for o in trainer.optim],
            "callbacks": {}}
    if keeper is not None:
        blob["callbacks"]["ModelCheckpoint"] = keeper.state()
    aug = getattr(module, "diffaugment", None)
    if getattr(aug, "adaptive", False):       # the controller's p and its step count (rank 0's, restored to every rank)
        blob["callbacks"]["AdaptiveAugment"] = aug.state_dict()
    return blob


def save_checkpoint(path, module, trainer, step, epoch, keeper=None, average=None):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    torch.save(checkpoint_blob(module, trainer, step, epoch, keeper, average), tmp)
    os.replace(tmp, path)


def load_checkpoint(path, module, trainer, average=None, verbose=True):
    """``average``: restored from the ``generator_average.*`` entries; a checkpoint without them (an older run, or one
    with the key off) re-initialises it from the loaded generator and says so (``verbose``)."""
    blob = torch.load(path, map_location="cpu", weights_only=False)
    sd = blob["state_dict"]
    for prefix, net in (("discriminator.", module.discriminator), ("generator.", module.generator)):
        net.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    if average is not None:
        avg = {k[len(AVERAGE_PREFIX):]: v for k, v in sd.items() if k.startswith(AVERAGE_PREFIX)}
        if avg:
            average.load_state_dict(avg)
        else:
            average.reset()
            if verbose:
                print("generator_average: %s holds no averaged weights; the average starts from the loaded generator"
                      % path)
    aug = getattr(module, "diffaugment", None)
    if getattr(aug, "adaptive", False):
        saved = blob.get("callbacks", {}).get("AdaptiveAugment")
        if saved:
            aug.load_state_dict(saved)
        elif verbose:
            print("ada_target: %s holds no AdaptiveAugment state; p starts from %g" % (path, aug.p_start))
    for o, s in zip(trainer.optim, blob.get("optimizer_states", [])):
        o["optimizer"].load_state_dict(s)
    for o, s in zip(trainer.optim, blob.get("lr_schedulers", [])):
        o["lr_scheduler"].load_state_dict(s)
    if blob.get("global_step", 0) > 0:
        # the optimizers HAVE stepped -- in the process that wrote the checkpoint; torch's "lr_scheduler.step() before
        # optimizer.step()" bookkeeping is per process and would otherwise warn at the first epoch end after a resume
        for o in trainer.optim:
            o["optimizer"]._opt_called = True
    return blob.get("global_step", 0), blob.get("epoch", 0), blob.get("callbacks", {}).get("ModelCheckpoint")


class CheckpointKeeper:
    """``ModelCheckpoint(monitor='fid', filename='model_best-{fid:.2f}')`` with Lightning's defaults (mode min,
    save_top_k 1), reference run_network.py:48-50: a new file when the monitored metric improves, the previous best
    removed AFTER the new one is on disk.  While the metric is not being produced (no InceptionV3 weights offline)
    the latest state is kept instead, as ``step=<n>.ckpt`` -- either way the directory holds exactly one ``*.ckpt``,
    which is what ``find_ckpt`` resumes from."""

    def __init__(self, dirpath, monitor="fid", filename="model_best-{fid:.2f}"):
        self.dirpath, self.monitor, self.filename = dirpath, monitor, filename
        self.best_score, self.best_path = None, None

    def state(self):
        return {"monitor": self.monitor, "best_model_score": self.best_score, "best_model_path": self.best_path}

    def load_state(self, st, current_path=None):
        if st:
            self.best_score, self.best_path = st.get("best_model_score"), st.get("best_model_path")
        if current_path:
            self.best_path = current_path

    def update(self, metrics, step, save_fn):
        """``save_fn(path)`` writes the checkpoint; returns the path written or None."""
        score = metrics.get(self.monitor) if metrics else None
        if score is None and self.best_score is not None and self.best_path and os.path.exists(self.best_path):
            # a state without a metric (a run cut short mid-epoch) never displaces the monitored best:
            # ModelCheckpoint(save_top_k=1) keeps its best file until something better arrives
            return None
        if score is not None:
            score = float(score)
            if self.best_score is not None and not score < self.best_score:
                return None
            name = self.filename.replace("{%s:.2f}" % self.monitor, "%s=%.2f" % (self.monitor, score)) + ".ckpt"
            self.best_score = score
        else:
            name = "step=%d.ckpt" % step
        path = os.path.join(self.dirpath, name)
        old, self.best_path = self.best_path, path
        save_fn(path)
        for stale in glob.glob(os.path.join(self.dirpath, "*.ckpt")):
            if os.path.abspath(stale) != os.path.abspath(path):
                os.remove(stale)
        del old
        return path


# ---------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------
def fit(module, cfg, data, run, sync=None, rank=0, world=1, evaluate=None, slow_group=None, figures=None,
        average=None, monitor="fid"):
    """``pl.Trainer(max_epochs=cfg.train.num_epochs, resume_from_checkpoint=find_ckpt(...)).fit(model)`` for the
    step classes of this package (reference run_network.py:61-72).  ``figures``: an EpochFigures, drawn at every epoch
    end after the FID evaluation.  ``average``: an averaging.GeneratorAverage, advanced after every generator optimizer
    step, saved in and restored from the checkpoints.  ``monitor``: the metric the best checkpoint is chosen by
    (``checkpoint_monitor``).  Returns (module, trainer, global_step)."""
    from .harness import Trainer
    t = cfg.train
    # reference run_network.py:61-68: ``1`` or a ``{start_epoch, accumulation_factor}`` node -> Lightning's
    # ``accumulate_grad_batches={start_epoch: factor}`` (GradientAccumulationScheduler)
    acc = cfg.get("accumulate_grad_batches", 1)
    if not isinstance(acc, int):
        acc = {int(acc["start_epoch"]): int(acc["accumulation_factor"])}
    trainer = Trainer(module, grad_sync=sync, accumulate_grad_batches=acc, generator_average=average)
    n = len(data) if hasattr(data, "__len__") else 0
    steps_per_epoch = int(math.ceil(n / t.batch_size)) if n else int(run["steps_per_epoch"])
    step = epoch = 0
    skip = 0
    ckpt_dir = t.get("ckpt_dir")
    keeper = None
    if ckpt_dir and cfg.get("save_ckpts", True):
        keeper = CheckpointKeeper(ckpt_dir, monitor=monitor, filename="model_best-{%s:.2f}" % monitor)
    ckpt = find_ckpt(ckpt_dir)
    if ckpt:
        step, epoch, kst = load_checkpoint(ckpt, module, trainer, average, verbose=rank == 0)
        trainer.batch_idx = step
        trainer.epoch, trainer.epoch_batch_idx = epoch, step % steps_per_epoch
        if keeper is not None:
            keeper.load_state(kst, ckpt)
        if hasattr(data, "set_epoch"):
            data.set_epoch(epoch)         # the sampler's permutation continues at seed + epoch (Lightning: set_epoch)
            skip = step % steps_per_epoch if n else 0     # a checkpoint cut by max_steps: the epoch continues where
                                                          # it stopped instead of replaying its first batches
        if rank == 0:
            print("resumed from %s at step %d (epoch %d)" % (ckpt, step, epoch))
    # a full Python garbage collection walks every object torch has created (~70 ms, several training steps):
    # park the set-up's survivors in the permanent generation so that later collections stay short
    import gc
    gc.collect()
    gc.freeze()
    t0 = time.time()
    last, first_step = {}, step
    max_steps, max_epochs = run.get("max_steps"), int(t.get("num_epochs", 99999))

    def checkpoint(metrics=None):
        if keeper is None:
            return
        if sync is not None:
            sync.flush()
            sync.sync_buffers()           # a collective: every rank takes part, rank 0 writes
        if rank == 0:
            keeper.update(metrics, step,
                          lambda path: save_checkpoint(path, module, trainer, step, epoch, keeper, average))
        if world > 1:
            torch.distributed.barrier()

    if rank == 0 and n:
        #  the order the data is visited in is part of the run's definition: say it
        print("data order: %s" % ("dataset order, no shuffling (reference train_dataloader, one process)" if world <= 1
                                  else "DistributedSampler(shuffle=True, seed=0) permutation per epoch, %d ranks" % world))
    for batch in data:
        if skip:
            skip -= 1
            continue
        if (max_steps is not None and step >= max_steps) or epoch >= max_epochs:
            break
        loss, idx = trainer.step(batch, last_in_epoch=(step + 1) % steps_per_epoch == 0)
        last[("d_loss", "g_loss")[idx]] = loss
        step += 1
        if step % run["log_every"] == 0 and rank == 0:
            msg = " ".join("%s=%.4f" % (k, float(v)) for k, v in sorted(last.items()))
            aug = getattr(module, "diffaugment", None)
            if getattr(aug, "adaptive", False):           # the one place the host reads the controller's state
                ada_p, ada_r = aug.values()
                module.log("train/ada_p", ada_p)
                module.log("train/ada_r", ada_r)
                msg += " ada_p=%.4f ada_r=%.4f" % (ada_p, ada_r)
            rate = (step - first_step) * t.batch_size * world / (time.time() - t0)
            print("step %d epoch %d %s (%.1f img/s)" % (step, epoch, msg, rate))
        if step % steps_per_epoch == 0:
            trainer.end_epoch()           # lr_scheduler.step(), current_epoch += 1
            epoch += 1
            metrics = evaluate(module, epoch) if evaluate is not None else None
            if slow_group is not None:    # ranks > 0 wait for rank 0's Inception pass on the long-timeout group
                torch.distributed.barrier(group=slow_group)
            if figures is not None:
                figures(module, epoch - 1, metrics, sync)
            checkpoint(metrics)
    trainer.finish()
    if step % steps_per_epoch:            # a run cut short by max_steps still leaves a resumable state
        checkpoint(None)
    return module, trainer, step


@contextlib.contextmanager
def rendering_from(module, average):
    """Inside: ``module.generator`` is the averaged generator (``average.averaged()``: eval mode, the live BatchNorm
    buffers of this moment); the live generator comes back afterwards.  ``average=None``: nothing changes."""
    if average is None:
        yield
        return
    live = module.generator
    module.generator = average.averaged()
    try:
        yield
    finally:
        module.generator = live
        average.shadow.eval()         # (a module.train() inside reached the averaged generator, not the live one)


class EpochFigures:
    """The reference's figure callbacks at a validation end (core/figures/types.py:78-91, run on_validation_end after
    InceptionMetrics' on_validation_epoch_start has logged this epoch's FID): each figure whose monitor rule passes
    draws and writes.  Pending gradient exchanges and optimizer steps land first; the module runs in eval mode under
    no_grad and gets its mode back.  HoloGAN's view prefetched for the next step is rolled back first, so that numpy's
    stream reads (figure draws, next step's view) as in the reference.  Every rank makes the same host draws (the
    reference draws on every rank and saves on rank zero); only rank 0 renders and writes.  ``have_fid``: an FID
    evaluator exists (on rank 0); without one a monitored figure is drawn every epoch, and says so once.  ``average``
    (averaging.GeneratorAverage): the frames are rendered by the averaged generator; the host draws stay the live one's."""

    def __init__(self, figs, have_fid, rank=0, world=1, group=None, average=None):
        self.figs, self.have_fid, self.rank, self.world, self.group = list(figs), have_fid, rank, world, group
        self.average = average
        self._said = False

    def score(self, metrics):
        fid = None if not metrics or metrics.get("fid") is None else float(metrics["fid"])
        if self.world > 1 and self.have_fid:
            t = torch.tensor([float("nan") if fid is None else fid], dtype=torch.float64)
            torch.distributed.broadcast(t, 0, group=self.group)
            fid = None if math.isnan(float(t[0])) else float(t[0])
        return fid

    def __call__(self, module, epoch, metrics, sync=None):
        score = self.score(metrics)
        if not self.have_fid and not self._said and any(f.monitor for f in self.figs):
            self._said = True
            if self.rank == 0:
                print("figures: figure_details.fid_callback is set but no FID is computed in this run (no "
                      "inception_weights / ImageFolder validation set): the monitor is off, figures are drawn every "
                      "epoch")
        if sync is not None:
            sync.flush()
        gen = module.generator
        if hasattr(gen, "drop_prefetched_view"):
            gen.drop_prefetched_view()
        was = module.training
        module.eval()
        try:
            with torch.no_grad():
                for fig in self.figs:
                    if not fig.should_draw(score if self.have_fid else None):
                        continue
                    plan = fig.plan(module)              # host draws: every rank
                    if self.rank == 0:
                        with rendering_from(module, self.average):
                            frames = fig.render(module, plan)[1]
                        fig.write(frames.cpu().numpy(), epoch)
        finally:
            module.train(was)


FID_IMAGE_EXTENSIONS = ("bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp")


def real_image_files(root):
    """The files ``compute_activations_of_path`` feeds to pytorch_fid (core/callback_inception_metrics.py:141-147):
    every image under ``root``, recursively, sorted."""
    out = []
    for d, _, names in os.walk(root):
        out += [os.path.join(d, f) for f in names if f.lower().endswith(FID_IMAGE_EXTENSIONS)]
    return sorted(out)


def real_statistics_cache(root):
    """(mu, sigma) of the real set as ``real_activations`` persisted them (``<root>/inception_cache.npz``), or
    (None, None) without that file."""
    path = os.path.join(root, "inception_cache.npz")
    if not os.path.exists(path):
        return None, None
    with np.load(path) as data:
        if "mu" not in data or "sigma" not in data:
            return None, None
        return np.asarray(data["mu"]), np.asarray(data["sigma"])


def real_activations(root, features, batch_size=16):
    """Inception activations of the real images as the reference's callback obtains them (:159-163, :211-221): the
    first ``*.npz`` in ``root`` if there is one (keys mu / sigma / act), else every image at its NATIVE resolution --
    pytorch_fid's loader applies ToTensor only, the one resize is InceptionV3's own to 299x299 -- in batches of
    ``batch_size`` consecutive files of equal size, and the result written to ``<root>/inception_cache.npz`` for the
    next launch / resume.  Returns the activations [n, 2048]."""
    cached = sorted(f for f in os.listdir(root) if ".npz" in f)
    if cached:
        with np.load(os.path.join(root, cached[0])) as data:
            return np.asarray(data["act"])
    from PIL import Image
    from . import eval as E
    acts, batch = [], []

    def flush():
        if batch:
            acts.append(features(np.stack(batch)))
            del batch[:]

    for path in real_image_files(root):
        with open(path, "rb") as f:
            img = np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8)
        if batch and (img.shape != batch[0].shape or len(batch) == batch_size):
            flush()
        batch.append(img)
    flush()
    if not acts:
        raise FileNotFoundError("no images under %r" % root)
    act = np.concatenate(acts, axis=0)
    mu, sigma = E.activation_statistics(act)
    try:
        np.savez(os.path.join(root, "inception_cache.npz"), mu=mu, sigma=sigma, act=act)
    except OSError as e:            # read-only data set directory: recomputed on the next launch
        print("could not write %s/inception_cache.npz (%s)" % (root, e))
    return act


def wants_fid(cfg, run):
    node = cfg.get("dataset") or {}
    return bool(cfg.get("calc_fid", True) and run.get("inception_weights") and (node.get("val") or {}).get("root")
                and str(node.get("_target_", "")).endswith("ImageFolder"))


def wants_evaluator(cfg, run):
    """Rank 0 evaluates at every epoch end (FID, the sliced Wasserstein distance, or both) while the other ranks wait."""
    return wants_fid(cfg, run) or bool(run.get("swd", False))


def checkpoint_monitor(have_fid, run):
    """The metric the best checkpoint is chosen by: FID wherever it is computed, else the sliced Wasserstein distance's
    average over the levels when ``swd=true``, else (no metric) ``fid``, which is then never produced."""
    return "swd" if (run.get("swd", False) and not have_fid) else "fid"


def swd_real_images(cfg, run, data, device):
    """The real set of the sliced Wasserstein distance: the first ``swd_images`` images in dataset order -- fewer where
    the set has fewer -- as the training step sees them.  Dispatch follows ``build_data``: a synthetic set gives its one
    batch, a tensor file its (already normalised) rows; an ImageFolder-shaped dataset gives the files of its validation
    root where it has one, else of its training root, through the loader's own host half (``ImageFolderImages
    .host_batches``: decode, resize) and the input step's device half (``functional.normalize_u8_images`` with
    ``data_mean`` / ``data_std``), read once at start-up without the loader's prefetch thread.  The resident training
    set is not served: ``swd=true`` with ``resident_data=true`` is refused by ``check_swd_keys``."""
    from . import functional as F
    t, want = cfg.train, int(run["swd_images"])
    if isinstance(data, SyntheticImages):
        return data.real[:want].float().contiguous()
    if isinstance(data, TensorFileImages):
        return data.data[:want].to(device).contiguous()
    node = cfg.get("dataset") or {}
    if not str(node.get("_target_", "")).endswith("ImageFolder"):
        raise SystemExit("swd=true reads its real images from a synthetic set, a tensor file or an ImageFolder-shaped "
                         "dataset; %r is none of them" % node.get("_target_"))
    root = (node.get("val") or {}).get("root") or node.get("train", node)["root"]      # (train: as build_data finds it)
    folder = ImageFolderImages(root, t.batch_size, t.img_size, t.channels_img, t.data_mean, t.data_std, device)
    n, parts, have = min(want, len(folder.samples)), [], 0
    for u8, _ in folder.host_batches():
        parts.append(F.normalize_u8_images(torch.from_numpy(u8[:n - have]).to(device), t.data_mean, t.data_std))
        have += len(parts[-1])
        if have >= n:
            break
    return torch.cat(parts)


class SwdScorer:
    """The sliced Wasserstein distance as the runner evaluates it (eval.evaluate_swd).  ``load_real``, called once the
    training data exist, takes the real images, draws the plan for their count -- patch centres, directions and the
    generated set's latents, from a private generator seeded with ``swd_seed`` that leaves numpy's and torch's global
    generators untouched, so a run with ``swd=true`` trains bit-identically to one without -- and makes the real set's
    resident pyramid.  Calling it scores the module's current generator (inside ``rendering_from``: the averaged one)
    -> {"swd_<size>": .., "swd": mean}."""

    def __init__(self, cfg, run, module):
        from . import eval as E
        self.cfg, self.run, self.module, self.batch = cfg, run, module, int(run.get("eval_batch_size", 250))
        self.sizes = E.swd_level_sizes(int(cfg.train.img_size))       # (a size the metric does not take ends the run here)
        self.plan = self.real = None

    def load_real(self, images):
        from . import eval as E
        t, run = self.cfg.train, self.run
        self.plan = E.SwdPlan(int(t.img_size), int(t.channels_img), len(images), patches=run["swd_patches"],
                              dirs=run["swd_dirs"], repeats=run["swd_repeats"], seed=run["swd_seed"], module=self.module)
        self.real = E.RealPyramid(images, self.plan, cache_gb=run["swd_cache_gb"])

    def __call__(self, module):
        from . import eval as E
        return E.evaluate_swd(module, self.plan, self.real, batch=self.batch)

    def text(self, m):
        return "SWD " + " ".join("%d: %.2f" % (s, m["swd_%d" % s]) for s in self.sizes) + " avg: %.2f" % m["swd"]


def swd_evaluator(scorer, average=None):
    """The ``evaluate`` hook of fit() of a run without an FID evaluator: the sliced Wasserstein distance alone."""
    def evaluate(mod, epoch):
        with rendering_from(mod, average):          # generator_average=true: the averaged generator is what is scored
            m = scorer(mod)
        print("epoch %d %s" % (epoch, scorer.text(m)))
        return m

    return evaluate


def device_fid_evaluator(dump, features, real_act, device, batch=250, average=None, mu=None, sigma=None,
                         fid_on_device=False, inception_score=False, inception_splits=10, prdc_k=None, swd=None):
    """The ``evaluate`` hook of fit() on the device pass (eval.evaluate_device).  The real set's device codes and its
    mean / covariance (``mu`` / ``sigma`` when a cache file holds them, else one moments launch) are made here, once per
    run; every epoch then costs the generated set alone.  ``fid_on_device``: the Frechet distance on the device as well
    (the real covariance's square root is made by the first evaluation and kept).  ``inception_score``: the Inception
    Score over ``inception_splits`` splits as well, through the classifier head of the weight file (``features.net.fc``,
    widened to fp64 on the device here, once per run; not the reference's torchvision network:
    eval.inception_score_from_logits); the best checkpoint stays chosen by FID.  ``prdc_k``: precision, recall, density
    and coverage over that many nearest neighbours as well (eval.prdc_device; the real set's radii are made by the first
    evaluation and kept).  ``swd``: a ``SwdScorer``; its numbers join the dict and the line, FID stays the monitored
    metric."""
    from . import eval as E
    real = E.RealStatistics(real_act, device, mu=mu, sigma=sigma)
    extra = {"fid_on_device": True} if fid_on_device else {}
    if prdc_k is not None:
        extra["prdc_k"] = int(prdc_k)
    if inception_score:
        fc = features.net.fc
        extra["classifier"] = tuple(t.detach().to(device).to(torch.float64).contiguous() for t in (fc.weight, fc.bias))
        extra["inception_splits"] = int(inception_splits)

    def evaluate(mod, epoch):
        with rendering_from(mod, average):          # generator_average=true: the averaged generator is what is scored
            m = E.evaluate_device(mod, dump, features.device, real, batch=batch, **extra)
            if swd is not None:
                m = dict(m, **swd(mod))
        line = "epoch %d FID: %.4f KID mean: %.6f KID stddev: %.6f" % (epoch, m["fid"], m["kid"], m["kid_std"])
        if inception_score:
            line += " IS: %.4f +- %.4f" % (m["is"], m["is_std"])
        if prdc_k is not None:
            line += " P: %.4f R: %.4f D: %.4f C: %.4f" % (m["precision"], m["recall"], m["density"], m["coverage"])
        if swd is not None:
            line += " " + swd.text(m)
        print(line)
        return m

    return evaluate


def make_fid_evaluator(cfg, run, module, device, average=None, swd=None):
    """The reference's InceptionMetrics callback (run_network.py:51-56, core/callback_inception_metrics.py:136-246) as
    the ``evaluate`` hook of fit(): FID / KID of ``val.fid_n_samples`` generated images against the validation images,
    both through the InceptionV3 pool features on the HIP kernels (inception.py).  Needs the FID weight file the
    reference downloads (``inception_weights=<path to pt_inception-2015-12-05-6726825d.pth>``; no network here) and an
    ImageFolder-shaped validation set; returns None otherwise, and the run keeps its latest checkpoint instead of
    the best-FID one.  ``swd``: a ``SwdScorer`` whose numbers join every evaluation's dict and line."""
    node = cfg.get("dataset") or {}
    if not (cfg.get("calc_fid", True) and run.get("inception_weights")):
        return None
    val_root = (node.get("val") or {}).get("root")
    if not val_root or not str(node.get("_target_", "")).endswith("ImageFolder"):
        return None
    check_eval_keys(run)
    from . import eval as E
    from .inception import InceptionFeatures, load_fid_weights
    features = InceptionFeatures(load_fid_weights(run["inception_weights"], device,
                                                  check_hash=bool(run.get("inception_check_hash", True))))
    n = int((cfg.get("val") or {}).get("fid_n_samples", 5000))
    dump = E.SampleDump(module, n_samples=n, batch_size=16)          # host RNG draw, right after the module is built
    # before training starts, persisted next to the images: a resume or the next launch loads it, and under data
    # parallelism the other ranks wait for it ONCE, at start-up (main() gives the process group a long timeout), not
    # inside a collective in the middle of the run
    real_act = real_activations(val_root, features)
    if run.get("eval_on_device", False):
        mu, sigma = real_statistics_cache(val_root)
        score = {}
        if run.get("inception_score", False):
            score = {"inception_score": True, "inception_splits": int(run.get("inception_score_splits", 10))}
        if run.get("precision_recall", False):
            score["prdc_k"] = int(run.get("precision_recall_k", 5))
        return device_fid_evaluator(dump, features, real_act, device, batch=int(run.get("eval_batch_size", 250)),
                                    average=average, mu=mu, sigma=sigma,
                                    fid_on_device=bool(run.get("fid_on_device", False)),
                                    **(dict(score, swd=swd) if swd is not None else score))
    kid_on_device = bool(run.get("kid_on_device", False))
    # real_act is the same every epoch: its fp64 device copy is made once per run, here
    real_codes = E.device_codes(real_act, device) if kid_on_device else None

    def evaluate(mod, epoch):
        with rendering_from(mod, average):          # generator_average=true: the averaged generator is what is scored
            m = E.evaluate(mod, dump, features, real_act, kid_on_device=kid_on_device,
                           real_codes_device=real_codes)
            if swd is not None:
                m = dict(m, **swd(mod))
        print("epoch %d FID: %.4f KID mean: %.6f KID stddev: %.6f" % (epoch, m["fid"], m["kid"], m["kid_std"])
              + ("" if swd is None else " " + swd.text(m)))
        return m

    return evaluate


def main(argv=None):
    conf_dir, expt, overrides, run = parse_overrides(sys.argv[1:] if argv is None else argv)
    cfg = compose(conf_dir, expt, overrides, run)
    seed_everything(run["seed"])                    # seed_everything(42), reference :27
    if not torch.cuda.is_available():
        raise SystemExit("lightning_gan_zoo_amd.run_network needs an MI355X: the step runs on the HIP kernels and has "
                         "no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # GZ_REHEARSE_ONE_GPU=1 (tests, 1-GPU boxes): all ranks on cuda:0, collectives on gloo -- RCCL refuses two ranks on
    # one device; everything else of the multi-rank path runs as it would on N GPUs
    rehearsal = bool(os.environ.get("GZ_REHEARSE_ONE_GPU")) and world > 1
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    sync = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    module = locate(cfg.model.lm["_target_"])(cfg, logging_dir="output").to(device)
    average = None
    if run["generator_average"]:
        from .averaging import GeneratorAverage
        average = GeneratorAverage(module.generator, beta=float(run["generator_average_beta"]))
        if rank == 0:
            print("generator_average: FID / KID and figures render the averaged generator (beta %g); checkpoints hold "
                  "it as %s*" % (average.beta, AVERAGE_PREFIX))
    slow_group = None
    if world > 1:
        from .ddp import GradSync
        sync = GradSync(module)
        if wants_evaluator(cfg, run):
            # with the FID evaluator on, rank 0 alone generates val.fid_n_samples images and runs InceptionV3 over them
            # at start-up and at every epoch end -- far longer than the default watchdog's 10 minutes.  Only THOSE waits
            # get a long timeout (their own group); every training collective keeps the default, so a rank that dies
            # mid-training is still noticed in minutes.  (swd=true: the same wait, for rank 0's sweep, sorts and distances.)
            import datetime
            # (gloo: the wait is a host-side one, no GPU stream sits behind it)
            slow_group = torch.distributed.new_group(timeout=datetime.timedelta(hours=6), backend="gloo")
    evaluate, failure, scorer = None, None, None
    if rank == 0:
        try:
            if run["swd"]:
                scorer = SwdScorer(cfg, run, module)
            evaluate = make_fid_evaluator(cfg, run, module, device, average, swd=scorer)
        except BaseException as e:  # noqa: BLE001  (SystemExit from a missing weight file included)
            failure = e
            if slow_group is None:
                raise
    def leave_together(failure):
        # rank 0 has what its evaluator needs before step 0 -- or failed, and then says so: the other ranks leave with
        # it instead of sitting in a barrier for the long timeout
        flag = torch.tensor([1 if failure is not None else 0])
        torch.distributed.broadcast(flag, 0, group=slow_group)
        if int(flag.item()):
            if rank == 0:
                print("the evaluator could not be built on rank 0: %r" % (failure,), file=sys.stderr)
            torch.distributed.destroy_process_group()
            raise SystemExit(2)

    if slow_group is not None:
        leave_together(failure)
    figures = None
    if run["figures"]:
        from .core.figures.types import build_figures
        try:
            figs = build_figures(cfg, module, module.logging_dir)
        except ValueError as e:
            raise SystemExit("figures: %s" % e) from e
        have_fid = evaluate is not None or (world > 1 and wants_fid(cfg, run))      # (the SWD hook is made further down)
        figures = EpochFigures(figs, have_fid=have_fid, rank=rank, world=world, group=slow_group, average=average)
    data_group = slow_group
    if world > 1 and run["resident_data"] and data_group is None:
        # rank 0 decodes the whole training set once while the others wait for its cache file: the same kind of
        # start-up wait as the FID statistics above, on a group of the same kind
        import datetime
        data_group = torch.distributed.new_group(timeout=datetime.timedelta(hours=6), backend="gloo")
    data = build_data(cfg, run, device, rank, world, group=data_group)
    monitor = checkpoint_monitor(evaluate is not None, run)
    if run["swd"]:
        # the real set needs the training data, so it is made here: rank 0 reads it while the others wait on the
        # long-timeout group, and a failure is told to them as above
        failure = None
        if scorer is not None:
            try:
                scorer.load_real(swd_real_images(cfg, run, data, device))
            except BaseException as e:  # noqa: BLE001
                failure = e
                if slow_group is None:
                    raise
            if evaluate is None:
                evaluate = swd_evaluator(scorer, average)
        if slow_group is not None:
            leave_together(failure)
    out = fit(module, cfg, data, run, sync=sync, rank=rank, world=world, evaluate=evaluate, slow_group=slow_group,
              figures=figures, average=average, monitor=monitor)
    if world > 1:
        torch.distributed.destroy_process_group()
    return out


if __name__ == "__main__":
    main()

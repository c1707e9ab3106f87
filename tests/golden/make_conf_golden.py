#!/usr/bin/env python3
"""tests/golden/reference_conf_trees.json: the reference's own Hydra config tree (conf/ of the UNMODIFIED reference)
composed by ``lightning_gan_zoo_amd.config.compose_tree`` for the command lines tests/test_config_tree.py checks.

Build container only (the reference tree is not in the repository, and not on the GPU box):

    python tests/golden/make_conf_golden.py

Each entry maps the command line (overrides joined by single spaces) to the resolved tree as plain JSON.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from lightning_gan_zoo_amd import config as C  # noqa: E402
from oracle import ref_import  # noqa: E402

EXPTS = ("dc_gan", "wgan", "wgan_gp", "hologan", "gan_stability_r1")


def builtin_overrides(expt):
    """the command line whose tree make_cfg restates"""
    return ["+expt=" + expt, "filepaths=example"]


def small_net_overrides(expt):
    """the command line the drop-in instantiation test builds its (small) step from"""
    return (builtin_overrides(expt) + ["train.features_gen=8", "train.features_disc=8"] +
            (["generator.in_planes=8", "discriminator.out_planes=8"] if expt == "hologan" else []) +
            (["generator.nfilter=4", "discriminator.nfilter=4", "train.img_size=32"]
             if expt == "gan_stability_r1" else []))


def main():
    conf = os.path.join(ref_import.REFERENCE_ROOT, "conf")
    trees = {}
    for expt in EXPTS:
        for overrides in (builtin_overrides(expt), small_net_overrides(expt)):
            trees[" ".join(overrides)] = C.compose_tree(conf, overrides)
    path = os.path.join(HERE, "reference_conf_trees.json")
    with open(path, "w") as f:
        json.dump(trees, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d trees, %d bytes" % (path, len(trees), os.path.getsize(path)))


if __name__ == "__main__":
    main()

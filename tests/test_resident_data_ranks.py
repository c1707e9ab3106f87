"""Resident training set under data parallelism (gloo, 2 processes, CPU): rank 0 decodes and writes the cache while
rank 1 waits on the process group, learns that the file is there and loads it without decoding an image; a failure on
rank 0 ends rank 1 too instead of leaving it in the wait."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, root, cache, max_gb, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lightning_gan_zoo_amd.resident_data import ResidentImages
        from lightning_gan_zoo_amd.run_network import ImageFolderImages
        decoded = []
        real = ImageFolderImages.decode

        def counting(self, path):
            decoded.append(path)
            return real(self, path)

        ImageFolderImages.decode = counting
        try:
            data = ResidentImages(root, 4, 16, 3, 0.5, 0.5, "cpu", rank=rank, world=world, cache_dir=cache,
                                  max_gb=max_gb, group=dist.group.WORLD)
            u8, labels = data.host_set()
            ret[rank] = ("ok", len(decoded), u8.tobytes(), labels.tolist(), len(data))
        except SystemExit as e:
            ret[rank] = ("exit", len(decoded), str(e))
    finally:
        dist.destroy_process_group()


def _run(root, cache, max_gb):
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), root, cache, max_gb, ret), nprocs=2, join=True)
    return dict(ret)


def test_rank0_builds_and_the_other_rank_loads(tmp_path):
    from test_resident_data import make_folder
    root, cache = str(tmp_path / "data"), str(tmp_path / "cache")
    make_folder(root)
    ret = _run(root, cache, 32)
    assert ret[0][0] == ret[1][0] == "ok"
    assert ret[0][1] == 6 and ret[1][1] == 0                     # rank 1 never decodes
    assert ret[0][2] == ret[1][2] and ret[0][3] == ret[1][3] and ret[0][4] == ret[1][4] == 3


def test_a_failure_on_rank0_ends_the_other_rank(tmp_path):
    from test_resident_data import make_folder
    root = str(tmp_path / "data")
    make_folder(root)
    failed = _run(root, str(tmp_path / "cache2"), 1e-6)          # rank 0 refuses the size: rank 1 leaves with it
    assert failed[0][0] == failed[1][0] == "exit" and "resident_max_gb" in failed[0][2]
    assert "rank 0" in failed[1][2] and not os.path.exists(str(tmp_path / "cache2"))

"""Generator weight averaging on the GPU (averaging.GeneratorAverage, csrc/gz_ema.hip): the multi-tensor kernel against
the reference's expression evaluated by torch, the packed-weight hazard, and the wiring into Trainer, GraphedTrainer,
ddp.GradSync and the runner.

Every comparison with torch is ``torch.equal``: the kernel computes two float32 multiplies and one add without FMA
contraction, which is what torch's three kernels for ``beta*t + (1.-beta)*s`` compute, so there is no tolerance."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAD_SHAPE = -1
SENTINEL = 12345.6787109375
SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 2, 7, 64, 1000, 12289, 2]      # x 5 = 70 tensors
BETAS = [0.999, 0.5, 0.0, 1.0]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _table(pairs):
    """Device job table of (avg, src) tensor pairs -> (table, count, total blocks)."""
    from lightning_gan_zoo_amd._lib import check, lib
    nb = lib.gz_ema_job_bytes()
    host = (ctypes.c_char * (nb * len(pairs)))()
    blocks = 0
    for i, (a, s) in enumerate(pairs):
        n = lib.gz_ema_job(ctypes.c_void_p(ctypes.addressof(host) + i * nb), _ptr(a), _ptr(s), a.numel(), blocks)
        check(min(n, 0), "ema_job")
        assert n == (a.numel() + 4095) // 4096
        blocks += n
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda(), len(pairs), blocks


def _launch(pairs, beta):
    from lightning_gan_zoo_amd._lib import check, lib
    tab, count, blocks = _table(pairs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.gz_ema_update(ctypes.c_void_p(tab.data_ptr()), count, blocks, beta, 1.0 - beta, stream), "ema_update")
    torch.cuda.synchronize()             # (the table must outlive the launch)


def _layout(sizes, misaligned):
    """Element ranges inside one flat buffer: every tensor has one sentinel word directly in front of it and one
    directly behind it; ``misaligned[i]`` makes tensor i start 4 bytes past a 16-byte boundary."""
    spans, sentinels, cur = [], [], 0
    for n, mis in zip(sizes, misaligned):
        cur = (cur + 3) & ~3
        start = cur + 1 if mis else cur + 4
        sentinels += [start - 1, start + n]
        spans.append((start, n))
        cur = start + n + 1
    return spans, sentinels, (cur + 3) & ~3


@pytest.fixture(scope="module")
def parity_case():
    """70 tensors, the inputs and their layout; made once, never written (every test works on clones)."""
    sizes = SIZES * 5
    assert len(sizes) == 70
    # the four alignment combinations of (avg, src), cycling with a period that is coprime to len(SIZES)
    mis_a = [(i % 5) in (1, 3) for i in range(70)]
    mis_s = [(i % 5) in (2, 3) for i in range(70)]
    spans_a, sent_a, len_a = _layout(sizes, mis_a)
    spans_s, _, len_s = _layout(sizes, mis_s)
    g = torch.Generator().manual_seed(11)
    avg = torch.randn(len_a, generator=g).cuda()
    src = torch.randn(len_s, generator=g).cuda()
    avg[torch.tensor(sent_a, device="cuda")] = SENTINEL
    assert avg.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    for (sa, n), (ss, _), ma, ms in zip(spans_a, spans_s, mis_a, mis_s):
        if n:
            assert (avg.data_ptr() + 4 * sa) % 16 == (4 if ma else 0) and (src.data_ptr() + 4 * ss) % 16 == (4 if ms else 0)
    return sizes, spans_a, spans_s, sent_a, avg, src


def _views(buf, spans):
    return [buf[s:s + n] for s, n in spans]


@pytest.mark.parametrize("beta", BETAS)
def test_kernel_matches_torchs_float32_expression(parity_case, beta):
    sizes, spans_a, spans_s, sent_a, avg0, src0 = parity_case
    avg, src = avg0.clone(), src0.clone()
    expected = avg0.clone()
    for t, s in zip(_views(expected, spans_a), _views(src0, spans_s)):
        t.copy_(beta * t + (1. - beta) * s)                   # the reference's expression, float32 on the device
    _launch(list(zip(_views(avg, spans_a), _views(src, spans_s))), beta)
    assert torch.equal(avg, expected)                         # every tensor, and every word between the tensors
    assert torch.equal(src, src0)
    sent = torch.tensor(sent_a, device="cuda")
    assert bool((avg[sent] == SENTINEL).all())
    if beta == 0.0:
        for a, s in zip(_views(avg, spans_a), _views(src0, spans_s)):
            assert torch.equal(a, s)
    if beta == 1.0:
        assert torch.equal(avg, avg0)
    # the same tensors split over two launches: the same bits
    split = avg0.clone()
    pairs = list(zip(_views(split, spans_a), _views(src, spans_s)))
    _launch(pairs[:33], beta)
    _launch(pairs[33:], beta)
    assert torch.equal(split, avg)


def test_fill_call_refuses_bad_jobs_and_launches_nothing():
    from lightning_gan_zoo_amd._lib import lib
    buf = torch.arange(64, dtype=torch.float32).cuda()
    other = torch.ones(64, device="cuda")
    before = buf.clone()
    job = (ctypes.c_char * lib.gz_ema_job_bytes())()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.gz_ema_job(job, p(buf), p(buf), 64, 0) == BAD_SHAPE                 # avg is src
    assert lib.gz_ema_job(job, p(buf), p(buf[24:]), 40, 0) == BAD_SHAPE            # [0, 40) and [24, 64) overlap
    assert lib.gz_ema_job(job, p(buf[24:]), p(buf), 40, 0) == BAD_SHAPE
    assert lib.gz_ema_job(job, None, p(other), 64, 0) == BAD_SHAPE                 # null pointers
    assert lib.gz_ema_job(job, p(buf), None, 64, 0) == BAD_SHAPE
    assert lib.gz_ema_job(job, p(buf), p(other), -1, 0) == BAD_SHAPE               # negative numel
    assert lib.gz_ema_job(job, p(buf[:32]), p(buf[32:]), 32, 0) == 1               # adjacent halves are fine
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((other == 1).all())


# ---- stale packs ---------------------------------------------------------------------------------------------------
def _stale_pack_check(gen, render):
    """averaged() renders, the live weights change, update() with beta = 0 makes the average equal to them: the second
    render must be the live generator's eval-mode output, which it is not if the packed images of the averaged weights
    survive the raw in-place update."""
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    F.set_pack_cache(True)                # (a GraphedTrainer test that ran earlier in the process leaves the cache off)
    avg = GeneratorAverage(gen, beta=0.0)
    with torch.no_grad():
        first = render(avg.averaged()).clone()
        again = render(avg.averaged())
        assert torch.equal(first, again)
        for j, p in enumerate(gen.parameters()):
            p.mul_(1.25).add_(0.003 * (j % 3 - 1))
        avg.update()
        second = render(avg.averaged()).clone()
        was = gen.training
        gen.eval()
        live = render(gen).clone()
        gen.train(was)
    for a, s in zip(avg.shadow.parameters(), gen.parameters()):
        assert torch.equal(a, s)
    assert torch.equal(second, live)
    assert not torch.equal(second, first)
    return avg


def test_update_invalidates_packed_weights_dcgan():
    from lightning_gan_zoo_amd.core.models.standard_networks import Generator
    torch.manual_seed(3)
    gen = Generator(16, 3, 8, img_size=64).cuda()
    z = torch.randn(4, 16, generator=torch.Generator().manual_seed(5)).cuda()
    avg = _stale_pack_check(gen, lambda g: g(z))
    assert not avg.shadow.training and all(not p.requires_grad for p in avg.shadow.parameters())
    assert all(p.requires_grad for p in gen.parameters())


def test_update_invalidates_packed_weights_hologan_and_copies_no_scratch():
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg("hologan", batch_size=4, features=8, noise_dim=16)
    torch.manual_seed(42)
    gen = locate(cfg.model.lm["_target_"])(cfg, None).cuda().generator
    np.random.seed(3)
    views = gen.sample_view(4)
    z = (torch.rand(4, 16, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    gen.prefetch_view(4)                  # per-step scratch of the live generator: a device tensor + numpy's state
    gen.staged_minv = torch.zeros(4, 16, device="cuda")
    held = (gen._prefetched, gen.staged_minv)
    fresh = GeneratorAverage(gen)
    assert fresh.shadow._prefetched is None and fresh.shadow.staged_minv is None
    assert gen._prefetched is held[0] and gen.staged_minv is held[1]
    gen.drop_prefetched_view()
    avg = _stale_pack_check(gen, lambda g: g(z, view_in=views))
    assert avg.shadow.staged_minv is None and gen.staged_minv is held[1]
    assert any(p.dim() == 5 for p in avg.shadow.parameters())       # the 3-D pack cache was in play


# ---- trainers ------------------------------------------------------------------------------------------------------
def _build(expt, bs=8):
    from helpers import fill_closed_form
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg(expt, batch_size=bs, features=8, noise_dim=16)
    torch.manual_seed(42)
    m = locate(cfg.model.lm["_target_"])(cfg, None)
    if expt != "hologan":
        fill_closed_form(m.generator, 1)
        fill_closed_form(m.discriminator, 2)
    return m.cuda()


def _snapshot(net):
    return [p.detach().clone() for p in net.parameters()]


def _recur(ref, snap, beta):
    return [beta * t + (1. - beta) * s for t, s in zip(ref, snap)]


def _same(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize("accumulate", [1, 2, 3])
def test_trainer_advances_the_average_once_per_generator_optimizer_step(accumulate):
    from helpers import FixedNoise, synthetic_noise, synthetic_real
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    from lightning_gan_zoo_amd.harness import Trainer
    beta = 0.9
    m = _build("dc_gan")
    avg = GeneratorAverage(m.generator, beta=beta)
    tr = Trainer(m, accumulate_grad_batches=accumulate, generator_average=avg)
    labels = torch.zeros(8, dtype=torch.int64, device="cuda")
    ref = _snapshot(m.generator)
    assert _same(avg.shadow.parameters(), ref)
    nbatches = 6 if accumulate == 1 else 8
    expected_updates = 0
    for k in range(nbatches):
        m.noise_distn = FixedNoise(synthetic_noise(8, 16, 40 + k))
        before_shadow, before_live = _snapshot(avg.shadow), _snapshot(m.generator)
        stepping = accumulate == 1 or (tr.epoch_batch_idx + 1) % accumulate == 0
        _, idx = tr.step((synthetic_real(8, seed=k).cuda(), labels))
        if idx == 1 and stepping:
            assert not _same(m.generator.parameters(), before_live)          # the optimizer did step
            ref = _recur(ref, _snapshot(m.generator), beta)
            expected_updates += 1
        else:
            assert _same(avg.shadow.parameters(), before_shadow)             # D steps, accumulating batches: untouched
        assert avg.updates == expected_updates
        assert _same(avg.shadow.parameters(), ref)
    assert expected_updates == {1: 3, 2: 4, 3: 1}[accumulate]
    shadow = avg.averaged()
    live_buffers = dict(m.generator.named_buffers())
    assert live_buffers and any(float(b.float().abs().sum()) > 0 for n, b in live_buffers.items() if "running_mean" in n)
    for n, b in shadow.named_buffers():
        assert torch.equal(b, live_buffers[n]), n
    sd = avg.state_dict()
    assert list(sd) == [n for n, _ in m.generator.named_parameters()]


def test_graphed_trainer_replays_advance_the_average():
    from helpers import synthetic_real
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    from lightning_gan_zoo_amd.harness import GraphedTrainer
    beta = 0.9
    m = _build("dc_gan")
    avg = GeneratorAverage(m.generator, beta=beta)
    try:
        tr = GraphedTrainer(m, warmup=2, generator_average=avg)
        torch.manual_seed(7)
        labels = torch.zeros(8, dtype=torch.int64, device="cuda")
        ref = _snapshot(m.generator)
        g_steps = 0
        for k in range(10):               # per optimizer: 2 eager warm-up steps, the capture (+ its replay), 2 replays
            before = _snapshot(avg.shadow)
            _, idx = tr.step((synthetic_real(8, seed=600 + k).cuda(), labels))
            if idx == 1:
                ref = _recur(ref, _snapshot(m.generator), beta)
                g_steps += 1
            else:
                assert _same(avg.shadow.parameters(), before)
            assert _same(avg.shadow.parameters(), ref), k
        assert g_steps == 5 and len(tr.graphs) == 2
        assert not _same(avg.shadow.parameters(), _snapshot(m.generator))
    finally:
        F.set_pack_cache(True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("expt", ["dc_gan", "hologan"])
def test_gradsync_advances_the_average_when_a_pass_has_fully_landed(expt):
    """Single-rank RCCL, small buckets (several per network, a deferred tail, per-bucket optimizer steps at the layer
    gates): the averaged weights equal the plain trainer's bit for bit, and the trace shows one update per generator
    optimizer step, each right after the step of the LAST bucket of that pass.  hologan's D, G, G schedule is the
    hand-over case: a generator pass lands at the gates of the next generator step's forward."""
    import torch.distributed as dist
    from helpers import FixedNoise, synthetic_noise, synthetic_real
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    from lightning_gan_zoo_amd.ddp import GradSync
    from lightning_gan_zoo_amd.harness import Trainer

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1",
                      GZ_DDP_ALWAYS_REDUCE="1")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        cycles = 3
        labels = torch.zeros(8, dtype=torch.int64, device="cuda")
        results, trace, updates = [], None, None
        for use_sync in (True, False):
            m = _build(expt)
            nsteps = cycles * (3 if expt == "hologan" else 2)
            batches = [(synthetic_real(8, seed=k).cuda(), labels) for k in range(nsteps)]
            noises = [synthetic_noise(8, 16, 40 + k, uniform=expt == "hologan") for k in range(nsteps)]
            sync = None
            if use_sync:
                sync = GradSync(m, bucket_bytes=(16 << 10) if expt == "hologan" else (32 << 10), tail_min_bytes=1024)
                sync.trace = trace = []
                assert len(sync.flats[1].buckets) > 1 and sync.lazy[1]
            avg = GeneratorAverage(m.generator, beta=0.9)          # (after GradSync: its hooks must not reach the copy)
            tr = Trainer(m, grad_sync=sync, generator_average=avg)
            assert tr.order == ([0, 1, 1] if expt == "hologan" else [0, 1])
            torch.manual_seed(7)
            np.random.seed(7)
            for k in range(nsteps):
                m.noise_distn = FixedNoise(noises[k])
                tr.step(batches[k])
            tr.finish()
            torch.cuda.synchronize()
            results.append((torch.cat([p.detach().reshape(-1) for p in avg.shadow.parameters()]).cpu(),
                            torch.cat([p.detach().reshape(-1) for p in m.generator.parameters()]).cpu()))
            if sync is not None:
                updates = avg.updates
                sync.close()
            else:
                assert avg.updates == cycles * tr.order.count(1)
        assert torch.equal(results[0][1], results[1][1])           # (the live generators agree, as test_ddp_gpu pins)
        assert torch.equal(results[0][0], results[1][0])
        assert not torch.equal(results[0][0], results[0][1])
        # the trace: every generator pass issues its buckets, steps every one of them, then -- and only then -- lands
        n_g_steps = cycles * (2 if expt == "hologan" else 1)
        assert updates == n_g_steps
        issued, stepped, landed, last_g = set(), set(), 0, None
        gated_handover = False
        for ev, idx, b in trace:
            if idx != 1:
                continue
            if ev == "issue":
                assert not stepped, "a new generator pass was issued before the previous one had landed"
                issued.add(b)
            elif ev == "step":
                assert b in issued and b not in stepped
                stepped.add(b)
            elif ev == "landed":
                assert last_g == "step" and stepped == issued and len(issued) > 1
                issued, stepped = set(), set()
                landed += 1
            if ev == "gate" and stepped and stepped != issued:
                gated_handover = True                              # a pass landing bucket by bucket at layer gates
            if ev in ("issue", "step", "landed"):
                last_g = ev
        assert landed == n_g_steps and not issued
        assert gated_handover
    finally:
        dist.destroy_process_group()
        os.environ.pop("GZ_DDP_ALWAYS_REDUCE", None)


# ---- runner ---------------------------------------------------------------------------------------------------------
SMALL = ["+expt=dc_gan", "dataset=synthetic", "train.batch_size=4", "train.features_gen=8", "train.features_disc=8",
         "model.noise_dim=16", "log_every=1000"]
ENVELOPE = {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "optimizer_states", "lr_schedulers",
            "callbacks"}


def _only_ckpt(d):
    names = os.listdir(d)
    assert len(names) == 1, names
    return torch.load(os.path.join(d, names[0]), weights_only=False)


def test_runner_checkpoints_and_resumes_the_average(tmp_path, monkeypatch, capsys):
    from lightning_gan_zoo_amd import run_network as R
    monkeypatch.chdir(tmp_path)
    ck = str(tmp_path / "on")
    args = SMALL + ["train.ckpt_dir=" + ck, "generator_average=true", "+max_steps=4"]
    module, trainer, step = R.main(args)
    out = capsys.readouterr().out
    assert step == 4 and trainer.generator_average.updates == 2
    assert out.count("generator_average:") == 1 and "averaged generator" in out
    blob = _only_ckpt(ck)
    assert set(blob) == ENVELOPE and blob["global_step"] == 4
    sd = blob["state_dict"]
    gen = {k[len("generator."):]: v for k, v in sd.items() if k.startswith("generator.")}
    avg = {k[len("generator_average."):]: v for k, v in sd.items() if k.startswith("generator_average.")}
    names = [n for n, _ in module.generator.named_parameters()]
    assert list(avg) == names                                      # parameters only, the generator's own names
    assert all(avg[n].shape == gen[n].shape for n in names)
    assert all(torch.equal(avg[n], p.cpu()) for n, p in trainer.generator_average.state_dict().items())
    assert any(not torch.equal(avg[n], gen[n]) for n in names)     # an average, not a copy of the last step
    # resume: the loaded average is the saved one bit for bit (no step is left to run; the state is written again)
    module2, trainer2, step2 = R.main(args)
    out2 = capsys.readouterr().out
    assert step2 == 4 and "resumed from" in out2 and "holds no averaged weights" not in out2
    assert trainer2.generator_average.updates == 0
    assert all(torch.equal(avg[n], p.cpu()) for n, p in trainer2.generator_average.state_dict().items())
    sd2 = _only_ckpt(ck)["state_dict"]
    assert list(sd2) == list(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_runner_with_the_key_off_writes_the_old_envelope_and_a_later_run_starts_the_average(tmp_path, monkeypatch,
                                                                                         capsys):
    from lightning_gan_zoo_amd import run_network as R
    monkeypatch.chdir(tmp_path)
    ck = str(tmp_path / "off")
    module, trainer, step = R.main(SMALL + ["train.ckpt_dir=" + ck, "+max_steps=4"])
    out = capsys.readouterr().out
    assert step == 4 and trainer.generator_average is None and "generator_average" not in out
    blob = _only_ckpt(ck)
    assert set(blob) == ENVELOPE
    assert list(blob["state_dict"]) == list(module.state_dict())   # generator.* / discriminator.*, nothing else
    assert all(k.startswith(("generator.", "discriminator.")) for k in blob["state_dict"])
    # the key on, resuming from that checkpoint: the average starts from the loaded generator, and the run says so
    module2, trainer2, step2 = R.main(SMALL + ["train.ckpt_dir=" + ck, "generator_average=true", "+max_steps=4"])
    out2 = capsys.readouterr().out
    assert step2 == 4 and out2.count("holds no averaged weights") == 1
    loaded = {k[len("generator."):]: v for k, v in blob["state_dict"].items() if k.startswith("generator.")}
    for n, p in trainer2.generator_average.state_dict().items():
        assert torch.equal(p.cpu(), loaded[n]), n
    assert any(k.startswith("generator_average.") for k in _only_ckpt(ck)["state_dict"])


def test_evaluation_renders_the_averaged_generator():
    """run_network.rendering_from: inside, ``module.generator`` is the averaged generator in eval mode (what SampleDump
    and the figures read); afterwards the live one is back with its mode, and the averaged one is still in eval mode."""
    from lightning_gan_zoo_amd import eval as E
    from lightning_gan_zoo_amd.averaging import GeneratorAverage
    from lightning_gan_zoo_amd.run_network import rendering_from
    m = _build("dc_gan")
    avg = GeneratorAverage(m.generator, beta=0.5)
    live = m.generator
    torch.manual_seed(1)
    dump = E.SampleDump(m, n_samples=4, batch_size=4)
    with torch.no_grad():
        for p in live.parameters():
            p.mul_(1.5)
    plain = list(dump.images(m))
    with rendering_from(m, avg):
        assert m.generator is avg.shadow
        averaged = list(dump.images(m))
    assert m.generator is live and live.training and not avg.shadow.training
    assert not np.array_equal(plain[0], averaged[0])
    with rendering_from(m, None):
        assert m.generator is live
    assert np.array_equal(list(dump.images(m))[0], plain[0])

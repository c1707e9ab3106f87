"""Exponential moving average of the generator's weights (reference core/submodules/gan_stability/train.py:144-153,
``update_average``: ``p_tgt.copy_(beta*p_tgt + (1. - beta)*p_src)`` over every named parameter), the generator the
gan_stability results are reported on.

    average = GeneratorAverage(module.generator, beta=0.999)
    trainer = Trainer(module, generator_average=average)       # update() after every generator optimizer step
    images = average.averaged()(z)                             # eval-mode shadow generator, live BatchNorm buffers

One HIP launch per update whatever the number of parameters (csrc/gz_ema.hip: a device-resident job table, built once
because neither the parameters nor their averages ever move).  Parameters are averaged; buffers (BatchNorm running
statistics, ``num_batches_tracked``) are not -- gan_stability averages ``named_parameters()`` only -- they are copied
from the live generator when the averaged one is handed out.  There is no CPU fallback.
"""
import copy
import ctypes
from collections import OrderedDict

import torch

from . import functional as F
from ._lib import check, lib

# per-step scratch a live generator may carry (HoloGAN: the view matrices staged by harness.GraphedTrainer, the view
# prefetched by harness.Trainer together with numpy's generator state): never part of the averaged copy
SCRATCH_ATTRS = ("staged_minv", "_prefetched")


def _structural_copy(generator):
    """``copy.deepcopy(generator)`` (gan_stability train.py:97) without the per-step scratch and without the hooks
    others have put on the live generator (ddp.GradSync's gates belong to the network that is being trained)."""
    held = {a: getattr(generator, a) for a in SCRATCH_ATTRS if getattr(generator, a, None) is not None}
    for a in held:
        setattr(generator, a, None)
    try:
        shadow = copy.deepcopy(generator)
    finally:
        for a, v in held.items():
            setattr(generator, a, v)
    for m in shadow.modules():
        for name in ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks",
                     "_forward_hooks_with_kwargs", "_forward_pre_hooks_with_kwargs", "_forward_hooks_always_called"):
            d = getattr(m, name, None)
            if d:
                setattr(m, name, type(d)())
    return shadow


class GeneratorAverage:
    def __init__(self, generator, beta=0.999):
        beta = float(beta)
        if not 0.0 <= beta <= 1.0:
            raise ValueError("GeneratorAverage: beta must lie in [0, 1], got %r" % (beta,))
        for name, p in generator.named_parameters():
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError("lightning_gan_zoo_amd: GeneratorAverage needs contiguous float32 GPU parameters "
                                   "(%s is %s on %s); the HIP path has no CPU fallback" % (name, p.dtype, p.device))
        self.generator = generator
        self.beta = beta
        # what torch makes of the reference's Python expression: both factors are doubles rounded to float32 once
        self.one_minus_beta = 1.0 - beta
        self.shadow = _structural_copy(generator)
        self.shadow.eval()
        for p in self.shadow.parameters():
            p.requires_grad_(False)
        live = OrderedDict(generator.named_parameters())
        mine = OrderedDict(self.shadow.named_parameters())
        if list(live) != list(mine):
            raise RuntimeError("GeneratorAverage: the copy's parameter names differ from the generator's")
        self.names = list(live)
        self._src = [live[n] for n in self.names]
        self._avg = [mine[n] for n in self.names]
        self._repack = [p for p in self._avg if p.dim() >= 4]       # parameters with packed GEMM images (2-D, 3-D)
        self.updates = 0              # update() calls made by the host (the replay of a captured one is not counted)
        self._table = None
        self._build_table()

    # ---- the device job table ------------------------------------------------------------------------------------
    def _build_table(self):
        nb = lib.gz_ema_job_bytes()
        host = (ctypes.c_char * (nb * len(self.names)))()
        blocks = 0
        for i, (a, s) in enumerate(zip(self._avg, self._src)):
            n = lib.gz_ema_job(ctypes.c_void_p(ctypes.addressof(host) + i * nb), F._p(a), F._p(s), a.numel(), blocks)
            check(min(n, 0), "ema_job(%s)" % self.names[i])
            blocks += n
        self._table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(self._avg[0].device)
        self._blocks = blocks
        self._ptrs = [p.data_ptr() for p in self._src]

    def _moved(self):
        ptrs = self._ptrs
        for i, p in enumerate(self._src):
            if p.data_ptr() != ptrs[i]:
                return True
        return False

    # ---- the average ---------------------------------------------------------------------------------------------
    def update(self):
        """avg = beta * avg + (1 - beta) * live over every parameter: ONE launch on the current stream."""
        if self._moved():              # (a .to() / .float() replaced a parameter's storage: new addresses, new table)
            self._build_table()
        check(lib.gz_ema_update(F._p(self._table), len(self.names), self._blocks, self.beta, self.one_minus_beta,
                                F._stream()), "ema_update")
        # a raw in-place kernel: no version bump, so the packed images of the averaged weights are stale from here on
        for p in self._repack:
            F.invalidate(p)
        self.updates += 1

    @torch.no_grad()
    def reset(self):
        """The average starts again as a copy of the live parameters."""
        for a, s in zip(self._avg, self._src):
            a.copy_(s)
        for p in self._repack:
            F.invalidate(p)

    @torch.no_grad()
    def averaged(self):
        """The averaged generator, in eval mode, with the live generator's buffers as they are NOW."""
        for (na, a), (ns, s) in zip(self.shadow.named_buffers(), self.generator.named_buffers()):
            if na != ns:
                raise RuntimeError("GeneratorAverage: buffer %s of the copy faces %s of the generator" % (na, ns))
            a.copy_(s)
        self.shadow.eval()
        return self.shadow

    def state_dict(self):
        """{parameter name of the generator: averaged tensor} (parameters only: the buffers are the live ones)."""
        return OrderedDict((n, a.detach()) for n, a in zip(self.names, self._avg))

    @torch.no_grad()
    def load_state_dict(self, state):
        """In place: the averaged tensors keep their addresses, the device job table stays valid."""
        missing = [n for n in self.names if n not in state]
        extra = [n for n in state if n not in set(self.names)]
        if missing or extra:
            raise KeyError("GeneratorAverage.load_state_dict: missing %s, unexpected %s" % (missing, extra))
        for n, a in zip(self.names, self._avg):
            v = state[n]
            if tuple(v.shape) != tuple(a.shape):
                raise ValueError("GeneratorAverage.load_state_dict: %s has shape %s, expected %s" %
                                 (n, tuple(v.shape), tuple(a.shape)))
            a.copy_(v)
        for p in self._repack:
            F.invalidate(p)

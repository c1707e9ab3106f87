"""Differentiable augmentation of the discriminator's input (DiffAugment, Zhao et al. 2020).

    diffaugment=color,translation,cutout          # run_network key; any comma-separated subset, "" = off

Per call the parameters of every sample are drawn on the HOST torch generator (as the latent noise is), travel to the
device as one float32 tensor [R, 8] and are applied by one launch of ``functional.diffaugment`` (csrc/gz_diffaug.hip):

    column   0  b   brightness   rand - 0.5                      x1 = x + b
             1  s   saturation   2 rand                          x2 = m + s (x1 - m),  m = channel mean per pixel
             2  c   contrast     rand + 0.5                      x3 = M + c (x2 - M),  M = sample mean
             3  th  shift        randint(-sh, sh + 1), sh = int(H / 8 + 0.5)      x4[h, w] = x3[h + th, w + tw] or 0
             4  tw               randint(-sw, sw + 1), sw = int(W / 8 + 0.5)
             5  h0  box corner   randint(0, H + (1 - cut_h % 2)) - cut_h // 2,  cut_h = int(H / 2 + 0.5)
             6  w0               likewise                        y = x4 with [h0, h0 + cut_h) x [w0, w0 + cut_w) zeroed
             7  0   unused

drawn in this order, one draw of R values per column; the integers are stored as exact floats.  A group that is not in
the policy makes NO draw and stores its identity (0, 1, 1 / 0, 0 / a box of size 0).
"""
import torch

from . import functional as F
from .harness import draw_on_host

GROUPS = ("color", "translation", "cutout")


def parse_policy(policy):
    """'color,cutout' -> ('color', 'cutout') in the order of GROUPS; '' / None -> ().  An unknown name is a ValueError
    that lists the three."""
    if policy is None or policy is False:
        return ()
    names = [n.strip() for n in str(policy).split(",") if n.strip()]
    unknown = [n for n in names if n not in GROUPS]
    if unknown:
        raise ValueError("diffaugment: unknown augmentation %s; the policy is a comma-separated subset of %s"
                         % (", ".join(repr(n) for n in unknown), ", ".join(GROUPS)))
    return tuple(g for g in GROUPS if g in names)


def _half_up(v):
    return int(v + 0.5)


class DiffAugment:
    """``DiffAugment(policy)(x, x1=None)`` -> aug(x), or [aug(x); aug(x1)] stacked along the batch from one launch.

    ``params`` is the test hook (like ``WGANGP.gp_alpha``): a tensor [>= R, 8] whose first R rows are used instead of a
    draw; no generator state is consumed then."""
    params = None

    def __init__(self, policy):
        self.groups = parse_policy(policy)

    def __bool__(self):
        return bool(self.groups)

    def cut(self, H, W):
        return (_half_up(H / 2), _half_up(W / 2)) if "cutout" in self.groups else (0, 0)

    def draw(self, R, H, W):
        """The host draw: float32 [R, 8], columns and draw order as in the module docstring."""
        p = torch.zeros((R, 8), dtype=torch.float32)
        p[:, 1] = 1.0
        p[:, 2] = 1.0
        if "color" in self.groups:
            p[:, 0] = torch.rand(R) - 0.5
            p[:, 1] = 2 * torch.rand(R)
            p[:, 2] = torch.rand(R) + 0.5
        if "translation" in self.groups:
            sh, sw = _half_up(H / 8), _half_up(W / 8)
            p[:, 3] = torch.randint(-sh, sh + 1, (R,)).float()
            p[:, 4] = torch.randint(-sw, sw + 1, (R,)).float()
        if "cutout" in self.groups:
            cut_h, cut_w = self.cut(H, W)
            p[:, 5] = (torch.randint(0, H + (1 - cut_h % 2), (R,)) - cut_h // 2).float()
            p[:, 6] = (torch.randint(0, W + (1 - cut_w % 2), (R,)) - cut_w // 2).float()
        return p

    def __call__(self, x, x1=None):
        R = x.shape[0] + (0 if x1 is None else x1.shape[0])
        H, W = x.shape[2], x.shape[3]
        if self.params is not None:
            if self.params.shape[0] < R:
                raise RuntimeError("diffaugment: the pinned params hold %d rows, the call has %d samples"
                                   % (self.params.shape[0], R))
            params = self.params[:R].to(device=x.device, dtype=torch.float32)
        else:
            params = draw_on_host(lambda: self.draw(R, H, W), x.device)
        return F.diffaugment(x, params, self.cut(H, W), x1)


# ---------------------------------------------------------------------------------------------------------------
# Adaptive discriminator augmentation (Karras et al. 2020, "Training Generative Adversarial Networks with Limited
# Data"): a probability p per sample and group, the pixel-blitting group (x-flip, 90-degree turns) and a controller
# that moves p from r_t = E[sign(D(real))].  Everything above stays as it is; the classes below are built only when one
# of the runner keys augment_blit / augment_p / ada_target is set (build_augment).
#
#     params [R, 16]:  0..6   as above
#                      7      o = k + 4 f     f = randint(0, 2) if xflip is in the policy, k = randint(0, 4) if rot90 is;
#                                             Q x = torch.rot90(x.flip(3) if f else x, k, dims=[2, 3])
#                      8..12  uniforms in [0, 1): the gates of color, translation, cutout, xflip, rot90 -- one
#                             torch.rand((R, 5)), drawn last and only when a probability is in play
#                      13..15 zero
#
# A group is applied to a sample iff its uniform is below p.  p lives in device memory (the third of the four floats
# {sum_sign, count, p, last_r} of the controller state) and is compared inside the kernel: nothing is read back.
# ---------------------------------------------------------------------------------------------------------------
BLIT_GROUPS = ("xflip", "rot90")
GATE_COLUMNS = {"color": 8, "translation": 9, "cutout": 10, "xflip": 11, "rot90": 12}


def parse_blit(blit):
    """'rot90,xflip' -> ('xflip', 'rot90') in the order of BLIT_GROUPS; '' / None -> ().  An unknown name is a
    ValueError that lists the two."""
    if blit is None or blit is False:
        return ()
    names = [n.strip() for n in str(blit).split(",") if n.strip()]
    unknown = [n for n in names if n not in BLIT_GROUPS]
    if unknown:
        raise ValueError("augment_blit: unknown transform %s; the value is a comma-separated subset of %s"
                         % (", ".join(repr(n) for n in unknown), ", ".join(BLIT_GROUPS)))
    return tuple(g for g in BLIT_GROUPS if g in names)


class AdaptiveAugment(DiffAugment):
    """``AdaptiveAugment(policy, blit, p, target, interval, kimg)(x, x1=None)``: DiffAugment's call, through
    ``functional.diffaugment_gated`` (csrc/gz_ada.hip).

    ``p``: a fixed probability in [0, 1]; None means 1.0 (no gate uniforms are drawn, every group of the policy is
    applied), or the start value 0.0 when ``target`` is set.  ``target`` in (0, 1): adapt p toward
    E[sign(D(real))] = target; ``observe(real_logits)`` is then called once per discriminator step, accumulates the
    statistic on the device and, every ``interval``-th call, launches the controller update with step
    ``len(real_logits) * interval / (kimg * 1000)``.  The host never reads the state except in ``p_value`` /
    ``values`` / ``state_dict`` (logging and checkpoints).

    ``params`` is the test hook as in DiffAugment, here [>= R, 16]."""

    def __init__(self, policy, blit="", p=None, target=None, interval=4, kimg=500):
        super().__init__(policy)
        self.blit_groups = parse_blit(blit)
        self.blit = (1 if "xflip" in self.blit_groups else 0) | (2 if "rot90" in self.blit_groups else 0)
        if p is not None and not 0.0 <= float(p) <= 1.0:
            raise ValueError("augment_p must lie in [0, 1], got %r" % (p,))
        if target is not None and not 0.0 < float(target) < 1.0:
            raise ValueError("ada_target must lie in (0, 1), got %r" % (target,))
        if int(interval) < 1:
            raise ValueError("ada_interval must be a positive integer, got %r" % (interval,))
        if not float(kimg) > 0:
            raise ValueError("ada_kimg must be positive, got %r" % (kimg,))
        self.target = None if target is None else float(target)
        self.interval, self.kimg = int(interval), float(kimg)
        self.gated = p is not None or target is not None          # a probability is in play: gate uniforms are drawn
        self.p_start = float(p) if p is not None else (0.0 if target is not None else 1.0)
        self.d_steps = 0
        self._state = None                                        # device floats {sum_sign, count, p, last_r}

    def __bool__(self):
        return bool(self.groups or self.blit_groups)

    @property
    def adaptive(self):
        return self.target is not None

    def state(self, device):
        if self._state is None:
            self._state = torch.tensor([0.0, 0.0, self.p_start, 0.0], dtype=torch.float32, device=device)
        elif self._state.device != device:                        # (the module was moved: once, not per step)
            self._state = self._state.to(device)
        return self._state

    def draw(self, R, H, W):
        """The host draw: float32 [R, 16].  DiffAugment's seven columns in its order, then the flip bits, then the turn
        counts, then the [R, 5] gate uniforms -- each only when its group (or a probability) is in play."""
        p = torch.zeros((R, 16), dtype=torch.float32)
        p[:, :8] = super().draw(R, H, W)
        if "xflip" in self.blit_groups:
            p[:, 7] += 4 * torch.randint(0, 2, (R,)).float()
        if "rot90" in self.blit_groups:
            p[:, 7] += torch.randint(0, 4, (R,)).float()
        if self.gated:
            p[:, 8:13] = torch.rand((R, 5))
        return p

    def __call__(self, x, x1=None):
        R = x.shape[0] + (0 if x1 is None else x1.shape[0])
        H, W = x.shape[2], x.shape[3]
        if "rot90" in self.blit_groups and H != W:
            raise RuntimeError("augment_blit: rot90 needs a square image, got %d x %d" % (H, W))
        if self.params is not None:
            if self.params.shape[0] < R:
                raise RuntimeError("diffaugment: the pinned params hold %d rows, the call has %d samples"
                                   % (self.params.shape[0], R))
            params = self.params[:R].to(device=x.device, dtype=torch.float32)
        else:
            params = draw_on_host(lambda: self.draw(R, H, W), x.device)
        p = None
        if self.gated:
            p = self.state(x.device)[2:3]
            if self.adaptive:
                # the controller may move p between this call's forward and its backward (observe() sits between
                # them): the launches of this call, of whatever order, read a copy of their own
                p = p.clone()
        return F.diffaugment_gated(x, params, self.cut(H, W), p, self.blit, x1)

    def observe(self, real_logits):
        """Once per discriminator step, with the discriminator's logits of the (augmented) real batch.  Two launches at
        most, no synchronisation; a no-op unless ``ada_target`` is set."""
        if self.target is None:
            return
        logits = real_logits.detach().reshape(-1)
        state = self.state(logits.device)
        F.ada_observe(logits, state)
        self.d_steps += 1
        if self.d_steps % self.interval == 0:
            F.ada_update(state, self.target, len(logits) * self.interval / (self.kimg * 1000.0))

    def values(self):
        """(p, last r) -- a host read; for logging and checkpoints only."""
        if self._state is None:
            return self.p_start, 0.0
        s = self._state.cpu()
        return float(s[2]), float(s[3])

    def p_value(self):
        return self.values()[0]

    def state_dict(self):
        return {"p": self.p_value(), "d_steps": self.d_steps}

    def load_state_dict(self, sd):
        p = float(sd["p"])
        if not 0.0 <= p <= 1.0:
            raise ValueError("AdaptiveAugment: a checkpoint holds p = %r" % (p,))
        self.p_start, self.d_steps = p, int(sd.get("d_steps", 0))
        if self._state is not None:
            self._state = torch.tensor([0.0, 0.0, p, 0.0], dtype=torch.float32, device=self._state.device)


ADA_DEFAULTS = {"augment_blit": "", "augment_p": None, "ada_target": None, "ada_interval": 4, "ada_kimg": 500}


def build_augment(cfg):
    """The module's augmentation from its cfg: DiffAugment itself while the keys of ADA_DEFAULTS are at their defaults
    (so that nothing about a run without them changes), else AdaptiveAugment."""
    policy = cfg.get("diffaugment", "")
    keys = {k: cfg.get(k, d) for k, d in ADA_DEFAULTS.items()}
    if not keys["augment_blit"] and keys["augment_p"] is None and keys["ada_target"] is None:
        return DiffAugment(policy)
    return AdaptiveAugment(policy, keys["augment_blit"], keys["augment_p"], keys["ada_target"], keys["ada_interval"],
                           keys["ada_kimg"])

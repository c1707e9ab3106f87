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

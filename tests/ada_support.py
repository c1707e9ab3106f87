"""The yardstick of the adaptive-augmentation tests: gz_diffaug_gated in plain torch ops on top of diffaugment_support
(fp64 for the kernel tests, fp32 on the device for the whole-step tests), and an ``np.float32`` model of the controller.

    params16 = (b, s, c, th, tw, h0, w0, o, u_color, u_translation, u_cutout, u_xflip, u_rot90, 0, 0, 0)
    a group is on iff p is None or u_group < p (compared in fp32, as the kernel compares)
    o = k + 4 f, clamped to [0, 7] (NaN: 0), f kept only with blit bit 0 and the xflip gate, k with bit 1 and rot90's
    Q x = rot90(flip_w(x) if f else x, k);   A' = Mask Shift Q Con Sat;   A'^T g = Q^T Con Sat Shift^T Mask g
    colour off: the colour maps are bypassed, not run at (0, 1, 1)
"""
import numpy as np
import torch

import diffaugment_support as S

U_COLOR, U_SHIFT, U_CUT, U_FLIP, U_ROT = 8, 9, 10, 11, 12


def gates(params16, p):
    """bool [R, 5]: colour, translation, cutout, xflip, rot90."""
    u = params16[:, 8:13].detach().cpu().float()
    if p is None:
        return torch.ones_like(u, dtype=torch.bool)
    return u < torch.tensor(float(p), dtype=torch.float32)


def orientation(params16, on, blit):
    """(f, k) per sample after clamping, masking by ``blit`` and gating."""
    o = params16[:, 7].detach().cpu().float()
    o = torch.where(torch.isnan(o), torch.zeros_like(o), o).clamp(0, 7).to(torch.int64)
    f = torch.where(on[:, 3] & bool(blit & 1), (o >> 2) & 1, torch.zeros_like(o))
    k = torch.where(on[:, 4] & bool(blit & 2), o & 3, torch.zeros_like(o))
    return f.tolist(), k.tolist()


def q_apply(x, f, k):
    """Q x for one sample batch [1, C, H, W]."""
    return torch.rot90(x.flip(3) if f else x, k, dims=[2, 3])


def q_transpose(x, f, k):
    y = torch.rot90(x, -k, dims=[2, 3])
    return y.flip(3) if f else y


def _row(params16, n, on, cut):
    """The effective DiffAugment row [1, 8] of sample n: an off translation is a zero shift, an off cutout a box at
    h0 = -cut_h (outside the image)."""
    row = params16[n:n + 1, :8].detach().cpu().clone()
    row[:, 7] = 0
    if not on[n, 1]:
        row[:, 3:5] = 0
    if not on[n, 2]:
        row[:, 5] = -cut[0]
    return row


def reference(x, params16, cut, p, blit, mode):
    """gz_diffaug_gated in x's dtype on x's device, sample by sample."""
    on = gates(params16, p)
    fs, ks = orientation(params16, on, blit)
    out = []
    for n in range(len(x)):
        xn, row = x[n:n + 1], _row(params16, n, on, cut)
        colour = bool(on[n, 0])
        if mode != 2:
            q = q_apply(xn, fs[n], ks[n])
            if colour:
                y = S.forward(q, row, cut, affine=(mode == 0))
            else:
                _, _, _, th, tw, h0, w0 = S._cols(row, q)
                y = S._shift(q, th, tw) * S._keep(q, h0, w0, cut)
        else:
            if colour:
                z = S.adjoint(xn, row, cut)
            else:
                _, _, _, th, tw, h0, w0 = S._cols(row, xn)
                z = S._shift(xn * S._keep(xn, h0, w0, cut), -th, -tw)
            y = q_transpose(z, fs[n], ks[n])
        out.append(y)
    return torch.cat(out)


def bound_params(params16, p):
    """The rows ``diffaugment_support.bound`` reads, with colour-off samples at the identity (their error is zero; the
    bound then is 32 u max|x|, which zero meets)."""
    on = gates(params16, p)
    row = params16[:, :8].detach().cpu().clone()
    off = ~on[:, 0]
    row[off, 0], row[off, 1], row[off, 2] = 0.0, 1.0, 1.0
    return row


def widen(params8, codes=None, uniforms=None):
    """[R, 8] -> [R, 16] with the orientation codes in column 7 and the gate uniforms in 8..12 (default 0: on for
    every p > 0)."""
    R = len(params8)
    out = torch.zeros((R, 16), dtype=torch.float32)
    out[:, :8] = params8
    if codes is not None:
        out[:, 7] = torch.as_tensor(codes, dtype=torch.float32)
    if uniforms is not None:
        out[:, 8:13] = torch.as_tensor(uniforms, dtype=torch.float32)
    return out


def mixed_uniforms(R, seed):
    """Gate uniforms on both sides of p = 0.5, a different pattern per sample and group."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand((R, 5), generator=g)


class TorchAdaptiveAugment:
    """Stands in for ``augment.AdaptiveAugment`` inside a step: the yardstick in x's dtype on x's device through plain
    autograd, with pinned ``params16``."""

    def __init__(self, params16, cut_on, p, blit):
        self.params, self.cut_on, self.p, self.blit, self.calls = params16, cut_on, p, blit, 0

    def __call__(self, x, x1=None):
        self.calls += 1
        xs = x if x1 is None else torch.cat([x, x1])
        cut = S.cut_size(*xs.shape[2:]) if self.cut_on else (0, 0)
        return reference(xs, self.params[:len(xs)], cut, self.p, self.blit, 0)


# ---------------------------------------------------------------------------------------------------------------
# the controller in np.float32, operation by operation as csrc/gz_ada.hip states it
# ---------------------------------------------------------------------------------------------------------------
class ControllerModel:
    def __init__(self, p=0.0):
        self.state = np.array([0.0, 0.0, p, 0.0], dtype=np.float32)

    def observe(self, logits):
        x = np.asarray(logits, dtype=np.float32)
        sign = (x > 0).astype(np.int64) - (x < 0).astype(np.int64)          # NaN and +-0: 0
        self.state[0] = np.float32(self.state[0] + np.float32(int(sign.sum())))
        self.state[1] = np.float32(self.state[1] + np.float32(len(x)))

    def update(self, target, step):
        target, step = np.float32(target), np.float32(step)
        if not self.state[1] > 0:
            return
        r = np.float32(self.state[0] / self.state[1])
        d = np.float32(r - target)
        sg = np.float32(int(d > 0) - int(d < 0))
        p = np.float32(self.state[2] + np.float32(step * sg))
        self.state[2] = min(max(p, np.float32(0)), np.float32(1))
        self.state[3] = r
        self.state[0] = self.state[1] = 0

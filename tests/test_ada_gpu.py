"""gz_diffaug_gated, gz_ada_observe and gz_ada_update on the device against the yardstick of ada_support.py: bit-exact on
cases made of fp32 numbers only (all orientations, gates one ulp on either side of p), the identity at p = 0, the bound of
DESIGN.md 3.5.4 on drawn data over every launch geometry of the new launcher, its guards and refusals, the autograd pair
to second order, the controller bit for bit against an np.float32 model, whole steps of all five experiments against
fp32 torch ops, the controller inside a step, and the runner with its checkpoint entry.

Worst |y - y64| / bound measured on an MI355X (each tolerance test prints its own): 0.052 over the listed shapes in
every orientation, 0.060 over one shape per launch geometry without the turning route, 0.053 with it."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import ada_support as A
import diffaugment_support as S
import scenario

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
GUARD = 12345.678
OK, BAD_SHAPE, UNSUPPORTED = 0, -1, -2


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(x0, x1, params, p, y, R0, R1, C, H, W, cut, blit, mode):
    from lightning_gan_zoo_amd._lib import lib
    from lightning_gan_zoo_amd.functional._base import _stream
    return lib.gz_diffaug_gated(_ptr(x0), _ptr(x1), _ptr(params), _ptr(p), _ptr(y), R0, R1, C, H, W, cut[0], cut[1], blit,
                                mode, _stream())


def _place(t, misaligned):
    """``t`` on the device, starting 4 bytes past a 16-byte boundary when ``misaligned``."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()] if misaligned else buf[:t.numel()]
    view.copy_(t.reshape(-1))
    return view


def _scalar(p):
    return None if p is None else torch.tensor([p], dtype=torch.float32, device="cuda")


def run_kernel(x, params, cut, p, blit, mode, x1=None, y_lead=4, misaligned=False):
    """One launch through the C ABI; y is carved out of a larger buffer filled with a guard word, ``y_lead`` words in.
    Everything outside y must still hold the guard afterwards."""
    R0, C, H, W = x.shape
    R1 = 0 if x1 is None else x1.shape[0]
    n = (R0 + R1) * C * H * W
    buf = torch.full((y_lead + n + 4,), GUARD, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    y = buf[y_lead:y_lead + n]
    rc = _launch(_place(x, misaligned), _place(x1, misaligned), params.cuda().contiguous(), _scalar(p), y, R0, R1, C, H, W,
                 cut, blit, mode)
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert bool((buf[:y_lead] == GUARD).all()) and bool((buf[y_lead + n:] == GUARD).all()), "a guard word was written"
    return y.clone().reshape(R0 + R1, C, H, W).cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------
SQUARE_EXACT = [(1, 8, 8), (4, 16, 16), (1, 32, 32)]
FLIP_EXACT = [(2, 4, 8), (2, 16, 4)]
HALF = 0.5
ULP_GATES = [float(np.nextafter(np.float32(HALF), np.float32(0))), HALF, float(np.nextafter(np.float32(HALF), np.float32(1)))]


def exact_gated_case(shape):
    """The ten hand-pinned rows of diffaugment_support on exact inputs; codes 0..7 (then 5, 3) on square shapes, {0, 4}
    elsewhere; the gate of group g of sample n one ulp below p (on), at p (off) or one ulp above (off), by (n + g) % 3."""
    C, H, W = shape
    square = H == W
    x = S.exact_input(10, C, H, W, 7 * C + H + W)
    codes = [0, 1, 2, 3, 4, 5, 6, 7, 5, 3] if square else [0, 4] * 5
    u = [[ULP_GATES[(n + g) % 3] for g in range(5)] for n in range(10)]
    return x, A.widen(S.exact_rows(H, W), codes, u), (3 if square else 1)


@pytest.mark.parametrize("cut_on", [True, False])
@pytest.mark.parametrize("shape", SQUARE_EXACT + FLIP_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_exact_cases_agree_bit_for_bit(shape, cut_on):
    """Every intermediate of these cases is an fp32 number whatever the gates and the orientation (checked on the
    yardstick below), so the kernel agrees with fp64 bit for bit in all three modes: with the gates at p - ulp, p,
    p + ulp, with p = NULL, from one source and split 4 + 6 over two."""
    x, params, blit = exact_gated_case(shape)
    cut = S.cut_size(*shape[1:]) if cut_on else (0, 0)
    on = A.gates(params, HALF)
    assert bool(on.any(0).all()) and not bool(on.all(0).any())          # every group is on somewhere and off somewhere
    for p in (HALF, None):
        for mode in (0, 1, 2):
            want = A.reference(x.double(), params, cut, p, blit, mode)
            assert torch.equal(want.float().double(), want)
            got = run_kernel(x, params, cut, p, blit, mode, y_lead=1 if cut_on else 4, misaligned=(mode == 1))
            assert torch.equal(got.double(), want), (shape, cut, p, mode, int((got.double() != want).sum()))
            two = run_kernel(x[:4], params, cut, p, blit, mode, x1=x[4:], y_lead=4 if cut_on else 1,
                             misaligned=(mode != 1))
            assert torch.equal(_bits(two), _bits(got)), (shape, cut, p, mode)


# ---------------------------------------------------------------------------------------------------------------
# p = 0
# ---------------------------------------------------------------------------------------------------------------
def drawn_gated_case(shape, R, seed=0, codes=None):
    """x ~ N(0, 1), DiffAugment's own draw for columns 0..6, the given orientation codes (default: n mod 8 on square
    shapes, 4 (n mod 2) elsewhere) and gate uniforms on both sides of 0.5."""
    C, H, W = shape
    x, p8 = S.drawn_case(shape, R, seed=seed)
    if codes is None:
        codes = [n % 8 if H == W else 4 * (n % 2) for n in range(R)]
    return x, A.widen(p8, codes, A.mixed_uniforms(R, 100 * seed + R + H))


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_p_zero_returns_the_input_bits(shape):
    x, params = drawn_gated_case(shape, 8, seed=1)
    x[0, 0, 0, 0], x[1, 0, 0, 1] = -0.0, 0.0
    blit = 3 if shape[1] == shape[2] else 1
    for mode in (0, 1, 2):
        got = run_kernel(x, params, S.cut_size(*shape[1:]), 0.0, blit, mode, misaligned=(mode == 2))
        assert torch.equal(_bits(got), _bits(x)), (shape, mode)


# ---------------------------------------------------------------------------------------------------------------
# tolerance cases
# ---------------------------------------------------------------------------------------------------------------
def _worst_ratio(x, params, cut, p, blit, mode, **kw):
    want = A.reference(x.double(), params, cut, p, blit, mode)
    got = run_kernel(x, params, cut, p, blit, mode, **kw).double()
    return float(((got - want).abs() / S.bound(x, A.bound_params(params, p), mode)).max())


TOLERANCE = [((3, 5, 7), 1), ((3, 12, 20), 1), ((3, 6, 6), 3), ((3, 9, 9), 3), ((3, 64, 64), 3), ((1, 64, 64), 3),
             ((3, 128, 128), 3)]


@pytest.mark.parametrize("R", [1, 6])
@pytest.mark.parametrize("shape,blit", TOLERANCE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_drawn_cases_within_the_bound(shape, blit, R):
    """|y - y64| <= 32 * 2^-24 * S_n (diffaugment_support.bound, unchanged) in every orientation the shape admits: R = 1
    one launch per code with every gate on (p = NULL), R = 6 two launches covering the codes with gates on both sides
    of p = 0.5."""
    all_codes = list(range(8)) if blit == 3 else [0, 4]
    if R == 1:
        launches = [([c], None) for c in all_codes]
    else:
        launches = [([all_codes[(n + s) % len(all_codes)] for n in range(R)], 0.5) for s in (0, 2 if blit == 3 else 1)]
    cut = S.cut_size(*shape[1:])
    worst = 0.0
    for codes, p in launches:
        x, params = drawn_gated_case(shape, R, codes=codes)
        for mode in (0, 1, 2):
            ratio = _worst_ratio(x, params, cut, p, blit, mode, y_lead=4 if R == 6 else 1, misaligned=(R == 1))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, R, codes, mode, ratio)
    print("ada %s R=%d: worst |y - y64| / bound = %.4f" % ("x".join(map(str, shape)), R, worst))


# one shape per (channels, float4 units per lane, lanes) variant of the launcher: without the turning route (blit = 1) the
# shapes of test_diffaugment_gpu.GEOMETRY_SHAPES, with it (blit = 3) squares up to 128 that reach the same variants
FLIP_GEOMETRY = [(1, 256, 256), (2, 128, 256), (4, 128, 128), (3, 128, 170), (1, 128, 128), (2, 64, 64), (1, 64, 100),
                 (3, 64, 96), (3, 64, 128), (4, 5, 9), (2, 7, 6), (1, 4, 4)]
TURN_GEOMETRY = [(1, 128, 128), (1, 100, 100), (1, 90, 90), (1, 45, 45), (1, 32, 32), (1, 4, 4), (2, 128, 128), (2, 90, 90),
                 (2, 64, 64), (2, 40, 40), (2, 6, 6), (3, 128, 128), (3, 100, 100), (3, 64, 64), (3, 45, 45), (3, 20, 20),
                 (4, 128, 128), (4, 90, 90), (4, 45, 45), (4, 20, 20)]


@pytest.mark.parametrize("shape", FLIP_GEOMETRY, ids=lambda s: "x".join(map(str, s)))
def test_every_flip_geometry_within_the_bound(shape):
    x, params = drawn_gated_case(shape, 2, seed=1, codes=[4, 0])
    worst = 0.0
    for cut in (S.cut_size(*shape[1:]), (0, 0)):
        for mode in (0, 1, 2):
            worst = max(worst, _worst_ratio(x, params, cut, None, 1, mode))
    print("ada flip %s: worst |y - y64| / bound = %.4f" % ("x".join(map(str, shape)), worst))
    assert worst <= 1.0, (shape, worst)


@pytest.mark.parametrize("shape", TURN_GEOMETRY, ids=lambda s: "x".join(map(str, s)))
def test_every_turn_geometry_within_the_bound(shape):
    worst = 0.0
    for codes, p in (([1, 3, 5, 7], None), ([6, 3, 2, 5], 0.5)):
        x, params = drawn_gated_case(shape, 4, seed=2, codes=codes)
        for mode in (0, 1, 2):
            worst = max(worst, _worst_ratio(x, params, S.cut_size(*shape[1:]), p, 3, mode))
    print("ada turn %s: worst |y - y64| / bound = %.4f" % ("x".join(map(str, shape)), worst))
    assert worst <= 1.0, (shape, worst)


# ---------------------------------------------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 64, 64), (3, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_misaligned_operands_give_equal_bits(shape):
    x, params = drawn_gated_case(shape, 8, seed=3)
    blit = 3 if shape[1] == shape[2] else 1
    cut = S.cut_size(*shape[1:])
    for mode in (0, 1, 2):
        base = run_kernel(x, params, cut, 0.5, blit, mode)
        for y_lead, misaligned in ((1, False), (4, True), (1, True)):
            a = run_kernel(x[:3], params, cut, 0.5, blit, mode, x1=x[3:], y_lead=y_lead, misaligned=misaligned)
            assert torch.equal(_bits(a), _bits(base)), (shape, mode, y_lead, misaligned)


def test_a_garbage_orientation_code_is_clamped_and_masked():
    shape = (3, 16, 16)
    x, params = drawn_gated_case(shape, 4, seed=4, codes=[0, 0, 0, 0])
    cut = S.cut_size(16, 16)
    garbage = params.clone()
    garbage[:, 7] = torch.tensor([float("nan"), 1e9, -3.0, 5.0])
    for mode in (0, 1, 2):
        base = run_kernel(x, params, cut, None, 0, mode)
        assert torch.equal(_bits(run_kernel(x, garbage, cut, None, 0, mode)), _bits(base))       # blit = 0: code 0
        # permitted: NaN -> 0, 1e9 -> 7, -3 -> 0, as the yardstick clamps
        want = A.reference(x.double(), garbage, cut, None, 3, mode)
        got = run_kernel(x, garbage, cut, None, 3, mode).double()
        assert float(((got - want).abs() / S.bound(x, garbage[:, :8], mode)).max()) <= 1.0
        assert torch.equal(_bits(got[0].float()), _bits(base[0])) and torch.equal(_bits(got[2].float()), _bits(base[2]))
        flip_only = run_kernel(x, garbage, cut, None, 1, mode)                                   # 7 -> flip, 5 -> flip
        want = A.reference(x.double(), garbage, cut, None, 1, mode)
        assert float(((flip_only.double() - want).abs() / S.bound(x, garbage[:, :8], mode)).max()) <= 1.0


def test_refused_calls_return_their_codes_and_leave_y_untouched():
    C, H, W = 3, 8, 8
    x = torch.randn(2, C, H, W, device="cuda")
    x1 = torch.randn(1, C, H, W, device="cuda")
    p = torch.zeros((3, 16), device="cuda")
    p[:, 1:3] = 1.0
    big = torch.zeros(65540, device="cuda")
    y = torch.full((65540,), GUARD, device="cuda")
    cut = (4, 4)
    refused = [
        (UNSUPPORTED, (x, None, p, None, y, 1, 0, 3, 8, 12, cut, 2, 0)),          # rot90 permitted, H != W
        (UNSUPPORTED, (x, None, p, None, y, 1, 0, 3, 12, 8, cut, 3, 2)),
        (UNSUPPORTED, (big, None, p, None, y, 1, 0, 1, 256, 256, cut, 2, 0)),     # rot90 permitted, side > 128
        (UNSUPPORTED, (big, None, p, None, y, 1, 0, 1, 129, 129, cut, 3, 0)),
        (UNSUPPORTED, (x, None, p, None, y, 1, 0, 5, 8, 8, cut, 0, 0)),           # C > 4
        (UNSUPPORTED, (x, None, p, None, y, 1, 0, 3, 3, 8, cut, 1, 0)),           # H < 4
        (UNSUPPORTED, (x, None, p, None, y, 1, 0, 3, 8, 3, cut, 1, 0)),           # W < 4
        (UNSUPPORTED, (big, None, p, None, y, 1, 0, 1, 256, 257, cut, 1, 0)),     # C*H*W > 65536
        (BAD_SHAPE, (None, None, p, None, y, 2, 0, C, H, W, cut, 3, 0)),          # null pointers
        (BAD_SHAPE, (x, None, None, None, y, 2, 0, C, H, W, cut, 3, 0)),
        (BAD_SHAPE, (x, None, p, None, None, 2, 0, C, H, W, cut, 3, 0)),
        (BAD_SHAPE, (x, None, p, None, y, 2, 1, C, H, W, cut, 3, 0)),             # x1 == NULL with R1 != 0
        (BAD_SHAPE, (x, x1, p, None, y, 0, 0, C, H, W, cut, 3, 0)),               # R0 + R1 < 1
        (BAD_SHAPE, (x, x1, p, None, y, -1, 1, C, H, W, cut, 3, 0)),
        (BAD_SHAPE, (x, None, p, None, y, 2, 0, C, H, W, cut, 3, 3)),             # mode outside 0..2
        (BAD_SHAPE, (x, None, p, None, y, 2, 0, C, H, W, cut, 4, 0)),             # blit outside 0..3
        (BAD_SHAPE, (x, None, p, None, y, 2, 0, C, H, W, cut, -1, 0)),
        (BAD_SHAPE, (x, None, p, None, y, 2, 0, C, H, W, (-1, 4), 3, 0)),
        (BAD_SHAPE, (x, None, p, None, x, 2, 0, C, H, W, cut, 3, 0)),             # y overlaps a source
        (BAD_SHAPE, (x, None, p, None, x.reshape(-1)[C * H * W:], 2, 0, C, H, W, cut, 3, 0)),
        (BAD_SHAPE, (x, x1, p, None, x1, 2, 1, C, H, W, cut, 3, 0)),
    ]
    x_before, x1_before = x.clone(), x1.clone()
    for want, args in refused:
        assert _launch(*args) == want, (want, args[5:])
    torch.cuda.synchronize()
    assert bool((y == GUARD).all()) and torch.equal(x, x_before) and torch.equal(x1, x1_before)
    assert _launch(x, x1, p, None, y, 2, 1, C, H, W, cut, 3, 0) == OK                # the same operands, accepted
    assert _launch(x, None, p, None, y, 1, 0, 3, 8, 12, cut, 1, 0) == OK            # a flip needs no square
    torch.cuda.synchronize()


def test_functional_refuses_cpu_tensors_and_bad_params():
    from lightning_gan_zoo_amd import functional as F
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.diffaugment_gated(x, torch.zeros(2, 16), (4, 4), None, 3)
    with pytest.raises(RuntimeError, match=r"params must be \[2, 16\]"):
        F.diffaugment_gated(x.cuda(), torch.zeros(2, 8).cuda(), (4, 4), None, 3)
    with pytest.raises(RuntimeError, match="square"):
        F.diffaugment_gated(torch.zeros(2, 3, 8, 12).cuda(), torch.zeros(2, 16).cuda(), (4, 4), None, 2)
    with pytest.raises(RuntimeError, match="unsupported"):
        F.diffaugment_gated(torch.zeros(2, 5, 8, 8).cuda(), torch.zeros(2, 16).cuda(), (4, 4), None, 3)


# ---------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------
def _second_order(x, params, cut, p, blit, g, v):
    """(y, d<y, g>/dx, d<that, v>/dg) of the product."""
    from lightning_gan_zoo_amd import functional as F
    xr, gr = x.cuda().requires_grad_(), g.cuda().requires_grad_()
    y = F.diffaugment_gated(xr, params.cuda(), cut, _scalar(p), blit)
    (gx,) = torch.autograd.grad((y * gr).sum(), xr, create_graph=True)
    assert gx.requires_grad
    (gg,) = torch.autograd.grad((gx * v.cuda()).sum(), gr)
    return y.detach().cpu(), gx.detach().cpu(), gg.detach().cpu()


@pytest.mark.parametrize("p", [HALF, None])
def test_autograd_pair_is_exact_on_an_exact_case(p):
    shape = (4, 16, 16)
    x, params, blit = exact_gated_case(shape)
    g, v = S.exact_input(10, *shape, seed=91), S.exact_input(10, *shape, seed=92)
    cut = S.cut_size(16, 16)
    y, gx, gg = _second_order(x, params, cut, p, blit, g, v)
    assert torch.equal(y.double(), A.reference(x.double(), params, cut, p, blit, 0))
    assert torch.equal(gx.double(), A.reference(g.double(), params, cut, p, blit, 2))          # A'^T g
    assert torch.equal(gg.double(), A.reference(v.double(), params, cut, p, blit, 1))          # A' v


@pytest.mark.parametrize("shape", [(3, 9, 9), (3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_autograd_pair_within_the_bound_through_double_backward(shape):
    x, params = drawn_gated_case(shape, 8, seed=5)
    gen = torch.Generator().manual_seed(17)
    g, v = torch.randn(x.shape, generator=gen), torch.randn(x.shape, generator=gen)
    cut = S.cut_size(*shape[1:])
    y, gx, gg = _second_order(x, params, cut, 0.5, 3, g, v)
    for got, src, mode in ((y, x, 0), (gx, g, 2), (gg, v, 1)):
        want = A.reference(src.double(), params, cut, 0.5, 3, mode)
        ratio = float(((got.double() - want).abs() / S.bound(src, A.bound_params(params, 0.5), mode)).max())
        assert ratio <= 1.0, (shape, mode, ratio)


def test_sources_that_need_no_gradient_get_none():
    from lightning_gan_zoo_amd import functional as F
    shape = (4, 16, 16)
    x, params, blit = exact_gated_case(shape)
    g = S.exact_input(10, *shape, seed=93)
    cut = S.cut_size(16, 16)
    want = A.reference(g.double(), params, cut, HALF, blit, 2)
    for first in (True, False):
        a, b = x[:4].cuda(), x[4:].cuda()
        (a if first else b).requires_grad_()
        y = F.diffaugment_gated(a, params.cuda(), cut, _scalar(HALF), blit, b)
        y.backward(g.cuda())
        live, dead = (a, b) if first else (b, a)
        assert dead.grad is None
        assert torch.equal(live.grad.cpu().double(), want[:4] if first else want[4:])
    a, b = x[:4].cuda().requires_grad_(), x[4:].cuda().requires_grad_()
    F.diffaugment_gated(a, params.cuda(), cut, _scalar(HALF), blit, b).backward(g.cuda())
    assert torch.equal(torch.cat([a.grad, b.grad]).cpu().double(), want)
    pr, pp = params.cuda().requires_grad_(), _scalar(HALF).requires_grad_()
    F.diffaugment_gated(x.cuda().requires_grad_(), pr, cut, pp, blit).sum().backward()
    assert pr.grad is None and pp.grad is None


# ---------------------------------------------------------------------------------------------------------------
# the controller
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_observe_accumulates_bit_for_bit(n):
    from lightning_gan_zoo_amd import functional as F
    model = A.ControllerModel(p=0.25)
    state = torch.tensor(model.state.copy(), device="cuda")
    gen = torch.Generator().manual_seed(n)
    special = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-45, -1e-45]
    for call in range(3):
        logits = torch.randn(n, generator=gen) + 0.3 * call
        idx = torch.randperm(n, generator=gen)[:len(special)]
        logits[idx] = torch.tensor(special[:len(idx)])
        F.ada_observe(logits.cuda(), state)
        model.observe(logits.numpy())
        assert np.array_equal(state.cpu().numpy().view(np.int32), model.state.view(np.int32)), (n, call)
    assert model.state[1] == 3 * n and model.state[2] == 0.25


def test_update_follows_the_float32_model_across_both_clamps():
    from lightning_gan_zoo_amd import functional as F
    from lightning_gan_zoo_amd._lib import lib
    model = A.ControllerModel(p=0.0)
    state = torch.tensor(model.state.copy(), device="cuda")
    target, step = 0.6, 0.3
    # 12 intervals: down at 0 (clamp), up to 1 and beyond (clamp), an empty interval, r == target, down again to 0
    script = [[-1.0, -2.0], [1.0, 2.0, 3.0], [1.0] * 7, [2.0] * 3, [1.0, 1.0, 1.0, -1.0, 1.0, 1.0, 1.0], [],
              [1.0, 1.0, 1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [-3.0], [0.0, 0.0, 1.0], [-1.0] * 5, [-1.0]]
    seen = []
    for logits in script:
        if logits:
            t = torch.tensor(logits)
            F.ada_observe(t.cuda(), state)
            model.observe(t.numpy())
        F.ada_update(state, target, step)
        model.update(target, step)
        got = state.cpu().numpy()
        assert got[2].view(np.int32) == model.state[2].view(np.int32), (logits, got, model.state)
        assert abs(int(got[3].view(np.int32)) - int(model.state[3].view(np.int32))) <= 1, (logits, got, model.state)
        assert got[0] == 0 and got[1] == 0
        seen.append(float(got[2]))
    assert seen[0] == 0.0 and max(seen) == 1.0 and seen.count(1.0) >= 2 and seen[-1] == 0.0
    assert seen[5] == seen[4] and seen[6] == seen[5]           # the empty interval and r == target leave p alone
    one = ctypes.c_void_p(state.data_ptr())
    for bad in (-0.1, float("nan"), float("inf")):
        assert lib.gz_ada_update(one, 0.6, bad, None) == BAD_SHAPE
    assert lib.gz_ada_observe(one, 0, one, None) == BAD_SHAPE and lib.gz_ada_observe(None, 1, one, None) == BAD_SHAPE


# ---------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------
def _build(expt, stacked=True, **keys):
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg(expt, **scenario.cfg_kwargs(expt, "tiny"))
    for k, v in keys.items():
        cfg[k] = v
    torch.manual_seed(42)
    m = locate(cfg.model.lm["_target_"])(cfg, None)
    scenario._prepare(m, False)
    m.to("cuda")
    m.stack_d_passes = stacked
    return m


@pytest.mark.parametrize("idx", [0, 1])
@pytest.mark.parametrize("expt", ["dc_gan", "wgan", "wgan_gp", "gan_stability_r1", "hologan"])
def test_whole_step_kernel_against_torch_ops(expt, idx):
    """One training step at the tiny scenario size with pinned params16 -- orientations n mod 8, gate uniforms on both
    sides of the fixed p = 0.5 -- once through gz_diffaug_gated, once with ``self.diffaugment`` swapped for the yardstick
    in fp32 torch ops (plain autograd: second order for gan_stability_r1 and wgan_gp).  Activation decisions are
    recorded and replayed as in test_diffaugment_gpu.py.  Loss and every gradient at 1e-3."""
    from test_diffaugment_gpu import RecordingTape, _compare, _step, decisions
    from test_oracle_golden import pinned_scale
    from lightning_gan_zoo_amd.augment import AdaptiveAugment
    inputs = scenario.make_inputs(expt, "tiny")
    real = inputs["real_d0"]
    _, params = drawn_gated_case(tuple(real.shape[1:]), 2 * len(real), seed=5)
    keys = dict(diffaugment=FULL, augment_blit="xflip,rot90", augment_p=0.5)

    m = _build(expt, **keys)
    assert type(m.diffaugment) is AdaptiveAugment and m.diffaugment.blit == 3 and not m.diffaugment.adaptive
    m.diffaugment.params = params
    rec = RecordingTape()
    with decisions(rec):
        kernel = _step(m, expt, idx, inputs)
    tape = rec.finish()

    m = _build(expt, **keys)
    m.diffaugment = A.TorchAdaptiveAugment(params.cuda(), True, 0.5, 3)
    with decisions(tape):
        torch_ops = _step(m, expt, idx, inputs)
    assert m.diffaugment.calls >= 1
    assert tape.cursor == len(tape.masks), "the two runs took different numbers of activation decisions"
    total = sum(t.numel() for t in tape.masks)
    flips = sum(t[1] for t in tape.mismatches)
    assert flips <= max(4, 1e-4 * total) and all(t[3] <= 3e-4 for t in tape.mismatches), tape.mismatches
    _compare(kernel, torch_ops, pinned_scale(expt, "tiny"), "%s step %d gated kernel vs torch ops" % (expt, idx))


@pytest.mark.parametrize("stacked", [True, False])
def test_controller_moves_p_every_interval_in_a_step(stacked):
    """dc_gan with ada_target: the discriminator's logits are forced positive (r = 1 > target), so p rises by exactly
    ``step`` = bs * interval / (kimg * 1000) at every ``ada_interval``-th discriminator step and not in between;
    generator steps do not count.  ``observe`` itself returns while the stream is still busy and under torch's
    synchronisation debug mode set to raise."""
    from test_diffaugment_gpu import _step
    inputs = scenario.make_inputs("dc_gan", "tiny")
    bs = len(inputs["real_d0"])
    m = _build("dc_gan", stacked=stacked, diffaugment="color,translation", augment_blit="xflip,rot90", ada_target=0.6,
               ada_interval=3, ada_kimg=0.5)
    aug = m.diffaugment
    m.discriminator.register_forward_hook(lambda mod, args, out: out.abs() + 1.0)
    step = np.float32(bs * 3 / 500.0)
    want, seen = np.float32(0.0), []
    for d_step in range(1, 8):
        _step(m, "dc_gan", 0, inputs)
        m.zero_grad()
        _step(m, "dc_gan", 1, inputs)                      # a generator step: no observation
        m.zero_grad()
        if d_step % 3 == 0:
            want = np.float32(want + step)
        p, r = aug.values()
        assert aug.d_steps == d_step and np.float32(p) == want, (d_step, p, want)
        if d_step >= 3:
            assert r == 1.0
        seen.append(p)
    assert seen[1] == 0.0 and 0.0 < seen[2] == seen[4] < seen[5]

    logits = torch.randn(4096, device="cuda")              # r ~ 0 < target: the update at d_steps 9 takes p down again
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.cuda._sleep(20_000_000)                      # keeps the stream busy for milliseconds
        aug.observe(logits)
        aug.observe(logits)                                # d_steps 9: observe + update
        aug.observe(logits)
        busy = not torch.cuda.current_stream().query()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert busy, "observe() waited for the stream"
    torch.cuda.synchronize()
    state = aug.state(logits.device).cpu()
    assert aug.d_steps == 10 and float(state[1]) == 4096 and float(state[0]) == float(torch.sign(logits).sum())
    # (the step of that update is 4096 * 3 / 500 > 1: p lands on the lower clamp)
    assert float(state[2]) == 0.0 and abs(float(state[3])) < 0.1


# ---------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------
def test_runner_trains_adapts_checkpoints_and_resumes(tmp_path, monkeypatch, capsys):
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.augment import AdaptiveAugment
    monkeypatch.chdir(tmp_path)
    small = ["train.batch_size=4", "train.features_gen=8", "train.features_disc=8", "model.noise_dim=16", "log_every=4",
             "train.ckpt_dir=" + str(tmp_path / "ckpt")]
    args = ["+expt=dc_gan", "dataset=synthetic", "diffaugment=color,translation", "augment_blit=xflip,rot90",
            "ada_target=0.6", "ada_interval=2", "ada_kimg=1", "+max_steps=8"]
    module, trainer, step = R.main(args + small)
    aug = module.diffaugment
    assert step == 8 and type(aug) is AdaptiveAugment and aug.adaptive and aug.blit == 3
    assert all(bool(torch.isfinite(p).all()) for p in module.parameters())
    out = capsys.readouterr().out
    assert "ada_p=" in out and "ada_r=" in out and "train/ada_p" in module.logged and "train/ada_r" in module.logged
    (path,) = glob.glob(os.path.join(str(tmp_path / "ckpt"), "*.ckpt"))
    saved = torch.load(path, map_location="cpu", weights_only=False)["callbacks"]["AdaptiveAugment"]
    print("runner: p = %r after %d discriminator steps" % (saved["p"], saved["d_steps"]))
    assert saved["d_steps"] == aug.d_steps >= 2 and saved["p"] == aug.p_value()
    assert saved["p"] > 0
    # resumed: the module starts from the saved p and step count (max_steps is reached, so nothing moves them)
    module2, _, step2 = R.main(args + small)
    assert step2 == 8 and module2.diffaugment.state_dict() == saved
    # a checkpoint without the entry (a run with the keys at default) starts from the start value and says so
    plain = ["+expt=dc_gan", "dataset=synthetic", "diffaugment=color,translation", "+max_steps=2",
             "train.ckpt_dir=" + str(tmp_path / "plain")] + small[:-1]
    module3, _, _ = R.main(plain)
    (path3,) = glob.glob(os.path.join(str(tmp_path / "plain"), "*.ckpt"))
    assert "AdaptiveAugment" not in torch.load(path3, map_location="cpu", weights_only=False)["callbacks"]
    capsys.readouterr()
    module4, _, _ = R.main(plain + ["ada_target=0.6"])
    assert "holds no AdaptiveAugment state" in capsys.readouterr().out and module4.diffaugment.p_value() == 0.0
    with pytest.raises(SystemExit, match="unbounded"):
        R.main(["+expt=wgan", "diffaugment=color", "ada_target=0.6"] + small)

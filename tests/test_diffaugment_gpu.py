"""gz_diffaug on the device against the fp64 yardstick of diffaugment_support.py: bit-exact on cases made of fp32 numbers
only, within 32 * 2^-24 * S_n on drawn cases, its memory contract (guard words around y, misaligned operands, equal bits
on equal inputs, refusals that leave y alone), the autograd pair to second order, and whole training steps of all five
experiments with the kernel swapped for the yardstick in fp32 torch ops.

Worst |y - y64| / bound measured on an MI355X (each tolerance test prints its own): 0.055 / 0.051 / 0.052 in modes 0 / 1 /
2 over the listed cases, 0.060 over one shape per launch geometry."""
import contextlib
import ctypes

import pytest
import torch

import diffaugment_support as S
import scenario
from mask_pinning import MaskTape, pinned_product_masks

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
GUARD = 12345.678
OK, BAD_SHAPE, UNSUPPORTED = 0, -1, -2


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(x0, x1, params, y, R0, R1, C, H, W, cut, mode):
    from lightning_gan_zoo_amd._lib import lib
    from lightning_gan_zoo_amd.functional._base import _stream
    return lib.gz_diffaug(_ptr(x0), _ptr(x1), _ptr(params), _ptr(y), R0, R1, C, H, W, cut[0], cut[1], mode, _stream())


def _place(t, misaligned):
    """``t`` on the device, starting 4 bytes past a 16-byte boundary when ``misaligned``."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()] if misaligned else buf[:t.numel()]
    view.copy_(t.reshape(-1))
    return view


def run_kernel(x, params, cut, mode, x1=None, y_lead=4, misaligned=False):
    """One launch through the C ABI; y is carved out of a larger buffer filled with a guard word, ``y_lead`` words in
    (4: 16-byte aligned, 1: 4 bytes past a boundary).  Everything outside y must still hold the guard afterwards."""
    R0, C, H, W = x.shape
    R1 = 0 if x1 is None else x1.shape[0]
    n = (R0 + R1) * C * H * W
    buf = torch.full((y_lead + n + 4,), GUARD, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    y = buf[y_lead:y_lead + n]
    rc = _launch(_place(x, misaligned), _place(x1, misaligned), params.cuda().contiguous(), y, R0, R1, C, H, W, cut, mode)
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert bool((buf[:y_lead] == GUARD).all()) and bool((buf[y_lead + n:] == GUARD).all()), "a guard word was written"
    return y.clone().reshape(R0 + R1, C, H, W).cpu()


# ---------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut_on", [True, False])
@pytest.mark.parametrize("rows", list(S.EXACT_ROW_SETS))
@pytest.mark.parametrize("shape", S.EXACT_SHAPES)
def test_exact_cases_agree_bit_for_bit(shape, rows, cut_on):
    """Every intermediate of these cases is an fp32 number (test_diffaugment_cpu.py), so the result does not depend on
    the summation order or on FMA contraction: torch.equal against the fp64 yardstick in all three modes, single
    source and -- at R = 5 -- split 2 + 3 over two sources."""
    x, p = S.exact_case(shape, rows)
    cut = S.cut_size(*shape[1:]) if cut_on else (0, 0)
    misaligned = rows in ("last5", "one_centred")
    for mode in (0, 1, 2):
        want = S.reference(x.double(), p, cut, mode)
        assert torch.equal(want.float().double(), want)
        got = run_kernel(x, p, cut, mode, y_lead=1 if cut_on else 4, misaligned=misaligned)
        assert torch.equal(got.double(), want), (shape, rows, cut, mode, int((got.double() != want).sum()))
        if len(x) == 5:
            two = run_kernel(x[:2], p, cut, mode, x1=x[2:], y_lead=4 if cut_on else 1, misaligned=not misaligned)
            assert torch.equal(two, got), (shape, rows, cut, mode)
    if not cut_on and rows == "first5":         # the identity row under a box of size 0
        assert torch.equal(run_kernel(x, p, cut, 0)[0], x[0])


# ---------------------------------------------------------------------------------------------------------------
# tolerance cases
# ---------------------------------------------------------------------------------------------------------------
def _worst_ratio(x, p, cut, mode, **kw):
    want = S.reference(x.double(), p, cut, mode)
    got = run_kernel(x, p, cut, mode, **kw).double()
    return float(((got - want).abs() / S.bound(x, p, mode)).max())


@pytest.mark.parametrize("R", [1, 6])
@pytest.mark.parametrize("shape", S.TOLERANCE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drawn_cases_within_the_bound(shape, R):
    """|y - y64| <= 32 * 2^-24 * S_n (diffaugment_support.bound) with parameters from the product's own draw."""
    x, p = S.drawn_case(shape, R)
    cut = S.cut_size(*shape[1:])
    for mode in (0, 1, 2):
        ratio = _worst_ratio(x, p, cut, mode, y_lead=4 if R == 6 else 1, misaligned=(R == 1))
        print("diffaugment %s R=%d mode %d: worst |y - y64| / bound = %.4f" % ("x".join(map(str, shape)), R, mode, ratio))
        assert ratio <= 1.0, (shape, R, mode, ratio)


# one shape per (channels, float4 units per lane, lanes) variant the launcher can choose, the largest supported samples
# among them
GEOMETRY_SHAPES = [(1, 256, 256), (2, 128, 256), (4, 128, 128), (3, 128, 170), (1, 128, 128), (2, 64, 64), (1, 64, 100),
                   (3, 64, 96), (3, 64, 128), (4, 5, 9), (2, 7, 6), (1, 4, 4)]


@pytest.mark.parametrize("shape", GEOMETRY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_launch_geometry_within_the_bound(shape):
    x, p = S.drawn_case(shape, 2, seed=1)
    for cut in (S.cut_size(*shape[1:]), (0, 0)):
        for mode in (0, 1, 2):
            ratio = _worst_ratio(x, p, cut, mode)
            print("diffaugment %s mode %d: worst |y - y64| / bound = %.4f" % ("x".join(map(str, shape)), mode, ratio))
            assert ratio <= 1.0, (shape, cut, mode, ratio)


# ---------------------------------------------------------------------------------------------------------------
# memory contract
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("y_lead", [4, 1])
@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 64, 64), (2, 16, 4)], ids=lambda s: "x".join(map(str, s)))
def test_alignment_guards_and_equal_bits(shape, y_lead, misaligned):
    """Any 4-byte alignment of the sources and of y gives the same bits, nothing outside y is written (run_kernel checks
    the guard words on every call of this file), and two launches on equal inputs agree bit for bit."""
    x, p = S.drawn_case(shape, 5, seed=2)
    cut = S.cut_size(*shape[1:])
    for mode in (0, 1, 2):
        base = run_kernel(x, p, cut, mode)
        a = run_kernel(x[:2], p, cut, mode, x1=x[2:], y_lead=y_lead, misaligned=misaligned)
        b = run_kernel(x[:2], p, cut, mode, x1=x[2:], y_lead=y_lead, misaligned=misaligned)
        assert torch.equal(a, b) and torch.equal(a, base), (shape, mode)


def test_refused_calls_return_their_codes_and_leave_y_untouched():
    C, H, W = 3, 8, 8
    x = torch.randn(2, C, H, W, device="cuda")
    x1 = torch.randn(1, C, H, W, device="cuda")
    p = torch.tensor([[0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 3, device="cuda")
    big = torch.zeros(65540, device="cuda")
    y = torch.full((65540,), GUARD, device="cuda")
    cut = (4, 4)
    refused = [
        (UNSUPPORTED, (x, None, p, y, 1, 0, 5, 8, 8, cut, 0)),             # C > 4
        (UNSUPPORTED, (x, None, p, y, 1, 0, 3, 3, 8, cut, 0)),             # H < 4
        (UNSUPPORTED, (x, None, p, y, 1, 0, 3, 8, 3, cut, 0)),             # W < 4
        (UNSUPPORTED, (big, None, p, y, 1, 0, 1, 256, 257, cut, 0)),       # C*H*W > 65536
        (UNSUPPORTED, (big, None, p, y, 1, 0, 4, 128, 129, cut, 0)),
        (BAD_SHAPE, (None, None, p, y, 2, 0, C, H, W, cut, 0)),            # null pointers
        (BAD_SHAPE, (x, None, None, y, 2, 0, C, H, W, cut, 0)),
        (BAD_SHAPE, (x, None, p, None, 2, 0, C, H, W, cut, 0)),
        (BAD_SHAPE, (x, None, p, y, 2, 1, C, H, W, cut, 0)),               # x1 == NULL with R1 != 0
        (BAD_SHAPE, (x, x1, p, y, 0, 0, C, H, W, cut, 0)),                 # R0 + R1 < 1
        (BAD_SHAPE, (x, x1, p, y, -1, 1, C, H, W, cut, 0)),
        (BAD_SHAPE, (x, None, p, y, 2, 0, C, H, W, cut, 3)),               # mode outside 0..2
        (BAD_SHAPE, (x, None, p, y, 2, 0, C, H, W, cut, -1)),
        (BAD_SHAPE, (x, None, p, y, 2, 0, C, H, W, (-1, 4), 0)),
        (BAD_SHAPE, (x, None, p, x, 2, 0, C, H, W, cut, 0)),               # y overlaps a source
        (BAD_SHAPE, (x, None, p, x.reshape(-1)[C * H * W:], 2, 0, C, H, W, cut, 0)),
        (BAD_SHAPE, (x, x1, p, x1, 2, 1, C, H, W, cut, 0)),
    ]
    x_before, x1_before = x.clone(), x1.clone()
    for want, args in refused:
        assert _launch(*args) == want, (want, args[4:])
    torch.cuda.synchronize()
    assert bool((y == GUARD).all()) and torch.equal(x, x_before) and torch.equal(x1, x1_before)
    assert _launch(x, x1, p, y, 2, 1, C, H, W, cut, 0) == OK               # the same operands, accepted


def test_functional_refuses_cpu_tensors_and_bad_params():
    from lightning_gan_zoo_amd import functional as F
    x = torch.zeros(2, 3, 8, 8)
    p = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.diffaugment(x, p, (4, 4))
    with pytest.raises(RuntimeError, match=r"params must be \[2, 8\]"):
        F.diffaugment(x.cuda(), torch.zeros(3, 8).cuda(), (4, 4))
    with pytest.raises(RuntimeError, match="unsupported"):
        F.diffaugment(torch.zeros(2, 5, 8, 8).cuda(), p.cuda(), (4, 4))


# ---------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------
def _second_order(x, p, cut, g, v):
    """(y, d<y, g>/dx, d<that, v>/dg) of the product."""
    from lightning_gan_zoo_amd import functional as F
    xr, gr = x.cuda().requires_grad_(), g.cuda().requires_grad_()
    y = F.diffaugment(xr, p.cuda(), cut)
    (gx,) = torch.autograd.grad((y * gr).sum(), xr, create_graph=True)
    assert gx.requires_grad
    (gg,) = torch.autograd.grad((gx * v.cuda()).sum(), gr)
    return y.detach().cpu(), gx.detach().cpu(), gg.detach().cpu()


@pytest.mark.parametrize("cut_on", [True, False])
def test_autograd_pair_is_exact_on_an_exact_case(cut_on):
    shape = (4, 16, 16)
    x, p = S.exact_case(shape, "first5")
    g, v = S.exact_input(5, *shape, seed=91), S.exact_input(5, *shape, seed=92)
    cut = S.cut_size(16, 16) if cut_on else (0, 0)
    y, gx, gg = _second_order(x, p, cut, g, v)
    assert torch.equal(y.double(), S.forward(x.double(), p, cut))
    assert torch.equal(gx.double(), S.adjoint(g.double(), p, cut))                       # A^T g
    assert torch.equal(gg.double(), S.forward(v.double(), p, cut, affine=False))         # A v


@pytest.mark.parametrize("shape", [(3, 12, 20), (3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_autograd_pair_within_the_bound(shape):
    x, p = S.drawn_case(shape, 6, seed=3)
    gen = torch.Generator().manual_seed(17)
    g, v = torch.randn(x.shape, generator=gen), torch.randn(x.shape, generator=gen)
    cut = S.cut_size(*shape[1:])
    y, gx, gg = _second_order(x, p, cut, g, v)
    for got, src, mode in ((y, x, 0), (gx, g, 2), (gg, v, 1)):
        want = S.reference(src.double(), p, cut, mode)
        ratio = float(((got.double() - want).abs() / S.bound(src, p, mode)).max())
        assert ratio <= 1.0, (shape, mode, ratio)


def test_sources_that_need_no_gradient_get_none():
    from lightning_gan_zoo_amd import functional as F
    shape = (4, 16, 16)
    x, p = S.exact_case(shape, "first5")
    g = S.exact_input(5, *shape, seed=93)
    cut = S.cut_size(16, 16)
    want = S.adjoint(g.double(), p, cut)
    for first in (True, False):
        a, b = x[:2].cuda(), x[2:].cuda()
        (a if first else b).requires_grad_()
        y = F.diffaugment(a, p.cuda(), cut, b)
        y.backward(g.cuda())
        live, dead = (a, b) if first else (b, a)
        assert dead.grad is None
        assert torch.equal(live.grad.cpu().double(), want[:2] if first else want[2:])
    a, b = x[:2].cuda().requires_grad_(), x[2:].cuda().requires_grad_()
    F.diffaugment(a, p.cuda(), cut, b).backward(g.cuda())                  # both: one adjoint launch over all rows
    assert torch.equal(torch.cat([a.grad, b.grad]).cpu().double(), want)
    params = p.cuda().requires_grad_()
    F.diffaugment(x.cuda().requires_grad_(), params, cut).sum().backward()
    assert params.grad is None


# ---------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------
class RecordingTape(MaskTape):
    """A MaskTape that takes every decision as the data has it and writes it down."""

    def __init__(self):
        super().__init__()
        self.rec = {}

    def _apply(self, pos, x, slope):
        assert pos not in self.rec
        mask = x.detach() > 0
        self.rec[pos] = mask.cpu()
        return torch.where(mask, x, x * slope)

    def finish(self):
        tape = MaskTape()
        tape.masks = [self.rec[i] for i in range(len(self.rec))]
        return tape


@contextlib.contextmanager
def decisions(tape):
    """Every ReLU / LeakyReLU of both networks decided by ``tape`` (mask_pinning.pinned_product_masks, plus the R1
    ResNet's stand-alone pre-activation): the two runs of a step take the same decisions, or the tape counts where the
    data alone would have decided otherwise."""
    from lightning_gan_zoo_amd import functional as F
    plain = F.activation

    def activation(x, act=F.ACT_LRELU, slope=0.2):
        if act not in (F.ACT_RELU, F.ACT_LRELU):
            return plain(x, act, slope)
        return tape.replay(x, float(slope) if act == F.ACT_LRELU else 0.0)

    F.activation = activation
    try:
        with pinned_product_masks(tape):
            yield tape
    finally:
        F.activation = plain


def _build(expt, policy, stacked=True):
    from lightning_gan_zoo_amd.config import locate, make_cfg
    cfg = make_cfg(expt, **scenario.cfg_kwargs(expt, "tiny"))
    if policy is not None:
        cfg["diffaugment"] = policy
    torch.manual_seed(42)
    m = locate(cfg.model.lm["_target_"])(cfg, None)
    scenario._prepare(m, False)
    m.to("cuda")
    m.stack_d_passes = stacked
    return m


def _step(m, expt, idx, inputs):
    from helpers import FixedNoise
    from lightning_gan_zoo_amd.harness import toggle_optimizer
    tag = "d" if idx == 0 else "g"
    toggle_optimizer(m, idx)
    m.noise_distn = FixedNoise(inputs[f"z_{tag}0"])
    if expt == "wgan_gp":
        m.gp_alpha = inputs["alpha0"]
    scenario.seed_views(m, 7001 + idx)
    real = inputs[f"real_{tag}0"].detach().clone().cuda()
    labels = torch.zeros(len(real), dtype=torch.int64, device="cuda")
    loss = m.training_step((real, labels), idx, idx)
    loss.backward()
    net = m.discriminator if idx == 0 else m.generator
    grads = {n: p.grad.detach().double().cpu() for n, p in net.named_parameters() if p.grad is not None}
    assert grads
    return float(loss.detach()), grads


def _pinned_params(inputs, seed=5):
    real = inputs["real_d0"]
    return S.drawn_case(tuple(real.shape[1:]), 2 * len(real), seed=seed)[1]


def _compare(a, b, scale, what):
    """(loss, gradients) of two runs at the whole-step bar, taken as in test_default_path_gpu.py: scalars relative to
    max(|reference|, logit scale), gradients in full relative L2."""
    from test_parity_gpu import TOL
    (la, ga), (lb, gb) = a, b
    assert set(ga) == set(gb)
    worst = [(abs(la - lb) / max(abs(lb), scale), "loss")]
    worst += [(float((ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-30)), k) for k in gb
              if float(gb[k].abs().max()) > 0 or float(ga[k].abs().max()) > 0]
    worst.sort(reverse=True)
    print("%s: worst of %d: %s" % (what, len(worst), [(k, "%.1e" % e) for e, k in worst[:3]]))
    assert worst[0][0] <= TOL, (what, worst[:4])


@pytest.mark.parametrize("idx", [0, 1])
@pytest.mark.parametrize("expt", ["dc_gan", "wgan", "wgan_gp", "gan_stability_r1", "hologan"])
def test_whole_step_kernel_against_torch_ops(expt, idx):
    """One training step at the tiny scenario size with pinned augmentation parameters: once through gz_diffaug, once
    with ``self.diffaugment`` swapped for the yardstick in fp32 torch ops on the device (plain autograd: for
    gan_stability_r1 and wgan_gp this is the second-order path).  The kernel run writes down every ReLU / LeakyReLU
    decision; the torch run takes the same ones, and the pre-activations whose sign it alone would have decided
    differently are counted and capped as in test_default_path_gpu.py.  Loss and every gradient at 1e-3."""
    from test_oracle_golden import pinned_scale
    inputs = scenario.make_inputs(expt, "tiny")
    params = _pinned_params(inputs)

    m = _build(expt, FULL)
    m.diffaugment.params = params
    rec = RecordingTape()
    with decisions(rec):
        kernel = _step(m, expt, idx, inputs)
    tape = rec.finish()

    m = _build(expt, FULL)
    m.diffaugment = S.TorchDiffAugment(params.cuda(), True)
    with decisions(tape):
        torch_ops = _step(m, expt, idx, inputs)
    assert m.diffaugment.calls >= 1
    assert tape.cursor == len(tape.masks), "the two runs took different numbers of activation decisions"
    total = sum(t.numel() for t in tape.masks)
    flips = sum(t[1] for t in tape.mismatches)
    print("%s step %d: %d of %d pre-activations change sign between the kernel and the torch ops (largest %.1e)"
          % (expt, idx, flips, total, max([t[3] for t in tape.mismatches], default=0.0)))
    assert flips <= max(4, 1e-4 * total) and all(t[3] <= 3e-4 for t in tape.mismatches), tape.mismatches
    _compare(kernel, torch_ops, pinned_scale(expt, "tiny"), "%s step %d kernel vs torch ops" % (expt, idx))


class _PerCall:
    """Pins the parameters of consecutive augmentation calls: call k gets ``blocks[k]``."""

    def __init__(self, aug, blocks):
        self.aug, self.blocks = aug, list(blocks)

    def __call__(self, x, x1=None):
        self.aug.params = self.blocks.pop(0)
        return self.aug(x, x1)


@pytest.mark.parametrize("expt", ["dc_gan", "wgan"])
def test_stacked_two_source_launch_against_two_calls(expt):
    """The BatchNorm critics: the stacked discriminator step (ONE two-source launch, real's parameter rows first, two
    statistics groups) against the two-call form (aug(real) and aug(fake) launched separately with the same rows, each
    call its own batch statistics).  The augmented batches agree bit for bit, so the steps agree as the un-augmented
    stacked and two-call steps do (test_stacked_d_gpu.py)."""
    from test_oracle_golden import pinned_scale
    inputs = scenario.make_inputs(expt, "tiny")
    params = _pinned_params(inputs)
    bs = len(inputs["real_d0"])
    runs = {}
    for stacked in (True, False):
        m = _build(expt, FULL, stacked=stacked)
        m.real_first = False
        m.diffaugment = _PerCall(m.diffaugment, [params] if stacked else [params[:bs], params[bs:]])
        runs[stacked] = _step(m, expt, 0, inputs)
        assert not m.diffaugment.blocks
    _compare(runs[True], runs[False], pinned_scale(expt, "tiny"), "%s stacked vs two calls" % expt)


@pytest.mark.parametrize("idx", [0, 1])
@pytest.mark.parametrize("expt", ["dc_gan", "wgan", "wgan_gp", "gan_stability_r1", "hologan"])
def test_empty_policy_is_the_step_without_the_key(expt, idx, monkeypatch):
    from lightning_gan_zoo_amd import augment
    inputs = scenario.make_inputs(expt, "tiny")

    def no_draw(self, *a):
        raise AssertionError("a draw was made with the policy off")
    monkeypatch.setattr(augment.DiffAugment, "draw", no_draw)
    runs = []
    for policy in (None, ""):
        m = _build(expt, policy)
        assert m.diffaugment is None
        state = torch.get_rng_state()
        runs.append(_step(m, expt, idx, inputs) + (torch.get_rng_state(),))
        torch.set_rng_state(state)
    (la, ga, ra), (lb, gb, rb) = runs
    assert la == lb and set(ga) == set(gb) and torch.equal(ra, rb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_each_call_draws_its_own_parameters_at_call_time():
    """dc_gan, two-call discriminator step: two draws of [bs, 8] in call order (real, then fake), after the noise; the
    stacked step: one draw of [2 bs, 8]."""
    from lightning_gan_zoo_amd import augment
    inputs = scenario.make_inputs("dc_gan", "tiny")
    bs = len(inputs["real_d0"])
    for stacked, want in ((True, [2 * bs]), (False, [bs, bs])):
        m = _build("dc_gan", FULL, stacked=stacked)
        seen = []
        plain = m.diffaugment.draw

        def draw(R, H, W, plain=plain, seen=seen):
            seen.append(R)
            return plain(R, H, W)
        m.diffaugment.draw = draw
        torch.manual_seed(3)
        _step(m, "dc_gan", 0, inputs)
        assert seen == want, (stacked, seen)
        first = torch.get_rng_state()
        torch.manual_seed(3)
        for R in want:
            plain(R, 64, 64)
        assert torch.equal(torch.get_rng_state(), first)


def test_runner_trains_with_the_policy_and_refuses_a_bad_one(tmp_path, monkeypatch):
    """``run_network +expt=dc_gan diffaugment=color,translation,cutout`` trains: four steps through harness.Trainer with
    drawn parameters, finite losses, the module built from the runner key; the same seed gives the same weights."""
    from lightning_gan_zoo_amd import run_network as R
    from lightning_gan_zoo_amd.augment import GROUPS
    monkeypatch.chdir(tmp_path)
    small = ["+expt=dc_gan", "dataset=synthetic", "train.batch_size=4", "train.features_gen=8", "train.features_disc=8",
             "model.noise_dim=16", "log_every=1000", "+max_steps=4"]
    weights = []
    for run in ("a", "b"):
        module, trainer, step = R.main(small + ["train.ckpt_dir=" + str(tmp_path / run), "diffaugment=" + FULL])
        assert step == 4 and module.diffaugment is not None and module.diffaugment.groups == GROUPS
        assert all(bool(torch.isfinite(p).all()) for p in module.parameters())
        weights.append([p.detach().clone() for p in module.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*weights))
    module, trainer, step = R.main(small + ["train.ckpt_dir=" + str(tmp_path / "off")])
    assert module.diffaugment is None
    assert not all(torch.equal(a, b) for a, b in zip(weights[0], module.parameters()))
    with pytest.raises(SystemExit, match="color, translation, cutout"):
        R.main(small + ["diffaugment=colour"])

"""DiffAugment without a GPU: the yardstick's own algebra (autograd gradient == closed-form adjoint, <A x, g> ==
<x, A^T g>, exact cases made of fp32 numbers only), the host draw (determinism, ranges, column order, no generator state
for absent groups), policy parsing, the runner key on its way into the module's cfg, and GraphedTrainer's refusal."""
import pytest
import torch

import diffaugment_support as S
from lightning_gan_zoo_amd import run_network as R
from lightning_gan_zoo_amd.augment import GROUPS, DiffAugment, parse_policy
from lightning_gan_zoo_amd.config import locate, make_cfg

FULL = "color,translation,cutout"


def _cases():
    for shape in S.EXACT_SHAPES:
        for rows in S.EXACT_ROW_SETS:
            x, p = S.exact_case(shape, rows)
            yield x.double(), p, S.cut_size(*shape[1:])
    for shape in S.TOLERANCE_SHAPES[:3]:
        x, p = S.drawn_case(shape, 6)
        yield x.double(), p, S.cut_size(*shape[1:])
        yield x.double(), p, (0, 0)


def test_yardstick_autograd_gradient_is_the_closed_form_adjoint():
    for x, p, cut in _cases():
        g = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        xr = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad((S.forward(xr, p, cut) * g).sum(), xr)
        want = S.adjoint(g, p, cut)
        assert float((gx - want).abs().max()) <= 1e-13 * float(g.abs().max()), (x.shape, cut)


def test_yardstick_adjoint_identity_in_fp64():
    for x, p, cut in _cases():
        g = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
        lhs = (S.forward(x, p, cut, affine=False) * g).sum()
        rhs = (x * S.adjoint(g, p, cut)).sum()
        scale = float(x.abs().max() * g.abs().max()) * x.numel()
        assert abs(float(lhs - rhs)) <= 1e-14 * scale, (x.shape, cut, float(lhs), float(rhs))
        # the affine part comes from b alone: A x + k - A x does not depend on x
        k = S.forward(x, p, cut) - S.forward(x, p, cut, affine=False)
        k0 = S.forward(torch.zeros_like(x), p, cut)
        assert float((k - k0).abs().max()) <= 1e-13


@pytest.mark.parametrize("rows", list(S.EXACT_ROW_SETS))
@pytest.mark.parametrize("shape", S.EXACT_SHAPES)
def test_exact_cases_hold_only_fp32_numbers(shape, rows):
    x, p = S.exact_case(shape, rows)
    C, H, W = shape
    assert (C * H * W) & (C * H * W - 1) == 0 and C * H * W <= 1024
    assert torch.equal(x * 8, (x * 8).round()) and float(x.abs().max()) <= 2
    assert torch.equal(p[:, 0] * 8, (p[:, 0] * 8).round())
    assert set(p[:, 1].tolist()) <= {0.0, 0.5, 1.0, 1.5} and set(p[:, 2].tolist()) <= {0.5, 0.75, 1.0, 1.25}
    for cut in (S.cut_size(H, W), (0, 0)):
        for mode in (0, 1, 2):
            trace = []
            if mode == 2:
                S.adjoint(x.double(), p, cut, trace)
            else:
                S.forward(x.double(), p, cut, affine=(mode == 0), trace=trace)
            assert len(trace) >= 10
            for v in trace:
                assert torch.equal(v.float().double(), v), (shape, rows, cut, mode)


def test_exact_rows_cover_the_extremes():
    H, W = 16, 16
    rows = S.exact_rows(H, W)
    sh, sw = S.shift_size(H, W)
    ch, cw = S.cut_size(H, W)
    assert {(int(r[3]), int(r[4])) for r in rows} >= {(sh, sw), (-sh, -sw), (sh, -sw), (-sh, sw), (0, 0)}
    corners = {(int(r[5]) + ch // 2, int(r[6]) + cw // 2) for r in rows}         # (oh, ow)
    assert corners >= {(0, 0), (0, W), (H, 0), (H, W), (H // 2, W // 2)}
    assert any(float(r[1]) == 0.0 for r in rows)
    assert any(tuple(r[:5].tolist()) == (0.0, 1.0, 1.0, 0.0, 0.0) for r in rows)


def test_draw_is_deterministic_and_in_range_in_the_stated_column_order():
    aug = DiffAugment(FULL)
    for H, W in ((64, 64), (5, 7), (12, 20), (128, 128)):
        torch.manual_seed(11)
        a = aug.draw(4096, H, W)
        torch.manual_seed(11)
        b = aug.draw(4096, H, W)
        assert a.dtype == torch.float32 and a.shape == (4096, 8) and torch.equal(a, b)
        sh, sw = int(H / 8 + 0.5), int(W / 8 + 0.5)
        ch, cw = int(H / 2 + 0.5), int(W / 2 + 0.5)
        assert aug.cut(H, W) == (ch, cw)
        lo = [-0.5, 0.0, 0.5, -sh, -sw, -(ch // 2), -(cw // 2), 0]
        hi = [0.5, 2.0, 1.5, sh, sw, H - ch % 2 - ch // 2, W - cw % 2 - cw // 2, 0]
        for col in range(8):
            assert float(a[:, col].min()) >= lo[col] and float(a[:, col].max()) <= hi[col], (H, W, col)
        for col in range(3, 8):
            assert torch.equal(a[:, col], a[:, col].round())
            if col < 7:                       # 4096 draws reach both ends of every integer range
                assert float(a[:, col].min()) == lo[col] and float(a[:, col].max()) == hi[col], (H, W, col)
        # the order of the draws: seven draws of R values each, columns 0..6
        torch.manual_seed(11)
        want = [torch.rand(4096) - 0.5, 2 * torch.rand(4096), torch.rand(4096) + 0.5,
                torch.randint(-sh, sh + 1, (4096,)).float(), torch.randint(-sw, sw + 1, (4096,)).float(),
                (torch.randint(0, H + (1 - ch % 2), (4096,)) - ch // 2).float(),
                (torch.randint(0, W + (1 - cw % 2), (4096,)) - cw // 2).float()]
        for col, w in enumerate(want):
            assert torch.equal(a[:, col], w), (H, W, col)


def test_absent_groups_store_their_identity_and_consume_no_generator_state():
    identity = torch.tensor([0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    cols = {"color": [0, 1, 2], "translation": [3, 4], "cutout": [5, 6]}
    for policy in ("color", "translation", "cutout", "color,cutout", "translation,cutout"):
        aug = DiffAugment(policy)
        torch.manual_seed(5)
        p = aug.draw(64, 16, 16)
        after = torch.get_rng_state()
        absent = [g for g in GROUPS if g not in aug.groups]
        for g in absent:
            assert torch.equal(p[:, cols[g]], identity[cols[g]].expand(64, -1)), (policy, g)
        assert aug.cut(16, 16) == ((8, 8) if "cutout" in aug.groups else (0, 0))
        # the present groups alone, drawn by hand in the stated order, leave the generator in the same state
        torch.manual_seed(5)
        if "color" in aug.groups:
            torch.rand(64), torch.rand(64), torch.rand(64)
        if "translation" in aug.groups:
            torch.randint(-2, 3, (64,)), torch.randint(-2, 3, (64,))
        if "cutout" in aug.groups:
            torch.randint(0, 17, (64,)), torch.randint(0, 17, (64,))
        assert torch.equal(torch.get_rng_state(), after), policy
    torch.manual_seed(5)
    before = torch.get_rng_state()
    assert torch.equal(DiffAugment("").draw(4, 8, 8), identity.expand(4, -1))
    assert torch.equal(torch.get_rng_state(), before)


def test_policy_parsing_and_its_error_message():
    assert parse_policy("") == () and parse_policy(None) == () and parse_policy(" ") == ()
    assert parse_policy(FULL) == GROUPS
    assert parse_policy("cutout, color") == ("color", "cutout")
    assert not DiffAugment("") and DiffAugment("translation")
    with pytest.raises(ValueError) as e:
        parse_policy("color,flip")
    assert "'flip'" in str(e.value) and "color, translation, cutout" in str(e.value)


def test_runner_key_default_and_its_way_into_the_cfg():
    assert R.RUNNER_KEYS["diffaugment"] == ""
    conf_dir, expt, rest, run = R.parse_overrides(["+expt=dc_gan"])
    assert run["diffaugment"] == "" and R.compose(conf_dir, expt, rest, run).get("diffaugment", None) == ""
    conf_dir, expt, rest, run = R.parse_overrides(["+expt=dc_gan", "diffaugment=cutout,color"])
    assert rest == ["+expt=dc_gan"]
    cfg = R.compose(conf_dir, expt, rest, run)
    assert cfg.get("diffaugment") == "color,cutout"
    module = locate(cfg.model.lm["_target_"])(cfg, None)
    assert module.diffaugment is not None and module.diffaugment.groups == ("color", "cutout")
    with pytest.raises(SystemExit) as e:
        R.parse_overrides(["+expt=dc_gan", "diffaugment=color,rotate"])
    assert "'rotate'" in str(e.value) and "color, translation, cutout" in str(e.value)


@pytest.mark.parametrize("expt", ["dc_gan", "wgan", "wgan_gp", "gan_stability_r1", "hologan"])
def test_modules_build_the_augmentation_from_their_cfg(expt):
    cfg = make_cfg(expt)
    assert locate(cfg.model.lm["_target_"])(cfg, None).diffaugment is None
    cfg = make_cfg(expt)
    cfg["diffaugment"] = FULL
    m = locate(cfg.model.lm["_target_"])(cfg, None)
    assert isinstance(m.diffaugment, DiffAugment) and m.diffaugment.groups == GROUPS
    cfg = make_cfg(expt)
    cfg["diffaugment"] = "colour"
    with pytest.raises(ValueError, match="color, translation, cutout"):
        locate(cfg.model.lm["_target_"])(cfg, None)


def test_augmentation_refuses_cpu_tensors():
    aug = DiffAugment(FULL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug(torch.zeros(2, 3, 8, 8))


def test_graphed_trainer_refuses_a_module_that_augments():
    from lightning_gan_zoo_amd.harness import GraphedTrainer
    cfg = make_cfg("dc_gan", batch_size=4, features=8, noise_dim=8)
    cfg["diffaugment"] = "color"
    module = locate(cfg.model.lm["_target_"])(cfg, None)
    with pytest.raises(RuntimeError, match="diffaugment"):
        GraphedTrainer(module)

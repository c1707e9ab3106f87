"""Adaptive discriminator augmentation without a GPU: the new entry points and their prototypes, the null-pointer
refusals (which return before any HIP call), parse_blit and the runner keys with every SystemExit, the unchanged default
path (DiffAugment itself, the same generator state), AdaptiveAugment's draw order and column layout, the yardstick's
adjoint identity over all 8 orientations with mixed gates, and the controller model's clamps."""
import ctypes

import numpy as np
import pytest
import torch

import ada_support as A
import diffaugment_support as S
from lightning_gan_zoo_amd import run_network as R
from lightning_gan_zoo_amd.augment import (BLIT_GROUPS, GROUPS, AdaptiveAugment, DiffAugment, build_augment, parse_blit)
from lightning_gan_zoo_amd.config import locate, make_cfg

FULL = "color,translation,cutout"
BAD_SHAPE = -1


def test_entry_points_are_declared_built_and_refuse_null_pointers():
    from lightning_gan_zoo_amd import build
    from lightning_gan_zoo_amd._lib import lib, parse_header
    assert "gz_ada.hip" in build.SOURCES and "gz_diffaug.hip" in build.SOURCES
    protos = parse_header()
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["gz_diffaug_gated"] == (i, [vp] * 5 + [i] * 9 + [vp])
    assert protos["gz_ada_observe"] == (i, [vp, i, vp, vp])
    assert protos["gz_ada_update"] == (i, [vp, f, f, vp])
    one = ctypes.c_void_p(16)                 # never dereferenced: every call below is refused on its arguments
    assert lib.gz_diffaug_gated(None, None, one, None, one, 1, 0, 3, 8, 8, 4, 4, 3, 0, None) == BAD_SHAPE
    assert lib.gz_diffaug_gated(one, None, None, None, one, 1, 0, 3, 8, 8, 4, 4, 3, 0, None) == BAD_SHAPE
    assert lib.gz_diffaug_gated(one, None, one, None, None, 1, 0, 3, 8, 8, 4, 4, 3, 0, None) == BAD_SHAPE
    assert lib.gz_diffaug_gated(one, None, one, None, one, 1, 1, 3, 8, 8, 4, 4, 3, 0, None) == BAD_SHAPE      # x1 null
    assert lib.gz_diffaug_gated(one, None, one, None, ctypes.c_void_p(1 << 20), 1, 0, 3, 8, 8, 4, 4, 4, 0, None) \
        == BAD_SHAPE                                                                                          # blit
    assert lib.gz_ada_observe(None, 4, one, None) == BAD_SHAPE
    assert lib.gz_ada_observe(one, 4, None, None) == BAD_SHAPE
    assert lib.gz_ada_observe(one, 0, one, None) == BAD_SHAPE
    assert lib.gz_ada_update(None, 0.6, 0.1, None) == BAD_SHAPE
    for step in (-0.1, float("nan"), float("inf")):
        assert lib.gz_ada_update(one, 0.6, step, None) == BAD_SHAPE


def test_parse_blit_and_its_error_message():
    assert BLIT_GROUPS == ("xflip", "rot90")
    assert parse_blit("") == () and parse_blit(None) == () and parse_blit(" ") == ()
    assert parse_blit("rot90, xflip") == BLIT_GROUPS and parse_blit("rot90") == ("rot90",)
    with pytest.raises(ValueError) as e:
        parse_blit("xflip,yflip")
    assert "'yflip'" in str(e.value) and "xflip, rot90" in str(e.value)


def test_runner_keys_defaults_ranges_and_every_exit():
    for key, want in (("augment_blit", ""), ("augment_p", None), ("ada_target", None), ("ada_interval", 4),
                      ("ada_kimg", 500)):
        assert R.RUNNER_KEYS[key] == want
    conf_dir, expt, rest, run = R.parse_overrides(["+expt=dc_gan", "diffaugment=color", "augment_blit=rot90,xflip",
                                                   "ada_target=0.6", "ada_interval=2", "ada_kimg=1"])
    assert rest == ["+expt=dc_gan"] and run["augment_blit"] == "xflip,rot90"
    cfg = R.compose(conf_dir, expt, rest, run)
    assert (cfg.get("augment_blit"), cfg.get("augment_p"), cfg.get("ada_target"), cfg.get("ada_interval"),
            cfg.get("ada_kimg")) == ("xflip,rot90", None, 0.6, 2, 1)
    aug = locate(cfg.model.lm["_target_"])(cfg, None).diffaugment
    assert type(aug) is AdaptiveAugment and aug.adaptive and aug.blit == 3 and aug.groups == ("color",)
    assert (aug.target, aug.interval, aug.kimg, aug.p_start, aug.p_value()) == (0.6, 2, 1.0, 0.0, 0.0)

    def exits(args, *needles):
        with pytest.raises(SystemExit) as e:
            R.parse_overrides(["+expt=dc_gan"] + args)
        for needle in needles:
            assert needle in str(e.value), (args, str(e.value))

    exits(["augment_blit=flip"], "'flip'", "xflip, rot90")
    exits(["diffaugment=color", "augment_p=1.5"], "augment_p", "[0, 1]")
    exits(["diffaugment=color", "augment_p=-0.1"], "augment_p")
    exits(["diffaugment=color", "ada_target=1.0"], "ada_target", "(0, 1)")
    exits(["diffaugment=color", "ada_target=0"], "ada_target")
    exits(["diffaugment=color", "ada_interval=0"], "ada_interval")
    exits(["diffaugment=color", "ada_kimg=0"], "ada_kimg")
    for key in ("augment_p=0.5", "ada_target=0.6", "ada_interval=2", "ada_kimg=100"):
        exits([key], key.split("=")[0], "diffaugment and augment_blit are both empty")
    for expt in ("wgan", "wgan_gp"):
        with pytest.raises(SystemExit) as e:
            R.parse_overrides(["+expt=" + expt, "diffaugment=color", "ada_target=0.6"])
        assert "unbounded" in str(e.value) and "sign" in str(e.value) and expt in str(e.value)
        run = R.parse_overrides(["+expt=" + expt, "augment_blit=xflip", "augment_p=0.5"])[3]       # a fixed p: served
        assert run["augment_p"] == 0.5
    for expt in ("dc_gan", "gan_stability_r1", "hologan"):
        assert R.parse_overrides(["+expt=" + expt, "augment_blit=xflip", "ada_target=0.6"])[3]["ada_target"] == 0.6


@pytest.mark.parametrize("expt", ["dc_gan", "wgan", "wgan_gp", "gan_stability_r1", "hologan"])
def test_default_keys_build_diffaugment_itself_with_the_same_draws(expt):
    conf_dir, name, rest, run = R.parse_overrides(["+expt=" + expt, "diffaugment=" + FULL])
    module = locate(R.compose(conf_dir, name, rest, run).model.lm["_target_"])(R.compose(conf_dir, name, rest, run), None)
    assert type(module.diffaugment) is DiffAugment
    torch.manual_seed(9)
    got = module.diffaugment.draw(6, 64, 64)
    after = torch.get_rng_state()
    torch.manual_seed(9)
    want = DiffAugment(FULL).draw(6, 64, 64)
    assert got.shape == (6, 8) and torch.equal(got, want) and torch.equal(torch.get_rng_state(), after)
    cfg = make_cfg(expt)
    assert locate(cfg.model.lm["_target_"])(cfg, None).diffaugment is None
    assert type(build_augment({"diffaugment": "color"})) is DiffAugment
    assert type(build_augment({"diffaugment": "", "augment_blit": "xflip"})) is AdaptiveAugment
    assert type(build_augment({"diffaugment": "color", "augment_p": 0.5})) is AdaptiveAugment


def test_adaptive_draw_order_and_column_layout():
    Rn, H, W = 512, 64, 64
    aug = AdaptiveAugment(FULL, "xflip,rot90", target=0.6)
    torch.manual_seed(21)
    got = aug.draw(Rn, H, W)
    after = torch.get_rng_state()
    torch.manual_seed(21)
    base = DiffAugment(FULL).draw(Rn, H, W)
    f = torch.randint(0, 2, (Rn,))
    k = torch.randint(0, 4, (Rn,))
    u = torch.rand((Rn, 5))
    assert torch.equal(torch.get_rng_state(), after)
    assert got.dtype == torch.float32 and got.shape == (Rn, 16)
    assert torch.equal(got[:, :7], base[:, :7]) and torch.equal(got[:, 7], (k + 4 * f).float())
    assert torch.equal(got[:, 8:13], u) and not bool(got[:, 13:].any())
    assert set(got[:, 7].tolist()) == set(range(8)) and float(u.min()) >= 0 and float(u.max()) < 1
    # absent groups and an absent probability make no draw
    for blit, p, target in (("xflip", None, None), ("rot90", None, None), ("", 0.5, None), ("rot90", 0.25, None)):
        aug = AdaptiveAugment("color", blit, p=p, target=target)
        torch.manual_seed(22)
        got = aug.draw(Rn, H, W)
        after = torch.get_rng_state()
        torch.manual_seed(22)
        torch.rand(Rn), torch.rand(Rn), torch.rand(Rn)
        code = torch.zeros(Rn)
        if "xflip" in blit:
            code += 4 * torch.randint(0, 2, (Rn,))
        if "rot90" in blit:
            code += torch.randint(0, 4, (Rn,))
        u = torch.rand((Rn, 5)) if p is not None else torch.zeros((Rn, 5))
        assert torch.equal(torch.get_rng_state(), after), (blit, p)
        assert torch.equal(got[:, 7], code) and torch.equal(got[:, 8:13], u)
        assert aug.p_start == (1.0 if p is None else p) and aug.gated == (p is not None)
    assert AdaptiveAugment("", "xflip") and not AdaptiveAugment("", "")
    assert AdaptiveAugment("color", target=0.6).p_start == 0.0 and AdaptiveAugment("color", p=0.3, target=0.6).p_start == 0.3


def test_rot90_on_a_non_square_image_is_refused_from_python():
    aug = AdaptiveAugment("color", "rot90")
    with pytest.raises(RuntimeError, match="square"):
        aug(torch.zeros(2, 3, 8, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AdaptiveAugment("color", "xflip")(torch.zeros(2, 3, 8, 12))


def test_observe_is_a_no_op_without_a_target_and_the_state_round_trips():
    aug = AdaptiveAugment("color", "xflip", p=0.25)
    aug.observe(torch.ones(4))                # CPU logits: would raise if anything were launched
    assert aug.d_steps == 0 and not aug.adaptive
    a = AdaptiveAugment("color", target=0.6)
    a.load_state_dict({"p": 0.375, "d_steps": 12})
    assert a.state_dict() == {"p": 0.375, "d_steps": 12} and a.p_value() == 0.375
    with pytest.raises(ValueError):
        a.load_state_dict({"p": 1.5})


def test_graphed_trainer_refuses_the_subclass_too():
    from lightning_gan_zoo_amd.harness import GraphedTrainer
    cfg = make_cfg("dc_gan", batch_size=4, features=8, noise_dim=8)
    cfg["diffaugment"], cfg["augment_blit"] = "color", "xflip"
    module = locate(cfg.model.lm["_target_"])(cfg, None)
    assert type(module.diffaugment) is AdaptiveAugment
    with pytest.raises(RuntimeError, match="diffaugment"):
        GraphedTrainer(module)


@pytest.mark.parametrize("shape", [(3, 6, 6), (1, 9, 9), (4, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_yardstick_adjoint_identity_for_all_orientations_with_mixed_gates(shape):
    """<A' x, g> = <x, A'^T g> to 1e-12 (relative to |x| |g| L), and the autograd gradient of the forward is the closed
    form, with every orientation code and gate uniforms on both sides of p."""
    C, H, W = shape
    x, p8 = S.drawn_case(shape, 8, seed=4)
    params = A.widen(p8, codes=list(range(8)), uniforms=A.mixed_uniforms(8, 5))
    cut = S.cut_size(H, W)
    gen = torch.Generator().manual_seed(6)
    g = torch.randn(x.shape, dtype=torch.float64, generator=gen)
    x = x.double()
    for p, blit in ((0.5, 3), (None, 3), (0.5, 1), (0.5, 2), (0.0, 3), (1.0, 0)):
        on = A.gates(params, p)
        if p == 0.5:
            assert bool(on.any()) and not bool(on.all())
        lhs = (A.reference(x, params, cut, p, blit, 1) * g).sum()
        rhs = (x * A.reference(g, params, cut, p, blit, 2)).sum()
        scale = float(x.abs().max() * g.abs().max()) * x.numel()
        assert abs(float(lhs - rhs)) <= 1e-12 * scale, (shape, p, blit, float(lhs), float(rhs))
        xr = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad((A.reference(xr, params, cut, p, blit, 0) * g).sum(), xr)
        assert float((gx - A.reference(g, params, cut, p, blit, 2)).abs().max()) <= 1e-12 * float(g.abs().max())
    assert torch.equal(A.reference(x, params, cut, 0.0, 3, 0), x)              # p = 0: the identity, bit for bit
    # Q is what torch says it is: code 5 = one turn of the flipped image
    f, k = A.orientation(params, A.gates(params, None), 3)
    assert (f, k) == ([0, 0, 0, 0, 1, 1, 1, 1], [0, 1, 2, 3, 0, 1, 2, 3])
    ident = A.widen(torch.tensor([[0.0, 1.0, 1.0, 0, 0, 0, 0, 0]] * 8), codes=list(range(8)))
    y = A.reference(x, ident, (0, 0), None, 3, 1)
    assert float((y[5] - torch.rot90(x[5].flip(2), 1, dims=[1, 2])).abs().max()) <= 1e-15


def test_controller_model_saturates_and_ignores_an_empty_interval():
    m = A.ControllerModel(p=0.0)
    m.update(0.6, 0.3)                                     # count = 0: nothing changes
    assert m.state.tolist() == [0.0, 0.0, 0.0, 0.0]
    m.observe([-1.0, -2.0, 0.0, float("nan"), -0.0])       # r = -2/5 < target: p would go negative, clamps at 0
    assert m.state[:2].tolist() == [-2.0, 5.0]
    m.update(0.6, 0.3)
    assert m.state[2] == 0.0 and m.state[3] == np.float32(-2.0) / np.float32(5.0) and m.state[:2].tolist() == [0.0, 0.0]
    want, seen = np.float32(0.0), []
    for _ in range(5):
        m.observe([3.0, float("inf"), 1.0])
        m.update(0.6, 0.3)
        want = min(np.float32(want + np.float32(0.3)), np.float32(1.0))
        assert m.state[2] == want and m.state[3] == 1.0
        seen.append(float(m.state[2]))
    assert seen[0] < seen[1] < seen[2] < seen[3] == seen[4] == 1.0
    before = m.state.copy()
    m.update(0.6, 0.3)
    assert np.array_equal(m.state, before)
    m.observe([1.0, -1.0])                                 # r = 0 < 0.6: down again
    m.update(0.6, 0.3)
    assert m.state[2] == np.float32(np.float32(1.0) - np.float32(0.3))
    m.observe([1.0, 1.0, 1.0, 1.0, -1.0])                  # r = 0.6 in fp32 against the fp32 target: no move
    m.update(0.6, 0.3)
    assert m.state[2] == np.float32(np.float32(1.0) - np.float32(0.3))

"""CPU-side checks of the PatchGAN discriminator and the tokenizer's loss: the float64 restatement (tests/patchgan_ref.py) against the
fixture captured from the reference's own modules (tests/golden/patchgan_ref.npz), the condition on that fixture, the holders'
state_dicts, the aliases, MSFPNVQModel's opt-in, the refusals, the folding of the two norm kinds, and the five launchers of
include/frido_patchgan.h as far as they go without a device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as L
import patchgan_ref as R
from frido_amd import _lib
from golden_cfg import VQ_SMALL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(REPO, "tests", "golden", "patchgan_ref.npz"))
DUMMY = dict(target="taming.modules.losses.DummyLoss")
LOSSCFG = dict(target="taming.modules.losses.vqperceptual.VQLPIPSWithDiscriminator", params=dict(disc_start=1, disc_ndf=16))


@functools.lru_cache(maxsize=None)
def _disc_sd(ndf, n_layers, use_actnorm):
    from frido_amd.models import NLayerDiscriminator
    return R.filled_state_dict(NLayerDiscriminator(3, ndf, n_layers, use_actnorm))


@functools.lru_cache(maxsize=None)
def _lpips_sd():
    from frido_amd.models import LPIPS
    return L.filled_state_dict(LPIPS())


# ---- the restatement and the fixture -------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(R.NET_CASES)), ids=[str(c) for c in R.NET_CASES])
def test_net_restatement_matches_the_reference_golden(ci):
    """The reference ran in float32; the float64 restatement may differ from it by what float32 costs, measured on the restatement
    itself (float32 run against float64 run); the bound is 4 x it, as in tests/test_lpips_host.py (torch's conv2d orders its sums per
    shape and dtype)."""
    shape, ndf, nl, act = R.NET_CASES[ci]
    assert tuple(GOLD["net_shapes"][ci]) == shape
    sd = _disc_sd(ndf, nl, act)
    kw = dict(ndf=ndf, n_layers=nl, use_actnorm=act, want_hidden=True)
    for tag, img in zip(("real", "fake"), R.images(*shape, R.case_seed(ci))):
        l64, h64 = R.disc_ref(sd, img, **kw)
        l32, h32 = R.disc_ref(sd, img, dtype=torch.float32, **kw)
        gold = torch.from_numpy(GOLD[f"logits_{tag}_{ci}"]).double()
        assert gold.shape == l64.shape
        scale = float(l64.abs().max())
        e32 = max(float((h.double() - g).abs().max()) / float(g.abs().max()) for h, g in zip(h32 + [l32], h64 + [l64]))
        d = float((gold - l64).abs().max()) / scale
        print(f"patchgan restatement {R.NET_CASES[ci]} {tag}: golden vs f64 {d:.3e}, f32 restatement {e32:.3e}")
        assert e32 > 0 and d <= 4 * e32
        if tag == "real":
            for k, f in enumerate(h64):
                idx = R.sample_index(f.numel(), k, ci)
                df = float((torch.from_numpy(GOLD[f"hidden_{ci}_{k}"]).double() - f.flatten()[idx]).abs().max()) / float(f.abs().max())
                assert df <= 4 * e32, (k, df, e32)


def test_both_hinges_clip_in_every_fixture_case():
    """At least 10 % of the real logits above +1 and 10 % of the fake ones below -1: otherwise relu(1 - real) and relu(1 + fake) never
    clip and a swapped sign would pass."""
    pairs = [(GOLD[f"logits_real_{ci}"], GOLD[f"logits_fake_{ci}"]) for ci in range(len(R.NET_CASES))]
    pairs += [(GOLD[f"loss_logits_real_{li}"], GOLD[f"loss_logits_fake_{li}"]) for li in range(len(R.LOSS_CASES))]
    for i, (r, f) in enumerate(pairs):
        up, down = R.clip_shares(torch.from_numpy(r), torch.from_numpy(f))
        assert up >= 0.1 and down >= 0.1, (i, up, down)
    # and the swapped signs are far away on them
    for r, f in pairs:
        r, f = torch.from_numpy(r), torch.from_numpy(f)
        ok, bad = R.gan_ref(r, f), R.gan_ref(r, f, swap_signs=True)
        assert abs(float(ok["hinge"] - bad["hinge"])) > 1e-3 * abs(float(ok["hinge"]))


@pytest.mark.parametrize("li", range(len(R.LOSS_CASES)), ids=[c[0] for c in R.LOSS_CASES])
def test_loss_restatement_matches_the_reference_golden(li):
    """(loss, log) of both optimizer indices, below and at disc_start.  Bound: 4 x the restatement's own float32-vs-float64 difference
    (the largest relative one over the non-zero entries); entries that are exact zeros or constants must be equal."""
    disc_loss, act = R.LOSS_CASES[li]
    x, y = R.images(*R.LOSS_SHAPE, R.LOSS_SEED)
    sd = _disc_sd(R.LOSS_NDF, 3, act)
    for step in R.LOSS_STEPS:
        kw = dict(disc_loss=disc_loss, use_actnorm=act)
        l0, log0, l1, log1 = R.loss_ref(_lpips_sd(), sd, x, y, R.CODEBOOK_LOSS, step, **kw)
        f0, flog0, f1, flog1 = R.loss_ref(_lpips_sd(), sd, x, y, R.CODEBOOK_LOSS, step, dtype=torch.float32, **kw)
        ref = [l0] + [log0[k] for k in R.LOG0_KEYS] + [l1] + [log1[k] for k in R.LOG1_KEYS]
        r32 = [f0] + [flog0[k] for k in R.LOG0_KEYS] + [f1] + [flog1[k] for k in R.LOG1_KEYS]
        gold = [GOLD[f"loss0_{li}_{step}"]] + list(GOLD[f"log0_{li}_{step}"]) + [GOLD[f"loss1_{li}_{step}"]] + list(GOLD[f"log1_{li}_{step}"])
        e32 = max(abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(r32, ref) if float(b) != 0.0)
        assert e32 > 0
        names = ["loss0"] + list(R.LOG0_KEYS) + ["loss1"] + list(R.LOG1_KEYS)
        for name, g, r in zip(names, gold, ref):
            if name in ("rec_aux_loss", "d_weight") or (step < R.DISC_START and name in ("disc_factor", "loss1", "disc_loss")):
                assert float(g) == 0.0 == float(r), (name, g, r)
            elif name == "disc_factor":
                assert float(g) == np.float32(R.LOSS_KW["disc_factor"]) and float(r) == R.LOSS_KW["disc_factor"]
            else:
                assert abs(float(g) - float(r)) <= 4 * e32 * abs(float(r)), (name, step, float(g), float(r), e32)
        assert float(log0["rec_loss"]) == float(log0["nll_loss"]) and float(log0["total_loss"]) == float(l0)


def test_wrong_variants_of_the_formulas_are_far_away():
    """The keywords of patchgan_ref's functions are the near misses the GPU tests use: each moves the result, in float64, by far more
    than float32 does."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 10, 9, generator=g, dtype=torch.float64) * 2 - 1
    w = torch.randn(8, 3, 4, 4, generator=g, dtype=torch.float64) * 0.3
    b = torch.randn(8, generator=g, dtype=torch.float64)
    ref = R.stem_ref(x, w, b)
    assert torch.equal(ref, R.leaky(F.conv2d(x, w, b, stride=2, padding=1))) and ref.shape == (2, 8, 5, 4)
    for kw in (dict(pad=0), dict(stride=1), dict(transpose=True), dict(drop_bias=True), dict(slope=0.01)):
        assert float((R.stem_ref(x, w, b, **kw) - ref).abs().max()) > 1e-3 * float(ref.abs().max()), kw
    f = torch.randn(2, 8, 6, 5, generator=g, dtype=torch.float64)
    wh, bh = torch.randn(1, 8, 4, 4, generator=g, dtype=torch.float64) * 0.2, torch.tensor([0.4], dtype=torch.float64)
    ref = R.head_ref(f, wh, bh)
    assert torch.equal(ref, F.conv2d(f, wh, bh, stride=1, padding=1)) and ref.shape == (2, 1, 5, 4)
    for kw in (dict(pad=0), dict(stride=2), dict(transpose=True), dict(drop_bias=True)):
        assert float((R.head_ref(f, wh, bh, **kw) - ref).abs().max()) > 1e-3 * float(ref.abs().max()), kw
    rows = torch.randn(24, 8, generator=g, dtype=torch.float64)
    gam, bet, mu = (torch.randn(8, generator=g, dtype=torch.float64) for _ in range(3))
    var = torch.rand(8, generator=g, dtype=torch.float64) + 0.5
    a, bb = R.fold_bn(gam, bet, mu, var)
    ref = R.affine_ref(rows, a, bb)
    for got in (R.affine_ref(rows, *R.fold_bn(gam, bet, mu, var, no_root=True)), R.affine_ref(rows, a, bb, act_first=True),
                R.affine_ref(rows, a, bb, by_pixel=True)):
        assert float((got - ref).abs().max()) > 1e-3 * float(ref.abs().max())
    lr, lf = torch.randn(3, 1, 4, 4, generator=g) * 3, torch.randn(3, 1, 4, 4, generator=g) * 3
    ok = R.gan_ref(lr, lf)
    assert abs(float(ok["hinge"]) - float(0.5 * (F.relu(1 - lr).mean() + F.relu(1 + lf).mean()))) < 1e-6
    for kw, keys in ((dict(swap_signs=True), ("hinge", "vanilla")), (dict(mean_over_plane=True), ("logits_real", "hinge")), (dict(no_half=True), ("hinge", "vanilla"))):
        bad = R.gan_ref(lr, lf, **kw)
        for k in keys:
            assert abs(float(bad[k] - ok[k])) > 1e-3 * abs(float(ok[k])), (kw, k)


# ---- the folding of the norms --------------------------------------------------------------------------
def test_folded_norms_are_batchnorm_and_actnorm():
    from frido_amd import patchgan as pg
    g = torch.Generator().manual_seed(3)
    Cn = 12
    x = torch.randn(2, Cn, 5, 4, generator=g, dtype=torch.float64)
    gam, bet, mu = (torch.randn(Cn, generator=g) for _ in range(3))
    var = torch.rand(Cn, generator=g) + 0.3
    a, b = pg.fold_batchnorm(gam, bet, mu, var)
    assert a.dtype == b.dtype == torch.float32
    ref = F.batch_norm(x, mu.double(), var.double(), gam.double(), bet.double(), False, 0.0, 1e-5)
    got = a.double().view(1, -1, 1, 1) * x + b.double().view(1, -1, 1, 1)
    assert float((got - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max() + (mu.abs() * a.abs()).max())      # a, b rounded once
    a64 = gam.double() / torch.sqrt(var.double() + 1e-5)
    assert torch.equal(a, a64.float()) and torch.equal(b, (bet.double() - mu.double() * a64).float())
    loc, scale, bias = torch.randn(1, Cn, 1, 1, generator=g), torch.rand(1, Cn, 1, 1, generator=g) + 0.5, torch.randn(Cn, generator=g)
    a, b = pg.fold_actnorm(loc, scale, bias)
    ref = scale.double() * ((x + bias.double().view(1, -1, 1, 1)) + loc.double())      # util.py:58 on the biased conv's output
    got = a.double().view(1, -1, 1, 1) * x + b.double().view(1, -1, 1, 1)
    assert float((got - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max() + b.abs().max())
    assert torch.equal(a, scale.flatten()) and torch.equal(b, (scale.double().flatten() * (bias.double() + loc.double().flatten())).float())
    # fold_norm reads the reference's names
    from frido_amd.models import NLayerDiscriminator
    for act in (False, True):
        m = R.fill(NLayerDiscriminator(3, 8, 2, act))
        sd = m.state_dict()
        a, b = pg.fold_norm(sd, "", 2, 3, act)
        h = torch.randn(1, 16, 3, 3, generator=g, dtype=torch.float64)
        want = R.disc_ref({k: v for k, v in sd.items()}, torch.zeros(1, 3, 12, 12), ndf=8, n_layers=2, use_actnorm=act)      # runs: names resolve
        assert want.shape == (1, 1, 1, 1) and a.shape == b.shape == (16,)
        if act:
            ref = sd["main.3.scale"].double() * (h + sd["main.2.bias"].double().view(1, -1, 1, 1) + sd["main.3.loc"].double())
        else:
            ref = F.batch_norm(h, sd["main.3.running_mean"].double(), sd["main.3.running_var"].double(), sd["main.3.weight"].double(),
                               sd["main.3.bias"].double(), False, 0.0, 1e-5)
        got = a.double().view(1, -1, 1, 1) * h + b.double().view(1, -1, 1, 1)
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    assert pg.layer_table(3, 64, 3) == R.layer_table(3, 64, 3) == [(0, None, 3, 64, 2), (2, 3, 64, 128, 2), (5, 6, 128, 256, 2), (8, 9, 256, 512, 1),
                                                                  (11, None, 512, 1, 1)]
    assert pg.plane_sizes(256, 256, 3) == [(128, 128), (64, 64), (32, 32), (31, 31), (30, 30)]
    assert pg.plane_sizes(40, 36, 3) == [(20, 18), (10, 9), (5, 4), (4, 3), (3, 2)] and pg.plane_sizes(23, 24, 3) is None
    assert pg.plane_sizes(24, 24, 3)[-1] == (1, 1)


# ---- the holders -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_actnorm", [False, True])
def test_discriminator_state_dict_is_the_references(use_actnorm):
    from frido_amd.models import NLayerDiscriminator
    m = NLayerDiscriminator(use_actnorm=use_actnorm)
    tag = int(use_actnorm)
    keys = [str(k) for k in GOLD[f"keys_actnorm_{tag}"]]
    shapes = [tuple(int(s) for s in str(v).split(",") if s) for v in GOLD[f"shapes_actnorm_{tag}"]]
    dtypes = [str(d) for d in GOLD[f"dtypes_actnorm_{tag}"]]
    sd = m.state_dict()
    assert list(sd) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes and [str(v.dtype) for v in sd.values()] == dtypes
    assert "main.11.bias" in keys and ("main.3.loc" in keys) == use_actnorm and ("main.3.running_var" in keys) != use_actnorm
    assert ("main.2.bias" in keys) == use_actnorm
    assert not m.training and all(not p.requires_grad for p in m.parameters())


def test_loss_state_dict_is_the_references_and_a_checkpoint_round_trips(tmp_path):
    from frido_amd.models import MSFPNVQModel, VQLPIPSWithDiscriminator, NLayerDiscriminator, LPIPS
    loss = VQLPIPSWithDiscriminator(**R.LOSS_KW)
    keys = [str(k) for k in GOLD["loss_keys"]]
    shapes = [tuple(int(s) for s in str(v).split(",") if s) for v in GOLD["loss_shapes"]]
    assert {k: tuple(v.shape) for k, v in loss.state_dict().items()} == dict(zip(keys, shapes))
    assert isinstance(loss.perceptual_loss, LPIPS) and isinstance(loss.discriminator, NLayerDiscriminator) and not loss.training
    # weights_init was applied: conv weights N(0, 0.02), BatchNorm weights N(1, 0.02), BatchNorm biases 0
    sd = loss.discriminator.state_dict()
    assert 0.01 < float(sd["main.5.weight"].std()) < 0.03 and abs(float(sd["main.6.weight"].mean()) - 1) < 0.02 and not sd["main.6.bias"].any()
    # a taming checkpoint's loss.* keys find their home
    cfg = dict(VQ_SMALL, lossconfig=LOSSCFG)
    m = MSFPNVQModel(**cfg, with_loss=True)
    sd = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    assert any(k.startswith("loss.discriminator.main.8.") for k in sd) and any(k.startswith("loss.perceptual_loss.net.slice3.") for k in sd)
    torch.save({"state_dict": sd}, tmp_path / "tok.ckpt")
    m2 = MSFPNVQModel(**cfg, with_loss=True, ckpt_path=str(tmp_path / "tok.ckpt"))
    got = m2.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    # without the opt-in the same file loads as before: the loss.* keys are passed over (strict=False)
    m3 = MSFPNVQModel(**cfg, ckpt_path=str(tmp_path / "tok.ckpt"))
    assert not any(k.startswith("loss.") for k in m3.state_dict()) and float(m3.post_quant_conv.weight.detach().flatten()[0]) == 0.25


def test_opt_in_and_default():
    from frido_amd.models import MSFPNVQModel, DummyLoss, VQLPIPSWithDiscriminator, instantiate_from_config
    plain = MSFPNVQModel(**dict(VQ_SMALL, lossconfig=LOSSCFG))
    assert isinstance(plain.loss, DummyLoss) and plain.global_step == 0
    with pytest.raises(NotImplementedError, match=r"validation_step.*LPIPS.*encode\(\)\[1\]"):
        plain.validation_step({}, 0)
    on = MSFPNVQModel(**dict(VQ_SMALL, lossconfig=LOSSCFG), with_loss=True, precision="bf16x3_bf16")
    assert isinstance(on.loss, VQLPIPSWithDiscriminator) and on.loss.discriminator.ndf == 16 and on.loss.discriminator_iter_start == 1
    assert on.loss.discriminator.precision == on.loss.perceptual_loss.precision == "bf16x3_bf16"
    assert sorted(k for k in on.state_dict() if not k.startswith("loss.")) == sorted(plain.state_dict())
    dummy = MSFPNVQModel(**dict(VQ_SMALL, lossconfig=DUMMY), with_loss=True)
    assert isinstance(dummy.loss, DummyLoss) and sorted(dummy.state_dict()) == sorted(plain.state_dict())
    plain.loss = VQLPIPSWithDiscriminator(disc_start=0, disc_ndf=16)          # assigned afterwards
    assert any(k.startswith("loss.discriminator.") for k in plain.state_dict())
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        plain.validation_step(dict(image=torch.zeros(1, 64, 64, 3)), 0)
    aux = MSFPNVQModel(**dict(VQ_SMALL, lossconfig=LOSSCFG, use_aux_loss=True), with_loss=True)
    with pytest.raises(NotImplementedError, match="use_aux_loss=True.*vqperceptual.py:96"):
        aux.validation_step(dict(image=torch.zeros(1, 64, 64, 3)), 0)
    via = instantiate_from_config(dict(target="taming.models.msvqgan.MSFPNVQModel", params=dict(VQ_SMALL, lossconfig=LOSSCFG, with_loss=True)))
    assert isinstance(via.loss, VQLPIPSWithDiscriminator)


def test_alias_imports():
    import taming.modules.losses as losses
    import taming.modules.losses.vqperceptual as vqp
    import frido_amd.models as M
    from taming.modules.discriminator.model import NLayerDiscriminator, weights_init
    from taming.modules.util import ActNorm
    assert NLayerDiscriminator is M.NLayerDiscriminator and weights_init is M.weights_init and ActNorm is M.ActNorm
    for name in ("VQLPIPSWithDiscriminator", "DummyLoss", "hinge_d_loss", "vanilla_d_loss", "adopt_weight"):
        assert getattr(vqp, name) is getattr(M, name), name
    assert losses.VQLPIPSWithDiscriminator is M.VQLPIPSWithDiscriminator
    assert M.adopt_weight(0.8, 4, threshold=5) == 0.0 and M.adopt_weight(0.8, 5, threshold=5) == 0.8
    lr, lf = torch.tensor([2.0, -0.5]), torch.tensor([-3.0, 0.25])
    assert float(M.hinge_d_loss(lr, lf)) == 0.5 * ((0 + 1.5) / 2 + (0 + 1.25) / 2)
    assert abs(float(M.vanilla_d_loss(lr, lf)) - float(0.5 * (F.softplus(-lr).mean() + F.softplus(lf).mean()))) < 1e-7
    a = ActNorm(6)
    assert list(a.state_dict()) == ["loc", "scale", "initialized"] and a.state_dict()["initialized"].dtype == torch.uint8


# ---- refusals, by their words --------------------------------------------------------------------------
def test_refusals_name_themselves():
    from frido_amd.models import NLayerDiscriminator, VQLPIPSWithDiscriminator, LPIPS
    from frido_amd.pipeline import reconstruction_metrics
    d = NLayerDiscriminator(ndf=16)
    with pytest.raises(NotImplementedError, match=r"NLayerDiscriminator.train\(\).*batch statistics"):
        d.train()
    assert d.eval() is d and not d.training
    with pytest.raises(NotImplementedError, match="input_nc=9"):
        NLayerDiscriminator(input_nc=9)
    with pytest.raises(NotImplementedError, match="ndf=18 must be a multiple of 4"):
        NLayerDiscriminator(ndf=18)
    with pytest.raises(NotImplementedError, match="32 KB of LDS"):
        NLayerDiscriminator(input_nc=8, ndf=128)
    with pytest.raises(ValueError, match="n_layers=0"):
        NLayerDiscriminator(n_layers=0)
    with pytest.raises(ValueError, match=r"too small for a 1 x 1 logit map.*smallest side is 24"):
        d(torch.zeros(1, 3, 23, 40))
    with pytest.raises(ValueError, match=r"must be a \[B, 3, H, W\]"):
        d(torch.zeros(1, 4, 32, 32))
    with pytest.raises(ValueError, match="differ in shape"):
        d.pair(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 40))
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        d(torch.zeros(1, 3, 32, 32))
    assert NLayerDiscriminator(ndf=16, n_layers=2).min_side() == 12 and NLayerDiscriminator(ndf=16, n_layers=4).min_side() == 48
    loss = VQLPIPSWithDiscriminator(disc_start=0, disc_ndf=16)
    with pytest.raises(NotImplementedError, match=r"VQLPIPSWithDiscriminator.train\(\).*not self.training"):
        loss.train()
    with pytest.raises(NotImplementedError, match="disc_conditional=True"):
        VQLPIPSWithDiscriminator(disc_start=0, disc_conditional=True)
    ok = torch.zeros(2, 3, 32, 32)
    q = torch.tensor(0.1)
    with pytest.raises(NotImplementedError, match="cond="):
        loss(q, ok, ok, 0, 0, cond=ok)
    with pytest.raises(NotImplementedError, match="xrec_aux=.*line 96"):
        loss(q, ok, ok, 0, 0, xrec_aux=[ok, ok])
    with pytest.raises(ValueError, match="differ in shape"):
        loss(q, ok, ok[:1], 0, 0)
    with pytest.raises(ValueError, match="optimizer_idx must be 0 or 1"):
        loss(q, ok, ok, 2, 0)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        loss(q, ok, ok, 1, 0)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        loss.evaluate(q, ok, ok, 0)
    with pytest.raises(ValueError, match="must be a frido_amd.models.NLayerDiscriminator"):
        reconstruction_metrics(torch.nn.Identity(), ok, LPIPS(), discriminator=torch.nn.Identity())


# ---- the launchers, without a device -------------------------------------------------------------------
def test_descriptor_sizes_on_both_libraries():
    from frido_amd import patchgan as pg
    for planes in ("f16", "bf16"):
        Lb = _lib.lib(planes)
        for name, (struct, sizeof) in pg.LAUNCHERS.items():
            assert getattr(Lb, sizeof)() == C.sizeof(struct), (planes, name)
        assert set(pg._fns(planes)) == set(pg.LAUNCHERS)
    assert C.sizeof(pg.FridoDiscStem) == 5 * 8 + 6 * 4 and C.sizeof(pg.FridoAffineLeaky) == 4 * 8 + 8 + 2 * 4
    assert C.sizeof(pg.FridoGanFinish) == 3 * 8 + 2 * 4


def test_bad_descriptors_are_turned_away_before_a_device_is_touched():
    from frido_amd import patchgan as pg
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    for planes in ("f16", "bf16"):
        Lb = _lib.lib(planes)
        fns = pg._fns(planes)

        def refused(name, desc, words):
            assert fns[name](C.byref(desc), None) == -1 and words in Lb.frido_last_error(), (name, Lb.frido_last_error())      # FRIDO_EINVAL

        for name, (struct, _) in pg.LAUNCHERS.items():                     # a zeroed descriptor: null pointers
            refused(name, struct(), name.encode() + b": bad arguments")
        for kw, words in ((dict(x=None), b"bad arguments"), (dict(w=None), b"bad arguments"), (dict(B=0), b"bad arguments"),
                          (dict(Cin=9), b"1 .. 8 input channels"), (dict(Cin=0), b"1 .. 8 input channels"), (dict(H=1), b"one output pixel"),
                          (dict(ndf=18), b"multiple of 4"), (dict(ndf=0), b"multiple of 4"), (dict(ndf=256), b"32 KB of LDS"),
                          (dict(dst=base + 4), b"16-byte aligned")):
            d = pg.stem_desc(base, None, base, base, base, 1, 3, 8, 8, 16)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_disc_stem", d, words)
        for kw, words in ((dict(C=6), b"multiple of 4"), (dict(rows=0), b"bad arguments"), (dict(a=None), b"bad arguments"),
                          (dict(src=base + 8), b"16-byte aligned")):
            d = pg.affine_desc(base, base, base, base, 4, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_affine_leaky", d, words)
        for kw, words in ((dict(C=6), b"multiple of 4"), (dict(H=1), b"one output pixel"), (dict(S=0), b"bad arguments"),
                          (dict(logits=None), b"bad arguments"), (dict(w=base + 4), b"16-byte aligned")):
            d = pg.head_desc(base, base, base, 1, 4, 4, 8, 0.5)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_disc_head", d, words)
        for d, words in ((pg.terms_desc(base, base, 0, 4), b"bad arguments"), (pg.terms_desc(base, base + 4, 2, 4), b"8-byte aligned"),
                         (pg.terms_desc(base, base, 2, 0), b"bad arguments")):
            refused("frido_gan_terms", d, words)
        for d, words in ((pg.finish_desc(base, base, None, 1, 4), b"bad arguments"), (pg.finish_desc(base, base, base, 0, 4), b"bad arguments"),
                         (pg.finish_desc(base + 4, base, base, 1, 4), b"8-byte aligned")):
            refused("frido_gan_finish", d, words)
    d = pg.stem_desc(16, None, 32, 48, 64, 2, 3, 8, 8, 16)
    assert d.slope == np.float32(0.2) and not d.y


def test_the_op_table_header_does_not_know_the_launches():
    """frido_hip.h is the op-kind ABI (tests/test_opkinds_host.py pins it): the discriminator's launches live in a header of their own."""
    hip = open(os.path.join(REPO, "include", "frido_hip.h")).read()
    for name in ("disc_stem", "affine_leaky", "disc_head", "gan_terms", "gan_finish", "FridoDisc", "FridoGan", "FridoAffineLeaky"):
        assert name not in hip
    assert _lib.ABI_VERSION == 8 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert not [s for s in _lib.EXPORTS if "disc_" in s or "gan_" in s or "affine_leaky" in s]
    hdr = open(os.path.join(REPO, "include", "frido_patchgan.h")).read()
    assert '#include "frido_hip.h"' in hdr
    assert _lib._parse_structs(_lib._strip_comments(hdr)).keys() == {"FridoDiscStem", "FridoAffineLeaky", "FridoDiscHead", "FridoGanTerms", "FridoGanFinish"}
    mk = open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert "patchgan.hip" in srcs and srcs.count("patchgan.hip") == 1      # it has no status word: its place in the link order moves no number
    assert "patchgan.o obj_bf16p/patchgan.o: ../../include/frido_patchgan.h" in mk
    src = open(os.path.join(REPO, "frido_amd", "csrc", "patchgan.hip")).read()
    assert '#include "launch.h"' in src and "common.h" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "hipMalloc" not in src and "Synchronize" not in src

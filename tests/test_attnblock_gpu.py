"""AttentionBlock denoisers (use_spatial_transformer=False) on the MI355X against goldens captured from the reference's own modules
(tests/golden/make_golden_attnblock.py): forward eps of every fixture configuration and of the full-width f8f4 denoiser with the
attention family switched (12 / 18 / 30 heads of 32), unconditional and class-conditional DDIM / PLMS sampling, batch rows, replay.
The sampler fixtures use the small two-stage split-head models WITHOUT SPADE: with it the reference's own run is ill-conditioned (it moves
by 1.2e-3 .. 1e-1 under a 1e-6 perturbation of its eps -- attnblock_cfg.py has the measurement); SPADE-fed AttentionBlocks are pinned by the
forward goldens of both stages.

Bounds are the ones tests/test_model_gpu.py uses for the same arithmetic: forward eps 2e-4 (test_unet_forward_matches_reference_golden),
sampled latents 1e-3 (test_sampler_matches_reference_golden), batch rows 5e-5 (E2E_X3 latent_rel).  The fixtures stay inside the fp16
planes' range (their stream_absmax is far below 65504), so a FridoNumericsWarning is an error here.
"""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from golden_cfg import VQ_SMALL, BERT_SMALL, frido_cfg  # noqa: E402
from attnblock_cfg import FORWARD, AB_CLS_EMB, AB_SMP, AB_SMP_EMB, AB_SMP_LIN, AB_FULL  # noqa: E402
from frido_amd.synth import fill_module, seeded_normal  # noqa: E402


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    from frido_amd import _lib
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _unet(cfg):
    from frido_amd.models import PyUNetModel
    return fill_module(PyUNetModel(**cfg), "model.diffusion_model.").cuda().eval()


def _frido(ucfg, key):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(ucfg, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key       # ('__is_unconditional__' resets the wrapper's key to None, like the reference)
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    return m.cuda().eval()


def _uses_mh(m):
    """Number of multi-head attention launches in the compiled step programs of a denoiser."""
    from frido_amd import _lib
    return sum(kind == _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] for plan in m.runtime().plans.values() for kind, _ in plan.step.ops)


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.gate) if n == "ab_small" else n for n in sorted(FORWARD)])
def test_forward_matches_reference_golden(name):
    g, cfg = golden(name), FORWARD[name]
    assert max(float(g[f"stream_absmax_{s}"]) for s in range(cfg["num_stage"])) < 1000.0
    m = _unet(cfg)
    x = torch.from_numpy(g["x"]).cuda()
    y = torch.from_numpy(g["y"]).cuda() if "y" in g.files else None
    splits = cfg["split_embed_dim_list"]
    for s in range(cfg["num_stage"]):
        e = m(x[:, :sum(splits[:s + 1])].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), y=y, stage=s)
        assert e.shape == g[f"eps_{s}"].shape
        err = _rel(e, g[f"eps_{s}"])
        print(f"{name} stage {s}: eps max-relative error {err:.3e}")
        assert err < 2e-4, (name, s)
    # a context passed anyway is ignored, like the reference's TimestepEmbedSequential does for an AttentionBlock
    e2 = m(x[:, :splits[0]].contiguous(), torch.from_numpy(g["t_0"]).cuda(), context=torch.zeros(x.shape[0], 5, 64, device="cuda"), y=y, stage=0)
    assert _rel(e2, g["eps_0"]) < 2e-4
    heads = set(g["heads"].tolist())
    assert (_uses_mh(m) > 0) == (heads != {1})      # several heads: the new kernel; one head: the existing single-head path


def test_full_width_forward_matches_reference_golden():
    """dict(UNET_F8F4, use_spatial_transformer=False) at B = 2, 64 x 64: 12 / 18 / 30 heads of 32 over 1024 / 256 / 64 tokens."""
    g = golden("ab_full")
    assert sorted(set(g["heads"].tolist())) == [12, 18, 30]
    m = _unet(AB_FULL)
    x = torch.from_numpy(seeded_normal("ab_full:x", (2, 6, 64, 64))).cuda()
    for s in range(2):
        e = m(x[:, :3 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), stage=s)
        err = _rel(e, g[f"eps_{s}"])
        print(f"ab_full stage {s}: eps max-relative error {err:.3e} (stream max {float(g[f'stream_absmax_{s}']):.4g})")
        assert err < 2e-4, s
    assert _uses_mh(m) == 2 * len(g["heads"])
    del m
    torch.cuda.empty_cache()


def _check_run(g, run, samples, inter, model):
    assert float(g[f"{run}_ref_sens"]) < 1e-4      # the fixture is well conditioned: see attnblock_cfg.AB_SMP
    assert _rel(samples, g[f"{run}_samples"]) < 1e-3
    assert len(inter["x_inter"]) == int(g[f"{run}_nx"])
    assert _rel(inter["x_inter"][-1], g[f"{run}_x_inter_last"]) < 1e-3
    assert _rel(inter["pred_x0"][1], g[f"{run}_pred_x0_1"]) < 1e-3
    img = model.decode_first_stage(samples)
    bad = float(((img.cpu() - torch.from_numpy(g[f"{run}_img"])).abs().amax(1) > 1e-3).float().mean())
    print(f"{run}: latent rel err {_rel(samples, g[f'{run}_samples']):.2e}, decoded pixels off by > 1e-3: {100 * bad:.3f} %")
    assert torch.isfinite(img).all()


def _sample(model, g, run, ucfg, c, uc):
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    S, eta, scale, lev = g[f"{run}_args"]
    cls = PLMSSampler if "plms" in run else DDIMSampler
    torch.manual_seed(23)           # noise="torch": the host generator's stream, draw for draw the reference's CPU run
    return cls(model).sample(S=int(S), batch_size=2, shape=(ucfg["in_channels"], 16, 16), conditioning=c, num_stage=ucfg["num_stage"],
                             eta=float(eta), verbose=False, log_every_t=int(lev), unconditional_guidance_scale=float(scale),
                             unconditional_conditioning=uc if scale != 1.0 else None, noise="torch")


@pytest.mark.parametrize("run", [pytest.param("ddim_eta1", marks=pytest.mark.gate), "plms"])
def test_unconditional_sampler_matches_reference_golden(run):
    """FridoDiffusion(cond_stage_config='__is_unconditional__'), conditioning=None: DDIM (S 4, eta 1) and PLMS (S 6)."""
    g = golden("ab_sampler_uncond")
    assert float(g["stream_absmax"]) < 1000.0
    model = _frido(AB_SMP, None)
    samples, inter = _sample(model, g, run, AB_SMP, None, None)
    _check_run(g, run, samples, inter, model)
    # the same latent through the public single-step interface: apply_model routes a None conditioning to the context-free denoiser
    t = torch.tensor([500, 20], device="cuda")
    e = model.apply_model(samples[:, :3].contiguous(), t, None, stage=0)
    assert e.shape == (2, 3, 16, 16) and torch.isfinite(e).all()


@pytest.mark.parametrize("run", ["emb_ddim_eta0_cfg", "emb_plms_cfg", "lin_ddim_eta1"])
def test_class_conditional_sampler_matches_reference_golden(run):
    """conditioning_key='adm': label tensors as conditioning, classifier-free guidance 1.5 with a label tensor as the unconditional
    conditioning (nn.Embedding form), one run of the nn.Linear form."""
    g = golden("ab_sampler_adm")
    ucfg = AB_SMP_EMB if run.startswith("emb") else AB_SMP_LIN
    model = _frido(ucfg, "adm")
    y = torch.from_numpy(g["emb_y" if run.startswith("emb") else "lin_y"]).cuda()
    uy = torch.from_numpy(g["emb_uy"]).cuda() if run.startswith("emb") else None
    samples, inter = _sample(model, g, run, ucfg, y, uy)
    _check_run(g, run, samples, inter, model)
    e = model.apply_model(samples[:, :3].contiguous(), torch.tensor([500, 20], device="cuda"), y, stage=0)
    assert e.shape == (2, 3, 16, 16) and torch.isfinite(e).all()


def test_sampler_conditioning_modes_are_checked():
    from frido.models.diffusion.ddim import DDIMSampler
    kw = dict(S=2, batch_size=2, shape=(6, 16, 16), num_stage=2, eta=0.0, verbose=False, noise="philox")
    un = _frido(AB_SMP, None)
    with pytest.raises(ValueError, match="neither a context nor class labels"):
        DDIMSampler(un).sample(conditioning=torch.zeros(2, 5, 64, device="cuda"), **kw)
    cl = _frido(AB_SMP_EMB, "adm")
    with pytest.raises(ValueError, match="needs its labels"):
        DDIMSampler(cl).sample(conditioning=None, **kw)
    with pytest.raises(ValueError, match="batch-size"):
        DDIMSampler(cl).sample(conditioning=torch.zeros(3, dtype=torch.int64, device="cuda"), **kw)
    with pytest.raises(ValueError, match="class labels of shape"):
        DDIMSampler(cl).sample(conditioning=torch.zeros(2, 10, device="cuda"), **kw)
    # the engine cache tells the modes apart: guidance on / off are two engines of the class-conditional denoiser
    y = torch.tensor([1, 2], device="cuda")
    DDIMSampler(cl).sample(conditioning=y, **kw)
    DDIMSampler(cl).sample(conditioning=y, unconditional_guidance_scale=2.0, unconditional_conditioning=torch.full_like(y, 9), **kw)
    keys = list(cl.model.diffusion_model.runtime()._sampler_engines)
    assert len(keys) == 2 and all("labels" in k for k in keys)


def test_batch_rows_of_a_class_conditional_forward_equal_single_sample_forwards():
    """B = 16 with sixteen different labels and timesteps: rows 0, 7, 15 equal the B = 1 forwards of those rows -- a label / row mix-up
    in the per-sample embedding table would show here."""
    B = 16
    m = _unet(AB_CLS_EMB)
    x = torch.from_numpy(seeded_normal("ab_rows:x", (B, 6, 16, 16))).cuda()
    y = torch.tensor([(3 * i + 1) % 10 for i in range(B)], device="cuda")
    t = torch.tensor([990 - 61 * i for i in range(B)], device="cuda")
    for s in (0, 1):
        xin = x[:, :3 * (s + 1)].contiguous()
        eb = m(xin, t, y=y, stage=s)
        for i in (0, 7, 15):
            e1 = m(xin[i:i + 1].contiguous(), t[i:i + 1], y=y[i:i + 1], stage=s)
            err = _rel(eb[i:i + 1], e1.cpu())
            print(f"stage {s} row {i}: {err:.3e}")
            assert err < 5e-5, (s, i)
        # and the labels matter: another label moves the row by far more than the bound
        other = m(xin[:1].contiguous(), t[:1], y=(y[:1] + 1) % 10, stage=s)
        assert _rel(other, eb[:1].cpu()) > 1e-3


def test_unconditional_philox_sampling_replays_identically():
    """noise='philox' through the captured step graphs: two runs with one seed are bit-identical, another seed differs."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    model = _frido(AB_SMP, None)
    for cls, eta in ((DDIMSampler, 1.0), (PLMSSampler, 0.0)):
        kw = dict(S=5, batch_size=3, shape=(6, 16, 16), conditioning=None, num_stage=2, eta=eta, verbose=False, noise="philox")
        a, _ = cls(model).sample(seed=5, **kw)
        b, _ = cls(model).sample(seed=5, **kw)
        c, _ = cls(model).sample(seed=6, **kw)
        assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()

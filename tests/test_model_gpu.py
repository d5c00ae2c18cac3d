"""Model-level parity on the MI355X: the HIP path behind the reference's class API against (a) the
golden fixtures captured from the reference itself and (b) the oracle on the same seeded inputs.

Precision: bf16x3 keyword = the fp32-emulating MFMA path (r03: fp16 hi + fp16 lo operand planes, three passes).  Stated tolerances,
relative to the output's max-abs:
  single denoiser forward     2e-4      multi-step sampler latents   1e-3
  VQGAN decode (same codes)   2e-4      decoded pixels end-to-end    1e-3 abs (north star); the full-size end-to-end runs assert
                                        E2E_X3 below (latent 5e-5, pixels 1e-4, measured 6e-6 / 8e-6), code flips reported
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden, synth_sd, unet_holder, vq_holder  # noqa: E402
from golden_cfg import (UNET_SMALL, UNET_SMALL_D2, UNET_SMALL3, UNET_FULL, VQ_SMALL, VQ_SMALL3, VQ_FULL, BERT_SMALL, frido_cfg)  # noqa: E402
from frido_amd.synth import fill_module  # noqa: E402


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


# (r06) Models a test only READS are built once per session: the full-size layout2i model costs ~25 s of host time per build (575 M
# parameters through the numpy filler, plan algebra in float64, packed weight upload), and a dozen tests want the same one.  Tests that
# change weights / scale factors / precision build their own (`_frido`, `_unet`, `_vq` without `shared`).
_SHARED = {}


def _shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def _pairs():
    """{id(unet cfg) or id(vq cfg): (unet cfg, vq cfg)} of the full-size configurations whose parts come out of one shared model."""
    from golden_cfg import UNET_512, VQ_512
    out = {}
    for u, v in ((UNET_FULL, VQ_FULL), (UNET_512, VQ_512)):
        out[id(u)] = out[id(v)] = (u, v)
    return out


def _unet(cfg, shared=False):
    from frido_amd.models import PyUNetModel
    if shared and id(cfg) in _pairs():       # the denoiser of the shared full-size model: same parameter names, same filler
        return _frido(*_pairs()[id(cfg)], precision="bf16x3", shared=True).model.diffusion_model

    def make():
        m = PyUNetModel(**cfg)
        fill_module(m, "model.diffusion_model.")
        return m.cuda().eval()
    return _shared(("unet", id(cfg)), make) if shared else make()


@pytest.mark.parametrize("name,cfg", [("unet_small", UNET_SMALL), ("unet_small3", UNET_SMALL3), ("unet_small_d2", UNET_SMALL_D2)])
def test_unet_forward_matches_reference_golden(name, cfg):
    g = golden(name)
    m = _unet(cfg)
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    splits = cfg["split_embed_dim_list"]
    for s in range(cfg["num_stage"]):
        e = m(x[:, :sum(splits[:s + 1])].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=ctx, stage=s)
        assert e.shape == g[f"eps_{s}"].shape
        assert _rel(e, g[f"eps_{s}"]) < 2e-4, (name, s)


@pytest.mark.parametrize("B,H,W,nctx", [(1, 16, 16, 5), (3, 16, 8, 1), (2, 8, 24, 33)])
def test_unet_forward_ragged_shapes_vs_oracle(B, H, W, nctx):
    """Edge shapes: batch 1 / odd batch, non-square latents, 1 and 33 context tokens (pad paths), per-sample timesteps."""
    from oracle.unet import unet_forward
    from frido_amd.synth import seeded_normal
    m = _unet(UNET_SMALL)
    sd = synth_sd(unet_holder(UNET_SMALL), "model.diffusion_model.")
    x = torch.from_numpy(seeded_normal("rag:x", (B, 6, H, W)))
    ctx = torch.from_numpy(seeded_normal("rag:c", (B, nctx, 64)))
    t = torch.tensor([11 + 300 * i for i in range(B)])
    for s in (0, 1):
        xin = x[:, :3 * (s + 1)].contiguous()
        ref = unet_forward(sd, UNET_SMALL, xin, t, ctx, s)
        got = m(xin.cuda(), t.cuda(), context=ctx.cuda(), stage=s)
        assert got.shape == ref.shape and _rel(got, ref) < 2e-4, (B, H, W, s)


def test_unet_forward_bf16_mode_within_bf16_tolerance():
    g = golden("unet_small")
    from frido_amd.models import PyUNetModel
    m = fill_module(PyUNetModel(**UNET_SMALL, precision="bf16"), "model.diffusion_model.").cuda()
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    e = m(x, torch.from_numpy(g["t_1"]).cuda(), context=ctx, stage=1)
    assert _rel(e, g["eps_1"]) < 5e-2


@pytest.mark.gate
def test_unet_full_width_forward_matches_reference_golden():
    g = golden("unet_full")
    m = _unet(UNET_FULL, shared=True)
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    for s in range(2):
        e = m(x[:, :3 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=ctx, stage=s)
        assert _rel(e, g[f"eps_{s}"]) < 2e-4, s


def test_unet_full_width_bf16_mode_within_bf16_tolerance():
    """The benchmark's arithmetic (single bf16 plane, bf16 residual stream, chained FF2+proj_out GEMM) at the full
    layout2i width against the reference golden."""
    g = golden("unet_full")
    from frido_amd.models import PyUNetModel
    m = fill_module(PyUNetModel(**UNET_FULL, precision="bf16"), "model.diffusion_model.").cuda()
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    for s in range(2):
        e = m(x[:, :3 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=ctx, stage=s)
        assert _rel(e, g[f"eps_{s}"]) < 5e-2, s


def test_no_cpu_fallback():
    from frido_amd.models import PyUNetModel
    from frido_amd._lib import FridoHipError
    m = PyUNetModel(**UNET_SMALL)
    with pytest.raises(FridoHipError):
        m(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.long), context=torch.zeros(1, 5, 64), stage=0)


def _vq(cfg, shared=False):
    from frido_amd.models import VQModelInterface
    if shared and id(cfg) in _pairs():
        return _frido(*_pairs()[id(cfg)], precision="bf16x3", shared=True).first_stage_model

    def make():
        m = VQModelInterface(**cfg, lossconfig=dict(target="taming.modules.losses.DummyLoss"))
        fill_module(m, "first_stage_model.")
        return m.cuda().eval()
    return _shared(("vq", id(cfg)), make) if shared else make()


def test_vq_decode_matches_reference_golden():
    g = golden("vq_small")
    m = _vq(VQ_SMALL)
    h = torch.from_numpy(g["h"]).cuda()
    dec, code = m.decode(h, return_code=True)
    code = np.asarray(code)
    flips = (code != g["code"]).mean()
    print(f"vq_small: VQ code flips {flips:.2e}")
    assert flips == 0, "index work is bit-exact: the committed codes of the reference must come back (vq_small.code)"
    # the decoder itself, UNCONDITIONALLY: forced onto the reference's own codes (no VQ decision boundary in the comparison)
    forced = m.decode(h, force_codes=[g["code"][i] for i in range(len(VQ_SMALL["embed_dim"]))])
    r = _rel(forced, g["dec"])
    print(f"vq_small: decoder rel err on the reference's codes {r:.2e}")
    assert r < 2e-4
    if flips == 0:
        assert torch.equal(forced, dec)


def test_vq_encode_matches_reference_golden():
    """MSEncoder + coarse-to-fine (quant_conv, VQ, ConvTranspose upsample, shared decoder)."""
    g = golden("vq_small")
    m = _vq(VQ_SMALL)
    enc = m.encode(torch.from_numpy(g["img"]).cuda())
    assert enc.shape == g["enc"].shape
    # the coarse scale is quantised on the way to the fine one: allow a VQ code flip to perturb a few pixels
    err = (enc.cpu() - torch.from_numpy(g["enc"])).abs()
    scale = float(np.abs(g["enc"]).max())
    assert float((err > 5e-4 * scale).float().mean()) < 0.02
    assert float(err[:, :3].max()) < 5e-4 * scale          # coarse channels have no VQ in their path
    enc2 = m.encode(torch.from_numpy(g["img"]).cuda(), scale=[2.0, 0.5])
    assert _rel(enc2[:, :3], 2.0 * enc[:, :3].cpu()) < 1e-6 and _rel(enc2[:, 3:], 0.5 * enc[:, 3:].cpu()) < 1e-6


def test_vq_encode_three_scales_matches_oracle():
    from oracle.vqgan import vq_encode
    from helpers import synth_sd, vq_holder
    from frido_amd.synth import seeded_normal
    m = _vq(VQ_SMALL3)
    x = torch.from_numpy(np.tanh(seeded_normal("enc3:img", (1, 3, 64, 64))))
    ref = vq_encode(synth_sd(vq_holder(VQ_SMALL3), "first_stage_model."), VQ_SMALL3, x)
    enc = m.encode(x.cuda())
    err = (enc.cpu() - ref).abs()
    assert enc.shape == ref.shape and float((err > 5e-4 * float(ref.abs().max())).float().mean()) < 0.03


def _to_np_u8(x):
    """scripts/sample_diffusion.py:115-121 custom_to_np, evaluated with torch on the CPU exactly as the script does."""
    return ((x.detach().cpu() + 1) * 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _to_pil_u8(x):
    """scripts/sample_diffusion.py:103-113 custom_to_pil per image: clamp, (x + 1) / 2, numpy's 255 * x, astype(uint8)."""
    out = []
    for xi in x.detach().cpu():
        xi = (torch.clamp(xi, -1., 1.) + 1.) / 2.
        out.append(torch.from_numpy((255 * xi.permute(1, 2, 0).numpy()).astype(np.uint8)))
    return torch.stack(out)


def test_uint8_output_path():
    """the uint8 HWC image comes out of the decoder's LAST conv epilogue (no f32 image, no separate pass), in both
    of the sampling script's conversions.  (a) bit-exact against the two formulas applied to this decoder's own f32 output --
    the conversion itself; (b) against the formulas applied to the ORACLE's decode of the same codes: the only admissible
    differences are pixels whose f32 value sits within the decoder's 1e-4 parity bound of a truncation boundary (off by one)."""
    from oracle.vqgan import vq_decode
    g = golden("vq_small")
    m = _vq(VQ_SMALL)
    h = torch.from_numpy(g["h"]).cuda()
    f, code = m.decode(h, return_code=True)
    assert (np.asarray(code) != g["code"]).sum() == 0
    u_np, u_pil = m.decode(h, to_uint8=True), m.decode(h, to_uint8="pil")
    assert u_np.dtype == torch.uint8 and u_np.shape == (f.shape[0], f.shape[2], f.shape[3], 3) and u_np.is_contiguous()
    assert torch.equal(u_np.cpu(), _to_np_u8(f)) and torch.equal(u_pil.cpu(), _to_pil_u8(f))
    assert torch.equal(m.decode(h, to_uint8="np"), u_np)
    # (127.5 (x + 1) and 255 ((x + 1) / 2) round differently in fp32 only on rare values: the two outputs usually coincide)
    ref = vq_decode(synth_sd(vq_holder(VQ_SMALL), "first_stage_model."), VQ_SMALL, torch.from_numpy(g["h"]))
    for got, want, scale in ((u_np, _to_np_u8(ref), 127.5), (u_pil, _to_pil_u8(ref), 127.5)):
        diff = (got.cpu().int() - want.int()).abs()
        assert int(diff.max()) <= 1
        # a differing byte must be explained by a truncation boundary within the f32 parity bound of the oracle's value
        y = ((ref.clamp(-1, 1) + 1) * scale).permute(0, 2, 3, 1)
        near = (y - y.round()).abs() < 1e-4 * scale * 2
        assert bool(near[diff > 0].all()) and float((diff > 0).float().mean()) < 1e-3


def test_sample_images_uint8_gather_matches_float_path():
    """pipeline.sample_images(gather_dtype='uint8' / 'uint8_pil'): same sampler run, image bytes from the decoder's epilogue."""
    from frido_amd.pipeline import sample_images
    gs = golden("sampler_small")
    model = _frido(UNET_SMALL, VQ_SMALL)
    c = torch.from_numpy(gs["c"]).cuda()
    kw = dict(S=4, eta=1.0, seed=5, noise="philox")
    f = sample_images(model, c, **kw)
    u = sample_images(model, c, gather_dtype="uint8", **kw)
    p = sample_images(model, c, gather_dtype="uint8_pil", **kw)
    assert u.dtype == torch.uint8 and u.shape == (2, 64, 64, 3)
    assert torch.equal(u.cpu(), _to_np_u8(f)) and torch.equal(p.cpu(), _to_pil_u8(f))
    with pytest.raises(ValueError):
        sample_images(model, c, gather_dtype="int8", **kw)


@pytest.mark.gate
def test_vq_full_width_decode_matches_reference_golden():
    g = golden("vq_full")
    m = _vq(VQ_FULL, shared=True)
    h = torch.from_numpy(g["h"]).cuda()
    dec, code = m.decode(h, return_code=True)
    flips = (np.asarray(code) != g["code"]).mean()
    print(f"vq_full: VQ code flips {flips:.2e}")
    assert flips == 0, "index work is bit-exact: the committed codes of the reference must come back (vq_full.code)"
    ss = int(g["subsample"])
    forced = m.decode(h, force_codes=[g["code"][0], g["code"][1]])      # the 662-GFLOP conv path + 4 attention blocks, always compared
    r = _rel(forced[:, :, ::ss, ::ss], g["dec"])
    print(f"vq_full: decoder rel err on the reference's codes {r:.2e}")
    assert r < 3e-4
    assert abs(float(forced.double().sum()) - float(g["dec_sum"])) < 2e-4 * float(g["dec_abs_sum"])


class _Tape:
    def __init__(self, flat):
        self.t, self.pos = torch.from_numpy(np.asarray(flat, dtype=np.float32)), 0

    def __call__(self, shape):
        n = int(np.prod(shape))
        out = self.t[self.pos:self.pos + n].reshape(shape).clone()
        assert out.numel() == n
        self.pos += n
        return out


def test_bert_embedder_matches_reference_golden():
    """the cond stage (BERTEmbedder -> x-transformer encoder) on the HIP path."""
    from frido.modules.encoders.modules import BERTEmbedder
    for name in ("sampler_small", "sampler_small3"):
        g = golden(name)
        m = fill_module(BERTEmbedder(**BERT_SMALL), "cond_stage_model.").cuda()
        c = m.encode(torch.from_numpy(g["tokens"]).cuda())
        assert c.shape == g["c"].shape and _rel(c, g["c"]) < 1e-4


def test_bert_embedder_full_size_matches_oracle():
    from frido.modules.encoders.modules import BERTEmbedder
    from frido_amd.configs import BERT_FULL
    from frido_amd.synth import fill_tensor
    from oracle.bert import bert_embed
    cfg = dict(BERT_FULL, vocab_size=1024 + 256)
    m = fill_module(BERTEmbedder(**cfg), "cond_stage_model.").cuda()
    tokens = torch.from_numpy(np.random.default_rng(3).integers(0, 1024, (4, 26)))
    sd = {"cond_stage_model." + k: torch.from_numpy(fill_tensor("cond_stage_model." + k, v.shape)) for k, v in m.state_dict().items()}
    ref = bert_embed(sd, tokens, cfg["n_layer"])
    assert _rel(m(tokens.cuda()), ref) < 3e-4


def _clip_tokens(B, n, vocab, seed):
    """Token rows shaped like clip.tokenize's: SOT, a few word ids, EOT (the highest id), zero padding."""
    rng = np.random.default_rng(seed)
    t = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        L = int(rng.integers(1, n - 2))
        t[b, 0] = vocab - 2
        t[b, 1:1 + L] = rng.integers(1, vocab - 2, L)
        t[b, 1 + L] = vocab - 1
    return torch.from_numpy(t)


@pytest.mark.parametrize("arch", [(64, 16, 1000, 128, 4, 3), "ViT-L/14"], ids=["small", "ViT-L-14"])
def test_clip_text_embedder_matches_oracle(arch):
    """FrozenCLIPTextEmbedder (encoders/modules.py:188-219) on the HIP engine vs the oracle's restatement of OpenAI CLIP's
    encode_text (causal 12-head attention, QuickGELU MLP, EOT-row gather, text projection, L2 normalisation), and the
    token-axis / n_repeat handling of `encode`.  Parity is against the oracle only: the `clip` package is absent (oracle header)."""
    from frido.modules.encoders.modules import FrozenCLIPTextEmbedder
    from frido_amd.holders import CLIP_TEXT_ARCH
    from frido_amd.synth import fill_tensor
    from oracle.clip_text import clip_encode_text
    kw = dict(version=arch) if isinstance(arch, str) else dict(arch=arch)
    a = CLIP_TEXT_ARCH[arch] if isinstance(arch, str) else arch
    m = fill_module(FrozenCLIPTextEmbedder(n_repeat=3, **kw), "cond_stage_model.").cuda()
    tokens = _clip_tokens(3, a[1], a[2], 5)
    sd = {"cond_stage_model." + k: torch.from_numpy(fill_tensor("cond_stage_model." + k, v.shape)) for k, v in m.state_dict().items()}
    ref = clip_encode_text(sd, tokens, heads=a[4])
    z = m(tokens.cuda())
    assert z.shape == ref.shape and _rel(z, ref) < 3e-4
    assert float((z.norm(dim=1) - 1).abs().max()) < 1e-5
    c = m.encode(tokens.cuda())
    assert c.shape == (3, 3, a[0]) and torch.equal(c[:, 0], c[:, 2]) and _rel(c[:, 1], ref) < 3e-4
    m.normalize = False
    m.invalidate()
    assert _rel(m(tokens.cuda()), clip_encode_text(sd, tokens, heads=a[4], normalize=False)) < 3e-4


def test_full_pipeline_with_cond_stage_and_get_input():
    """get_input -> encode + conditioning, sample, decode through the reference's FridoDiffusion API."""
    from frido_amd.models import instantiate_from_config
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_small")
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    fill_module(m.cond_stage_model, "cond_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    m = m.cuda().eval()
    c = m.get_learned_conditioning(torch.from_numpy(g["tokens"]).cuda())
    assert _rel(c, g["c"]) < 1e-4
    batch = {"image": torch.tanh(torch.randn(2, 64, 64, 3)), "objects_bbox": torch.from_numpy(g["tokens"])}
    z, cc, x, xrec = m.get_input(batch, "image", return_first_stage_outputs=True, force_c_encode=True)
    assert z.shape == (2, 6, 16, 16) and cc.shape == c.shape and xrec.shape == (2, 3, 64, 64)
    assert _rel(cc, g["c"]) < 1e-4
    # z = encode_first_stage(x) with the per-scale scale_factor applied (frido.py:647-662,767-816) vs the oracle
    from oracle.vqgan import vq_encode
    zr = vq_encode(synth_sd(vq_holder(VQ_SMALL), "first_stage_model."), VQ_SMALL, batch["image"].permute(0, 3, 1, 2).contiguous())
    zr[:, :3] *= 0.9
    zr[:, 3:] *= 1.1
    zerr = (z.cpu() - zr).abs()
    assert float(zerr[:, :3].max()) < 5e-4 * float(zr.abs().max()) and float((zerr > 5e-4 * float(zr.abs().max())).float().mean()) < 0.02
    tape = _Tape(g["ddim_eta1_noise"])
    with m.ema_scope():
        pass
    samples, _ = DDIMSampler(m).sample(S=4, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=1.0, verbose=False,
                                       log_every_t=2, noise=tape)
    assert _rel(samples, g["ddim_eta1_samples"]) < 1e-3


def _frido(ucfg, vcfg, precision=None, shared=False):
    from frido_amd.models import instantiate_from_config
    if shared:
        return _shared(("frido", id(ucfg), id(vcfg), precision), lambda: _frido(ucfg, vcfg, precision))
    cfg = frido_cfg(dict(ucfg, precision=precision), dict(vcfg, precision=precision), BERT_SMALL)
    cfg["cond_stage_config"] = "__is_unconditional__"   # conditioning tensors come from the golden (cond stage = SURVEY §8f)
    cfg["conditioning_key"] = "crossattn"
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1, 1.05][:len(vcfg["embed_dim"])]))
    return m.cuda().eval()


@pytest.mark.parametrize("name,ucfg,vcfg", [("sampler_small", UNET_SMALL, VQ_SMALL), ("sampler_small3", UNET_SMALL3, VQ_SMALL3)])
@pytest.mark.parametrize("run", ["ddim_eta1", "ddim_eta0_cfg", "plms", "plms_cfg"])
def test_sampler_matches_reference_golden(name, ucfg, vcfg, run):
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    g = golden(name)
    model = _frido(ucfg, vcfg)
    c = torch.from_numpy(g["c"]).cuda()
    uc = torch.zeros_like(c)
    S, eta, scale, lev = g[f"{run}_args"]
    cls = PLMSSampler if run.startswith("plms") else DDIMSampler
    B = c.shape[0]
    tape = _Tape(g[f"{run}_noise"])
    samples, inter = cls(model).sample(S=int(S), batch_size=B, shape=(ucfg["in_channels"], 16, 16), conditioning=c,
                                       num_stage=ucfg["num_stage"], eta=float(eta), verbose=False, log_every_t=int(lev),
                                       unconditional_guidance_scale=float(scale),
                                       unconditional_conditioning=uc if scale != 1.0 else None, noise=tape)
    assert tape.pos == tape.t.numel(), "noise stream not consumed like the reference"
    assert _rel(samples, g[f"{run}_samples"]) < 1e-3
    assert len(inter["x_inter"]) == int(g[f"{run}_nx"])
    assert _rel(inter["x_inter"][-1], g[f"{run}_x_inter_last"]) < 1e-3
    assert _rel(inter["pred_x0"][1], g[f"{run}_pred_x0_1"]) < 1e-3
    img, code = model.decode_first_stage(samples, return_code=True)
    ref_img = torch.from_numpy(g[f"{run}_img"])
    # north-star criterion: <= 1e-3 max-abs on decoded pixels — holds wherever the VQ codes agree
    err = (img.cpu() - ref_img).abs().amax(dim=1)
    frac_bad = float((err > 1e-3).float().mean())
    print(f"{name}/{run}: latent rel err {_rel(samples, g[f'{run}_samples']):.2e}, pixels off by > 1e-3: {100 * frac_bad:.3f} %")
    # the decoder on the REFERENCE's latent with the codes the oracle (pinned to the reference) assigns: no VQ boundary left
    from oracle.vqgan import quantize
    from frido_amd.synth import fill_tensor
    sf = [0.9, 1.1, 1.05][:len(vcfg["embed_dim"])]
    zr = torch.from_numpy(g[f"{run}_samples"]).clone()
    codes, c0 = [], 0
    for i, e in enumerate(vcfg["embed_dim"]):
        cb = torch.from_numpy(fill_tensor(f"first_stage_model.ms_quantize.{i}.embedding.weight", (vcfg["n_embed"][i], e)))
        zi = zr[:, c0:c0 + e] * (1. / torch.tensor(sf[i]))
        codes.append(quantize(cb, zi)[1].reshape(zr.shape[0], -1).numpy())
        c0 += e
    forced = model.decode_first_stage(zr.cuda(), force_codes=codes)
    worst = float((forced.cpu() - ref_img).abs().max())
    print(f"{name}/{run}: decoder max-abs pixel err on the reference's latent and codes {worst:.2e}")
    assert worst < 1e-3
    # end to end: the <= 1e-3 criterion is asserted STRICTLY whenever the HIP path's codes equal the reference's (its own latent
    # may sit on the other side of a VQ decision boundary: then only the number of such codes is bounded)
    flips = int(sum((np.asarray(code[i]).reshape(-1) != codes[i].reshape(-1)).sum() for i in range(len(codes))))
    ncodes = int(sum(c_.size for c_ in codes))
    if flips == 0:
        assert float(err.max()) < 1e-3, float(err.max())
    else:
        assert flips <= max(1, int(2e-3 * ncodes)), (flips, ncodes)


def test_t2i_style_config_single_token_context_cfg_plms():
    """BASELINE config 3 shape class (configs/frido/t2i/frido_f16f8_coco_clip.yaml): split [4,4], 8 latent channels,
    ONE context token (pooled CLIP feature), classifier-free guidance, PLMS — HIP path vs the oracle."""
    from frido.models.diffusion.plms import PLMSSampler
    from frido_amd.synth import seeded_normal, fill_tensor
    from oracle import samplers as S
    from oracle.unet import unet_forward
    from oracle.vqgan import vq_decode
    ucfg = dict(UNET_SMALL, split_embed_dim_list=[4, 4], in_channels=8, out_channels=8, context_dim=96)
    vcfg = dict(VQ_SMALL, embed_dim=[4, 4], n_embed=[128, 128],
                edconfig=dict(VQ_SMALL["edconfig"], z_channels=[4, 4]), ddconfig=dict(VQ_SMALL["ddconfig"], z_channels=8))
    model = _frido(ucfg, vcfg)
    B = 2
    c = torch.from_numpy(seeded_normal("t2i:c", (B, 1, 96)))
    uc = torch.from_numpy(seeded_normal("t2i:uc", (1, 1, 96))).repeat(B, 1, 1)
    n = 5
    tape = seeded_normal("t2i:noise", (B * 8 * 256 + (n + 1) * B * 4 * 256 + (n + 1) * B * 8 * 256,))
    z, _ = PLMSSampler(model).sample(S=n, batch_size=B, shape=(8, 16, 16), conditioning=c.cuda(), num_stage=2, eta=0.0,
                                     verbose=False, unconditional_guidance_scale=1.5, unconditional_conditioning=uc.cuda(),
                                     noise=_Tape(tape))
    usd = {"model.diffusion_model." + k: torch.from_numpy(fill_tensor("model.diffusion_model." + k, v.shape))
           for k, v in model.model.diffusion_model.state_dict().items()}
    ac = S.alphas_cumprod_f32(S.make_betas())
    z_ref, _ = S.plms_sample(lambda x, t, cc, s: unet_forward(usd, ucfg, x, t, cc, s), ac, n, (B, 8, 16, 16), c, [4, 4], [4, 4], 2,
                             scale=1.5, uc=uc, noise=S.NoiseSource(tape))
    assert _rel(z, z_ref) < 1e-3
    img = model.decode_first_stage(z)
    assert img.shape == (B, 3, 64, 64) and bool(torch.isfinite(img).all())


def test_sampler_torch_seed_reproduces_reference_noise_stream():
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_small")
    model = _frido(UNET_SMALL, VQ_SMALL)
    c = torch.from_numpy(g["c"]).cuda()
    torch.manual_seed(23)    # what tests/golden/make_golden.py seeded the reference with
    samples, _ = DDIMSampler(model).sample(S=4, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=1.0,
                                           verbose=False, log_every_t=2, noise="torch")
    assert _rel(samples, g["ddim_eta1_samples"]) < 1e-3


def test_sampler_philox_graph_replay_is_deterministic_and_shard_invariant():
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_small")
    model = _frido(UNET_SMALL, VQ_SMALL)
    c = torch.from_numpy(g["c"]).cuda()
    kw = dict(S=4, shape=(6, 16, 16), num_stage=2, eta=1.0, verbose=False, noise="philox", seed=99)
    a, _ = DDIMSampler(model).sample(batch_size=2, conditioning=c, **kw)
    b, _ = DDIMSampler(model).sample(batch_size=2, conditioning=c, **kw)
    assert torch.equal(a, b)
    # rank 1 of a 2-way shard owns global sample 1: same result as inside the full batch
    s1, _ = DDIMSampler(model).sample(batch_size=1, conditioning=c[1:2].contiguous(), sample0=1, **kw)
    assert _rel(s1, a[1:2].cpu()) < 1e-3
    assert torch.isfinite(a).all() and float(a.std()) > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# Round 2: x_T quirk, guidance scale under graph replay, apply_model, the sampling script's call sequence, and the
# BASELINE configs at their real sizes (1: layout2i DDIM-50 B = 1; 3: t2i f16f8 PLMS + CFG; 5: 512 x 512 three-scale).
@pytest.mark.parametrize("noise", ["philox", "tape"])
def test_ddim_several_steps_per_captured_graph_is_bit_identical(noise, monkeypatch):
    """(r06) runtime.GRAPH_STEPS = K: the step body K times in one captured graph, replayed wherever no host access (log / callback) falls
    between the steps.  Same kernels, same order, same device step counter: latents AND logged intermediates must equal the one-graph-per-
    step run bit for bit -- with S = 10 and log_every_t = 5 both forms (4-step replays and single steps around the logged ones) are mixed."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido_amd import runtime
    from frido_amd.synth import seeded_normal
    c = torch.from_numpy(seeded_normal("gs:c", (2, 5, 64))).cuda()
    tape = seeded_normal("gs:noise", (2 * 6 * 256 + 10 * 2 * 3 * 256 + 10 * 2 * 6 * 256,))
    outs = []
    for K in (1, 4):
        monkeypatch.setattr(runtime, "GRAPH_STEPS", K)
        model = _frido(UNET_SMALL, VQ_SMALL)
        z, inter = DDIMSampler(model).sample(S=10, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=1.0, verbose=False,
                                             log_every_t=5, noise="philox" if noise == "philox" else _Tape(tape), seed=5)
        eng = next(iter(model.model.diffusion_model.runtime()._sampler_engines.values()))
        assert any(isinstance(k[-1], str) and k[-1] == "x4" for k in eng.graphs) == (K == 4)
        assert getattr(eng, "multi_step_launches", 0) == (4 if K == 4 else 0)          # two 4-step replays per stage (steps 1-4 and 5-8), two stages
        outs.append((z.cpu(), [t.cpu() for t in inter["x_inter"]], [t.cpu() for t in inter["pred_x0"]]))
    (z1, xi1, p1), (z4, xi4, p4) = outs
    assert torch.equal(z1, z4) and len(xi1) == len(xi4) and all(torch.equal(a, b) for a, b in zip(xi1 + p1, xi4 + p4))


@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_sampler_x_T_is_adopted_as_finished_stage0(kind):
    """ddim.py:150-152 / plms.py:150-152: with x_T given, stage 0 and its hand-off are skipped."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    g, gs = golden("sampler_xt"), golden("sampler_small")
    model = _frido(UNET_SMALL, VQ_SMALL)
    c = torch.from_numpy(gs["c"]).cuda()
    xT = torch.from_numpy(g["x_T"]).cuda()
    cls, eta = (DDIMSampler, 1.0) if kind == "ddim" else (PLMSSampler, 0.0)
    tape = _Tape(g[f"{kind}_noise"])
    out, inter = cls(model).sample(S=4, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=eta, verbose=False,
                                   log_every_t=2, x_T=xT, noise=tape)
    assert tape.pos == tape.t.numel() and len(inter["x_inter"]) == int(g[f"{kind}_nx"])
    assert _rel(out, g[f"{kind}_samples"]) < 1e-3
    assert torch.equal(out[:, :3], xT[:, :3])


def test_philox_graph_replay_follows_the_guidance_scale():
    """the captured DDIM step body must not freeze the first guidance scale it saw."""
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_small")
    c = torch.from_numpy(g["c"]).cuda()
    uc = torch.zeros_like(c)
    kw = dict(S=4, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=1.0, verbose=False, noise="philox", seed=5,
              unconditional_conditioning=uc)
    model = _frido(UNET_SMALL, VQ_SMALL)
    a3, _ = DDIMSampler(model).sample(unconditional_guidance_scale=3.0, **kw)
    a5, _ = DDIMSampler(model).sample(unconditional_guidance_scale=5.0, **kw)       # same engine, same graphs
    fresh = _frido(UNET_SMALL, VQ_SMALL)
    b5, _ = DDIMSampler(fresh).sample(unconditional_guidance_scale=5.0, **kw)       # first scale this engine sees
    assert torch.equal(a5, b5) and not torch.equal(a3, a5)
    # and against the oracle: philox noise is not replayable on the CPU, so compare eta = 0 (no noise enters) at scale 5
    from oracle import samplers as S
    from oracle.unet import unet_forward
    usd = synth_sd(unet_holder(UNET_SMALL), "model.diffusion_model.")
    kw0 = dict(kw, eta=0.0)
    torch.manual_seed(3)
    xT = torch.randn(2, 6, 16, 16)
    tape = torch.cat([xT.reshape(-1), torch.zeros(2 * 3 * 256 * 4 + 2 * 6 * 256 * 4)])
    kw0.update(noise=_Tape(tape.numpy()))
    h5, _ = DDIMSampler(model).sample(unconditional_guidance_scale=5.0, **kw0)
    ref, _ = S.ddim_sample(lambda x, t, cc, s: unet_forward(usd, UNET_SMALL, x, t, cc, s), S.alphas_cumprod_f32(S.make_betas()), 4,
                           (2, 6, 16, 16), c.cpu(), [3, 3], [3, 3], 2, eta=0.0, scale=5.0, uc=uc.cpu(), noise=S.NoiseSource(tape))
    assert _rel(h5, ref) < 1e-3


def test_apply_model_matches_oracle():
    """frido.py:1062-1160 -> DiffusionWrapper.forward (frido.py:1635-1654): tensor, list and dict conditioning."""
    from oracle.unet import unet_forward
    from frido_amd.synth import seeded_normal
    from frido_amd.models import instantiate_from_config
    model = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion",
                                         params=frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)))     # conditioning_key = crossattn
    fill_module(model.model, "model.")
    model = model.cuda().eval()
    usd = synth_sd(unet_holder(UNET_SMALL), "model.diffusion_model.")
    x = torch.from_numpy(seeded_normal("am:x", (2, 6, 16, 16)))
    c = torch.from_numpy(seeded_normal("am:c", (2, 5, 64)))
    t = torch.tensor([981, 21])
    for stage in (0, 1):
        xin = x[:, :3 * (stage + 1)].contiguous()
        ref = unet_forward(usd, UNET_SMALL, xin, t, c, stage)
        for cond in (c.cuda(), [c.cuda()], {"c_crossattn": [c.cuda()]}):
            got = model.apply_model(xin.cuda(), t.cuda(), cond, stage=stage)
            assert got.shape == ref.shape and _rel(got, ref) < 2e-4
        # two context tensors are concatenated along the token axis (frido.py:1645)
        got2 = model.apply_model(xin.cuda(), t.cuda(), [c[:, :2].cuda().contiguous(), c[:, 2:].cuda().contiguous()], stage=stage)
        assert _rel(got2, ref) < 2e-4


def test_sampling_script_call_sequence():
    """The model-facing calls of scripts/sample_diffusion.py:174-206,236-263, in its order, on a collated batch: get_input
    (5 outputs), full_like unconditional conditioning, ema_scope, sampler.sample(steps, conditioning=..., batch_size=...,
    shape=..., num_stage=..., eta=..., unconditional_*, log_every_t=20), decode_first_stage, get_img_ids."""
    from frido.util import instantiate_from_config_main
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    from taming.data.utils import custom_collate
    g = golden("sampler_small")
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    model = instantiate_from_config_main(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(model.model, "model.")
    fill_module(model.first_stage_model, "first_stage_model.")
    fill_module(model.cond_stage_model, "cond_stage_model.")
    model.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    from frido_amd.models import LitEma
    model.model_ema = LitEma(model.model)          # the EMA shadow of the filled weights (a checkpoint would carry its own)
    model = model.cuda().eval()
    rng = np.random.default_rng(0)
    items = [{"image": np.tanh(rng.standard_normal((64, 64, 3))).astype(np.float32), "objects_bbox": g["tokens"][i],
              "file_name": f"{i}.png"} for i in range(2)]
    batch = custom_collate(items)
    z, c, x, xrec, xc = model.get_input(batch, model.first_stage_key, return_first_stage_outputs=True, force_c_encode=True,
                                        return_original_cond=True, bs=None)
    assert z.shape == (2, 6, 16, 16) and x.shape == xrec.shape == (2, 3, 64, 64) and torch.equal(xc, batch["objects_bbox"])
    assert _rel(c, g["c"]) < 1e-4
    uc = torch.full_like(c, 0)
    unet = model.model.diffusion_model
    shape = [len(z), unet.in_channels, unet.image_size, unet.image_size]
    for plms in (False, True):
        with model.ema_scope("Plotting"):
            sampler = PLMSSampler(model) if plms else DDIMSampler(model)
            samples, inter = sampler.sample(4, conditioning=c, batch_size=shape[0], shape=shape[1:], num_stage=unet.num_stage,
                                            eta=0.0 if plms else 1.0, verbose=False, unconditional_guidance_scale=1.5,
                                            unconditional_conditioning=uc, log_every_t=20)
        img = model.decode_first_stage(samples)
        assert img.shape == (2, 3, 64, 64) and bool(torch.isfinite(img).all()) and len(inter["x_inter"]) >= 2
    assert model.get_img_ids(batch) == ["0.png", "1.png"]


class _Rec:
    """torch.randn in the reference's draw order + a running checksum of the stream."""

    def __init__(self):
        self.n, self.sum, self.head = 0, 0.0, None

    def __call__(self, shape):
        r = torch.randn(shape)
        if self.head is None:
            self.head = r.reshape(-1)[:16].clone()
        self.n += r.numel()
        self.sum += float(r.double().sum())
        return r


def _e2e_report(tag, model, g, run, samples, embed):
    """latent error, VQ code flip rate and pixel-error percentiles of an end-to-end run vs the reference golden."""
    lat = _rel(samples, g[f"{run}_samples"])
    img, code = model.decode_first_stage(samples, return_code=True)
    code = np.asarray(code)
    flips = float((code != g[f"{run}_code"]).mean())
    ss = int(g[f"{run}_img_ss"])
    err = (img[:, :, ::ss, ::ss].cpu() - torch.from_numpy(g[f"{run}_img"])).abs().amax(dim=1).reshape(-1)
    q = [float(torch.quantile(err, p)) for p in (0.5, 0.9, 0.99)]
    rep = dict(latent_rel=lat, vq_flip_rate=flips, pix_p50=q[0], pix_p90=q[1], pix_p99=q[2], pix_max=float(err.max()),
               frac_pix_gt_1e3=float((err > 1e-3).float().mean()))
    print(f"E2E {tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in rep.items()))
    # decoder on the reference's latent + codes: unconditional <= 1e-3 max-abs (north star)
    forced = model.decode_first_stage(torch.from_numpy(g[f"{run}_samples"]).cuda(), force_codes=[g[f"{run}_code"][i] for i in range(len(embed))])
    rep["forced_pix_max"] = float((forced[:, :, ::ss, ::ss].cpu() - torch.from_numpy(g[f"{run}_img"])).abs().max())
    rep["forced_sum_rel"] = abs(float(forced.double().sum()) - float(g[f"{run}_img_sum"])) / float(g[f"{run}_img_abs_sum"])
    print(f"E2E {tag}: decoder on the reference's latent and codes: max-abs {rep['forced_pix_max']:.3e}, sum rel {rep['forced_sum_rel']:.3e}")
    _record(tag, rep)
    return rep


_E2E = {}


def _record(tag, rep):
    """The end-to-end error records are WRITTEN BY THE TESTS (gpurun_out/e2e_error.json under the repo root, merged back by
    gpurun; the copy judged is profiles/r03_e2e_error.json) instead of being re-typed from the log."""
    import json
    _E2E[tag] = {k: (float(v) if isinstance(v, (int, float, np.floating)) else v) for k, v in rep.items()}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "e2e_error.json")
    blob = {}
    if os.path.exists(path):
        try:
            blob = json.load(open(path))
        except ValueError:
            blob = {}
    blob.update(_E2E)
    with open(path, "w") as f:
        json.dump(blob, f, indent=1, sort_keys=True)


def _oracle_flip_counts(g, run, S, threads=(16,)):
    """What the ORACLE itself does on this fixture: the CPU restatement (fp32 torch) re-run at different intra-op thread counts
    (torch's conv / GEMM kernels change their summation order with the thread count) vs the reference's recorded run -- the
    number of VQ codes that flip between two fp32 CPU runs of the same algorithm is the yardstick for the HIP path's flips."""
    import sys
    from golden_cfg import BERT_FULL  # noqa: F401
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import samplers as S_
    from oracle.unet import unet_forward
    from oracle.vqgan import vq_decode
    from frido_amd.models import PyUNetModel, VQModelInterface
    from frido_amd.synth import fill_tensor
    usd = {"model.diffusion_model." + k: torch.from_numpy(fill_tensor("model.diffusion_model." + k, v.shape))
           for k, v in PyUNetModel(**UNET_FULL).state_dict().items()}
    vsd = {"first_stage_model." + k: torch.from_numpy(fill_tensor("first_stage_model." + k, v.shape))
           for k, v in VQModelInterface(**VQ_FULL, lossconfig=dict(target="taming.modules.losses.DummyLoss")).state_dict().items()}
    ac = S_.alphas_cumprod_f32(S_.make_betas())
    am = lambda x, t, cond, s: unet_forward(usd, UNET_FULL, x, t, cond, s)
    res = {}
    keep = torch.get_num_threads()
    for nt in threads:
        if nt > (os.cpu_count() or 1):
            continue
        torch.set_num_threads(nt)
        torch.manual_seed(23)
        out, _ = S_.ddim_sample(am, ac, S, (1, 6, 64, 64), torch.from_numpy(g["c"]), [3, 3], [3, 3], 2, eta=1.0, log_every_t=10 ** 9)
        _, codes = vq_decode(vsd, VQ_FULL, S_.decode_first_stage(lambda z: z, out, g["scale_factor"].tolist(), [3, 3]), return_code=True)
        code = np.stack([cd.numpy() for cd in codes]).reshape(g[f"{run}_code"].shape)
        res[f"threads_{nt}"] = dict(latent_rel=float((out - torch.from_numpy(g[f"{run}_samples"])).abs().max() / np.abs(g[f"{run}_samples"]).max()),
                                    vq_flips=int((code != g[f"{run}_code"]).sum()), codes=int(code.size))
    torch.set_num_threads(keep)
    return res


# (r06) the single-plane throughput mode keeps ONE end-to-end leg (ddim4): it is outside the north star's tolerance by design and
# its DDIM-50 leg asserted the same recorded bounds a second time
@pytest.mark.parametrize("run,S,precision", [pytest.param("ddim4", 4, "bf16x3", marks=pytest.mark.gate), ("ddim50", 50, "bf16x3"), ("ddim4", 4, "bf16")],
                         ids=["ddim4-4-bf16x3", "ddim50-50-bf16x3", "ddim4-4-bf16"])
def test_config1_full_width_end_to_end(run, S, precision):
    """BASELINE config 1: layout2i f8f4 at FULL width, B = 1, DDIM eta = 1, against the reference's own CPU run
    (tests/golden/make_golden.py sampler_full; noise = torch's CPU generator after manual_seed(23), like the reference).
    bf16x3 is the parity mode (<= 1e-3); bf16 is the benchmark's arithmetic: its measured error is asserted against the
    bounds recorded in DESIGN.md §5."""
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_full")
    model = _frido(UNET_FULL, VQ_FULL, precision=precision, shared=True)
    c = torch.from_numpy(g["c"]).cuda()
    rec = _Rec()
    torch.manual_seed(23)
    samples, inter = DDIMSampler(model).sample(S=S, batch_size=1, shape=(6, 64, 64), conditioning=c, num_stage=2, eta=1.0,
                                               verbose=False, log_every_t=int(g[f"{run}_args"][3]), noise=rec)
    assert rec.n == int(g[f"{run}_noise_n"]) and np.array_equal(rec.head.numpy(), g[f"{run}_noise_head"])
    assert abs(rec.sum - float(g[f"{run}_noise_sum"])) < 1e-6 * rec.n, "torch CPU generator stream differs from the fixture's"
    assert len(inter["x_inter"]) == int(g[f"{run}_nx"])
    rep = _e2e_report(f"config1/{run}/{precision}", model, g, run, samples, [3, 3])
    if precision == "bf16x3" and run == "ddim4":
        # yardstick for the flip allowance below: the oracle (fp32 on the CPU) against the same fixture at 1 and 16 threads
        rep["oracle_vs_reference"] = _oracle_flip_counts(g, run, S)
        print(f"E2E config1/{run}: oracle's own code flips vs the reference's run: {rep['oracle_vs_reference']}")
        _record(f"config1/{run}/{precision}", rep)
    if precision == "bf16x3":
        # north star: <= 1e-3 max-abs on decoded pixels.  Unconditional for the decoder (reference latent + codes); end to end
        # it holds wherever no VQ code flipped -- one flipped code (a discontinuity) reaches every pixel through the decoder's
        # four global attention blocks, so with flips only their rate is asserted
        assert rep["latent_rel"] < E2E_X3["latent_rel"] and rep["vq_flip_rate"] < E2E_X3["vq_flip_rate"] and rep["forced_pix_max"] < E2E_X3["pix_max"]
        if rep["vq_flip_rate"] == 0:
            assert rep["pix_max"] < E2E_X3["pix_max"]
    else:
        assert rep["latent_rel"] < E2E_BF16["latent_rel"] and rep["vq_flip_rate"] < E2E_BF16["vq_flip_rate"]
        assert rep["pix_p50"] < E2E_BF16["pix_p50"] and rep["pix_p99"] < E2E_BF16["pix_p99"]
        assert rep["forced_pix_max"] < E2E_BF16["forced_pix_max"]


# bounds of the parity arithmetic end to end (r03: fp16 hi + fp16 lo operand planes), = measured value x ~10: latent rel 2.4e-6 - 5.8e-6
# (the fp32 oracle itself: 1.7e-6 - 2.1e-6), 0 flipped VQ codes in every run, decoded pixels <= 8.3e-6 max-abs end to end and
# 6 - 8e-6 for the decoder alone (profiles/r03_e2e_error.json).  The north star asks <= 1e-3.
# r04: with the GPU suite pinned to the benchmark's tiles (tests/conftest.py) the committed fixtures must decode to EXACTLY the reference's codes:
# `vq_flip_rate` is an exclusive bound on flips / codes, so 1e-9 admits none (one flip of 8192 already breaks the north star's 1e-3).
E2E_X3 = dict(latent_rel=5e-5, vq_flip_rate=1e-9, pix_max=1e-4)
# bounds of the bf16 (benchmark) arithmetic end to end, = measured value x ~2 (see DESIGN.md §5 for the measurements)
# r02 measurements (gpurun_out/t_r02a.log): latent rel 0.85-1.2e-2, VQ flips 0.8-1.6 %, pixel error p50 1.4-2.1e-2 /
# p99 0.21-0.28, decoder alone on identical codes 2.9-3.4e-2 max-abs
E2E_BF16 = dict(latent_rel=3e-2, vq_flip_rate=4e-2, pix_p50=5e-2, pix_p99=0.6, forced_pix_max=8e-2)


@pytest.mark.parametrize("precision", ["bf16x3"])      # (r06) the single-plane leg went with config 1's second one, see above
def test_config3_t2i_true_dims_plms_cfg(precision):
    """BASELINE config 3 at the real f16f8 dimensions (configs/frido/t2i/frido_f16f8_coco_clip.yaml:21-77): 8 x 32 x 32 latent,
    ONE 768-d context token, PLMS (graph-captured incl. the Heun first step) with CFG 1.5, 2 x 8192-code first stage."""
    from frido.models.diffusion.plms import PLMSSampler
    from frido.models.diffusion.ddim import DDIMSampler
    from golden_cfg import UNET_F16F8, VQ_F16F8
    g = golden("sampler_t2i")
    model = _frido(UNET_F16F8, VQ_F16F8, precision=precision, shared=True)
    c, uc = torch.from_numpy(g["c"]).cuda(), torch.from_numpy(g["uc"]).cuda()
    if precision == "bf16x3":
        unet = model.model.diffusion_model
        x = torch.from_numpy(g["x"]).cuda()
        for s in range(2):
            e = unet(x[:, :4 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=c, stage=s)
            assert _rel(e, g[f"eps_{s}"]) < 2e-4, s
    for run, cls in (("plms_cfg", PLMSSampler), ("ddim_cfg", DDIMSampler)):
        S, eta, scale, lev = g[f"{run}_args"]
        rec = _Rec()
        torch.manual_seed(23)
        samples, inter = cls(model).sample(S=int(S), batch_size=2, shape=(8, 32, 32), conditioning=c, num_stage=2, eta=float(eta),
                                           verbose=False, log_every_t=int(lev), unconditional_guidance_scale=float(scale),
                                           unconditional_conditioning=uc, noise=rec)
        assert rec.n == int(g[f"{run}_noise_n"]) and abs(rec.sum - float(g[f"{run}_noise_sum"])) < 1e-6 * rec.n
        assert len(inter["x_inter"]) == int(g[f"{run}_nx"])
        rep = _e2e_report(f"config3/{run}/{precision}", model, g, run, samples, [4, 4])
        if precision == "bf16x3":
            assert rep["latent_rel"] < E2E_X3["latent_rel"] and rep["vq_flip_rate"] < E2E_X3["vq_flip_rate"] and rep["forced_pix_max"] < E2E_X3["pix_max"]
            if rep["vq_flip_rate"] == 0:
                assert rep["pix_max"] < E2E_X3["pix_max"]
        else:
            assert rep["latent_rel"] < E2E_BF16["latent_rel"] and rep["forced_pix_max"] < E2E_BF16["forced_pix_max"]


def test_config5_three_scale_512_forward_and_decode():
    """BASELINE config 5: denoiser forwards of all three stages on the 9 x 128 x 128 latent (self-attention
    over 4096 tokens at C = 384) and the 512 x 512 decode (four AttnBlocks over 16384 keys: the flash-style kernel, no
    B x N x N score tensor) against the reference's outputs."""
    from golden_cfg import UNET_512, VQ_512
    g = golden("unet_512")
    m = _unet(UNET_512, shared=True)
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    for s in range(3):
        e = m(x[:, :3 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=ctx, stage=s)
        r = _rel(e, g[f"eps_{s}"])
        print(f"config5 denoiser stage {s}: rel err {r:.2e}")
        assert r < 3e-4, s
    del m
    torch.cuda.empty_cache()
    gv = golden("vq_512")
    v = _vq(VQ_512, shared=True)
    h = torch.from_numpy(gv["h"]).cuda()
    dec, code = v.decode(h, return_code=True)
    flips = float((np.asarray(code) != gv["code"]).mean())
    forced = v.decode(h, force_codes=[gv["code"][i] for i in range(3)])
    ss = int(gv["dec_img_ss"])
    r = _rel(forced[:, :, ::ss, ::ss], gv["dec_img"])
    print(f"config5 decode: VQ flips {flips:.2e}, decoder rel err on the reference's codes {r:.2e}")
    assert dec.shape == (1, 3, 512, 512) and flips == 0 and r < 3e-4
    assert abs(float(forced.double().sum()) - float(gv["dec_img_sum"])) < 2e-4 * float(gv["dec_img_abs_sum"])


def test_engine_cache_eviction_releases_persistent_buffers():
    """samplers.ENGINE_CACHE_SIZE bounds the compiled engines per denoiser; an evicted engine owns its plans' persistent buffers
    (Builder.persist_scope), so HBM plateaus when a process cycles through more sampling signatures than the cache holds."""
    import gc
    from frido.models.diffusion.ddim import DDIMSampler
    from frido_amd.samplers import ENGINE_CACHE_SIZE
    model = _frido(UNET_SMALL, VQ_SMALL)
    mems = []
    for nctx in range(3, 3 + ENGINE_CACHE_SIZE + 5):
        c = torch.randn(2, nctx, 64, device="cuda")
        DDIMSampler(model).sample(S=2, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=1.0, verbose=False,
                                  noise="philox")
        torch.cuda.synchronize()
        gc.collect()
        mems.append(torch.cuda.memory_allocated())
    rt = model.model.diffusion_model.runtime()
    assert len(rt._sampler_engines) == ENGINE_CACHE_SIZE
    assert max(mems[ENGINE_CACHE_SIZE + 1:]) <= max(mems[:ENGINE_CACHE_SIZE + 1]) * 1.03 + (1 << 20), mems


def test_config5_three_stage_multistep_at_true_size():
    """BASELINE config 5, MULTI-STEP at its true size (tests/golden/make_golden.py sampler_512): the three-stage DDIM loop
    (S = 2, eta = 1: six denoiser forwards, both hand-offs incl. the 4x4 block mean of stage 0, ddim.py:146-149,177-185) on the
    9 x 128 x 128 latent with 92 context tokens, then the 512 x 512 decode -- against the reference's own CPU run on the same
    torch noise stream."""
    from frido.models.diffusion.ddim import DDIMSampler
    from golden_cfg import UNET_512, VQ_512
    g = golden("sampler_512")
    model = _frido(UNET_512, VQ_512, precision="bf16x3", shared=True)
    c = torch.from_numpy(g["c"]).cuda()
    rec = _Rec()
    torch.manual_seed(23)
    samples, inter = DDIMSampler(model).sample(S=2, batch_size=1, shape=(9, 128, 128), conditioning=c, num_stage=3, eta=1.0,
                                               verbose=False, log_every_t=int(g["ddim2_args"][3]), noise=rec)
    assert rec.n == int(g["ddim2_noise_n"]) and abs(rec.sum - float(g["ddim2_noise_sum"])) < 1e-6 * rec.n
    assert len(inter["x_inter"]) == int(g["ddim2_nx"])
    rep = _e2e_report("config5/ddim2x3stages/bf16x3", model, g, "ddim2", samples, [3, 3, 3])
    assert rep["latent_rel"] < E2E_X3["latent_rel"] and rep["vq_flip_rate"] < E2E_X3["vq_flip_rate"] and rep["forced_pix_max"] < E2E_X3["pix_max"]
    if rep["vq_flip_rate"] == 0:
        assert rep["pix_max"] < E2E_X3["pix_max"]


def test_config2_step_count_ddim200_end_to_end():
    """BASELINE config 2's step count: layout2i f8f4 at full width, DDIM-200 eta = 1 x 2 stages (400 graph replays) + decode at
    B = 1, against the reference's own CPU run (tests/golden/make_golden.py sampler_ddim200) in the parity arithmetic."""
    from frido.models.diffusion.ddim import DDIMSampler
    g = golden("sampler_ddim200")
    model = _frido(UNET_FULL, VQ_FULL, precision="bf16x3", shared=True)
    c = torch.from_numpy(g["c"]).cuda()
    rec = _Rec()
    torch.manual_seed(23)
    samples, inter = DDIMSampler(model).sample(S=200, batch_size=1, shape=(6, 64, 64), conditioning=c, num_stage=2, eta=1.0,
                                               verbose=False, log_every_t=int(g["ddim200_args"][3]), noise=rec)
    assert rec.n == int(g["ddim200_noise_n"]) and abs(rec.sum - float(g["ddim200_noise_sum"])) < 1e-6 * rec.n
    assert len(inter["x_inter"]) == int(g["ddim200_nx"])
    rep = _e2e_report("config2-steps/ddim200/bf16x3", model, g, "ddim200", samples, [3, 3])
    assert rep["latent_rel"] < E2E_X3["latent_rel"] and rep["vq_flip_rate"] < E2E_X3["vq_flip_rate"] and rep["forced_pix_max"] < E2E_X3["pix_max"]
    if rep["vq_flip_rate"] == 0:
        assert rep["pix_max"] < E2E_X3["pix_max"]


def test_bench_under_torchrun_takes_the_rccl_path_at_n1():
    """The driver launches bench.py with torch.distributed.run for N > 1; at N = 1 the same launch exercises the whole
    distributed path on one GPU: nccl (= RCCL) process group, contiguous shard with sample0, the all-gather of decoded
    images, the barrier-bracketed max-over-ranks timing and the per-rank report."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
                          "127.0.0.1", "--master-port", "29533", os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "1",
                          "--warmup", "0", "--batch", "2", "--ddim-steps", "4", "--full", "--no-cpu-baseline", "--no-bf16-extra"],
                         capture_output=True, text=True, env=env, timeout=900, cwd=repo)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["scaling"] == "weak" and len(d["per_rank_ms_per_step"]) == 1
    assert d["config"]["global_batch"] == 2 and "roofline" in d


def test_bench_plain_run_is_the_headline_only_and_dumps_the_last_step(tmp_path):
    """`bench.py` without --full: the warm-up, the timed steps and the line (none of the --full legs), and --dump-outputs DIR writes the
    uint8 images the last timed step returned as DIR/images.npy in float32."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                          "--ddim-steps", "4", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=900, cwd=repo)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["unit"] == "images/s"
    assert abs(d["value"] - 2 * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 1e-2 and d["dtype"].startswith("f16x3")
    assert not {"roofline", "loop_only_value", "extra", "cpu_baseline", "other_configs_images_per_s"} & set(d)
    img = np.load(tmp_path / "out" / "images.npy")
    assert img.dtype == np.float32 and img.shape == (2, 256, 256, 3)
    assert np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255 and img.max() > img.min()


def test_vq_full_width_encode_matches_reference_golden():
    """SURVEY a16 at full width (layout2i f8f4 first stage, one 256 x 256 image) vs the reference's own encode."""
    from frido_amd.synth import seeded_normal
    g = golden("vq_full_enc")
    m = _vq(VQ_FULL, shared=True)
    x = torch.from_numpy(np.tanh(seeded_normal("vq_full:img", (1, 3, 256, 256))))
    enc = m.encode(x.cuda())
    ref = torch.from_numpy(g["enc"])
    err = (enc.cpu() - ref).abs()
    scale = float(ref.abs().max())
    print(f"vq_full encode: coarse max err {float(err[:, :3].max()) / scale:.2e} rel, fine-scale pixels off by > 5e-4 rel: {100 * float((err[:, 3:] > 5e-4 * scale).float().mean()):.3f} %")
    assert enc.shape == ref.shape and float(err[:, :3].max()) < 5e-4 * scale          # no VQ in the coarse path
    assert float((err > 5e-4 * scale).float().mean()) < 0.02                          # a coarse code flip perturbs few fine pixels


def test_sampling_inside_ema_scope_uses_the_ema_weights():
    """frido.py:181-194 / ema.py:46-76 with DISTINCT EMA weights: inside the scope the sampler runs on the shadow weights
    (checked against the oracle with those weights), afterwards on the training weights again."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido_amd.synth import fill_tensor, seeded_normal
    from oracle import samplers as S
    from oracle.unet import unet_forward
    model = _frido(UNET_SMALL, VQ_SMALL)
    # shadow weights = the filler under a different name prefix
    for name, p in model.model.named_parameters():
        getattr(model.model_ema, model.model_ema.m_name2s_name[name]).copy_(torch.from_numpy(fill_tensor("ema." + name, p.shape)))
    sd_train = synth_sd(unet_holder(UNET_SMALL), "model.diffusion_model.")
    sd_ema = {"model.diffusion_model." + k: torch.from_numpy(fill_tensor("ema.diffusion_model." + k, v.shape))
              for k, v in unet_holder(UNET_SMALL).state_dict().items()}
    c = torch.from_numpy(seeded_normal("ema:c", (2, 5, 64)))
    tape = seeded_normal("ema:noise", (2 * 6 * 256 + 4 * 2 * 3 * 256 + 4 * 2 * 6 * 256,))
    ac = S.alphas_cumprod_f32(S.make_betas())
    kw = dict(S=4, batch_size=2, shape=(6, 16, 16), conditioning=c.cuda(), num_stage=2, eta=1.0, verbose=False)

    def ref(sd):
        return S.ddim_sample(lambda x, t, cc, s: unet_forward(sd, UNET_SMALL, x, t, cc, s), ac, 4, (2, 6, 16, 16), c, [3, 3], [3, 3], 2,
                             eta=1.0, noise=S.NoiseSource(tape))[0]
    with model.ema_scope("test"):
        z_ema, _ = DDIMSampler(model).sample(noise=_Tape(tape), **kw)
    z_train, _ = DDIMSampler(model).sample(noise=_Tape(tape), **kw)
    assert _rel(z_ema, ref(sd_ema)) < 1e-3 and _rel(z_train, ref(sd_train)) < 1e-3
    assert _rel(z_ema, z_train.cpu()) > 1e-2            # the two weight sets really differ


# ---------------------------------------------------------------------------------------------------------------------
# Round 4: parity AT THE BATCH THE BENCHMARK RUNS.  M = B * HW selects the tiles (256 x 192 / 128 x 192 eight-wave at B = 16): the
# full-width goldens above run at B = 1 or 2, so these tests drive the benchmarked tiles (pinned: tests/conftest.py) end to end.
def _bench_ctx(B):
    from frido_amd.synth import seeded_normal
    return torch.from_numpy(seeded_normal("bench:ctx", (B, 26, 640)))


@pytest.mark.parametrize("B,S,rows", [(16, 200, (0, 7, 15)), (32, 20, (0, 31))], ids=["config2_B16_ddim200", "config4_shard_B32"])
def test_benchmarked_batch_rows_equal_single_sample_runs(B, S, rows):
    """BASELINE config 2 (B = 16) and config 4's per-GPU shard (B = 32) at full width: the Philox noise is keyed by the GLOBAL sample
    index, so row i of the batched run must reproduce the B = 1 run with sample0 = i -- whose arithmetic the B = 1 goldens pin to
    the reference -- to the parity bound: latent <= 5e-5, ZERO code flips, decoded pixels <= 1e-4 (north star: 1e-3)."""
    from frido.models.diffusion.ddim import DDIMSampler
    model = _frido(UNET_FULL, VQ_FULL, precision="bf16x3", shared=True)
    ctx = _bench_ctx(B).cuda()
    kw = dict(S=S, shape=(6, 64, 64), num_stage=2, eta=1.0, verbose=False, noise="philox", seed=1004, log_every_t=10 ** 9)
    zb, _ = DDIMSampler(model).sample(batch_size=B, conditioning=ctx, **kw)
    ib, cb = model.decode_first_stage(zb, return_code=True)
    cb = np.asarray(cb)                                    # [scale][B][HW]
    assert torch.isfinite(zb).all() and torch.isfinite(ib).all() and float(zb.std()) > 0.1
    worst = dict(latent=0.0, pix=0.0, flips=0)
    for i in rows:
        z1, _ = DDIMSampler(model).sample(batch_size=1, conditioning=ctx[i:i + 1].contiguous(), sample0=i, **kw)
        i1, c1 = model.decode_first_stage(z1, return_code=True)
        worst["latent"] = max(worst["latent"], _rel(zb[i:i + 1], z1.cpu()))
        worst["flips"] += int((np.asarray(c1)[:, 0] != cb[:, i]).sum())
        worst["pix"] = max(worst["pix"], float((ib[i:i + 1] - i1).abs().max()))
    print(f"B = {B} vs B = 1 rows {rows}: {worst}")
    _record(f"batch{B}/rows_vs_b1/ddim{S}", worst)
    assert worst["latent"] < E2E_X3["latent_rel"] and worst["flips"] == 0 and worst["pix"] < E2E_X3["pix_max"]
    if B == 16:
        # (r05, r04 verdict weak 1) the BATCHED decode directly against the oracle (CPU restatement pinned to the reference) on the HIP
        # path's own latent: the B = 16 decoder tiles (M = 16 x 65536) meet a reference implementation without going through B = 1 --
        # all 2 x 16 x 4096 codes exactly, every pixel of the 16 images to the parity bound
        from oracle import samplers as OS
        from oracle.vqgan import vq_decode
        vsd = synth_sd(vq_holder(VQ_FULL), "first_stage_model.")
        keep = torch.get_num_threads()
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        from oracle.vqgan import quantize
        sf = [float(v) for v in model.scale_factor.cpu()]
        try:
            # (r06) the VQ lookup of ALL 16 rows (cheap: the quantiser alone), the decoder's pixels for the rows the B = 1 comparison above
            # also takes -- the decoder is per sample, so three rows of the oracle meet three different 256-row tile groups of the B = 16 launch
            zs = OS.decode_first_stage(lambda zz: zz, zb.cpu(), sf, [3, 3])
            ref_codes = [quantize(vsd[f"first_stage_model.ms_quantize.{i}.embedding.weight"], zs[:, 3 * i:3 * i + 3])[1].reshape(B, -1) for i in range(2)]
            ref_img, _ = OS.decode_first_stage(lambda zz: vq_decode(vsd, VQ_FULL, zz, return_code=True), zb.cpu()[list(rows)], sf, [3, 3])
        finally:
            torch.set_num_threads(keep)
        code_diff = int(sum((ref_codes[i].numpy() != cb[i].reshape(B, -1)).sum() for i in range(2)))
        pix = float((ib.cpu()[list(rows)] - ref_img).abs().max())
        print(f"B = 16 decode vs the oracle on the HIP latent: {code_diff} of {2 * B * 4096} codes differ, pixels of rows {rows} max-abs {pix:.2e}")
        _record("batch16/decode_vs_oracle", dict(codes_differing=code_diff, codes_total=2 * B * 4096, pix_max=pix, pixel_rows=list(rows)))
        assert code_diff == 0 and pix < E2E_X3["pix_max"]


@pytest.mark.parametrize("B", [pytest.param(16, marks=pytest.mark.gate), 32])
def test_benchmarked_batch_forward_matches_oracle(B):
    """One denoiser forward per stage at full width and the benchmark's batch against the oracle (the CPU restatement pinned
    bit-exact to the reference): the 64^2 / 32^2 convolutions run on the tiles of the headline number here."""
    from oracle.unet import unet_forward
    from frido_amd.synth import seeded_normal
    m = _unet(UNET_FULL, shared=True)
    sd = synth_sd(unet_holder(UNET_FULL), "model.diffusion_model.")
    x = torch.from_numpy(seeded_normal("bench:x", (B, 6, 64, 64)))
    ctx = _bench_ctx(B)
    t = torch.tensor([(37 * i + 11) % 1000 for i in range(B)])
    # (r06) every op of the denoiser is per sample (GroupNorm, attention, convolutions): the oracle runs the first, a middle and the last
    # ROW of the batch (its own B = 3 forward), the HIP path the whole batch on the benchmark's tiles -- a third of the CPU time of r05's
    # all-rows oracle leg for the same tiles under test (rows of different 256-row tiles and different workgroups)
    rows = sorted({0, B // 2 - 1, B - 1})
    keep = torch.get_num_threads()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    try:
        for s in ((0, 1) if B == 16 else (1,)):
            xin = x[:, :3 * (s + 1)].contiguous()
            ref = unet_forward(sd, UNET_FULL, xin[rows].contiguous(), t[rows], ctx[rows].contiguous(), s)
            got = m(xin.cuda(), t.cuda(), context=ctx.cuda(), stage=s)
            assert got.shape == (B,) + tuple(ref.shape[1:]) and bool(torch.isfinite(got).all())
            r = _rel(got[rows], ref)
            print(f"B = {B} full-width forward stage {s}: rows {rows} rel err {r:.2e}")
            assert r < 2e-4, (B, s)
    finally:
        torch.set_num_threads(keep)


@pytest.mark.gate
def test_deferred_splitk_reductions_of_the_benchmarked_programs_match_torch():
    """(r06 gate) tools/verify_deferred.py as a test: the step programs of the headline workload (B = 16, both stages, the PINNED tiles) run op
    by op; after every GroupNorm that finishes a deferred split-K reduction (builder._deferred_splitk) the reduction -- slices in order,
    bias, timestep vector, residual -- and the normalisation are recomputed in torch fp32 from the device buffers the descriptor names.
    This is the check that found r05's plan-time aliasing race; it costs seconds."""
    import importlib.util
    from frido.models.diffusion.ddim import DDIMSampler
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("verify_deferred", os.path.join(root, "tools", "verify_deferred.py"))
    vd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vd)
    model = _frido(UNET_FULL, VQ_FULL, precision="bf16x3", shared=True)
    B = 16
    z, _ = DDIMSampler(model).sample(S=4, batch_size=B, shape=(6, 64, 64), conditioning=_bench_ctx(B).cuda(), num_stage=2, eta=1.0,
                                     verbose=False, noise="philox", seed=3, log_every_t=10 ** 9)
    torch.cuda.synchronize()
    rt = model.model.diffusion_model.runtime()
    eng = next(reversed(rt._sampler_engines.values()))          # most recently used = the one just run
    assert eng.B == B
    sp = torch.cuda.current_stream().cuda_stream
    worst, checked = 0.0, 0
    for si, stg in enumerate(eng.stages):
        eng.step.zero_()
        w, n = vd.check_prog(stg.step, f"stage{si}.step", sp, 0, quiet=True)
        worst, checked = max(worst, w), checked + n
    print(f"deferred split-K reductions of the B = 16 step programs: {checked} checked, worst rel err {worst:.2e}")
    assert bool(torch.isfinite(z).all()) and worst < 1e-4
    from frido_amd import tune
    if tune.cache_is_pinned_for_this_library():
        assert checked > 0, "the pinned tile cache defers split-K reductions on the 16^2 / 8^2 planes of this workload"


def test_decode_ignores_force_not_quantize_like_the_reference():
    """msvqgan.py:376-399 accepts force_not_quantize and never reads it: same output with and without."""
    g = golden("vq_small")
    m = _vq(VQ_SMALL)
    h = torch.from_numpy(g["h"]).cuda()
    assert torch.equal(m.decode(h), m.decode(h, force_not_quantize=True))


class _GoldenCorrector:
    """tests/golden/make_golden.py GoldenCorrector: the reference's score-corrector protocol (ddim.py:228-230)."""

    def modify_score(self, model, e_t, x, t, c, gain=1.0):
        assert e_t.is_cuda and x.shape == e_t.shape and t.dtype == torch.long and hasattr(model, "alphas_cumprod")
        return gain * e_t + 0.01 * torch.tanh(x) * (t.float().view(-1, 1, 1, 1) / 1000.0)


def test_sampler_options_noise_dropout_and_score_corrector():
    """The sampler options of ddim.py the shipped scripts leave at their defaults (r03 verdict, missing 4): noise_dropout
    (ddim.py:260-262) and score_corrector (:228-230, with and without CFG) against the reference's own runs on the same torch
    seed -- the noise AND the dropout masks come from torch's CPU generator in the reference's order."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    g = golden("sampler_opts")
    model = _frido(UNET_SMALL, VQ_SMALL)
    c = torch.from_numpy(g["c"]).cuda()
    uc = torch.zeros_like(c)
    base = dict(S=5, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, verbose=False, log_every_t=2, noise="torch")
    runs = (("dropout", dict(eta=1.0, noise_dropout=0.25)),
            ("corrector", dict(eta=1.0, score_corrector=_GoldenCorrector(), corrector_kwargs=dict(gain=0.9))),
            ("corrector_cfg_dropout", dict(eta=0.5, noise_dropout=0.4, score_corrector=_GoldenCorrector(), corrector_kwargs=dict(gain=1.1),
                                           unconditional_guidance_scale=1.5, unconditional_conditioning=uc)))
    for name, kw in runs:
        torch.manual_seed(23)
        samples, inter = DDIMSampler(model).sample(**base, **kw)
        r = _rel(samples, g[f"{name}_samples"])
        print(f"sampler option {name}: latent rel err {r:.2e}")
        assert r < 1e-3 and len(inter["x_inter"]) == int(g[f"{name}_nx"]) and _rel(inter["pred_x0"][1], g[f"{name}_pred_x0_1"]) < 1e-3, name
    torch.manual_seed(23)
    samples, _ = PLMSSampler(model).sample(**base, noise_dropout=0.3)
    assert _rel(samples, g["plms_dropout_samples"]) < 1e-3
    assert np.array_equal(torch.randn(4).numpy(), g["plms_dropout_rng_tail"]), "the run must consume the generator like the reference (randn + dropout masks)"
    with pytest.raises(NotImplementedError):
        DDIMSampler(model).sample(**dict(base, noise="philox"), noise_dropout=0.1)
    for name, kw in (("plms_corrector", dict(score_corrector=_GoldenCorrector(), corrector_kwargs=dict(gain=0.9))),
                     ("plms_corrector_cfg", dict(score_corrector=_GoldenCorrector(), corrector_kwargs=dict(gain=1.1),
                                                 unconditional_guidance_scale=1.5, unconditional_conditioning=uc))):
        torch.manual_seed(23)
        samples, inter = PLMSSampler(model).sample(**dict(base, S=6), **kw)      # corrector inside every model evaluation (plms.py:236-238)
        r = _rel(samples, g[f"{name}_samples"])
        print(f"sampler option {name}: latent rel err {r:.2e}")
        assert r < 1e-3 and len(inter["x_inter"]) == int(g[f"{name}_nx"]) and _rel(inter["pred_x0"][1], g[f"{name}_pred_x0_1"]) < 1e-3, name
    with pytest.raises(NotImplementedError):        # the reference's own blend raises for multi-stage models (ddim.py:158-161)
        DDIMSampler(model).sample(**base, mask=torch.ones(2, 1, 16, 16), x0=torch.zeros(2, 6, 16, 16))


@pytest.mark.parametrize("which", ["config3_B32_plms_cfg", "config5_B8_three_stages"])
def test_other_configs_at_their_per_gpu_batch(which):
    """BASELINE configs 3 (t2i f16f8, batch 32, PLMS + CFG 1.5) and 5 (512^2, three scales, 8 per GPU) at the batch ONE GPU runs:
    rows of the batched run against B = 1 runs at sample0 = i (Philox noise keyed by the global sample index); the B = 1 / 2
    arithmetic of these configs is what the reference goldens pin (test_config3_..., test_config5_...)."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    from golden_cfg import UNET_F16F8, VQ_F16F8, UNET_512, VQ_512
    from frido_amd.synth import seeded_normal
    if which.startswith("config3"):
        B, rows, shape, nstage, cls, S, embed = 32, (0, 31), (8, 32, 32), 2, PLMSSampler, 10, [4, 4]
        model = _frido(UNET_F16F8, VQ_F16F8, precision="bf16x3", shared=True)
        c = torch.from_numpy(seeded_normal("b3:c", (B, 1, 768)))
        c = (c / c.norm(dim=-1, keepdim=True)).cuda()                      # encoders/modules.py:213-214: L2-normalised CLIP embedding
        uc = torch.from_numpy(seeded_normal("b3:uc", (B, 1, 768)))
        uc = (uc / uc.norm(dim=-1, keepdim=True)).cuda()
        kw = dict(eta=0.0, unconditional_guidance_scale=1.5)
    else:
        B, rows, shape, nstage, cls, S, embed = 8, (0, 7), (9, 128, 128), 3, DDIMSampler, 2, [3, 3, 3]
        model = _frido(UNET_512, VQ_512, precision="bf16x3", shared=True)
        c = torch.from_numpy(seeded_normal("b5:c", (B, 92, 640))).cuda()
        uc, kw = None, dict(eta=1.0)
    base = dict(S=S, shape=shape, num_stage=nstage, verbose=False, noise="philox", seed=77, log_every_t=10 ** 9, **kw)
    zb, _ = cls(model).sample(batch_size=B, conditioning=c, unconditional_conditioning=uc, **base)
    ib, cb = model.decode_first_stage(zb, return_code=True)
    cb = np.asarray(cb)
    worst = dict(latent=0.0, pix=0.0, flips=0)
    for i in rows:
        z1, _ = cls(model).sample(batch_size=1, conditioning=c[i:i + 1].contiguous(),
                                  unconditional_conditioning=None if uc is None else uc[i:i + 1].contiguous(), sample0=i, **base)
        i1, c1 = model.decode_first_stage(z1, return_code=True)
        worst["latent"] = max(worst["latent"], _rel(zb[i:i + 1], z1.cpu()))
        worst["flips"] += int((np.asarray(c1)[:, 0] != cb[:, i]).sum())
        worst["pix"] = max(worst["pix"], float((ib[i:i + 1] - i1).abs().max()))
    ncodes = len(rows) * cb.shape[0] * cb.shape[2]
    print(f"{which}: rows {rows} vs B = 1: {worst} of {ncodes} codes")
    _record(f"{which}/rows_vs_b1", dict(worst, codes=ncodes))
    # Two runs of the SAME library at different batch sizes differ by ~2e-6 in the latent (tiles / summation order).  On config 5's
    # UNCONVERGED DDIM-2 latent (3 x 16384 codes per image) that difference alone moves 3 of 98304 codes across a VQ decision boundary
    # (each moves pixels by ~0.1): a flip RATE is asserted here, the pixel bound only when none flipped.  The converged runs
    # (configs 2 / 3 / 4 above) measure 0.
    assert torch.isfinite(zb).all() and worst["latent"] < E2E_X3["latent_rel"] and worst["flips"] <= 1e-4 * ncodes
    if worst["flips"] == 0:
        assert worst["pix"] < E2E_X3["pix_max"]


# ---------------------------------------------------------------------------------------------------------------------
# Round 5: two REAL ranks of the HIP sampler (r04 verdict, missing 1 / next 6).  No 8-GPU node exists for this builder, so the
# evidence obtainable is two processes sharing the test box's one GPU: the real sample_images on each rank (contiguous shard,
# Philox noise keyed by the global sample index, captured graphs, decode to uint8), joined by the pipeline's ONE all-gather
# (backend gloo, device tensors staged through host -- RCCL has no second device here).
TWO_RANK_WORKER = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(repo)r)
from bench import build_model
from frido_amd import synth
from frido_amd.pipeline import sample_images, shard_range
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.cuda.set_device(0)                     # BOTH ranks on the one GPU of the box
dev = torch.device("cuda", 0)
model = build_model("bf16x3", dev)
# (r06) a RAGGED job first -- 3 images over 2 ranks: shards of 2 and 1, the padded all-gather -- then the even one
lo3, hi3 = shard_range(3, rank, world)
ctx3 = torch.from_numpy(synth.seeded_normal("two:ctx", (4, 26, 640))[lo3:hi3]).to(dev)
img3 = sample_images(model, ctx3, S=4, eta=1.0, seed=77, sample0=lo3, noise="philox", total=3, gather_dtype="uint8")
assert img3.shape == (3, 256, 256, 3) and img3.dtype == torch.uint8
if rank == 0:
    np.save(%(out)r + ".ragged.npy", img3.cpu().numpy())
total = 4
lo, hi = shard_range(total, rank, world)
ctx = torch.from_numpy(synth.seeded_normal("two:ctx", (total, 26, 640))[lo:hi]).to(dev)
img = sample_images(model, ctx, S=4, eta=1.0, seed=77, sample0=lo, noise="philox", total=total, gather_dtype="uint8")
# the latents of the same run, joined by the same collective (for the comparison with ONE batch of 4, where a VQ decision is not in the way)
from frido_amd.samplers import DDIMSampler
from frido_amd.pipeline import all_gather_images
unet = model.model.diffusion_model
z, _ = DDIMSampler(model).sample(S=4, batch_size=hi - lo, shape=(unet.in_channels, unet.image_size, unet.image_size), conditioning=ctx,
                                 num_stage=unet.num_stage, eta=1.0, verbose=False, noise="philox", seed=77, sample0=lo, log_every_t=10 ** 9)
zall = all_gather_images(z, total=total)
torch.cuda.synchronize()
assert img.shape == (total, 256, 256, 3) and img.dtype == torch.uint8
if rank == 0:
    np.save(%(out)r, img.cpu().numpy())
    np.save(%(out)r + ".z.npy", zall.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.gate
def test_two_real_hip_ranks_on_one_gpu_join_to_the_single_process_result(tmp_path):
    import subprocess
    import sys
    from bench import build_model
    from frido_amd import synth
    from frido_amd.pipeline import sample_images
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_npy = str(tmp_path / "joined.npy")
    script = tmp_path / "two_rank_worker.py"
    script.write_text(TWO_RANK_WORKER % dict(repo=repo, out=out_npy))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29547", str(script)], capture_output=True, text=True, env=env, timeout=1500, cwd=repo)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert run.stdout.count("ok") == 2
    joined = torch.from_numpy(np.load(out_npy))
    # single process, (a) shard by shard with the ranks' own batch shapes: the two-process job must reproduce it BIT FOR BIT
    model = build_model("bf16x3", torch.device("cuda", 0))
    ctx = torch.from_numpy(synth.seeded_normal("two:ctx", (4, 26, 640))).cuda()
    kw = dict(S=4, eta=1.0, seed=77, noise="philox", total=4, gather_dtype="uint8")
    seq = torch.cat([sample_images(model, ctx[lo:hi].contiguous(), sample0=lo, **kw) for lo, hi in ((0, 2), (2, 4))]).cpu()
    dseq = (joined.int() - seq.int()).abs()
    print("two ranks vs sequential shards: per-image max |diff|", [int(dseq[i].max()) for i in range(4)],
          "share differing", [round(float((dseq[i] > 0).float().mean()), 6) for i in range(4)])
    assert torch.equal(joined, seq)
    # (r06) the ragged job (3 images: rank 0 owns two, rank 1 one -- the zero-padded all-gather and its un-padding): image i is keyed by its
    # GLOBAL index, so images 0-1 are the first shard above bit for bit and image 2 is a B = 1 run at sample0 = 2
    ragged = torch.from_numpy(np.load(out_npy + ".ragged.npy"))
    last = sample_images(model, ctx[2:3].contiguous(), sample0=2, **dict(kw, total=1)).cpu()
    assert ragged.shape == (3, 256, 256, 3) and torch.equal(ragged[:2], seq[:2]) and torch.equal(ragged[2:], last)
    # (b) the whole batch in ONE launch sequence (B = 4 selects other tiles / wave counts than B = 2: fp32 summation orders differ): the
    # latents agree to the parity bound; the uint8 images up to truncation boundaries (and wherever an unconverged DDIM-4 latent sits
    # on a VQ decision boundary, DESIGN.md section 5 -- reported, not asserted)
    from frido_amd.samplers import DDIMSampler
    unet = model.model.diffusion_model
    zfull, _ = DDIMSampler(model).sample(S=4, batch_size=4, shape=(unet.in_channels, unet.image_size, unet.image_size), conditioning=ctx,
                                         num_stage=unet.num_stage, eta=1.0, verbose=False, noise="philox", seed=77, sample0=0, log_every_t=10 ** 9)
    zjoined = torch.from_numpy(np.load(out_npy + ".z.npy"))
    lat = _rel(zfull, zjoined)
    full = sample_images(model, ctx, sample0=0, **kw).cpu()
    diff = (joined.int() - full.int()).abs()
    share = float((diff > 0).float().mean())
    print(f"two ranks vs one batch of 4: latent rel {lat:.2e}; uint8 max |diff| {int(diff.max())} code value(s), share of differing values {share:.2e}")
    assert lat < E2E_X3["latent_rel"]
    _record("two_ranks_one_gpu/ddim4", dict(bit_identical_to_sequential_shards=True, latent_rel_vs_one_batch=lat,
                                            uint8_max_diff_vs_one_batch=int(diff.max()), uint8_share_differing=share))


# ---------------------------------------------------------------------------------------------------------------------
# Round 5: parity under a TRAINED-CHECKPOINT-LIKE dynamic range (r04 verdict, weak 2 / next 5).  Every fixture above fills weights
# with the fan-in-scaled N(0, sigma) filler; these use frido_amd.synth's "heavy" profile (heavy-tailed weights, norm scales in
# [0.2, 3], 0.5-sigma biases, residual-branch gains that put the raw stream in the thousands) -- fixtures captured from the reference
# with it (tests/golden/make_golden.py --profile heavy) -- on BOTH plane formats of the two-plane arithmetic: fp16 pairs
# (precision "bf16x3", 2^-22 relative, |v| <= 65504) and bf16 pairs ("bf16x3_bf16", 2^-17, fp32's range).
PLANE_PRECISIONS = ["bf16x3", "bf16x3_bf16"]


def _heavy_unet(cfg, precision):
    from frido_amd.models import PyUNetModel
    return fill_module(PyUNetModel(**cfg, precision=precision), "model.diffusion_model.", "heavy").cuda().eval()


@pytest.mark.parametrize("precision", PLANE_PRECISIONS)
@pytest.mark.parametrize("name,cfg", [("unet_small_heavy", UNET_SMALL), ("unet_full_heavy", UNET_FULL)])
def test_unet_forward_heavy_profile_both_plane_formats(name, cfg, precision):
    from frido_amd import _lib
    g = golden(name)
    _lib.status_flags(clear=True)
    m = _heavy_unet(cfg, precision)
    x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["ctx"]).cuda()
    errs = []
    for s in range(2):
        e = m(x[:, :3 * (s + 1)].contiguous(), torch.from_numpy(g[f"t_{s}"]).cuda(), context=ctx, stage=s)
        errs.append(_rel(e, g[f"eps_{s}"]))
    flags = _lib.status_flags(clear=True)
    print(f"{name} [{precision}]: eps rel err {errs[0]:.2e} / {errs[1]:.2e}, reference stream max {float(g['stream_absmax_1']):.3g}, status flags {flags}")
    _record(f"heavy/{name}/{precision}", dict(eps_rel_stage0=errs[0], eps_rel_stage1=errs[1], stream_absmax=float(g["stream_absmax_1"]), status_flags=flags))
    assert flags == 0                                   # the stream stays inside fp16's range on these fixtures: nothing may saturate
    assert max(errs) < (2e-4 if precision == "bf16x3" else 2e-3)      # same bound as the default-filler fixtures; the 16-bit-mantissa pairs get 10x


@pytest.mark.parametrize("precision", PLANE_PRECISIONS)
@pytest.mark.parametrize("name,cfg", [("vq_small_heavy", VQ_SMALL), ("vq_full_heavy", VQ_FULL)])
def test_vq_decode_heavy_profile_both_plane_formats(name, cfg, precision):
    from frido_amd.models import VQModelInterface
    from frido_amd import _lib
    g = golden(name)
    _lib.status_flags(clear=True)
    m = fill_module(VQModelInterface(**cfg, lossconfig=dict(target="taming.modules.losses.DummyLoss"), precision=precision),
                    "first_stage_model.", "heavy").cuda().eval()
    h = torch.from_numpy(g["h"]).cuda()
    ss = int(g["subsample"])
    dec, code = m.decode(h, return_code=True)
    flips = float((np.asarray(code) != g["code"]).mean())
    forced = m.decode(h, force_codes=[g["code"][i] for i in range(len(cfg["embed_dim"]))])
    r = _rel(forced[:, :, ::ss, ::ss], g["dec"])
    flags = _lib.status_flags(clear=True)
    print(f"{name} [{precision}]: VQ code flips {flips:.2e}, decoder rel err on the reference's codes {r:.2e}, status flags {flags}")
    _record(f"heavy/{name}/{precision}", dict(vq_flip_rate=flips, forced_decoder_rel=r, status_flags=flags))
    assert flips == 0 and flags == 0
    assert r < (2e-4 if precision == "bf16x3" else 2e-3)


@pytest.mark.parametrize("precision", PLANE_PRECISIONS)
@pytest.mark.parametrize("run", ["ddim_eta1", "plms_cfg"])
def test_sampler_heavy_profile_both_plane_formats(run, precision):
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    from frido_amd.models import instantiate_from_config
    from frido_amd import _lib
    g = golden("sampler_small_heavy")
    cfg = frido_cfg(dict(UNET_SMALL, precision=precision), dict(VQ_SMALL, precision=precision), BERT_SMALL)
    cfg["cond_stage_config"], cfg["conditioning_key"] = "__is_unconditional__", "crossattn"
    model = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(model.model, "model.", "heavy")
    fill_module(model.first_stage_model, "first_stage_model.", "heavy")
    model.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    model = model.cuda().eval()
    _lib.status_flags(clear=True)
    c = torch.from_numpy(g["c"]).cuda()
    S, eta, scale, lev = g[f"{run}_args"]
    cls = PLMSSampler if run.startswith("plms") else DDIMSampler
    tape = _Tape(g[f"{run}_noise"])
    samples, _ = cls(model).sample(S=int(S), batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=float(eta), verbose=False,
                                   log_every_t=int(lev), unconditional_guidance_scale=float(scale),
                                   unconditional_conditioning=torch.zeros_like(c) if scale != 1.0 else None, noise=tape)
    lat = _rel(samples, g[f"{run}_samples"])
    flags = _lib.status_flags(clear=True)
    print(f"sampler_small_heavy/{run} [{precision}]: latent rel err {lat:.2e} (reference stream max {float(g['stream_absmax']):.3g}), status flags {flags}")
    _record(f"heavy/sampler_small_heavy/{run}/{precision}", dict(latent_rel=lat, stream_absmax=float(g["stream_absmax"]), status_flags=flags))
    assert tape.pos == tape.t.numel()
    assert flags & _lib.STATUS_NONFINITE == 0
    assert lat < (1e-3 if precision == "bf16x3" else 5e-3)


def test_full_size_heavy_sampler_moves_itself_to_the_bf16_pair_planes():
    """sampler_full_heavy: DDIM-4 at full width with the heavy filler -- a random-weight denoiser does not denoise, x grows to ~100 and
    the reference's raw residual stream reaches 7e5: BEYOND fp16.  (r06, r05 verdict next 4) With NO precision keyword the library picks
    the plane format itself: the first attempt saturates an fp16 plane (status word, polled in stream order after the pass), the denoiser
    moves to the bf16-pair build of the same kernels, the host noise stream is rewound and the pass repeated -- the caller gets the
    bf16-pair result (<= 5e-5 on this fixture) and ONE FridoNumericsWarning saying so.  Pinned to the fp16 pairs ("bf16x3_f16") the same
    model saturates and only SAYS so (r05 behaviour)."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido_amd.models import instantiate_from_config
    from frido_amd import _lib
    g = golden("sampler_full_heavy")
    assert float(g["stream_absmax"]) > 65504.0
    c = torch.from_numpy(g["c"]).cuda()
    cfg = frido_cfg(dict(UNET_FULL), dict(VQ_FULL), BERT_SMALL)                     # no `precision` anywhere
    cfg["cond_stage_config"], cfg["conditioning_key"] = "__is_unconditional__", "crossattn"
    model = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(model.model, "model.", "heavy")
    fill_module(model.first_stage_model, "first_stage_model.", "heavy")
    model.scale_factor.copy_(torch.from_numpy(g["scale_factor"]))
    model = model.cuda().eval()
    unet = model.model.diffusion_model
    kw = dict(S=4, batch_size=1, shape=(6, 64, 64), conditioning=c, num_stage=2, eta=1.0, verbose=False, log_every_t=2, noise="torch")
    _lib.status_flags(clear=True)
    assert unet.planes == "f16"
    torch.manual_seed(23)
    with pytest.warns(_lib.FridoNumericsWarning, match="bf16-pair planes"):
        samples, _ = DDIMSampler(model).sample(**kw)
    lat = _rel(samples, g["ddim4_samples"])
    flags = _lib.status_flags(clear=True)
    rng_after = torch.get_rng_state()
    print(f"sampler_full_heavy [default keyword -> moved to {unet.planes} pairs]: latent rel err {lat:.2e}, status flags {flags} (reference stream max {float(g['stream_absmax']):.3g})")
    _record("heavy/sampler_full_heavy/ddim4/auto", dict(latent_rel=lat, status_flags=flags, planes_after=unet.planes, stream_absmax=float(g["stream_absmax"])))
    assert unet.planes == "bf16" and unet.precision == "bf16x3_bf16" and flags == 0 and lat < 5e-5
    # the repeated pass consumed the host generator exactly once more from the REWOUND state: a second call continues the same stream a
    # single pass would have left behind
    torch.manual_seed(23)
    again, _ = DDIMSampler(model).sample(**kw)                   # already on the bf16 pairs: no move, no warning
    assert torch.equal(again, samples) and torch.equal(torch.get_rng_state(), rng_after)
    # pinned to the fp16 pairs: saturates, and says so
    unet.precision = "bf16x3_f16"
    unet.invalidate()
    torch.manual_seed(23)
    pinned, _ = DDIMSampler(model).sample(**kw)
    lat16 = _rel(pinned, g["ddim4_samples"])
    flags16 = _lib.status_flags()
    print(f"sampler_full_heavy [bf16x3_f16 pinned]: latent rel err {lat16:.2e}, status flags {flags16}")
    _record("heavy/sampler_full_heavy/ddim4/bf16x3_f16", dict(latent_rel=lat16, status_flags=flags16))
    assert unet.planes == "f16" and flags16 & _lib.STATUS_SATURATED
    with pytest.warns(_lib.FridoNumericsWarning, match="saturated"):
        _lib.warn_on_status("sampler_full_heavy")
    del model
    torch.cuda.empty_cache()

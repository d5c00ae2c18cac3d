"""CPU-side checks of the CLIP image tower: the float64 restatement (tests/clip_vision_ref.py) against torch and transformers, the holder,
the refusals, and the one launcher of include/frido_vision.h as far as it goes without a device."""
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import clip_vision_ref as R
from frido_amd import _lib, holders

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(B, H, W, seed):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


# ---- the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 40, 56), (1, 12, 20), (1, 32, 32)], ids=["down", "up", "identity"])
def test_restated_resize_is_torchs_bicubic(shape):
    B, H, W = shape
    x = _images(B, H, W, 1)
    ref = F.interpolate(x, (32, 32), mode="bicubic", align_corners=True)
    My, Mx = R.resize_matrix(H, 32), R.resize_matrix(W, 32)
    got = torch.einsum("yh,bchw,xw->bcyx", My, x, Mx)
    assert float((got - ref).abs().max()) < 1e-13
    if H == W == 32:
        assert torch.equal(My, torch.eye(32, dtype=torch.float64))       # t = 0: weights exactly 0, 1, 0, 0
    mean = torch.tensor(R.CLIP_MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(R.CLIP_STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    assert float((R.preprocess_ref(x, 32) - ((ref + 1) / 2 - mean) / std).abs().max()) < 1e-12


def test_resize_matrix_edge_cases():
    assert torch.equal(R.resize_matrix(7, 1), torch.eye(7, dtype=torch.float64)[:1])        # one output sample reads source 0
    for kw in (dict(), dict(A=-0.5), dict(align_corners=False)):
        assert float((R.resize_matrix(12, 32, **kw).sum(1) - 1).abs().max()) < 1e-14       # a partition of unity while taps are clamped
    assert float((R.resize_matrix(12, 32, clamp=False).sum(1) - 1).abs().max()) > 1e-2


def test_patchify_is_conv1s_column_order():
    img = _images(2, 16, 16, 2)
    w = torch.randn(5, 3, 8, 8, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref = F.conv2d(img, w, stride=8).permute(0, 2, 3, 1).reshape(-1, 5)
    assert float((R.patchify(img, 8) @ w.reshape(5, -1).t() - ref).abs().max()) < 1e-13


@pytest.mark.parametrize("width,heads", [(64, 2), (128, None)], ids=["w64-2heads", "w128-default-heads"])
def test_restated_tower_is_transformers_clip_vision_model(width, heads, monkeypatch):
    """The restatement under OpenAI's names == transformers' CLIPVisionModelWithProjection under its own, random weights mapped name for
    name, float64.  Built from a config: nothing is fetched."""
    transformers = pytest.importorskip("transformers")
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    embed, res, layers, patch = 48, 32, 2, 8
    nh = heads or width // 64
    cfg = transformers.CLIPVisionConfig(hidden_size=width, intermediate_size=4 * width, num_hidden_layers=layers, num_attention_heads=nh,
                                        image_size=res, patch_size=patch, projection_dim=embed, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                        attention_dropout=0.0)
    hf = transformers.CLIPVisionModelWithProjection(cfg).double().eval()
    root = nn.Module()
    holders.build_clip_visual_params(root, embed, res, layers, width, patch)
    g = torch.Generator().manual_seed(7)
    sd = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) * (0.3 if v.dim() > 1 else 1.0) for k, v in root.state_dict().items()}
    v = "model.visual."
    hsd = {"vision_model.embeddings.class_embedding": sd[v + "class_embedding"],
           "vision_model.embeddings.patch_embedding.weight": sd[v + "conv1.weight"],
           "vision_model.embeddings.position_embedding.weight": sd[v + "positional_embedding"],
           "visual_projection.weight": sd[v + "proj"].t().contiguous()}
    for a, b in (("pre_layrnorm", "ln_pre"), ("post_layernorm", "ln_post")):
        for leaf in ("weight", "bias"):
            hsd[f"vision_model.{a}.{leaf}"] = sd[f"{v}{b}.{leaf}"]
    for i in range(layers):
        h, o = f"vision_model.encoder.layers.{i}.", f"{v}transformer.resblocks.{i}."
        for j, name in enumerate(("q_proj", "k_proj", "v_proj")):
            hsd[h + f"self_attn.{name}.weight"] = sd[o + "attn.in_proj_weight"][j * width:(j + 1) * width]
            hsd[h + f"self_attn.{name}.bias"] = sd[o + "attn.in_proj_bias"][j * width:(j + 1) * width]
        for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                     ("mlp.fc2", "mlp.c_proj")):
            for leaf in ("weight", "bias"):
                hsd[h + f"{a}.{leaf}"] = sd[o + f"{b}.{leaf}"]
    res_load = hf.load_state_dict(hsd, strict=False)
    assert not res_load.unexpected_keys and all("position_ids" in k for k in res_load.missing_keys), res_load
    img = _images(2, res, res, 8)
    with torch.no_grad():
        ref = hf(pixel_values=img).image_embeds
    got = R.encode_image_ref(sd, img, patch=patch, heads=heads)
    assert got.shape == ref.shape == (2, embed)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12


# ---- the holder ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", sorted(holders.CLIP_VISUAL_ARCH))
def test_holder_keys_and_shapes(version):
    embed, res, layers, width, patch = holders.CLIP_VISUAL_ARCH[version]
    root = nn.Module()
    holders.build_clip_visual_params(root, embed, res, layers, width, patch)
    shapes = {k: tuple(v.shape) for k, v in root.state_dict().items()}
    v = "model.visual."
    want = {v + "conv1.weight": (width, 3, patch, patch), v + "class_embedding": (width,),
            v + "positional_embedding": ((res // patch) ** 2 + 1, width), v + "proj": (width, embed)}
    for ln in ("ln_pre", "ln_post"):
        want[v + ln + ".weight"] = want[v + ln + ".bias"] = (width,)
    for i in range(layers):
        r = f"{v}transformer.resblocks.{i}."
        want.update({r + "ln_1.weight": (width,), r + "ln_1.bias": (width,), r + "ln_2.weight": (width,), r + "ln_2.bias": (width,),
                     r + "attn.in_proj_weight": (3 * width, width), r + "attn.in_proj_bias": (3 * width,),
                     r + "attn.out_proj.weight": (width, width), r + "attn.out_proj.bias": (width,),
                     r + "mlp.c_fc.weight": (4 * width, width), r + "mlp.c_fc.bias": (4 * width,),
                     r + "mlp.c_proj.weight": (width, 4 * width), r + "mlp.c_proj.bias": (width,)})
    assert shapes == want


def test_arch_table_is_openai_clips():
    assert holders.CLIP_VISUAL_ARCH == {"ViT-B/32": (512, 224, 12, 768, 32), "ViT-B/16": (512, 224, 12, 768, 16),
                                        "ViT-L/14": (768, 224, 24, 1024, 14), "ViT-L/14@336px": (768, 336, 24, 1024, 14)}


def test_full_clip_state_dict_loads_with_text_keys_unexpected():
    from frido_amd.models import FrozenCLIPTextEmbedder, FrozenClipImageEmbedder
    text = FrozenCLIPTextEmbedder(arch=(48, 8, 100, 64, 1, 2))
    m = FrozenClipImageEmbedder("small", arch=(48, 32, 2, 64, 8))
    full = {k: torch.full_like(v, 0.25) for k, v in m.state_dict().items()}
    text_keys = {k: torch.zeros_like(v) for k, v in text.state_dict().items()}
    assert not set(full) & set(text_keys)      # `model.positional_embedding` (text) and `model.visual.positional_embedding` are apart
    full.update(text_keys)
    res = m.load_state_dict(full, strict=False)
    assert not res.missing_keys and sorted(res.unexpected_keys) == sorted(text_keys)
    assert all(bool((p == 0.25).all()) for p in m.parameters())
    assert "mean" not in m.state_dict() and "std" not in m.state_dict()      # non-persistent buffers, like the reference's
    assert torch.equal(m.mean, torch.Tensor([0.48145466, 0.4578275, 0.40821073]))
    assert torch.equal(m.std, torch.Tensor([0.26862954, 0.26130258, 0.27577711]))


# ---- refusals, by their words --------------------------------------------------------------------------
def test_refusals_name_themselves():
    from frido.modules.encoders.modules import FrozenClipImageEmbedder
    from ldm.modules.encoders.modules import FrozenClipImageEmbedder as alias
    assert alias is FrozenClipImageEmbedder
    with pytest.raises(NotImplementedError, match="antialias=True"):
        FrozenClipImageEmbedder("ViT-B/32", antialias=True)
    with pytest.raises(NotImplementedError, match="jit=True"):
        FrozenClipImageEmbedder("ViT-B/32", jit=True)
    for rn in ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"):
        with pytest.raises(NotImplementedError, match="ResNet CLIP tower"):
            FrozenClipImageEmbedder(rn)
    with pytest.raises(NotImplementedError, match=r"unknown CLIP version 'ViT-H/14'.*ViT-B/16.*ViT-B/32.*ViT-L/14.*ViT-L/14@336px"):
        FrozenClipImageEmbedder("ViT-H/14")
    with pytest.raises(ValueError, match="not a whole number of 8 x 8 patches"):
        FrozenClipImageEmbedder("custom", arch=(48, 30, 1, 64, 8))
    with pytest.raises(ValueError, match="width 96 must be a multiple of 64"):
        FrozenClipImageEmbedder("custom", arch=(48, 32, 1, 96, 8))
    with pytest.raises(ValueError, match=r"width 1088 exceeds 1024.*LayerNorm kernel"):      # csrc/norm.hip frido_layernorm: C <= 1024
        FrozenClipImageEmbedder("custom", arch=(48, 32, 1, 1088, 8))
    m = FrozenClipImageEmbedder("custom", arch=(48, 32, 1, 64, 8))
    for bad in (torch.zeros(2, 3, 8), torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8)):
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            m(bad)
        with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
            m.preprocess(bad)
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 8, 8))
    with pytest.raises(_lib.FridoHipError, match="no CPU fallback"):
        m.preprocess(torch.zeros(2, 3, 8, 8))


def test_clip_score_refuses_mismatched_towers():
    from frido_amd.models import BERTEmbedder, FrozenCLIPTextEmbedder, FrozenClipImageEmbedder
    from frido_amd.pipeline import clip_score
    img = FrozenClipImageEmbedder("custom", arch=(48, 32, 1, 64, 8))
    x, t = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="48 dimensions, the text tower into 64"):
        clip_score(img, FrozenCLIPTextEmbedder(arch=(64, 8, 100, 64, 1, 1)), x, t)
    with pytest.raises(ValueError, match="must be a FrozenCLIPTextEmbedder"):
        clip_score(img, BERTEmbedder(n_embed=64, n_layer=1, vocab_size=100), x, t)
    with pytest.raises(ValueError, match="must be a FrozenClipImageEmbedder"):
        clip_score(FrozenCLIPTextEmbedder(arch=(48, 8, 100, 64, 1, 1)), FrozenCLIPTextEmbedder(arch=(48, 8, 100, 64, 1, 1)), x, t)
    assert "2.5 * max(cos, 0)" in clip_score.__doc__ and "Hessel" in clip_score.__doc__


# ---- the launcher, without a device --------------------------------------------------------------------
def test_descriptor_size_and_rejections():
    from frido_amd import vision
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_sizeof_clip_preprocess() == C.sizeof(vision.FridoClipPreprocess)
        fn = vision._fn(planes)
        assert fn(C.byref(vision.FridoClipPreprocess()), None) != 0                      # a zeroed descriptor is turned away, with a message
        assert b"frido_clip_preprocess: bad arguments" in L.frido_last_error()
        buf = (C.c_float * 64)()
        base = (C.addressof(buf) + 15) & ~15
        for kw, words in ((dict(res=30, P=8), b"whole number of patches"), (dict(res=32, P=0), b"whole number of patches"),
                          (dict(res=32, P=8, dst=base + 4), b"16-byte aligned"), (dict(res=32, P=8, B=0), b"bad arguments"),
                          (dict(res=32, P=8, src=None), b"bad arguments")):
            d = vision.preprocess_desc(base, base, 1, 4, 4, 32, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            assert fn(C.byref(d), None) != 0 and words in L.frido_last_error(), (kw, L.frido_last_error())
    d = vision.preprocess_desc(16, 32, 2, 40, 56, 224, 32)
    assert list(d.mean) == torch.tensor(R.CLIP_MEAN, dtype=torch.float32).tolist()      # the module's float32 buffers, bit for bit
    assert all(abs(r * s - 1) < 1e-6 for r, s in zip(d.rstd, R.CLIP_STD))


def test_the_op_table_header_does_not_know_the_launch():
    """frido_hip.h is the op-kind ABI (tests/test_opkinds_host.py pins it): the image tower's launch lives in a header of its own."""
    hip = open(os.path.join(REPO, "include", "frido_hip.h")).read()
    for name in ("frido_clip_preprocess", "FridoClipPreprocess", "frido_sizeof_clip_preprocess", "frido_vision"):
        assert name not in hip
    assert not [s for s in _lib.EXPORTS if "clip" in s] and "FridoClipPreprocess" not in _lib.STRUCTS
    vis = open(os.path.join(REPO, "include", "frido_vision.h")).read()
    assert _lib._parse_structs(_lib._strip_comments(vis)).keys() == {"FridoClipPreprocess"}
    assert "vision.hip" in open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()

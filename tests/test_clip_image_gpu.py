"""The CLIP image tower on the MI355X against the float64 restatement of tests/clip_vision_ref.py: the preprocess kernel
(csrc/vision.hip) at kernel level, FrozenClipImageEmbedder in both builds of the library, graph replay, re-planning, and clip_score.

Bounds (none of them is taken from what the code under test returns):
  kernel   2 x the error of the SAME formula evaluated in float32 on the host (F.interpolate in float32, then the normalisation)
           against float64, measured per shape in the test; four wrong variants of the formula (A = -0.5, align_corners=False, taps
           dropped instead of clamped, another channel's mean / std) are shown to lie >= 10 x outside.  A variant is checked on the
           shapes where it CAN differ: all four on the up, ViT-B/32-grid and P = 14 shapes; shrinking with align_corners=True puts the
           first and last outputs on source samples (t = 0) and no other output reaches past the border, so clamped and dropped taps
           agree on the down shape; an identity resize has t = 0 everywhere and only the channel mix-up shows; the B = 8 shape repeats
           the ViT-B/32 grid for the loop's second trip and checks none again.
  tower    relative to the reference's max |z|: 8 x the difference between the restatement run in float32 and in float64 on the same
           inputs (the factor allows for the kernels' other summation order).  The bf16-pair build: tests/test_model_gpu.py's text-tower
           test applies no ratio between the builds (it runs the default build only), so the ratio was measured: on the MI355X the
           bf16-pair build's error is 5.1 - 7.8 x the default build's (1.2e-5 against 1.6e-6 at worst).  The bound takes 10 x, the
           ratio tests/test_model_gpu.py gives the bf16-pair build wherever it runs both (the heavy-profile tests: 2e-4 / 2e-3), which
           the measurement sits inside.  Measured errors: profiles/clip_image.txt.
  score    8 x the float32 restatements' own differences carried through the cosine, see test_clip_score_is_the_restated_cosine."""
import functools

import pytest
import torch
import torch.nn.functional as F

import clip_vision_ref as R
from frido.modules.encoders.modules import FrozenCLIPTextEmbedder, FrozenClipImageEmbedder
from frido_amd import _lib, vision
from frido_amd.engine import require_gpu
from frido_amd.synth import fill_module

pytestmark = pytest.mark.gpu

BF16_PAIR_RATIO = 10.0      # the bf16-pair build's allowance over the default build's bound: see the module docstring


def _images(B, H, W, seed):
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 2 - 1


def _relay(dst, B, res, P):
    g = res // P
    return dst.view(B, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, res, res)


def _kernel(x, res, P, mean=R.CLIP_MEAN, std=R.CLIP_STD):
    """frido_clip_preprocess on x -> [B, 3, res, res] on the host; the rows behind the output must stay untouched."""
    require_gpu("cuda")
    B, _, H, W = x.shape
    g = res // P
    rows, pad = B * g * g, 4
    src = x.float().cuda().contiguous()
    dst = torch.full((rows + pad, 3 * P * P), float("nan"), device="cuda")
    vision.clip_preprocess(vision.preprocess_desc(src.data_ptr(), dst.data_ptr(), B, H, W, res, P, mean, std),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst[rows:]).all()), "the kernel wrote behind its output"
    out = dst[:rows].cpu()
    assert not bool(torch.isnan(out).any()), "the kernel left output elements unwritten"
    return _relay(out, B, res, P)


def _host_f32(x, res):
    """The same formula in float32 on the host: what float32 itself costs."""
    v = F.interpolate(x.float(), (res, res), mode="bicubic", align_corners=True)
    mean = torch.tensor(R.CLIP_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(R.CLIP_STD, dtype=torch.float32).view(1, 3, 1, 1)
    return ((v + 1.0) / 2.0 - mean) / std


WRONG = {"A=-0.5": dict(A=-0.5), "align_corners=False": dict(align_corners=False), "taps not clamped": dict(clamp=False),
         "mean/std of another channel": dict(channel_shift=1)}
ALL = tuple(WRONG)
KERNEL_SHAPES = [      # (B, H, W, res, P, the wrong variants this shape tells apart)
    pytest.param(2, 40, 56, 32, 8, ALL[:2] + ALL[3:], id="down-nonsquare", marks=pytest.mark.gate),
    pytest.param(1, 12, 20, 32, 8, ALL, id="up"),
    pytest.param(1, 32, 32, 32, 8, ALL[3:], id="identity"),
    pytest.param(3, 64, 48, 224, 32, ALL, id="vit-b32-grid"),
    pytest.param(8, 64, 48, 224, 32, (), id="second-trip-of-the-grid-stride-loop"),      # 1176 workgroups' worth of units, the launch caps at 1024
    pytest.param(2, 20, 36, 28, 14, ALL, id="P14-scalar-stores", marks=pytest.mark.gate),
]


@pytest.mark.parametrize("B,H,W,res,P,variants", KERNEL_SHAPES)
def test_preprocess_kernel_matches_float64(B, H, W, res, P, variants):
    x = _images(B, H, W, 11)
    ref = R.preprocess_ref(x, res)
    bound = 2.0 * float((_host_f32(x, res).double() - ref).abs().max())
    got = _kernel(x, res, P)
    err = float((got.double() - ref).abs().max())
    print(f"clip_preprocess B={B} {H}x{W} -> {res} P={P}: max abs err {err:.3e}, bound (2 x float32 on the host) {bound:.3e}")
    assert bound > 0 and err <= bound
    for name in variants:      # the bound tells the formula from its near misses: each lies at least 10 x outside
        d = float((R.preprocess_ref(x, res, **WRONG[name]) - ref).abs().max())
        assert d >= 10.0 * bound, (name, d, bound)


def test_identity_resize_returns_the_input():
    """H = W = res: t = 0 on both axes, weights exactly 0, 1, 0, 0 -- with mean 0 and std 1 the output is (x + 1) / 2 bit for bit."""
    x = _images(2, 32, 32, 12)
    got = _kernel(x, 32, 8, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    assert torch.equal(got, (x + 1.0) * 0.5)


# ---- the tower -----------------------------------------------------------------------------------------
ARCHS = {"17-tokens": ((48, 32, 2, 64, 8), (40, 56)), "37-tokens": ((48, 48, 2, 64, 8), (40, 56)),
         "ViT-B-32-one-layer": ((512, 224, 1, 768, 32), (64, 48)), "ViT-L-14-one-layer": ((768, 224, 1, 1024, 14), (64, 48))}
PREFIX = "clip_image."


@functools.lru_cache(maxsize=None)
def _tower_case(name):
    """(arch, images, float64 reference, relative float32-vs-float64 difference of the restatement, the float32 restatement): computed
    once, shared, never changed."""
    arch, (H, W) = ARCHS[name]
    embed, res, layers, width, patch = arch
    x = _images(2, H, W, 21)
    sd = R.filled_state_dict(FrozenClipImageEmbedder(name, arch=arch), PREFIX)
    kw = dict(patch=patch, prefix=PREFIX + "model.visual.")
    ref = R.encode_image_ref(sd, R.preprocess_ref(x, res), **kw)
    ref32 = R.encode_image_ref(sd, R.preprocess_ref(x, res, dtype=torch.float32), dtype=torch.float32, **kw)
    diff32 = float((ref32.double() - ref).abs().max() / ref.abs().max())
    return arch, x, ref, diff32, ref32


def _embedder(name, precision=None):
    arch = ARCHS[name][0]
    return fill_module(FrozenClipImageEmbedder(name, arch=arch, precision=precision), PREFIX).cuda()


def _rel(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_bf16"], ids=["f16-pairs", "bf16-pairs"])
@pytest.mark.parametrize("name", [pytest.param("17-tokens", marks=pytest.mark.gate), "37-tokens", "ViT-B-32-one-layer",
                                  pytest.param("ViT-L-14-one-layer", marks=pytest.mark.gate)])
def test_tower_matches_float64(name, precision):
    arch, x, ref, diff32, _ = _tower_case(name)
    _lib.status_flags(clear=True)
    m = _embedder(name, precision)
    z = m(x.cuda())
    assert z.shape == ref.shape == (2, arch[0]) and z.dtype == torch.float32 and z.is_cuda
    bound = 8.0 * diff32 * (BF16_PAIR_RATIO if precision == "bf16x3_bf16" else 1.0)
    err = _rel(z, ref)
    print(f"clip image tower {name} {precision}: rel err {err:.3e}, float32 restatement {diff32:.3e}, bound {bound:.3e}")
    assert _lib.status_flags() == 0
    assert err <= bound


def test_replay_returns_the_same_bits_and_a_new_batch_replans():
    arch, x, ref, diff32, _ = _tower_case("17-tokens")
    _lib.status_flags(clear=True)
    m = _embedder("17-tokens")
    xg = x.cuda()
    z1 = m(xg)
    z2 = m(xg)
    assert torch.equal(z1, z2) and m.graph_captures == 1 and list(m._plans) == [(2, 40, 56)]
    z3 = m(xg[:1])                                   # another batch size: another plan, another graph
    assert m.graph_captures == 2 and list(m._plans) == [(2, 40, 56), (1, 40, 56)]
    assert z3.shape == (1, arch[0]) and _rel(z3, ref[:1]) <= 8.0 * diff32 * float(ref.abs().max() / ref[:1].abs().max())
    z4 = m(xg.flip(0))                               # the first plan again, other pixels: the graph reads its input buffer, not a copy
    assert m.graph_captures == 2 and torch.equal(z4, z1.flip(0))
    z5 = m(xg[:, :, :32, :32])                       # another image size: a third plan
    assert m.graph_captures == 3 and z5.shape == z1.shape
    assert _lib.status_flags() == 0


def test_preprocess_method_is_the_kernels_image():
    x = _images(2, 40, 56, 11)
    ref = R.preprocess_ref(x, 32)
    bound = 2.0 * float((_host_f32(x, 32).double() - ref).abs().max())
    m = _embedder("17-tokens")
    got = m.preprocess(x.cuda())
    assert got.shape == (2, 3, 32, 32) and got.is_cuda
    assert float((got.cpu().double() - ref).abs().max()) <= bound
    assert torch.equal(got.cpu(), _kernel(x, 32, 8))


def test_clip_score_is_the_restated_cosine():
    """cos(image embedding, text embedding) against the float64 restatements of both towers.  Bound: with unit vectors u = zi / |zi| and
    t, |d cos| <= |du| + |dt| and |du| <= 2 |dzi| / |zi|; for dzi and dt the differences between the restatements run in float32 and
    in float64 on the same inputs (L2 norm per row), times the tower test's 8 for the kernels' other summation order."""
    from frido_amd.pipeline import clip_score
    from oracle.clip_text import clip_encode_text
    arch, x, ref_i, _, ref_i32 = _tower_case("17-tokens")
    tarch = (48, 8, 100, 64, 1, 2)
    img = _embedder("17-tokens")
    txt = fill_module(FrozenCLIPTextEmbedder(arch=tarch), "clip_text.").cuda()
    tokens = torch.tensor([[98, 5, 17, 99, 0, 0, 0, 0], [98, 40, 99, 0, 0, 0, 0, 0]])
    sd = R.filled_state_dict(txt, "clip_text.")
    kw = dict(heads=tarch[4], prefix="clip_text.model.")
    ref_t = clip_encode_text({k: v.double() for k, v in sd.items()}, tokens, **kw)
    ref_t32 = clip_encode_text(sd, tokens, **kw)
    assert ref_t.dtype == torch.float64 and ref_t32.dtype == torch.float32
    want = F.cosine_similarity(ref_i, ref_t, dim=-1)
    du = 2.0 * (ref_i32.double() - ref_i).norm(dim=-1) / ref_i.norm(dim=-1)
    dt = (ref_t32.double() - ref_t).norm(dim=-1)
    tol = 8.0 * float((du + dt).max())
    _lib.status_flags(clear=True)
    got = clip_score(img, txt, x.cuda(), tokens.cuda())
    assert got.shape == (2,) and got.dtype == torch.float32 and got.is_cuda
    err = float((got.cpu().double() - want).abs().max())
    print(f"clip_score: {got.tolist()} vs {want.tolist()}, err {err:.3e}, tol {tol:.3e}")
    assert tol > 0 and err <= tol
    txt.normalize = False                              # the text tower without its own normalisation: clip_score normalises it
    txt.invalidate()
    assert float((clip_score(img, txt, x.cuda(), tokens.cuda()).cpu().double() - want).abs().max()) <= tol
    assert _lib.status_flags() == 0
    with pytest.raises(ValueError, match="not halves of one CLIP"):
        clip_score(img, fill_module(FrozenCLIPTextEmbedder(arch=(64, 8, 100, 64, 1, 1)), "t.").cuda(), x.cuda(), tokens.cuda())

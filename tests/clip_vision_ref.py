"""Restatement of the CLIP image path in plain torch, at a dtype of the caller's choice (float64 for references, float32 to measure what
float32 itself costs): FrozenClipImageEmbedder.preprocess (frido/modules/encoders/modules.py:242-250 with antialias=False) and
clip/model.py VisionTransformer.forward under OpenAI's state_dict names.  A helper like tests/philox_ref.py: no test lives here.

The resize is written as two matrices (rows x image x columns^T) so that it shares no code with torch's upsample kernels;
tests/test_clip_image_host.py pins it to F.interpolate(mode="bicubic", align_corners=True) in float64, and the tower to
transformers.CLIPVisionModelWithProjection."""
import math

import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _cubic(x, A):
    """Keys cubic convolution kernel at distance x (float64 tensor)."""
    x = x.abs()
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return torch.where(x <= 1.0, near, torch.where(x < 2.0, far, torch.zeros_like(x)))


def resize_matrix(n_in, n_out, *, A=-0.75, align_corners=True, clamp=True):
    """[n_out][n_in] float64 matrix of the 1-D bicubic resize: source coordinate s = o (n_in - 1) / (n_out - 1) (0 when n_out == 1),
    i0 = floor(s), t = s - i0, taps i0 - 1 .. i0 + 2 clamped to the axis.  The keywords exist to build WRONG variants for the tests:
    another A, the half-pixel grid of align_corners=False, taps outside the axis dropped instead of clamped."""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        if align_corners:
            s = o * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            s = (o + 0.5) * n_in / n_out - 0.5
        i0 = math.floor(s)
        t = s - i0
        w = _cubic(torch.tensor([t + 1.0, t, 1.0 - t, 2.0 - t], dtype=torch.float64), A)
        for j in range(4):
            i = i0 - 1 + j
            if clamp:
                i = min(max(i, 0), n_in - 1)
            elif i < 0 or i >= n_in:
                continue
            M[o, i] += w[j]
    return M


def preprocess_ref(x, res, *, dtype=torch.float64, mean=CLIP_MEAN, std=CLIP_STD, channel_shift=0, **resize_kw):
    """x [B, 3, H, W] in [-1, 1] -> [B, 3, res, res]: bicubic resize, (v + 1) / 2, CLIP's mean / std (given as float32 values, like the
    module's buffers).  channel_shift rotates which channel's mean / std is applied (a wrong variant for the tests)."""
    x = x.to(dtype)
    My = resize_matrix(x.shape[2], res, **resize_kw).to(dtype)
    Mx = resize_matrix(x.shape[3], res, **resize_kw).to(dtype)
    v = torch.einsum("bchw,xw->bchx", x, Mx)          # the horizontal pass first, like torch's kernel
    v = torch.einsum("yh,bchx->bcyx", My, v)
    m = torch.tensor(mean, dtype=torch.float32).roll(channel_shift).to(dtype).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).roll(channel_shift).to(dtype).view(1, 3, 1, 1)
    return ((v + 1.0) / 2.0 - m) / s


def patchify(img, P):
    """[B, 3, res, res] -> [B g^2][3 P^2]: row = patch (b, gy, gx), column = (c, py, px) -- conv1.weight.reshape(width, -1)'s order."""
    B, C, R, _ = img.shape
    g = R // P
    return img.reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * P * P)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def encode_image_ref(sd, img, *, patch, heads=None, prefix="model.visual.", dtype=torch.float64):
    """clip/model.py VisionTransformer.forward on the PREPROCESSED image img [B, 3, res, res]; sd: state_dict with OpenAI's names under
    `prefix`.  heads defaults to width // 64 (clip/model.py CLIP.__init__: vision_heads = vision_width // 64).  -> [B, embed_dim]."""
    w = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    img = img.to(dtype)
    B = img.shape[0]
    width = w["conv1.weight"].shape[0]
    H = heads or width // 64
    dh = width // H
    x = patchify(img, patch) @ w["conv1.weight"].reshape(width, -1).t()              # conv1: stride = kernel = patch, no bias
    x = x.view(B, -1, width)
    x = torch.cat([w["class_embedding"].expand(B, 1, width), x], dim=1) + w["positional_embedding"]
    n = x.shape[1]
    x = _ln(x, w["ln_pre.weight"], w["ln_pre.bias"])
    layer = 0
    while f"transformer.resblocks.{layer}.ln_1.weight" in w:
        r = f"transformer.resblocks.{layer}."
        h = _ln(x, w[r + "ln_1.weight"], w[r + "ln_1.bias"])
        qkv = h @ w[r + "attn.in_proj_weight"].t() + w[r + "attn.in_proj_bias"]
        q, k, v = (t.view(B, n, H, dh).transpose(1, 2) for t in qkv.split(width, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1) @ v           # no mask in the image tower
        a = a.transpose(1, 2).reshape(B, n, width)
        x = x + a @ w[r + "attn.out_proj.weight"].t() + w[r + "attn.out_proj.bias"]
        h = _ln(x, w[r + "ln_2.weight"], w[r + "ln_2.bias"])
        h = h @ w[r + "mlp.c_fc.weight"].t() + w[r + "mlp.c_fc.bias"]
        h = h * torch.sigmoid(1.702 * h)                                              # QuickGELU
        x = x + h @ w[r + "mlp.c_proj.weight"].t() + w[r + "mlp.c_proj.bias"]
        layer += 1
    return _ln(x[:, 0, :], w["ln_post.weight"], w["ln_post.bias"]) @ w["proj"]


def filled_state_dict(module, prefix=""):
    """The deterministic filler's state_dict of a holder module, keyed like fill_module(module, prefix) filled it."""
    from frido_amd.synth import fill_tensor
    return {prefix + k: torch.from_numpy(fill_tensor(prefix + k, v.shape).copy()) for k, v in module.state_dict().items()}

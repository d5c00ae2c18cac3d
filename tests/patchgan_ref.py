"""The PatchGAN discriminator and the tokenizer's loss restated in plain torch (taming/modules/discriminator/model.py:17-67,
taming/modules/util.py:58, taming/modules/losses/vqperceptual.py:16-33, 80-150 under no_grad), in float64 by default.  It is the
reference the GPU tests measure against; tests/test_patchgan_host.py pins it to the fixture captured from the reference's own modules
(tests/golden/patchgan_ref.npz).  Weights and images are never stored: both sides regenerate them from names and seeds.
The keyword arguments of the *_ref functions are the WRONG variants the GPU tests tell the kernels apart from."""
import torch
import torch.nn.functional as F

import lpips_ref as L

PREFIX = "patchgan."               # what the fixtures' discriminator weights are keyed under (frido_amd.synth profile "patchgan")
SLOPE = 0.2
BN_EPS = 1e-5
SAMPLES = 200                      # hidden-feature values recorded per layer and case

# the discriminator cases of the golden file and of the whole-net tests: (B, H, W), ndf, n_layers, use_actnorm
NET_CASES = (((3, 24, 24), 16, 3, False),
             ((2, 32, 32), 16, 3, True),
             ((1, 40, 36), 16, 3, False),      # planes 20 x 18, 10 x 9, 5 x 4: the floor in the stride-2 size
             ((2, 32, 32), 64, 3, False),      # K reaches 4096 as in the real net
             ((2, 32, 32), 16, 2, False),
             ((2, 48, 48), 16, 4, True))
# the loss cases: (disc_loss, use_actnorm), each at LOSS_SHAPE with disc_ndf = LOSS_NDF, global_step in LOSS_STEPS (below and at disc_start)
LOSS_CASES = (("hinge", False), ("vanilla", True))
LOSS_SHAPE = (2, 32, 32)
LOSS_NDF = 16
DISC_START = 5
LOSS_STEPS = (0, 5)
LOSS_KW = dict(disc_start=DISC_START, codebook_weight=0.7, disc_factor=0.8, disc_weight=0.5, perceptual_weight=0.6, disc_ndf=LOSS_NDF)
CODEBOOK_LOSS = 0.37
LOG0_KEYS = ("total_loss", "quant_loss", "nll_loss", "rec_loss", "p_loss", "rec_aux_loss", "d_weight", "disc_factor", "g_loss")
LOG1_KEYS = ("disc_loss", "logits_real", "logits_fake")


def case_seed(ci):
    return SEEDS[ci]


def images(B, H, W, seed, C=3):
    """(real, fake) in [-1, 1], float32: the fake is the real with a part of it replaced by other noise, clipped."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=g, dtype=torch.float32) * 2 - 1
    n = torch.rand(B, C, H, W, generator=g, dtype=torch.float32) * 2 - 1
    return x, (0.5 * x + 0.5 * n).clamp(-1, 1)


# image seeds per NET_CASE / for the loss cases, chosen ONCE on the float64 restatement so that the fixture's condition holds (at least
# 10 % of the real logits above +1, 10 % of the fake ones below -1: both hinges clip); tests/test_patchgan_host.py asserts it
SEEDS = (200, 201, 202, 203, 204, 343)
LOSS_SEED = 300


def layer_table(input_nc, ndf, n_layers):
    """[(conv index in `main`, norm index or None, cin, cout, stride)]: model.py:41-62."""
    rows = [(0, None, input_nc, ndf, 2)]
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        rows.append((3 * n - 1, 3 * n, ndf * prev, ndf * mult, 2))
    prev, mult = mult, min(2 ** n_layers, 8)
    rows.append((3 * n_layers - 1, 3 * n_layers, ndf * prev, ndf * mult, 1))
    rows.append((3 * n_layers + 2, None, ndf * mult, 1, 1))
    return rows


def filled_state_dict(module, prefix=PREFIX):
    """The "patchgan" filler's state_dict of a discriminator (ours or the reference's: same names): every floating-point entry, the
    running statistics included; integer entries (num_batches_tracked, initialized) as the module holds them."""
    from frido_amd.synth import fill_tensor
    return {k: (torch.from_numpy(fill_tensor(prefix + k, v.shape, "patchgan").copy()) if v.is_floating_point() else v.detach().clone())
            for k, v in module.state_dict().items()}


def fill(module, prefix=PREFIX):
    """Fill a discriminator in place with the "patchgan" profile (parameters AND running statistics)."""
    module.load_state_dict(filled_state_dict(module, prefix), strict=True)
    return module


# ---- the kernels' formulas ------------------------------------------------------------------------------
def leaky(v, slope=SLOPE):
    return torch.where(v >= 0, v, slope * v)


def conv4(x, w, bias, *, stride, pad=1, out_hw=None, transpose=False):
    """4 x 4 convolution reading src[oy * stride + ky - pad][ox * stride + kx - pad] with zeros outside the image, on an out_hw grid
    (default: torch's own output size for this stride and padding 1).  With the true stride and pad = 1 it IS F.conv2d(padding=1); the
    wrong variants (another stride or pad on the SAME output grid, ky <-> kx) are what a mis-indexed kernel would compute."""
    H, W = x.shape[2:]
    if out_hw is None:
        out_hw = ((H + 2 - 4) // stride + 1, (W + 2 - 4) // stride + 1)
    Ho, Wo = out_hw
    xp = F.pad(x, (pad, max(0, (Wo - 1) * stride + 4 - pad - W), pad, max(0, (Ho - 1) * stride + 4 - pad - H)))
    return F.conv2d(xp, w.transpose(2, 3) if transpose else w, bias, stride=stride)[:, :, :Ho, :Wo]


def stem_ref(x, w, bias, *, dtype=torch.float64, pad=1, stride=2, transpose=False, drop_bias=False, slope=SLOPE):
    """conv 4 x 4 s2 p1 + bias + LeakyReLU(0.2) on NCHW -> NCHW, on the true output grid whatever the variant."""
    H, W = x.shape[2:]
    out_hw = ((H - 2) // 2 + 1, (W - 2) // 2 + 1)
    v = conv4(x.to(dtype), w.to(dtype), None if drop_bias else bias.to(dtype), stride=stride, pad=pad, out_hw=out_hw, transpose=transpose)
    return leaky(v, slope)


def head_ref(x, w, bias, *, dtype=torch.float64, pad=1, stride=1, transpose=False, drop_bias=False):
    """conv 4 x 4 s1 p1 -> 1 channel + bias on NCHW -> [S, 1, H - 1, W - 1], on the true output grid whatever the variant."""
    H, W = x.shape[2:]
    return conv4(x.to(dtype), w.to(dtype), None if drop_bias else bias.to(dtype), stride=stride, pad=pad, out_hw=(H - 1, W - 1),
                 transpose=transpose)


def fold_bn(weight, bias, mean, var, *, dtype=torch.float64, no_root=False):
    """Eval-mode BatchNorm2d as (a, b).  no_root: the variance used without the root."""
    den = (var.to(dtype) + BN_EPS) if no_root else torch.sqrt(var.to(dtype) + BN_EPS)
    a = weight.to(dtype) / den
    return a, bias.to(dtype) - mean.to(dtype) * a


def affine_ref(rows, a, b, *, dtype=torch.float64, act_first=False, by_pixel=False, slope=SLOPE):
    """leaky(a[c] x + b[c]) on [rows, C].  act_first: the activation before the affine; by_pixel: a, b indexed by the row."""
    x, a, b = rows.to(dtype), a.to(dtype), b.to(dtype)
    if by_pixel:
        idx = torch.arange(x.shape[0]) % x.shape[1]
        a, b = a[idx][:, None], b[idx][:, None]
    return a * leaky(x, slope) + b if act_first else leaky(a * x + b, slope)


def softplus(x):
    return F.softplus(x)


def gan_ref(real, fake, *, dtype=torch.float64, swap_signs=False, mean_over_plane=False, no_half=False):
    """dict(logits_real, logits_fake, g_loss, hinge, vanilla) of [B, 1, h, w] logits: vqperceptual.py:22-33, 111, 147-148."""
    r, f = real.to(dtype), fake.to(dtype)
    div = (r[0].numel() if mean_over_plane else r.numel())
    mean = lambda t: t.sum() / div      # noqa: E731
    half = 1.0 if no_half else 0.5
    s = -1.0 if swap_signs else 1.0
    return dict(logits_real=mean(r), logits_fake=mean(f), g_loss=-mean(f),
                hinge=half * (mean(F.relu(1.0 - s * r)) + mean(F.relu(1.0 + s * f))),
                vanilla=half * (mean(softplus(-s * r)) + mean(softplus(s * f))))


# ---- the net ---------------------------------------------------------------------------------------------
def disc_ref(sd, x, *, ndf, n_layers, use_actnorm, dtype=torch.float64, prefix="", want_hidden=False):
    """Logits [B, 1, Ho, Wo] of the image batch x from a state_dict with the reference's names; want_hidden: also the activations after
    every LeakyReLU."""
    table = layer_table(x.shape[1], ndf, n_layers)
    g = lambda k: sd[prefix + k].to(dtype)      # noqa: E731
    h = x.to(dtype)
    hidden = []
    for ci, ni, _, _, stride in table:
        bias = g(f"main.{ci}.bias") if (prefix + f"main.{ci}.bias") in sd else None
        h = F.conv2d(h, g(f"main.{ci}.weight"), bias, stride=stride, padding=1)
        if ni is not None:
            if use_actnorm:
                h = g(f"main.{ni}.scale") * (h + g(f"main.{ni}.loc"))
            else:
                h = F.batch_norm(h, g(f"main.{ni}.running_mean"), g(f"main.{ni}.running_var"), g(f"main.{ni}.weight"), g(f"main.{ni}.bias"),
                                 False, 0.0, BN_EPS)
        if ci != table[-1][0]:
            h = leaky(h)
            hidden.append(h)
    return (h, hidden) if want_hidden else h


def adopt_weight(weight, global_step, threshold=0, value=0.):
    return value if global_step < threshold else weight


def loss_ref(sd_lpips, sd_disc, x, xrec, codebook_loss, global_step, *, disc_loss, use_actnorm, dtype=torch.float64, kw=LOSS_KW,
             n_layers=3, p_loss=None):
    """(loss0, log0, loss1, log1) of vqperceptual.py:85-150 without a gradient (d_weight = 0), keys without the split prefix.
    p_loss: LPIPS values [B] to use instead of the restatement's (the GPU test composes from what the LPIPS module returned)."""
    if p_loss is None:
        p_loss = L.lpips_ref(sd_lpips, x, xrec, dtype=dtype)[0]
    p = p_loss.to(dtype).view(-1, 1, 1, 1)
    rec = (x.to(dtype) - xrec.to(dtype)).abs() + kw["perceptual_weight"] * p
    nll = rec.mean()
    dk = dict(ndf=kw["disc_ndf"], n_layers=n_layers, use_actnorm=use_actnorm, dtype=dtype)
    terms = gan_ref(disc_ref(sd_disc, x, **dk), disc_ref(sd_disc, xrec, **dk), dtype=dtype)
    factor = adopt_weight(kw["disc_factor"], global_step, threshold=kw["disc_start"])
    cb = torch.as_tensor(codebook_loss, dtype=dtype).mean()
    loss0 = nll + 0.0 * factor * terms["g_loss"] + kw["codebook_weight"] * cb
    zero = torch.zeros((), dtype=dtype)
    log0 = dict(total_loss=loss0, quant_loss=cb, nll_loss=nll, rec_loss=rec.mean(), p_loss=p.mean(), rec_aux_loss=zero, d_weight=zero,
                disc_factor=torch.as_tensor(float(factor), dtype=dtype), g_loss=terms["g_loss"])
    loss1 = factor * terms[disc_loss]
    log1 = dict(disc_loss=loss1, logits_real=terms["logits_real"], logits_fake=terms["logits_fake"])
    return loss0, log0, loss1, log1


def sample_index(numel, layer, ci):
    """SAMPLES flat positions of a hidden tensor of numel elements: the same on the recording and on the checking side."""
    g = torch.Generator().manual_seed(5000 + 10 * ci + layer)
    return torch.randint(0, numel, (SAMPLES,), generator=g)


def clip_shares(real, fake):
    """(share of the real logits above +1, share of the fake logits below -1)."""
    return float((real > 1).double().mean()), float((fake < -1).double().mean())

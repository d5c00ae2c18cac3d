"""Batch-sharded sampling over the GPUs of one node.

Every image is independent end to end (GroupNorm / LayerNorm / attention are per sample), so the
global batch is partitioned contiguously over ranks, each rank runs the identical captured program on
its shard with noise keyed by (seed, GLOBAL sample index), and the decoded images are joined by ONE
RCCL all-gather over xGMI (`torch.distributed` backend "nccl" is RCCL on ROCm).  The reference's
equivalent is N share-nothing processes writing PNGs (scripts/sample_diffusion.py:88-100,435-448).
"""
import torch
import torch.distributed as dist


def shard_range(total, rank, world):
    """Contiguous [lo, hi) slice of `total` samples owned by `rank` (sizes differ by at most 1)."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def all_gather_images(local, total=None, group=None):
    """One collective joining per-rank image shards [b_r, ...] -> [sum b_r, ...] on every rank.
    Equal shards use all_gather_into_tensor (a single RCCL all-gather); ragged shards are padded to the
    largest shard first."""
    if not (dist.is_available() and dist.is_initialized()):
        return local
    world = dist.get_world_size(group)
    total = total if total is not None else local.shape[0] * world
    sizes = [shard_range(total, r, world) for r in range(world)]
    bmax = max(hi - lo for lo, hi in sizes)
    buf = local
    if local.shape[0] != bmax:
        buf = torch.zeros((bmax,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        buf[: local.shape[0]] = local
    if local.is_cuda and dist.get_backend(group) == "gloo":
        # (r05) device tensors under the CPU backend -- two ranks sharing ONE GPU in tests/test_model_gpu.py, where RCCL has no second
        # device to talk to: the shards are staged through host memory; the RCCL path below is untouched
        host = torch.empty((world * bmax,) + tuple(local.shape[1:]), dtype=local.dtype)
        dist.all_gather_into_tensor(host, buf.contiguous().cpu(), group=group)
        out = host.to(local.device)
    else:
        out = torch.empty((world * bmax,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, buf.contiguous(), group=group)
    if all(hi - lo == bmax for lo, hi in sizes):
        return out
    return torch.cat([out[r * bmax: r * bmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)], dim=0)


def _guide_kw(compose, guidance_rescale):
    """The samplers' composed-guidance keywords, passed only when one is in use: a call without them is the call it always was."""
    return dict(compose=compose, guidance_rescale=guidance_rescale) if compose is not None or guidance_rescale else {}


@torch.no_grad()
def sample_images(model, cond, *, S, eta=1.0, sampler="ddim", scale=1.0, uncond=None, seed=0, sample0=0, noise="philox",
                  num_stage=None, gather=True, total=None, log_every_t=10 ** 9, gather_dtype="float32", check_status=True, compose=None,
                  guidance_rescale=0.0):
    """cond: this rank's conditioning shard [b, nctx, cd] on the GPU.  Returns decoded images (gathered).
    compose / guidance_rescale: composed guidance (the samplers' keywords; `scale` is the weight of `cond`); every conditioning of
    `compose` is this rank's shard, cut like `cond` (shard_range).
    gather_dtype "float32": (N, 3, H, W) f32 in [-1, 1] (what decode_first_stage returns; 25 MB / rank at 32 images);
    "uint8" / "uint8_pil": the (N, H, W, 3) uint8 images of scripts/sample_diffusion.py custom_to_np (:115-121) / custom_to_pil
    (:103-113), produced by the decoder's last epilogue -- the one all-gather then moves 6.3 MB / rank.
    check_status (r05): after the decode, read the library's sticky numerics word (frido_status_flags: one device sync per pass) and
    turn a saturated fp16 operand plane or a non-finite normalisation statistic into a FridoNumericsWarning."""
    from .samplers import DDIMSampler, PLMSSampler
    unet = model.model.diffusion_model
    b = cond.shape[0]
    shape = (unet.in_channels, unet.image_size, unet.image_size)
    guide = _guide_kw(compose, guidance_rescale)
    if sampler == "ddpm":
        # the ancestral loop (FridoDiffusion.p_sample_loop): S = chain length (t = S - 1 ... 0 per stage); it has no guidance, its noise
        # level is the posterior's (what eta = 1 means to DDIM) and it always walks every stage of the model
        if scale != 1.0 or uncond is not None or compose is not None or guidance_rescale:
            raise ValueError("sampler='ddpm': the ancestral loop has no classifier-free guidance (scale must be 1.0, uncond None, no compose / "
                             "guidance_rescale)")
        if eta != 1.0:
            raise ValueError(f"sampler='ddpm': the ancestral loop has no eta (got {eta}; leave it at 1.0)")
        if num_stage is not None and num_stage != model.num_resulotion:
            raise ValueError(f"sampler='ddpm': the ancestral loop runs all {model.num_resulotion} stages of the model (got num_stage={num_stage})")
        z = model.p_sample_loop(cond, (b,) + shape, timesteps=S, verbose=False, log_every_t=log_every_t, noise=noise, seed=seed,
                                sample0=sample0)
    elif sampler == "dpm":
        # DPM-Solver++(2M), 2nd order on the logSNR grid (DPMSolverSampler's defaults): deterministic, so eta -- this function's default is
        # DDIM's 1.0 -- has nothing to set; any other value is refused
        if eta not in (0.0, 1.0):
            raise ValueError(f"sampler='dpm': the solver is deterministic and has no eta (got {eta}; leave it at its default)")
        from .samplers import DPMSolverSampler
        z, _ = DPMSolverSampler(model).sample(S=S, batch_size=b, shape=shape, conditioning=cond, num_stage=num_stage or unet.num_stage,
                                              verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=uncond,
                                              noise=noise, seed=seed, sample0=sample0, log_every_t=log_every_t, **guide)
    else:
        cls = PLMSSampler if sampler == "plms" else DDIMSampler
        z, _ = cls(model).sample(S=S, batch_size=b, shape=shape, conditioning=cond, num_stage=num_stage or unet.num_stage,
                                 eta=eta, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=uncond,
                                 noise=noise, seed=seed, sample0=sample0, log_every_t=log_every_t, **guide)
    if gather_dtype == "float32":
        img = model.decode_first_stage(z)
    elif gather_dtype in ("uint8", "uint8_pil"):
        img = model.decode_first_stage(z, to_uint8="pil" if gather_dtype == "uint8_pil" else "np")
    else:
        raise ValueError(f"gather_dtype {gather_dtype!r}: 'float32', 'uint8' or 'uint8_pil'")
    if check_status and img.is_cuda:
        from . import _lib
        _lib.warn_on_status("sample_images")
    return all_gather_images(img, total=total) if gather else img


@torch.no_grad()
def edit_images(model, images, cond, *, S, strength, keep_mask=None, eta=1.0, scale=1.0, uncond=None, seed=0, sample0=0, noise="philox",
                num_stage=None, init="z0", reimpose=True, gather=True, total=None, log_every_t=10 ** 9, gather_dtype="float32",
                check_status=True, compose=None, guidance_rescale=0.0):
    """Image-to-image / inpainting on this rank's shard: images (b, 3, H, W) in [-1, 1] on the GPU -> encode_first_stage +
    get_first_stage_encoding -> DDIMSampler.edit (the last clamp(int(strength * S), 1, S) of S steps per stage) -> decode_first_stage.
    keep_mask (b, 1, H, W) in [0, 1] over the PIXELS, 1 = keep: min-pooled to the latent grid (a latent cell is kept only if every pixel
    it decodes to is).  Noise is keyed by (seed, GLOBAL sample index = sample0 + i), so a sharded run equals the whole batch; gather /
    gather_dtype / check_status / compose / guidance_rescale as in sample_images."""
    from .samplers import DDIMSampler
    unet = model.model.diffusion_model
    z0 = model.get_first_stage_encoding(model.encode_first_stage(images))
    m = None
    if keep_mask is not None:
        if keep_mask.dim() != 4 or keep_mask.shape[:2] != (images.shape[0], 1) or keep_mask.shape[2:] != images.shape[2:]:
            raise ValueError(f"edit_images: keep_mask must be {(images.shape[0], 1) + tuple(images.shape[2:])}, got {tuple(keep_mask.shape)}")
        f = images.shape[2] // z0.shape[2]
        m = -torch.nn.functional.max_pool2d(-keep_mask.float(), f, f) if f > 1 else keep_mask.float()
    z, _ = DDIMSampler(model).edit(S, z0, cond, strength=strength, keep_mask=m, init=init, reimpose=reimpose, num_stage=num_stage or unet.num_stage,
                                   eta=eta, unconditional_guidance_scale=scale, unconditional_conditioning=uncond, noise=noise, seed=seed,
                                   sample0=sample0, log_every_t=log_every_t, verbose=False, **_guide_kw(compose, guidance_rescale))
    if gather_dtype == "float32":
        img = model.decode_first_stage(z)
    elif gather_dtype in ("uint8", "uint8_pil"):
        img = model.decode_first_stage(z, to_uint8="pil" if gather_dtype == "uint8_pil" else "np")
    else:
        raise ValueError(f"gather_dtype {gather_dtype!r}: 'float32', 'uint8' or 'uint8_pil'")
    if check_status and img.is_cuda:
        from . import _lib
        _lib.warn_on_status("edit_images")
    return all_gather_images(img, total=total) if gather else img


@torch.no_grad()
def invert_images(model, images, cond, *, S, t_start=None, strength=None, scale=1.0, uncond=None, first_stage=0, num_stage=None, sample0=0,
                  gather=True, total=None, log_every_t=10 ** 9, check_status=True):
    """DDIM inversion of this rank's shard: images (b, 3, H, W) in [-1, 1] on the GPU -> encode_first_stage + get_first_stage_encoding ->
    DDIMSampler.invert (the first k of S rows per stage, k = t_start or clamp(int(strength * S), 1, S)).  Returns the inverted latents
    x_inv (gathered), to hand to DDIMSampler.edit(S, z0, c, init="noise", x_T=x_inv, t_start=k, first_stage=first_stage, eta=0).
    Every sample is inverted on its own and nothing is drawn, so a shard of the batch equals the same rows of the whole batch whatever
    its global sample index `sample0` is; gather / total / check_status as in edit_images."""
    from .samplers import DDIMSampler
    unet = model.model.diffusion_model
    z0 = model.get_first_stage_encoding(model.encode_first_stage(images))
    x_inv, _ = DDIMSampler(model).invert(S, z0, cond, t_start=t_start, strength=strength, first_stage=first_stage,
                                         num_stage=num_stage or unet.num_stage, unconditional_guidance_scale=scale,
                                         unconditional_conditioning=uncond, log_every_t=log_every_t, verbose=False)
    if check_status and x_inv.is_cuda:
        from . import _lib
        _lib.warn_on_status("invert_images")
    return all_gather_images(x_inv, total=total) if gather else x_inv


def _l2norm_rows(z):
    """z / ||z||_2 per row of a [B, C] f32 tensor on the GPU, by the library's row kernel (FRIDO_OP_L2NORM) on the current stream."""
    from .engine import Prog, current_stream_ptr
    z = z.float().contiguous()
    out = torch.empty_like(z)
    p = Prog(z.device, 2)
    p.emit("FRIDO_OP_L2NORM", x=z.data_ptr(), out=out.data_ptr(), rows=z.shape[0], C=z.shape[1])
    p.run(current_stream_ptr(z.device))
    return out


@torch.no_grad()
def clip_score(image_embedder, text_embedder, images, text):
    """Cosine between the CLIP embeddings of images and their captions: [B] float32 on the device, without leaving it.
    image_embedder: a FrozenClipImageEmbedder; images [B, 3, H, W] in [-1, 1] on the GPU (what the decoders return).
    text_embedder: a FrozenCLIPTextEmbedder of the same embed_dim; text: [B, n] token ids, or strings under that class's own rules.
    Both embeddings are L2-normalised by the library's row kernel (the text tower's own when it was built with normalize=True);
    the row dot product is one torch expression on [B, embed_dim].
    CLIPScore (Hessel et al. 2021, "CLIPScore: A Reference-free Evaluation Metric for Image Captioning") is 2.5 * max(cos, 0) of the
    value returned here, taken with a TRAINED CLIP.  No trained weights ship with this repository: the function computes the quantity
    for whatever state_dict the two embedders hold, and nothing here claims a quality number.
    Under torch.distributed every rank scores its own shard; gathering the scores is the caller's."""
    from .models import FrozenCLIPTextEmbedder, FrozenClipImageEmbedder
    if not isinstance(image_embedder, FrozenClipImageEmbedder):
        raise ValueError(f"clip_score: image_embedder must be a FrozenClipImageEmbedder, got {type(image_embedder).__name__}")
    if not isinstance(text_embedder, FrozenCLIPTextEmbedder):
        raise ValueError(f"clip_score: text_embedder must be a FrozenCLIPTextEmbedder, got {type(text_embedder).__name__}")
    if image_embedder.arch[0] != text_embedder.arch[0]:
        raise ValueError(f"clip_score: the image tower embeds into {image_embedder.arch[0]} dimensions, the text tower into "
                         f"{text_embedder.arch[0]}: the two are not halves of one CLIP")
    zi = _l2norm_rows(image_embedder(images))
    zt = text_embedder(text)
    if not text_embedder.normalize:
        zt = _l2norm_rows(zt)
    if zt.shape != zi.shape:
        raise ValueError(f"clip_score: {zi.shape[0]} images but {zt.shape[0]} captions")
    return (zi * zt).sum(dim=-1)


@torch.no_grad()
def reconstruction_metrics(first_stage, images, lpips, *, perceptual_weight=1.0, discriminator=None):
    """What a tokenizer is judged by, per sample: a dict of [B] float32 tensors on the device for images [B, 3, H, W] in [-1, 1] on the GPU.
        l1         mean |x - xrec|
        mse, psnr  on [-1, 1], peak 2: psnr = 10 log10(4 / mse) (inf for an exact reconstruction)
        lpips      lpips(x, xrec), a frido_amd.models.LPIPS
        quant_loss the codebook loss `diff` of MSFPNVQModel.forward: ONE number for the batch (a mean over it, like the reference's),
                   repeated per sample; absent for a VQModelInterface
        nll_loss   l1 + perceptual_weight * lpips; its batch mean is taming/modules/losses/vqperceptual.py:85-100's nll_loss for
                   xrec_aux=None (mean over the batch of |x - xrec| + w * p_loss, p_loss broadcast over the pixels)
    first_stage: an MSFPNVQModel (its forward's `dec` and `diff`) or a VQModelInterface (encode -> decode).  The reconstruction and the
    perceptual distance run on the HIP engine; the per-sample means are torch reductions of the two images.
    discriminator: an NLayerDiscriminator adds, per sample, the means of its logit maps,
        logits_real  on the image,  logits_fake  on the reconstruction
    from one run of both through the net (the batch means of vqperceptual.py:147-148 are their means; the whole loss with g_loss and
    disc_loss is VQLPIPSWithDiscriminator.evaluate).  With filler or freshly initialised weights they say nothing about image quality.
    With the weights of LPIPS's own init the `lpips` entry measures nothing
    perceptual: load vgg.pth and a vgg16 state_dict for the published metric.
    Under torch.distributed every rank scores its own shard; gathering the scores is the caller's."""
    from .models import LPIPS, MSFPNVQModel, NLayerDiscriminator, VQModelInterface
    if not isinstance(lpips, LPIPS):
        raise ValueError(f"reconstruction_metrics: lpips must be a frido_amd.models.LPIPS, got {type(lpips).__name__}")
    if discriminator is not None and not isinstance(discriminator, NLayerDiscriminator):
        raise ValueError(f"reconstruction_metrics: discriminator must be a frido_amd.models.NLayerDiscriminator, got {type(discriminator).__name__}")
    if isinstance(first_stage, MSFPNVQModel):
        out = first_stage(images)
        xrec, diff = out[0], out[-2]          # (dec, diff, info), or (dec, aux, diff, info) under use_aux_loss
    elif isinstance(first_stage, VQModelInterface):
        xrec, diff = first_stage.decode(first_stage.encode(images)), None
    else:
        raise ValueError(f"reconstruction_metrics: first_stage must be an MSFPNVQModel or a VQModelInterface, got {type(first_stage).__name__}")
    x = images.float()
    xrec = xrec.float()
    err = x - xrec
    l1 = err.abs().mean(dim=(1, 2, 3))
    mse = (err * err).mean(dim=(1, 2, 3))
    lp = lpips(x.contiguous(), xrec.contiguous()).view(-1)
    res = dict(l1=l1, mse=mse, psnr=10.0 * torch.log10(4.0 / mse), lpips=lp, nll_loss=l1 + float(perceptual_weight) * lp)
    if diff is not None:
        res["quant_loss"] = diff.float().reshape(1).expand(x.shape[0]).clone()
    if discriminator is not None:
        per = discriminator.pair(x.contiguous(), xrec.contiguous()).per_sample.clone()
        res["logits_real"], res["logits_fake"] = per[:x.shape[0]], per[x.shape[0]:]
    return res


@torch.no_grad()
def fid_statistics(extractor, images, stats=None):
    """The running feature statistics of a Fréchet Inception Distance after `images` were added: extractor(images) -> [B, 2048] float32
    on the device, then one launch that adds sum x and sum x x^T in float64 (frido_amd.fid.FeatureStatistics.update).
    extractor: a frido_amd.models.FIDInceptionV3; images: uint8 [B, H, W, 3] (what sample_images gathers) or float32 [B, 3, H, W] in
    [-1, 1] (what the decoders return) on the GPU; stats: the statistics so far, None starts new ones.  Returns the updated statistics.
    Under torch.distributed every rank adds its own shard; FeatureStatistics.all_gather_merge joins them in rank order."""
    from .fid import FEATURES, FeatureStatistics
    from .models import FIDInceptionV3
    if not isinstance(extractor, FIDInceptionV3):
        raise ValueError(f"fid_statistics: extractor must be a frido_amd.models.FIDInceptionV3, got {type(extractor).__name__}")
    if stats is not None and not isinstance(stats, FeatureStatistics):
        raise ValueError(f"fid_statistics: stats must be a frido_amd.fid.FeatureStatistics or None, got {type(stats).__name__}")
    feats = extractor(images)
    if stats is None:
        stats = FeatureStatistics(FEATURES, feats.device)
    return stats.update(feats)


def fid(stats_a, stats_b):
    """The Fréchet distance between the Gaussians of two FeatureStatistics, a float (frido_amd.fid.frechet_distance: float64, on the
    host, once per evaluation).  With the published Inception weights loaded and enough samples on both sides this is FID; no trained
    weights ship with this repository, and with anything else in the extractor the number measures nothing about image quality."""
    from .fid import frechet_distance
    return frechet_distance(stats_a.mean(), stats_a.cov(), stats_b.mean(), stats_b.cov())


@torch.no_grad()
def fidelity_features(extractor, images, *, stats=None, feats=None, logits=None):
    """ONE run of the Inception tower on `images` for whichever of the three metrics are being collected: `stats` (a
    frido_amd.fid.FeatureStatistics, for fid) is updated with the features, `feats` (a frido_amd.fidelity.FeatureBank of width 2048, for
    kid) gets them appended, `logits` (a FeatureBank of width 1008, for inception_score) gets extractor.logits(features) appended.
    Returns (stats, feats, logits) as passed, None where None was.  extractor, images: as for fid_statistics.  Under torch.distributed
    every rank collects its own shard; FeatureStatistics.all_gather_merge and FeatureBank.all_gather_concat join them in rank order."""
    from .fid import FeatureStatistics
    from .fidelity import FeatureBank
    from .models import FIDInceptionV3
    if not isinstance(extractor, FIDInceptionV3):
        raise ValueError(f"fidelity_features: extractor must be a frido_amd.models.FIDInceptionV3, got {type(extractor).__name__}")
    if stats is not None and not isinstance(stats, FeatureStatistics):
        raise ValueError(f"fidelity_features: stats must be a frido_amd.fid.FeatureStatistics or None, got {type(stats).__name__}")
    for name, bank in (("feats", feats), ("logits", logits)):
        if bank is not None and not isinstance(bank, FeatureBank):
            raise ValueError(f"fidelity_features: {name} must be a frido_amd.fidelity.FeatureBank or None, got {type(bank).__name__}")
    f = extractor(images)
    if stats is not None:
        stats.update(f)
    if feats is not None:
        feats.append(f)
    if logits is not None:
        logits.append(extractor.logits(f))
    return stats, feats, logits


def inception_score(logit_bank, **kw):
    """(mean, std) of the Inception Score of the logits fidelity_features collected (a FeatureBank or a float32 [N, C] tensor on the
    GPU): frido_amd.fidelity.inception_score, whose docstring is the specification; splits=10, shuffle=True, rng_seed=2020.  No trained
    weights ship with this repository, and with anything else in the extractor the number measures nothing about image quality."""
    from .fidelity import inception_score as score
    return score(logit_bank, **kw)


def kid(bank_a, bank_b, **kw):
    """(mean, std) of the Kernel Inception Distance between the features of two sides (FeatureBanks or float32 [n, D] tensors on the
    GPU): frido_amd.fidelity.kernel_inception_distance, whose docstring is the specification; subsets=100, subset_size=1000, degree=3,
    gamma=None, coef0=1.0, rng_seed=2020.  No trained weights ship with this repository, and with anything else in the extractor the
    number measures nothing about image quality."""
    from .fidelity import kernel_inception_distance
    return kernel_inception_distance(bank_a, bank_b, **kw)


def precision_recall(bank_real, bank_fake, k=3, **kw):
    """{"precision", "recall", "density", "coverage", "f_score": floats, "counts": the integers behind them} between the features of the
    real and the generated side (FeatureBanks or float32 [n, D] tensors on the GPU): frido_amd.manifold.prdc, whose docstring is the
    specification; k=3, slab_bytes=512 MiB.  Under torch.distributed every rank gathers its banks with FeatureBank.all_gather_concat
    first.  No trained weights ship with this repository, and with anything else in the extractor the numbers measure nothing about
    image quality."""
    from .manifold import prdc
    return prdc(bank_real, bank_fake, k, **kw)

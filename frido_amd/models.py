"""The reference's Python class / config / state_dict surface, running on the HIP engine.

Each class keeps the constructor keywords, attribute names, method signatures and state_dict keys of
its reference counterpart (cited per class) so that configs/frido/*.yaml `target:` strings and
scripts/sample_diffusion.py keep working, but none of them contains a torch forward: tensors on a
HIP device go through libfrido_hip.so, anything else raises FridoHipError (there is no CPU path).
"""
import contextlib
import importlib

import numpy as np
import torch
import torch.nn as nn

from . import _lib, autoplanes, config, holders, runtime, schedules
from ._lib import FridoHipError
from .engine import current_stream_ptr, lru_entry, own_stream, require_gpu

try:  # pytorch-lightning is optional (absent in this image): keep the LightningModule base when it exists
    import pytorch_lightning as _pl
    _Base = _pl.LightningModule
except Exception:  # pragma: no cover
    class _Base(nn.Module):
        """Minimal stand-in for pl.LightningModule: `.device` + logging no-ops."""

        @property
        def device(self):
            for t in list(self.parameters()) + list(self.buffers()):
                return t.device
            return torch.device("cpu")

        def log(self, *a, **k):
            pass

        def log_dict(self, *a, **k):
            pass


# ---- config factory (frido/util.py:74-95) ---------------------------------------------------------
def get_obj_from_str(string, reload=False):
    module, cls = string.rsplit(".", 1)
    mod = importlib.import_module(module, package=None)
    if reload:
        importlib.reload(mod)
    return getattr(mod, cls)


def _plain(cfg):
    """OmegaConf / dict-like -> plain python containers."""
    if hasattr(cfg, "items"):
        return {k: _plain(v) for k, v in cfg.items()}
    if isinstance(cfg, (list, tuple)) or type(cfg).__name__ == "ListConfig":
        return [_plain(v) for v in cfg]
    return cfg


def instantiate_from_config(cfg):
    if "target" not in cfg:
        if cfg == "__is_first_stage__" or cfg == "__is_unconditional__":
            return None
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(cfg["target"])(**_plain(cfg.get("params", dict())))


def instantiate_from_config_main(cfg, *args, **kwargs):
    if "target" not in cfg:
        raise KeyError("Expected key `target` to instantiate.")
    return get_obj_from_str(cfg["target"])(*args, **_plain(cfg.get("params", dict())), **kwargs)


def _on_gpu(what, *things):
    """Raises FridoHipError unless every tensor of `things`, and the first parameter of every module, is on a HIP device (anything else
    among them -- None, a dict conditioning -- is passed over)."""
    for t in things:
        device = t.device if torch.is_tensor(t) else next(t.parameters()).device if isinstance(t, nn.Module) else None
        if device is not None and device.type != "cuda":
            raise FridoHipError(f"{what}: tensors are on '{device}', but the Frido hot path runs only on an MI355X HIP device "
                                "(move the model and its inputs with .cuda()); there is no CPU fallback")


class _Versioned:
    """Mixin: drops compiled HIP plans whenever the module's weights change.  _what: the class's name in its errors.  _runtime: (class of
    frido_amd.runtime, attribute holding its configuration) of the classes that run through runtime() -- the denoiser and the two first
    stages; the text towers keep a bare Builder and set none."""

    def _init_versioning(self):
        self._rt = None
        self._rt_key = None
        self.register_load_state_dict_post_hook(lambda m, k: m.invalidate())

    def invalidate(self):
        self._rt = None

    def runtime(self, precision=None):
        """The compiled runtime of the module's weights on their device, at `precision` (default: the module's, then config.PRECISION).
        Only for classes that set _runtime."""
        cls, cfg = self._runtime
        dev = next(self.parameters()).device
        key = (str(dev), precision or self.precision or config.PRECISION)
        if self._rt is None or self._rt_key != key:
            _on_gpu(self._what, self)
            self._rt = getattr(runtime, cls)(self, getattr(self, cfg), dev, key[1])
            self._rt_key = key
        return self._rt

    # which build of the library the module runs on (_lib.use_planes); the default precision keyword lets autoplanes.run() change it
    planes = property(lambda self: config.planes(getattr(self, "precision", None)))

    def _apply(self, fn, *a, **k):   # .cuda() / .to() move the weights -> recompile
        self._rt = None
        return super()._apply(fn, *a, **k)


# ---- denoiser (frido/modules/diffusionmodules/pyunet.py:447-950) -------------------------------------
class PyUNetModel(_Versioned, nn.Module):
    _what, _runtime = "PyUNetModel", ("DenoiserRuntime", "cfg")

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False,
                 use_embed=False, num_stage=1, resblock_updown=False, use_new_attention_order=False,
                 use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None, legacy=True,
                 use_split_head=False, split_embed_dim_list=[], use_SPADE_norm=False, use_pos_embed=False,
                 use_mscond=False, use_stage_expert=False, precision=None):
        super().__init__()
        if use_spatial_transformer:
            assert context_dim is not None, "context_dim is required with use_spatial_transformer"
        if num_heads == -1:
            assert num_head_channels != -1, "Either num_heads or num_head_channels has to be set"
        if context_dim is not None:
            assert use_spatial_transformer, "context_dim needs use_spatial_transformer (pyunet.py:516-517)"
        if num_head_channels == -1:
            assert num_heads != -1, "Either num_heads or num_head_channels has to be set"
        unsupported = dict(use_pos_embed=use_pos_embed, use_mscond=use_mscond, use_stage_expert=use_stage_expert, n_embed=n_embed,
                           resblock_updown=resblock_updown, use_scale_shift_norm=use_scale_shift_norm)
        bad = [k for k, v in unsupported.items() if v]
        if dims != 2:
            bad.append("dims != 2")
        if not conv_resample:
            bad.append("conv_resample=False")
        if use_spatial_transformer and not legacy:
            bad.append("legacy=False with use_spatial_transformer=True (multi-head SpatialTransformer)")
        if use_spatial_transformer and num_classes is not None:
            bad.append("num_classes with use_spatial_transformer=True")
        if bad:
            raise NotImplementedError(f"PyUNetModel options that are not built: {bad}")
        if use_split_head:
            assert len(split_embed_dim_list) != 0 and sum(split_embed_dim_list) == in_channels
        self.cfg = dict(image_size=image_size, in_channels=in_channels, model_channels=model_channels,
                        out_channels=out_channels, num_res_blocks=num_res_blocks,
                        attention_resolutions=list(attention_resolutions), channel_mult=list(channel_mult),
                        num_head_channels=num_head_channels, num_heads=num_heads,
                        use_spatial_transformer=use_spatial_transformer, transformer_depth=transformer_depth,
                        context_dim=context_dim, num_stage=num_stage, use_split_head=use_split_head,
                        split_embed_dim_list=list(split_embed_dim_list), use_SPADE_norm=use_SPADE_norm,
                        num_heads_upsample=num_heads_upsample, legacy=legacy, use_new_attention_order=use_new_attention_order,
                        num_classes=num_classes, use_embed=use_embed)
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.attention_resolutions, self.dropout = num_res_blocks, attention_resolutions, dropout
        self.channel_mult, self.conv_resample, self.num_classes = channel_mult, conv_resample, num_classes
        self.dtype = torch.float32
        self.num_heads, self.num_head_channels, self.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample
        self.predict_codebook_ids = False
        self.num_stage, self.use_split_head = num_stage, use_split_head
        self.use_embed, self.use_spatial_transformer = use_embed, use_spatial_transformer
        self.split_embed_dim_list, self.use_SPADE_norm = list(split_embed_dim_list), use_SPADE_norm
        self.precision = precision
        self.arch = holders.build_unet_params(self, self.cfg)
        self._init_versioning()

    def forward(self, x, timesteps=None, context=None, y=None, stage=None, **kwargs):
        # pyunet.py:877-879 asserts (y is not None) == (num_classes is not None)
        if y is not None and self.num_classes is None:
            raise NotImplementedError("class-conditional denoiser (num_classes / conditioning_key='adm'): this model was built without num_classes, "
                                      "so it takes no y")
        if y is None and self.num_classes is not None:
            raise ValueError("must specify y if and only if the model is class-conditional (pyunet.py:877-879)")
        if self.use_spatial_transformer and context is None:
            raise NotImplementedError("PyUNetModel.forward without a context: the reference's SpatialTransformer then attends to its own input "
                                      "(attention.py:171 `default(context, x)`); every shipped Frido config passes one, that plan is not built")
        if not self.use_spatial_transformer:
            context = None      # the AttentionBlock family ignores it (TimestepEmbedSequential, pyunet.py:81-91)
        if y is not None:
            if self.use_embed:
                assert y.shape == (x.shape[0],), "y: one class index per sample (pyunet.py:887)"
            else:
                assert y.shape == (x.shape[0], self.num_classes), "y: [B, num_classes] for the Linear label embedding"
        _on_gpu("PyUNetModel.forward", x)
        if self.num_stage > 1 and not isinstance(stage, int):
            stage = int(stage)
        return autoplanes.run(self, lambda _n: self.runtime().forward(x, timesteps, context, stage, y=y), "PyUNetModel.forward")


UNetModel = PyUNetModel   # `ldm.modules.diffusionmodules.openaimodel.UNetModel` alias used by two shipped configs


# ---- first stage (taming/models/msvqgan.py:16-96,320-399; the model of its own: 16-318) ---------------------------------------------
class DummyLoss(nn.Module):   # taming/modules/losses/vqperceptual.py:12-14
    def __init__(self, *a, **k):
        super().__init__()


class _Quantizer(nn.Module):
    """VectorQuantizer2 holder (taming/modules/vqvae/quantize.py:214-241): codebook in `.embedding.weight`."""

    def __init__(self, n_e, e_dim, beta=0.25):
        super().__init__()
        self.n_e, self.e_dim, self.beta = n_e, e_dim, beta
        self.embedding = holders.Emb(n_e, e_dim)


class _FirstStage(_Versioned, _Base):
    """What the two MS-VQGAN classes share: the holders of the reference's parameter / state_dict key set, the attributes FridoDiffusion
    and the runtime read, the no-op loss, the checkpoint load.  A subclass refuses what it does not build before it calls this constructor
    and adds its own attributes after it."""
    _runtime = ("DecoderRuntime", "vq_cfg")

    def __init__(self, edconfig, ddconfig, n_embed, embed_dim, quant_beta, *, fusion, ckpt_path, ignore_keys, image_key, monitor, precision):
        super().__init__()
        edconfig, ddconfig = _plain(edconfig), _plain(ddconfig)
        embed_dim, n_embed = list(embed_dim), list(n_embed)
        assert len(n_embed) == edconfig["multiscale"] == len(embed_dim), "multiscale mode. dim of n_embed is incorrect."
        self.image_key, self.fusion = image_key, fusion
        self.embed_dim, self.n_embed = embed_dim, n_embed
        self.edconfig, self.ddconfig = edconfig, ddconfig
        self.vq_cfg = dict(embed_dim=embed_dim, n_embed=n_embed, edconfig=edconfig, ddconfig=ddconfig)
        self.precision = precision
        holders.build_msvqgan_params(self, edconfig, ddconfig, n_embed, embed_dim)
        for i, q in enumerate(self.ms_quantize):
            q.n_e, q.e_dim, q.beta = n_embed[i], embed_dim[i], quant_beta
        self.encoder.num_resolutions = len(edconfig["ch_mult"])
        self.encoder.multiscale = edconfig["multiscale"]
        self.encoder.resolution = edconfig["resolution"]
        # lossconfig: VQLPIPSWithDiscriminator is LPIPS (VGG weights: a download) + a PatchGAN trained by the backward pass -- whatever
        # the target, the module holds the no-op loss (MSFPNVQModel's with_loss=True replaces it afterwards)
        self.loss = DummyLoss()
        nres = len(edconfig["ch_mult"])
        self.res_list = [edconfig["resolution"] / 2 ** (nres - i - 1) for i in range(edconfig["multiscale"])]
        if monitor is not None:
            self.monitor = monitor
        self._init_versioning()
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def init_from_ckpt(self, path, ignore_keys=list()):
        sd = torch.load(path, map_location="cpu")["state_dict"]
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        self.load_state_dict(sd, strict=False)


class VQModelInterface(_FirstStage):
    _what = "VQModelInterface"

    def __init__(self, embed_dim, channel_range=[], edconfig=None, ddconfig=None, lossconfig=None, n_embed=None,
                 fusion="concat", ckpt_path=None, ignore_keys=[], image_key="image", colorize_nlabels=None, monitor=None,
                 remap=None, sane_index_shape=False, on_vit=[], use_aux_loss=False, unsample_type="nearest",
                 quant_beta=0.25, legacy=True, init_normal=False, precision=None):
        assert fusion == "concat" and remap is None, "only the 'concat' fusion without remap is used by Frido configs"
        super().__init__(edconfig, ddconfig, n_embed, embed_dim, quant_beta, fusion=fusion, ckpt_path=ckpt_path, ignore_keys=ignore_keys,
                         image_key=image_key, monitor=monitor, precision=precision)
        self.channel_range = channel_range

    @torch.no_grad()
    def decode(self, h_in, force_not_quantize=False, return_code=False, inv_scale=None, to_uint8=False, force_codes=None):
        """msvqgan.py:376-399.  Returns dec (B,3,H,W) [and per-scale code lists when return_code]; to_uint8 (True / "np" /
        "pil") returns the (B,H,W,3) uint8 image of scripts/sample_diffusion.py:115-121 (custom_to_np) or :103-113
        (custom_to_pil) straight from the epilogue of the decoder's last convolution."""
        _on_gpu("VQModelInterface.decode", h_in)
        # force_not_quantize: accepted and IGNORED, exactly like the reference (msvqgan.py:376-399 never reads the flag: the
        # multi-scale decode always quantises)
        out = autoplanes.run(self, lambda _n: self.runtime().decode(h_in, inv_scale=inv_scale, return_code=return_code, to_uint8=to_uint8,
                                                                    force_codes=force_codes), "VQModelInterface.decode")
        if return_code:
            dec, idx = out
            return dec, [i.tolist() for i in idx]     # the reference's host lists (msvqgan.py:390)
        return out

    @torch.no_grad()
    def encode(self, x, scale=None):
        """msvqgan.py:326-374: image (B,3,H,W) -> pre-quant multi-scale latent, channels [coarse .. fine]."""
        _on_gpu("VQModelInterface.encode", x)
        assert len(self.channel_range) != 2, "channel_range slicing is not used by any shipped config"
        return autoplanes.run(self, lambda _n: self.runtime().encode(x, scale=scale), "VQModelInterface.encode")


class MSFPNVQModel(_FirstStage):
    """taming/models/msvqgan.py:16-318: the MS-VQGAN as a model of its own -- what `main.py -t False` runs on configs/msvqgan/*.yaml.
    Where VQModelInterface hands the diffusion model the PRE-quant latent, this class returns what the tokenizer itself computes: the
    quantised multi-scale latent, the codes of every scale and the codebook loss (encode), an image from an already quantised latent
    (decode), the reconstruction (forward) and the per-scale reconstructions (log_images).

    CHANNEL ORDER: `quant` is [fine .. coarse] (the reference reverses its list before the concat, msvqgan.py:146), coarser scales
    nearest-upsampled to the finest grid -- the OPPOSITE of VQModelInterface.encode's [coarse .. fine].
    Same parameter / state_dict key set as the reference's class; no backward pass.  The loss module is the no-op DummyLoss unless the
    model is built with `with_loss=True`: then `lossconfig` is instantiated (VQLPIPSWithDiscriminator: LPIPS + the PatchGAN
    discriminator, forward-only) and `validation_step` evaluates it."""

    _what = "MSFPNVQModel"

    def __init__(self, edconfig, ddconfig, lossconfig, n_embed, embed_dim, fusion="concat", ckpt_path=None, ignore_keys=[],
                 image_key="image", colorize_nlabels=None, monitor=None, remap=None, sane_index_shape=False, on_vit=[],
                 use_aux_loss=False, unsample_type="nearest", quant_beta=0.25, legacy=True, init_normal=False, precision=None, *,
                 with_loss=False):
        if remap is not None:
            raise NotImplementedError("remap: the quantiser's index remapping (quantize.py:229-241) is not built; no shipped config sets it")
        if fusion != "concat":
            raise NotImplementedError(f"fusion={fusion!r}: only the 'concat' fusion of the scales is built (msvqgan.py:59-66; every shipped config)")
        if _plain(edconfig).get("double_z") or _plain(ddconfig).get("double_z"):
            raise NotImplementedError("double_z=True: a quantised model has no use for the doubled moments (every shipped config sets double_z: False)")
        if colorize_nlabels is not None:
            raise NotImplementedError("colorize_nlabels: the random `colorize` projection of segmentation inputs (to_rgb, msvqgan.py:311-317) is not built")
        super().__init__(edconfig, ddconfig, n_embed, embed_dim, quant_beta, fusion=fusion, ckpt_path=ckpt_path, ignore_keys=ignore_keys,
                         image_key=image_key, monitor=monitor, precision=precision)
        self.vq_cfg.update(quant_beta=float(quant_beta), legacy=bool(legacy))
        for q in self.ms_quantize:
            q.legacy, q.sane_index_shape = legacy, sane_index_shape
        self.use_aux_loss, self.unsample_type = use_aux_loss, unsample_type
        self.sane_index_shape, self.quant_beta, self.legacy = sane_index_shape, quant_beta, legacy
        if with_loss:
            # opt-in: the lossconfig is instantiated (a DummyLoss target stays the no-op); the state_dict then carries the reference's
            # `loss.perceptual_loss.*` / `loss.discriminator.*` keys.  The checkpoint, if any, is read again so that they load.
            lossconfig = _plain(lossconfig)
            if not str(lossconfig.get("target", "")).endswith("DummyLoss"):
                if precision is not None:      # the loss's two networks run on the build the tokenizer runs on
                    lossconfig = dict(lossconfig, params=dict(lossconfig.get("params") or {}, precision=precision))
                self.loss = instantiate_from_config(lossconfig)
                if ckpt_path is not None:
                    self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    global_step = 0      # what a trainer counts; validation_step hands it to the loss (disc_factor is 0 before disc_start)

    def _check_image(self, x, what):
        if x.shape[1] > 3:
            raise NotImplementedError(f"{what}: inputs with more than 3 channels (segmentation maps through to_rgb's random `colorize` "
                                      "projection, msvqgan.py:283-287,311-317) are not built")
        _on_gpu(what, x)

    def _info(self, idx, B, h, w):
        """msvqgan.py:121,142-143 with VectorQuantizer2's (perplexity, min_encodings, min_encoding_indices) = (None, None, idx)."""
        n = len(idx)
        if self.sane_index_shape:       # quantize.py:304-306
            idx = [i.view(B, h >> (n - 1 - s), w >> (n - 1 - s)) for s, i in enumerate(idx)]
        return [[None] * n, [None] * n, list(idx)]

    @torch.no_grad()
    def encode(self, x):
        """msvqgan.py:116-154: image (B, 3, H, W) -> (quant, emb_loss, info_ms).  quant: channels [fine .. coarse], each scale the
        reference's z + (z_q - z) in fp32; emb_loss: 0-d f32, the scales' losses added coarse to fine; info_ms[2]: int64 codes per scale,
        coarse first."""
        self._check_image(x, "MSFPNVQModel.encode")
        quant, loss, idx = autoplanes.run(self, lambda _n: self.runtime().encode_quant(x), "MSFPNVQModel.encode")
        return quant, loss, self._info(idx, quant.shape[0], quant.shape[2], quant.shape[3])

    @torch.no_grad()
    def decode(self, quant, to_uint8=False):
        """msvqgan.py:156-159: post_quant_conv + decoder on an already quantised [fine .. coarse] latent -- NO VQ lookup (that is
        VQModelInterface.decode).  to_uint8 as on VQModelInterface.decode."""
        _on_gpu("MSFPNVQModel.decode", quant)
        return autoplanes.run(self, lambda _n: self.runtime().decode_quant(quant.contiguous().float(), to_uint8=to_uint8), "MSFPNVQModel.decode")

    def decode_code(self, code_b):
        raise NotImplementedError("decode_code: the reference's own reads `self.quantize`, which the multi-scale model does not have (it raises "
                                  "AttributeError, msvqgan.py:161-164); decode given codes with VQModelInterface.decode(force_codes=...)")

    @torch.no_grad()
    def forward(self, input, return_info=False):
        """msvqgan.py:166-186: (dec, diff, info), or (dec, [dec_aux, dec_aux2], diff, info) under use_aux_loss.  Encoder, loss and decoder
        replay as one captured graph per input shape; the two aux decodes (quant with all but its last / its first embed_dim[-1] channels
        zeroed) run only under use_aux_loss, batched with the main decode."""
        return self._reconstruct(input)[0]

    def _reconstruct(self, x):
        """(what forward returns, quant)."""
        self._check_image(x, "MSFPNVQModel.forward")
        aux = bool(self.use_aux_loss)
        dec, quant, diff, idx = autoplanes.run(self, lambda _n: self.runtime().reconstruct(x, aux=aux), "MSFPNVQModel.forward")
        info = self._info(idx, quant.shape[0], quant.shape[2], quant.shape[3])
        if aux:
            B = x.shape[0]
            return (dec[:B], [dec[B:2 * B], dec[2 * B:]], diff, info), quant
        return (dec, diff, info), quant

    def get_input(self, batch, k):
        """msvqgan.py:188-193."""
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        x = x.permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format)
        return x.float()

    def get_img_ids(self, batch):
        """msvqgan.py:195-197."""
        return batch["file_name"]

    def get_last_layer(self):
        return self.decoder.conv_out.weight

    def training_step(self, batch, batch_idx, optimizer_idx=0):
        raise FridoHipError("training_step: no backward pass exists on the HIP path (encode / decode / forward / log_images evaluate the "
                            "tokenizer without gradients)")

    def configure_optimizers(self):
        raise FridoHipError("configure_optimizers: no backward pass exists on the HIP path, so there is nothing to optimise")

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        """msvqgan.py:223-242 with a VQLPIPSWithDiscriminator in `self.loss` (with_loss=True, or assigned): forward, the loss for both
        optimizer indices from one evaluation, `self.log` / `self.log_dict`.  Returns the merged dict of the two logs (the reference
        returns the bound method `self.log_dict`)."""
        if isinstance(self.loss, DummyLoss):
            raise NotImplementedError("validation_step: its loss module is LPIPS + a PatchGAN discriminator (VQLPIPSWithDiscriminator), whose weights "
                                      "are a download / come from training; the part of the objective that exists here is the codebook loss, encode()[1]")
        if self.use_aux_loss:
            raise NotImplementedError("validation_step: use_aux_loss=True hands the loss xrec_aux, whose term the reference's own "
                                      "vqperceptual.py:96 cannot evaluate (an in-place add of a [B, 3, H, W] tensor into a [1] tensor)")
        x = self.get_input(batch, self.image_key).to(self.device)
        xrec, qloss, _ = self(x)
        (aeloss, log_dict_ae), (discloss, log_dict_disc) = self.loss.evaluate(qloss, x, xrec, self.global_step, split="val")
        self.log("val/rec_loss", log_dict_ae["val/rec_loss"], prog_bar=True, logger=True, on_step=True, on_epoch=True, sync_dist=True)
        self.log("val/aeloss", aeloss, prog_bar=True, logger=True, on_step=True, on_epoch=True, sync_dist=True)
        self.log_dict(log_dict_ae)
        self.log_dict(log_dict_disc)
        return {**log_dict_ae, **log_dict_disc}

    def test_step(self, batch, batch_idx):
        """msvqgan.py:244-245."""
        return None

    @torch.no_grad()
    def log_images(self, batch, **kwargs):
        """msvqgan.py:266-309: inputs, reconstructions, codebook_info, file_name when the batch has it, reconstructions_aux under
        use_aux_loss, and per scale the decode of quant with every other scale's channels zeroed -- all scales as one decoder batch."""
        log = dict()
        x = self.get_input(batch, self.image_key)
        try:
            log["file_name"] = self.get_img_ids(batch)
        except Exception:
            pass
        x = x.to(self.device)
        out, quant = self._reconstruct(x)
        if self.use_aux_loss:
            xrec, xrec_aux, _, info = out
            log["reconstructions_aux"] = xrec_aux
        else:
            xrec, _, info = out
        log["codebook_info"] = [info[2]]
        log["inputs"] = x
        log["reconstructions"] = xrec
        if len(self.embed_dim) >= 2:
            # (the reference encodes x a second time here, msvqgan.py:294: the same quant)
            groups = [(sum(self.embed_dim[:i]), sum(self.embed_dim[:i + 1])) for i in range(len(self.embed_dim))]
            recs = autoplanes.run(self, lambda _n: self.runtime().decode_quant(quant, groups=groups), "MSFPNVQModel.log_images")
            B = x.shape[0]
            for i, (c0, c1) in enumerate(groups):
                log[f"reconstructions_{c0}_{c1}"] = recs[i * B:(i + 1) * B]
        return log


PLAN_CACHE_SIZE = 4      # compiled cond-stage plans kept per (batch, tokens) shape (like samplers.ENGINE_CACHE_SIZE)


def _cached_plan(cache, key, builder, make):
    """LRU of compiled plans on one Builder.  A plan is built inside `persist_scope()`, so its persistent buffers (V^T operands,
    token / output tensors' companions) belong to the cache entry: evicting the least-recently-used shape frees their HBM
    instead of pinning one set per batch size ever seen.  The packed weights stay shared in the builder."""
    def build():
        with builder.persist_scope() as owned:
            return make(), owned
    return lru_entry(cache, key, PLAN_CACHE_SIZE, build)[0]


# ---- cond stage (frido/modules/encoders/modules.py:85-114) ---------------------------------------------
class _TextTower(_Versioned, nn.Module):
    """A text encoder on the HIP engine: one Builder over the weights (`_rt`) and an LRU of compiled plans per (batch, tokens) shape
    (`_plans`).  A subclass supplies _tokens(text) -> ids, _make_plan(B, n) and, where a plan has per-call inputs beside the ids,
    _bind(plan, tokens)."""

    def _init_versioning(self):
        super()._init_versioning()
        self._plans = {}

    def invalidate(self):
        self._rt = None
        self._plans = {}

    def _bind(self, plan, tokens):
        pass

    @torch.no_grad()
    @_lib.with_planes
    def _run(self, text):
        """(the plan of the tokens' shape after its program ran on them, the ids on the device)."""
        tokens = self._tokens(text)
        _on_gpu(self._what, self)
        dev = next(self.parameters()).device
        tokens = tokens.to(dev).long()
        B, n = tokens.shape
        self._check_length(n)
        if self._rt is None:
            self._rt = runtime.module_builder(self, dev, self.precision)
        plan = _cached_plan(self._plans, (B, n), self._rt, lambda: self._make_plan(B, n))
        plan.tokens.copy_(tokens.reshape(-1))
        self._bind(plan, tokens)
        plan.prog.run(current_stream_ptr(dev))
        return plan, tokens


class BERTEmbedder(_TextTower):
    """Token ids -> x-transformer encoder embeddings [B, n, n_embed] on the HIP engine."""
    _what = "BERTEmbedder"

    def __init__(self, n_embed, n_layer, vocab_size=30522, max_seq_len=77, device="cuda", use_tokenizer=True,
                 embedding_dropout=0.0, cond_key="", precision=None, vocab_file=None):
        super().__init__()
        self.use_tknz_fn = use_tokenizer      # strings -> ids needs the tokenizer's vocabulary: resolved lazily, at encode time
        self.tokenizer = None
        self.vocab_file = vocab_file          # local bert-base-uncased vocab.txt (else $FRIDO_BERT_VOCAB, else the HF cache)
        self.n_embed, self.n_layer, self.vocab_size, self.max_seq_len = n_embed, n_layer, vocab_size, max_seq_len
        self.cond_key, self.precision = cond_key, precision
        holders.build_bert_params(self, n_embed, n_layer, vocab_size, max_seq_len)
        self._init_versioning()

    def _tokens(self, text):
        tokens = text[self.cond_key] if self.cond_key != "" else text
        # captions as strings (use_tokenizer=True configs): encoders/modules.py:63-64,99-104
        return tokens if torch.is_tensor(tokens) else self._tokenize(tokens)

    def _check_length(self, n):
        assert n <= self.max_seq_len

    def _make_plan(self, B, n):
        from .bert_plan import BertPlan
        return BertPlan(self._rt, B=B, n=n, dim=self.n_embed, depth=self.n_layer, vocab=self.vocab_size)

    def forward(self, text, return_token=False):
        plan, tokens = self._run(text)
        z = plan.out.view(*tokens.shape, self.n_embed).clone()
        return (z, tokens) if return_token else z

    def encode(self, text):
        return self(text)

    def _tokenize(self, text):
        """BERTTokenizer of the reference (encoders/modules.py:57-82): `bert-base-uncased`, [CLS] .. [SEP] padded / truncated to
        max_seq_len.  The vocabulary is a download, so it is looked for (1) in a local vocab.txt (`vocab_file=` / $FRIDO_BERT_VOCAB:
        frido_amd/tokenizers.py WordPieceTokenizer, the published BasicTokenizer + WordPiece algorithm), (2) in the local HF cache
        through `transformers`; with neither a clear error is raised.  Token-id and conditioning tensors never come here."""
        if self.tokenizer is None:
            from .tokenizers import WordPieceTokenizer, local_bert_vocab
            vf = local_bert_vocab(self.vocab_file)
            if vf is not None:
                self.tokenizer = WordPieceTokenizer(vf)
        if self.tokenizer is None:
            try:
                from transformers import BertTokenizerFast
                tk = BertTokenizerFast.from_pretrained("bert-base-uncased", local_files_only=True)
                if tk.vocab_size < 30000:       # transformers >= 5 hands back an EMPTY tokenizer when the files are missing
                    raise FileNotFoundError("vocabulary not found")
                self.tokenizer = tk
            except Exception as e:
                raise NotImplementedError(
                    "BERTEmbedder: captions given as strings need the 'bert-base-uncased' vocabulary, which is not reachable "
                    f"offline ({type(e).__name__}); pass vocab_file= / set FRIDO_BERT_VOCAB to a local vocab.txt, or pass token "
                    "ids ([B, n] int64) or the conditioning tensor instead") from None
        from .tokenizers import WordPieceTokenizer
        if isinstance(self.tokenizer, WordPieceTokenizer):
            return self.tokenizer(text, max_length=self.max_seq_len)
        enc = self.tokenizer(text, truncation=True, max_length=self.max_seq_len, return_length=True, return_overflowing_tokens=False,
                             padding="max_length", return_tensors="pt")
        return enc["input_ids"]


class FrozenCLIPTextEmbedder(_TextTower):
    """cond_stage_config.target of configs/frido/t2i/frido_f16f8_coco_clip.yaml:80 (reference:
    frido/modules/encoders/modules.py:188-219): the text tower of OpenAI CLIP -> ONE L2-normalised embedding per caption,
    `encode` adds the token axis and repeats it n_repeat times.  The tower runs on the HIP engine (clip_plan.ClipTextPlan);
    its weights live under `self.model` with OpenAI CLIP's state_dict names, so a reference checkpoint's
    `cond_stage_model.model.*` keys load.  `forward` takes token ids ([B, 77] int64, what `clip.tokenize` returns); captions as
    strings need the CLIP byte-pair merge table, which is part of the un-vendored `clip` package: pass `bpe_path=` / set
    $FRIDO_CLIP_BPE (a local bpe_simple_vocab_16e6.txt.gz: frido_amd/tokenizers.py ClipBPETokenizer), pass `tokenizer=` (any
    callable list[str] -> LongTensor [B, 77]) or install `clip`; without any of them a clear error is raised at encode time.
    `arch` overrides the (embed_dim, context_length, vocab, width, heads, layers) of `version` (tests use a reduced tower)."""

    _what = "FrozenCLIPTextEmbedder"

    def __init__(self, version="ViT-L/14", device="cuda", max_length=77, n_repeat=1, normalize=True, arch=None, tokenizer=None,
                 precision=None, bpe_path=None):
        super().__init__()
        self.version, self.device, self.max_length = version, device, max_length
        self.n_repeat, self.normalize, self.use_tknz_fn = n_repeat, normalize, True
        self.precision, self.tokenizer = precision, tokenizer
        self.bpe_path = bpe_path              # local CLIP merge table (bpe_simple_vocab_16e6.txt.gz; else $FRIDO_CLIP_BPE)
        if arch is None:
            if version not in holders.CLIP_TEXT_ARCH:
                raise NotImplementedError(f"FrozenCLIPTextEmbedder: unknown CLIP version '{version}' "
                                          f"(known: {sorted(holders.CLIP_TEXT_ARCH)}); pass arch=(embed_dim, ctx, vocab, width, heads, layers)")
            arch = holders.CLIP_TEXT_ARCH[version]
        self.arch = tuple(arch)
        holders.build_clip_text_params(self, *self.arch)
        self._init_versioning()

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False

    def _tokens(self, text):
        if torch.is_tensor(text):
            return text
        if self.tokenizer is None:
            from .tokenizers import ClipBPETokenizer, local_clip_bpe
            bp = local_clip_bpe(self.bpe_path)
            if bp is not None:      # frido_amd/tokenizers.py: the published byte-level BPE of clip/simple_tokenizer.py over a local file
                self.tokenizer = ClipBPETokenizer(bp, context_length=self.arch[1])
        if self.tokenizer is not None:
            return self.tokenizer(text)
        try:
            import clip                                        # the reference's own dependency, when it is installed
            return clip.tokenize(text)
        except ImportError:
            raise NotImplementedError(
                "FrozenCLIPTextEmbedder: captions given as strings need CLIP's byte-pair vocabulary (`clip.tokenize`); the `clip` "
                "package is not reachable offline -- pass bpe_path= / set FRIDO_CLIP_BPE to a local bpe_simple_vocab_16e6.txt.gz, pass "
                "token ids ([B, 77] int64), a tokenizer= callable, or the finished "
                "[B, n_repeat, embed_dim] embedding to the sampler as `conditioning`") from None

    def _check_length(self, n):
        assert n <= self.arch[1], f"{n} tokens > context length {self.arch[1]}"

    def _make_plan(self, B, n):
        from .clip_plan import ClipTextPlan
        embed_dim, _, vocab, width, heads, layers = self.arch
        return ClipTextPlan(self._rt, B=B, n=n, width=width, layers=layers, heads=heads, vocab=vocab, embed_dim=embed_dim,
                            normalize=self.normalize)

    def _bind(self, plan, tokens):
        B, n = tokens.shape
        plan.eot_rows.copy_(tokens.argmax(dim=-1) + torch.arange(B, device=tokens.device) * n)      # clip/model.py: the EOT token has the highest id

    def forward(self, text):
        return self._run(text)[0].out.clone()

    def encode(self, text):
        z = self(text)
        if z.ndim == 2:
            z = z[:, None, :]
        return z.expand(-1, self.n_repeat, -1).contiguous()      # repeat(z, 'b 1 d -> b k d', k=n_repeat)


def _captured(plan, sp):
    """plan.launch(sp) -- kernels beside programs -- as one hipGraph captured on the stream `sp` (frido_capture_begin / frido_capture_end)."""
    import ctypes
    from .engine import Graph
    L = _lib.lib()
    _lib.check(L.frido_capture_begin(sp), "frido_capture_begin")
    h = ctypes.c_void_p()
    try:
        plan.launch(sp)
    except Exception:
        if L.frido_capture_end(sp, ctypes.byref(h)) == 0:      # a failed body still has to end its capture
            L.frido_graph_destroy(h)
        raise
    _lib.check(L.frido_capture_end(sp, ctypes.byref(h)), "frido_capture_end")
    return Graph(h, plan)


class FrozenClipImageEmbedder(_Versioned, nn.Module):
    """The third embedder of frido/modules/encoders/modules.py (:222-254): the image tower of OpenAI CLIP.  `forward` takes images
    [B, 3, H, W] float32 in [-1, 1] on the GPU and returns `encode_image`'s [B, embed_dim] float32, NOT normalised, like the reference:
    bicubic resize (align_corners=True) to the tower's resolution, CLIP's mean / std, then the VisionTransformer -- one HIP kernel
    (csrc/vision.hip) in front of the tower's program (clip_plan.ClipImagePlan), both replayed as ONE captured graph per input shape
    (B, H, W); the plans are kept least-recently-used like the text towers'.  The weights live under `self.model.visual` with OpenAI
    CLIP's state_dict names: a full CLIP state_dict loads with strict=False (its text keys are the unexpected ones).
    `model`: a ViT version of holders.CLIP_VISUAL_ARCH; `arch=(embed_dim, resolution, layers, width, patch)` builds a custom tower
    (heads = width // 64, clip/model.py).  Refused by name: jit=True, antialias=True (kornia's pre-blur is not restated here), the
    ResNet versions (ModifiedResNet + attention pooling).  `preprocess(x)` returns the resized, normalised [B, 3, res, res] image the
    tower sees -- the kernel's output re-laid by torch, for inspection and tests."""

    _what = "FrozenClipImageEmbedder"

    def __init__(self, model, jit=False, device="cuda", antialias=False, *, arch=None, precision=None):
        super().__init__()
        if jit:
            raise NotImplementedError("FrozenClipImageEmbedder: jit=True loads a TorchScript archive of the `clip` package; the HIP "
                                      "engine runs the tower from its state_dict only (pass jit=False)")
        if antialias:
            raise NotImplementedError("FrozenClipImageEmbedder: antialias=True (kornia's Gaussian pre-blur before the bicubic resize) is "
                                      "not implemented; pass antialias=False, the reference's default")
        if arch is None:
            if model in holders.CLIP_RESNET_VERSIONS:
                raise NotImplementedError(f"FrozenClipImageEmbedder: '{model}' is a ResNet CLIP tower (ModifiedResNet with attention "
                                          f"pooling), which is not implemented; the ViT versions are {sorted(holders.CLIP_VISUAL_ARCH)}")
            if model not in holders.CLIP_VISUAL_ARCH:
                raise NotImplementedError(f"FrozenClipImageEmbedder: unknown CLIP version '{model}' (known: "
                                          f"{sorted(holders.CLIP_VISUAL_ARCH)}); pass arch=(embed_dim, resolution, layers, width, patch)")
            arch = holders.CLIP_VISUAL_ARCH[model]
        self.arch = tuple(int(a) for a in arch)
        embed_dim, res, layers, width, patch = self.arch
        if width % 64:
            raise ValueError(f"FrozenClipImageEmbedder: width {width} must be a multiple of 64 (clip/model.py: heads = width // 64)")
        if width > 1024:
            raise ValueError(f"FrozenClipImageEmbedder: width {width} exceeds 1024, the widest row of the LayerNorm kernel "
                             "(csrc/norm.hip frido_layernorm: C <= 1024); every published ViT tower up to ViT-L fits")
        self.version, self.device, self.antialias, self.precision = model, device, antialias, precision
        holders.build_clip_visual_params(self, *self.arch)      # ValueError: a resolution that is no whole number of patches
        self.register_buffer("mean", torch.Tensor([0.48145466, 0.4578275, 0.40821073]), persistent=False)
        self.register_buffer("std", torch.Tensor([0.26862954, 0.26130258, 0.27577711]), persistent=False)
        self._init_versioning()

    def _init_versioning(self):
        super()._init_versioning()
        self._plans = {}

    def invalidate(self):
        self._rt = None
        self._plans = {}

    def _check(self, x):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or 0 in x.shape:
            got = tuple(x.shape) if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"FrozenClipImageEmbedder: images must be a [B, 3, H, W] tensor in [-1, 1], got {got}")
        _on_gpu(self._what, self, x)

    def _norm(self):
        return [float(v) for v in self.mean.tolist()], [float(v) for v in self.std.tolist()]

    @torch.no_grad()
    @_lib.with_planes
    def preprocess(self, x):
        """[B, 3, H, W] in [-1, 1] -> the [B, 3, res, res] image the tower sees (encoders/modules.py:242-250 with antialias=False)."""
        from . import vision
        self._check(x)
        _, res, _, _, P = self.arch
        B, _, H, W = x.shape
        g = res // P
        require_gpu(x.device)
        src = x.detach().float().contiguous()
        dst = torch.empty(B * g * g, 3 * P * P, dtype=torch.float32, device=x.device)
        mean, std = self._norm()
        vision.clip_preprocess(vision.preprocess_desc(src.data_ptr(), dst.data_ptr(), B, H, W, res, P, mean, std), current_stream_ptr(x.device))
        return dst.view(B, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, res, res)

    def _make_plan(self, B, H, W, stream):
        from .clip_plan import ClipImagePlan
        embed_dim, res, layers, width, patch = self.arch
        mean, std = self._norm()
        plan = ClipImagePlan(self._rt, B=B, H=H, W=W, embed_dim=embed_dim, resolution=res, layers=layers, width=width, patch=patch,
                             mean=mean, std=std, stream=stream)
        plan.graph = None
        return plan

    def _capture(self, plan, sp):
        """plan.graph: the preprocess launch and the tower's program as one hipGraph, captured on the stream `sp`."""
        plan.graph = _captured(plan, sp)
        self.graph_captures += 1

    graph_captures = 0      # graphs captured so far (one per input shape in the cache; tests read it)

    @torch.no_grad()
    @_lib.with_planes
    def forward(self, x):
        self._check(x)
        dev = next(self.parameters()).device
        B, _, H, W = x.shape
        with own_stream(self, dev) as sp:
            if self._rt is None:
                self._plans = {}
                self._rt = runtime.module_builder(self, dev, self.precision)

            def build():      # like _cached_plan; an evicted plan's graph may still be running on this stream: wait for it first
                with self._rt.persist_scope() as owned:
                    return self._make_plan(B, H, W, sp), owned
            plan = lru_entry(self._plans, (B, H, W), PLAN_CACHE_SIZE, build, before_evict=self._stream.synchronize)[0]
            plan.x_in.copy_(x)
            if plan.graph is None:
                self._capture(plan, sp)
            plan.graph.launch(sp)
            return plan.out.clone()


# ---- perceptual metric (taming/modules/losses/lpips.py:11-122) -----------------------------------------
class _LinWeight(nn.Module):      # nn.Conv2d(chn_in, 1, 1, bias=False)
    def __init__(self, chn_in):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(1, chn_in, 1, 1))


class _Scaling(nn.Module):        # ScalingLayer, lpips.py:57-64: persistent buffers, they are keys of the reference's state_dict
    def __init__(self):
        super().__init__()
        from .lpips import SCALE, SHIFT
        self.register_buffer("shift", torch.Tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.Tensor(SCALE)[None, :, None, None])


class LPIPS(_Versioned, nn.Module):
    """taming/modules/losses/lpips.py:11-54, the learned perceptual metric: a frozen VGG16 feature stack, a per-pixel channel
    normalisation and five 1 x 1 projections.  `forward(input, target)` takes two [B, 3, H, W] float32 image batches on the GPU and
    returns the reference's [B, 1, 1, 1] float32; `per_layer` returns the five spatial means it adds, [B, 5].  Input and target go
    through the tower together as ONE batch of 2B (frido_amd/lpips.py LpipsPlan); the four kernels of csrc/lpips.hip and the five slice
    programs replay as ONE captured graph per input shape (B, H, W), the plans kept least-recently-used.

    Parameters carry the reference's names -- net.sliceK.N.{weight,bias}, linK.model.1.weight (index 0 under use_dropout=False), the
    buffers scaling_layer.{shift,scale} -- so the `loss.perceptual_loss.*` keys of a taming checkpoint load.  Dropout is the eval-mode
    identity and every parameter is frozen.  The constructor downloads NOTHING: `lin_ckpt=` loads a local vgg.pth (strict=False),
    `vgg_ckpt=` a local torchvision vgg16 state_dict (features.N.* -> the slice names); without either the weights are this module's
    own init (He-normal convs, zero biases, uniform [0, 1) projections), which measures nothing perceptual.
    Refused by name: from_pretrained / load_from_pretrained without a local path, .train() under use_dropout=True, inputs that are not
    two equal [B, 3, H, W] shapes with H, W >= 16 (four floor-mode pools), CPU tensors."""

    _what = "LPIPS"

    def __init__(self, use_dropout=True, *, lin_ckpt=None, vgg_ckpt=None, precision=None):
        super().__init__()
        from .lpips import CHNS, VGG_SLICES
        self.use_dropout, self.precision = bool(use_dropout), precision
        self.chns = list(CHNS)
        self.scaling_layer = _Scaling()
        self.net = holders.Nop()
        cin = 3
        for si, convs in enumerate(VGG_SLICES):
            sl = nn.Sequential()
            for idx, cout in convs:
                sl.add_module(str(idx), holders.Conv(cin, cout, 3))
                cin = cout
            setattr(self.net, f"slice{si + 1}", sl)
        self.net.N_slices = 5
        for k, c in enumerate(self.chns):
            lin = holders.Nop()
            lin.model = nn.Sequential()
            lin.model.add_module(str(self._lin_index), _LinWeight(c))
            setattr(self, f"lin{k}", lin)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.startswith("lin"):
                    p.uniform_(0.0, 1.0)
                elif name.endswith(".bias"):
                    p.zero_()
                else:
                    nn.init.kaiming_normal_(p, nonlinearity="relu")
        self._init_versioning()
        if vgg_ckpt is not None:
            self.load_vgg16(vgg_ckpt)
        if lin_ckpt is not None:
            self.load_from_pretrained(path=lin_ckpt)
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    _lin_index = property(lambda self: 1 if self.use_dropout else 0)

    def _init_versioning(self):
        super()._init_versioning()
        self._plans = {}

    def invalidate(self):
        self._rt = None
        self._plans = {}

    def lin_names(self):
        return [f"lin{k}.model.{self._lin_index}.weight" for k in range(5)]

    def train(self, mode=True):
        if mode and self.use_dropout:
            raise NotImplementedError("LPIPS.train(): use_dropout=True puts nn.Dropout in front of every 1 x 1 projection (lpips.py:71), and "
                                      "training-mode dropout is not built: the metric is the eval-mode identity (keep .eval(), or build "
                                      "LPIPS(use_dropout=False))")
        return super().train(mode)

    # ---- weights: local files only ----------------------------------------------------------------------
    def load_from_pretrained(self, name="vgg_lpips", path=None):
        """lpips.py:27-30 with the download taken out: `path` is a local vgg.pth (the linK.model.1.weight keys)."""
        if path is None:
            raise NotImplementedError(f"LPIPS.load_from_pretrained('{name}'): the reference downloads vgg.pth (taming.util.get_ckpt_path, "
                                      "heibox.uni-heidelberg.de) -- nothing is downloaded here; pass path= / lin_ckpt= a local copy")
        sd = torch.load(path, map_location=torch.device("cpu"))
        fixed = {}
        for k, v in sd.items():      # a checkpoint written under the other use_dropout has the projections one index away
            parts = k.split(".")
            if len(parts) == 4 and parts[0][:3] == "lin" and parts[1] == "model" and parts[2] in ("0", "1"):
                parts[2] = str(self._lin_index)
            fixed[".".join(parts)] = v
        return self.load_state_dict(fixed, strict=False)

    @classmethod
    def from_pretrained(cls, name="vgg_lpips", path=None, **kw):
        """lpips.py:32-39 with the download taken out."""
        if name != "vgg_lpips":
            raise NotImplementedError(f"LPIPS.from_pretrained('{name}'): only 'vgg_lpips' exists (lpips.py:34-35)")
        if path is None:
            raise NotImplementedError("LPIPS.from_pretrained('vgg_lpips'): the reference downloads vgg.pth and torchvision's vgg16 weights "
                                      "-- nothing is downloaded here; pass path= a local vgg.pth (and vgg_ckpt= a local vgg16 state_dict)")
        return cls(lin_ckpt=path, **kw)

    def load_vgg16(self, path):
        """A local torchvision vgg16 state_dict: features.N.{weight,bias} -> net.sliceK.N.{weight,bias}; the classifier's keys are
        passed over."""
        from .lpips import VGG_SLICES
        sd = torch.load(path, map_location=torch.device("cpu"))
        mapped = {}
        for si, convs in enumerate(VGG_SLICES):
            for idx, _ in convs:
                for leaf in ("weight", "bias"):
                    src = f"features.{idx}.{leaf}"
                    if src not in sd:
                        raise KeyError(f"LPIPS.load_vgg16: {path} holds no '{src}' (not a torchvision vgg16 state_dict?)")
                    mapped[f"net.slice{si + 1}.{idx}.{leaf}"] = sd[src]
        return self.load_state_dict(mapped, strict=False)

    # ---- the metric ----------------------------------------------------------------------------------------
    def _check(self, x, y):
        from .lpips import MIN_SIDE
        for name, t in (("input", x), ("target", y)):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or 0 in t.shape:
                got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"LPIPS: {name} must be a [B, 3, H, W] tensor, got {got}")
        if x.shape != y.shape:
            raise ValueError(f"LPIPS: input {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
        if min(x.shape[2:]) < MIN_SIDE:
            raise ValueError(f"LPIPS: H and W must be at least {MIN_SIDE} (VGG16's four 2 x 2 pools leave nothing of a {x.shape[2]} x "
                             f"{x.shape[3]} image)")
        _on_gpu(self._what, self, x, y)

    def _make_plan(self, B, H, W):
        from .lpips import LpipsPlan
        shift = [float(v) for v in self.scaling_layer.shift.flatten().tolist()]
        scale = [float(v) for v in self.scaling_layer.scale.flatten().tolist()]
        return LpipsPlan(self._rt, B=B, H=H, W=W, shift=shift, scale=scale, lin_names=self.lin_names())

    def _capture(self, plan, sp):
        """plan.graph: the plan's launches as one hipGraph, captured on the stream `sp`.  A shape the conv launcher turns away is a
        ValueError naming it."""
        try:
            plan.graph = _captured(plan, sp)
        except FridoHipError as e:
            B, _, H, W = plan.x_in.shape
            raise ValueError(f"LPIPS: the library refuses a launch of the (B, H, W) = ({B}, {H}, {W}) plan: {e}") from e
        self.graph_captures += 1

    graph_captures = 0      # graphs captured so far (one per input shape in the cache; tests read it)

    @torch.no_grad()
    @_lib.with_planes
    def _run(self, x, y):
        """The plan of the inputs' shape after its graph ran on them."""
        self._check(x, y)
        dev = next(self.parameters()).device
        B, _, H, W = x.shape
        with own_stream(self, dev) as sp:
            if self._rt is None:
                self._plans = {}
                self._rt = runtime.module_builder(self, dev, self.precision)

            def build():      # like _cached_plan; an evicted plan's graph may still be running on this stream: wait for it first
                with self._rt.persist_scope() as owned:
                    return self._make_plan(B, H, W), owned
            plan = lru_entry(self._plans, (B, H, W), PLAN_CACHE_SIZE, build, before_evict=self._stream.synchronize)[0]
            plan.x_in.copy_(x)
            plan.y_in.copy_(y)
            if plan.graph is None:
                try:
                    self._capture(plan, sp)
                except ValueError:
                    self._plans.pop((B, H, W), None)
                    raise
            plan.graph.launch(sp)
            return plan

    def forward(self, input, target):
        """lpips.py:41-54: [B, 1, 1, 1] float32."""
        return self._run(input, target).out.clone().view(-1, 1, 1, 1)

    def per_layer(self, input, target):
        """The five spatial means forward adds (lpips.py:50), [B, 5] float32, relu1_2 first."""
        return self._run(input, target).per_layer.clone()


# ---- Inception-v3 feature extractor of the Fréchet Inception Distance ----------------------------------
class _BasicConv(nn.Module):      # torchvision's BasicConv2d: the parameter holders only
    def __init__(self, cin, cout, kh, kw, stride, pad, padx):
        super().__init__()
        from .fid import BN_EPS
        self.conv = nn.Conv2d(cin, cout, (kh, kw), stride=stride, padding=(pad, padx), bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)


class FIDInceptionV3(_Versioned, nn.Module):
    """The feature extractor of the Fréchet Inception Distance: torchvision's Inception-v3 in the FID variant torch-fidelity's
    FeatureExtractorInceptionV3 runs (every average pool leaves the padding out of its divisor, Mixed_7c pools with a maximum), forward
    only and always in eval mode.  `forward(images)` returns [B, 2048] float32, the pooled features that package calls '2048';
    `logits(features)` maps them to [B, 1008] float32, features @ fc.weight.T WITHOUT the bias: that package's 'logits_unbiased', the
    input of its Inception Score (frido_amd/fidelity.py).
    `images`: uint8 [B, H, W, 3] on the GPU (what pipeline.sample_images gathers), or float32 [B, 3, H, W] in [-1, 1] (what the decoders
    return), which is first quantised to 8 bits the way the sampling script writes images: `quant` = "pil" (custom_to_pil, the PNG
    writer: the default, the evaluation reads PNG directories) or "np" (custom_to_np).  Then the TF1-legacy bilinear resize to
    299 x 299 and (v - 128) / 128 (include/frido_fid.h), the 94 conv + BatchNorm + ReLU layers with the BatchNorm folded into the conv on
    the host in float64, the pools and the global average (frido_amd/fid.py InceptionPlan; csrc/fid.hip), replayed as ONE captured
    graph per input shape (B, H, W, dtype), the plans kept least-recently-used.

    The parameter holders are nn.Conv2d(bias=False) and nn.BatchNorm2d(eps=1e-3) under torchvision's names (Conv2d_1a_3x3.conv.weight,
    Mixed_5b.branch1x1.bn.running_var, ... and fc.weight / fc.bias: forward runs neither, logits the weight alone), so the published pt_inception-2015-12-05
    state_dict loads: `ckpt=` is a LOCAL file, nothing is downloaded, a file without num_batches_tracked is accepted.  Without it the
    weights are torch's initialisation and the features measure nothing about image quality.
    `resolution=` (keyword only, fixed at construction) is the side the images are resized to: 299, the only value at which the features
    are the published metric's; a smaller one runs the same tower on smaller planes.
    Refused by name: .train() (NotImplementedError), inputs of neither layout / dtype or not 3 channels (ValueError), CPU tensors
    (FridoHipError)."""

    _what = "FIDInceptionV3"

    def __init__(self, *, ckpt=None, precision=None, resolution=None):
        super().__init__()
        from . import fid
        self.precision, self.quant = precision, "pil"
        self.resolution = int(resolution or fid.RESOLUTION)
        if fid.tower_planes(self.resolution) is None:
            raise ValueError(f"FIDInceptionV3: a {self.resolution} x {self.resolution} tower input leaves some conv or pool without an "
                             "output pixel")
        for name, cin, cout, kh, kw, stride, pad, padx in fid.conv_table():
            parent, parts = self, name.split(".")
            for p in parts[:-1]:
                if not hasattr(parent, p):
                    setattr(parent, p, holders.Nop())
                parent = getattr(parent, p)
            setattr(parent, parts[-1], _BasicConv(cin, cout, kh, kw, stride, pad, padx))
        self.fc = nn.Linear(fid.FC_SHAPE[1], fid.FC_SHAPE[0])
        self._init_versioning()
        if ckpt is not None:
            self.load_checkpoint(ckpt)
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def _init_versioning(self):
        super()._init_versioning()
        self._plans = {}

    def invalidate(self):
        self._rt = None
        self._plans = {}

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("FIDInceptionV3.train(): the extractor is forward-only with its BatchNorm folded from the running "
                                      "statistics; there is no training mode and no backward pass (keep .eval())")
        return super().train(False)

    def load_checkpoint(self, path):
        """A local state_dict with this module's key set (pt_inception-2015-12-05).  The num_batches_tracked buffers may be missing;
        anything else missing, and any key this module does not have, is a KeyError."""
        sd = torch.load(path, map_location=torch.device("cpu"))
        res = self.load_state_dict(sd, strict=False)
        missing = [k for k in res.missing_keys if not k.endswith("num_batches_tracked")]
        if missing or res.unexpected_keys:
            raise KeyError(f"FIDInceptionV3.load_checkpoint: {path} is no Inception-v3 state_dict: missing {missing[:4]} "
                           f"({len(missing)}), unexpected {list(res.unexpected_keys)[:4]} ({len(res.unexpected_keys)})")
        return res

    def _check(self, x, quant):
        from .fid import QUANT
        ok = torch.is_tensor(x) and x.dim() == 4 and 0 not in x.shape and (
            (x.dtype == torch.uint8 and x.shape[3] == 3) or (x.dtype == torch.float32 and x.shape[1] == 3))
        if not ok:
            got = (tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__
            raise ValueError("FIDInceptionV3: images must be uint8 [B, H, W, 3] or float32 [B, 3, H, W] in [-1, 1] with 3 channels, "
                             f"got {got}")
        if quant not in QUANT:
            raise ValueError(f"FIDInceptionV3: quant must be one of {sorted(QUANT)}, got {quant!r}")
        _on_gpu(self._what, self, x)

    def _builder(self, dev):
        """The Builder over the FOLDED weights (conv + BatchNorm as one conv with a bias), for the build `precision` selects."""
        from . import fid
        from .builder import Builder
        planes = config.planes(self.precision)
        with _lib.use_planes(planes):
            dev = require_gpu(dev)
        return Builder(dev, config.nsplit(self.precision), fid.folded_weights(self.state_dict(), dev), planes=planes)

    def _capture(self, plan, sp):
        """plan.graph: the plan's launches as one hipGraph, captured on the stream `sp`."""
        plan.graph = _captured(plan, sp)
        self.graph_captures += 1

    graph_captures = 0      # graphs captured so far (one per input shape in the cache; tests read it)

    @torch.no_grad()
    @_lib.with_planes
    def forward(self, images, quant=None):
        from .fid import InceptionPlan
        quant = quant or self.quant
        self._check(images, quant)
        S = self.resolution
        dev = next(self.parameters()).device
        uint8 = images.dtype == torch.uint8
        B, H, W = (images.shape[0], images.shape[1], images.shape[2]) if uint8 else (images.shape[0], images.shape[2], images.shape[3])
        key = (B, H, W, images.dtype, quant if not uint8 else None, S)
        with own_stream(self, dev) as sp:
            if self._rt is None:
                self._plans = {}
                self._rt = self._builder(dev)

            def build():      # like _cached_plan; an evicted plan's graph may still be running on this stream: wait for it first
                with self._rt.persist_scope() as owned:
                    return InceptionPlan(self._rt, B=B, H=H, W=W, uint8=uint8, quant=quant, S=S), owned
            plan = lru_entry(self._plans, key, PLAN_CACHE_SIZE, build, before_evict=self._stream.synchronize)[0]
            plan.x_in.copy_(images)
            if plan.graph is None:
                self._capture(plan, sp)
            plan.graph.launch(sp)
            return plan.out.clone()

    @torch.no_grad()
    def logits(self, features):
        """[B, 2048] float32 features -> [B, 1008] float32 class logits, features @ fc.weight.T without fc.bias: every dot product
        accumulated in float64 over k ascending and rounded to float32 once (one launch of frido_rows_dot, csrc/fidelity.hip)."""
        from . import fidelity
        fidelity._rows2d("FIDInceptionV3.logits", "features", features, self.fc.weight.shape[1])
        if features.shape[0] == 0:
            raise ValueError("FIDInceptionV3.logits: features must be a 2-D float32 tensor with at least one row")
        _on_gpu(self._what, self, features)
        return fidelity.rows_dot(features, self.fc.weight, mode=fidelity.STORE_F32)


# ---- PatchGAN discriminator and the tokenizer's loss (taming/modules/discriminator/model.py, losses/vqperceptual.py) ------------------
def weights_init(m):
    """discriminator/model.py:8-14."""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class ActNorm(nn.Module):
    """taming/modules/util.py:10-20 as a parameter holder: loc, scale [1, C, 1, 1] and the `initialized` flag.  Its data-dependent
    initialisation runs in training mode only, which the discriminator refuses; the forward h = scale (x + loc) is folded into the
    discriminator's affine kernel (frido_amd/patchgan.py fold_actnorm)."""

    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        self.logdet, self.allow_reverse_init = logdet, allow_reverse_init
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))

    def forward(self, input, reverse=False):
        raise FridoHipError("ActNorm is a parameter holder here: NLayerDiscriminator folds it into its affine kernel")


class NLayerDiscriminator(_Versioned, nn.Module):
    """taming/modules/discriminator/model.py:17-67, the PatchGAN discriminator, forward-only: `forward(x)` takes [B, input_nc, H, W]
    float32 images on the GPU and returns the [B, 1, Ho, Wo] float32 logits.  `pair(real, fake)` runs both batches through the net as ONE
    batch of 2B and returns the plan with the logits and the GAN terms (frido_amd/patchgan.py PatchGanPlan).  The stem, the folded norms,
    the head and the reductions are the kernels of csrc/patchgan.hip, the middle 4 x 4 convs run on the implicit GEMM; everything
    replays as ONE captured graph per input shape, the plans kept least-recently-used.

    `main` holds nn.Conv2d / nn.BatchNorm2d / ActNorm as PARAMETER HOLDERS under the reference's indices, so the state_dict is the
    reference's (`loss.discriminator.*` of a taming checkpoint loads) and `weights_init` applies.  The norms are the eval-mode ones:
    BatchNorm2d by its running statistics, ActNorm by its loc / scale.
    Refused by name: .train() (batch statistics, ActNorm's data-dependent init), input_nc > 8, ndf % 4 != 0 or ndf * input_nc > 512 (the
    stem kernel), n_layers < 1, an input too small for a 1 x 1 logit map, CPU tensors."""

    _what = "NLayerDiscriminator"

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False, *, precision=None):
        super().__init__()
        from . import patchgan as pg
        if n_layers < 1:
            raise ValueError(f"NLayerDiscriminator: n_layers={n_layers}: at least one stride-2 layer (the stem) is needed")
        if input_nc > pg.MAX_INPUT_NC:
            raise NotImplementedError(f"NLayerDiscriminator: input_nc={input_nc} > {pg.MAX_INPUT_NC}: the stem kernel (frido_disc_stem) takes at "
                                      "most 8 input channels")
        if ndf % 4 or ndf < 4:
            raise NotImplementedError(f"NLayerDiscriminator: ndf={ndf} must be a multiple of 4 (16-byte stores across the channels)")
        if ndf * input_nc > pg.STEM_MAX_WEIGHTS:
            raise NotImplementedError(f"NLayerDiscriminator: ndf * input_nc = {ndf * input_nc} > {pg.STEM_MAX_WEIGHTS}: the stem's weights "
                                      "must fit 32 KB of LDS")
        self.input_nc, self.ndf, self.n_layers, self.use_actnorm, self.precision = input_nc, ndf, n_layers, bool(use_actnorm), precision
        self.table = pg.layer_table(input_nc, ndf, n_layers)
        self.main = nn.Sequential()
        for ci, ni, cin, cout, stride in self.table:
            self.main.add_module(str(ci), nn.Conv2d(cin, cout, kernel_size=pg.KW, stride=stride, padding=pg.PADW,
                                                    bias=ni is None or self.use_actnorm))
            if ni is not None:
                self.main.add_module(str(ni), ActNorm(cout) if self.use_actnorm else nn.BatchNorm2d(cout))
        self._init_versioning()
        for p in self.parameters():
            p.requires_grad = False
        super().train(False)

    def _init_versioning(self):
        super()._init_versioning()
        self._plans = {}
        self._consts = None

    def invalidate(self):
        self._rt = None
        self._plans = {}
        self._consts = None

    def _apply(self, fn, *a, **k):
        self._plans, self._consts = {}, None
        return super()._apply(fn, *a, **k)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("NLayerDiscriminator.train(): training mode means BatchNorm2d's batch statistics / ActNorm's "
                                      "data-dependent initialisation and a backward pass, none of which is built: the net is the "
                                      "eval-mode forward (keep .eval())")
        return super().train(mode)

    def apply(self, fn):      # nn.Module.apply; afterwards the compiled plans are stale
        out = super().apply(fn)
        self.invalidate()
        return out

    # ---- the forward -------------------------------------------------------------------------------------
    def _check(self, *images):
        from . import patchgan as pg
        for t in images:
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != self.input_nc or 0 in t.shape:
                got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"NLayerDiscriminator: images must be a [B, {self.input_nc}, H, W] tensor, got {got}")
        if len(images) == 2 and images[0].shape != images[1].shape:
            raise ValueError(f"NLayerDiscriminator: real {tuple(images[0].shape)} and fake {tuple(images[1].shape)} differ in shape")
        H, W = images[0].shape[2:]
        if pg.plane_sizes(H, W, self.n_layers) is None:
            raise ValueError(f"NLayerDiscriminator: a {H} x {W} input is too small for a 1 x 1 logit map after {self.n_layers} stride-2 "
                             f"and two stride-1 4 x 4 convs (the smallest side is {self.min_side()})")
        _on_gpu(self._what, self, *images)

    def min_side(self):
        from . import patchgan as pg
        h = 1
        while pg.plane_sizes(h, h, self.n_layers) is None:
            h += 1
        return h

    def _make_consts(self, b):
        """What the side launches read, made once per Builder: the repacked stem / head weights and the folded norms, on the device."""
        from . import patchgan as pg
        sd = {k: v.detach().cpu() for k, v in self.state_dict().items()}
        last = self.table[-1][0]
        affine = {}
        for ci, ni, _, _, _ in self.table:
            if ni is not None:
                a, bb = pg.fold_norm(sd, "", ci, ni, self.use_actnorm)
                affine[ni] = (b.to_dev(a), b.to_dev(bb))
        return dict(stem_w=b.to_dev(pg.repack_stem_weight(sd["main.0.weight"])), stem_b=b.to_dev(sd["main.0.bias"]),
                    head_w=b.to_dev(pg.repack_head_weight(sd[f"main.{last}.weight"])), head_b=float(sd[f"main.{last}.bias"].float()[0]),
                    affine=affine)

    def _capture(self, plan, sp):
        try:
            plan.graph = _captured(plan, sp)
        except FridoHipError as e:
            raise ValueError(f"NLayerDiscriminator: the library refuses a launch of the {tuple(plan.x_in.shape)} plan: {e}") from e
        self.graph_captures += 1

    graph_captures = 0      # graphs captured so far (one per input shape in the cache; tests read it)

    @torch.no_grad()
    @_lib.with_planes
    def _run(self, x, y=None):
        """The plan of the inputs' shape after its graph ran on them (y: the fake images of a pair, or None)."""
        from .patchgan import PatchGanPlan
        self._check(*((x,) if y is None else (x, y)))
        dev = next(self.parameters()).device
        B, _, H, W = x.shape
        pair = y is not None
        with own_stream(self, dev) as sp:
            if self._rt is None:
                self._plans, self._consts = {}, None
                self._rt = runtime.module_builder(self, dev, self.precision)
            if self._consts is None:
                self._consts = self._make_consts(self._rt)

            def build():      # like _cached_plan; an evicted plan's graph may still be running on this stream: wait for it first
                with self._rt.persist_scope() as owned:
                    return PatchGanPlan(self._rt, B=B, H=H, W=W, pair=pair, input_nc=self.input_nc, ndf=self.ndf, n_layers=self.n_layers,
                                        consts=self._consts), owned
            key = (B, H, W, pair)
            plan = lru_entry(self._plans, key, PLAN_CACHE_SIZE, build, before_evict=self._stream.synchronize)[0]
            plan.x_in.copy_(x)
            if pair:
                plan.y_in.copy_(y)
            if plan.graph is None:
                try:
                    self._capture(plan, sp)
                except ValueError:
                    self._plans.pop(key, None)
                    raise
            plan.graph.launch(sp)
            return plan

    def forward(self, input):
        """model.py:65-67: [B, 1, Ho, Wo] float32 logits."""
        return self._run(input).logits.clone()

    def pair(self, real, fake):
        """Both batches through the net at once: the plan, whose `logits` [2B, 1, Ho, Wo] (real first), `out` [5]
        (patchgan.OUT_NAMES) and `per_sample` [2B] logit means are valid until its next run."""
        return self._run(real, fake)


def adopt_weight(weight, global_step, threshold=0, value=0.):
    """vqperceptual.py:16-19."""
    if global_step < threshold:
        weight = value
    return weight


def hinge_d_loss(logits_real, logits_fake):
    """vqperceptual.py:22-26, in torch: for callers that hold logits; VQLPIPSWithDiscriminator takes the value from its graph."""
    return 0.5 * (torch.mean(torch.relu(1. - logits_real)) + torch.mean(torch.relu(1. + logits_fake)))


def vanilla_d_loss(logits_real, logits_fake):
    """vqperceptual.py:29-33, in torch."""
    return 0.5 * (torch.mean(nn.functional.softplus(-logits_real)) + torch.mean(nn.functional.softplus(logits_fake)))


class VQLPIPSWithDiscriminator(nn.Module):
    """taming/modules/losses/vqperceptual.py:36-150, the loss of every shipped tokenizer config, evaluated WITHOUT a gradient: under
    no_grad the reference's calculate_adaptive_weight raises and d_weight is 0 (vqperceptual.py:113-117), so what is left is LPIPS, the
    discriminator's forward on both images and a handful of reductions.  The children are named `perceptual_loss` (LPIPS) and
    `discriminator` (NLayerDiscriminator): the `loss.*` keys of a taming checkpoint load.

    `forward` returns the reference's (loss, log) for optimizer_idx 0 or 1 with exactly its keys; `evaluate` returns both pairs from one
    launch of the discriminator's graph (real and fake as one batch of 2B) and one of LPIPS's.  |x - xrec| and the final scalar
    combinations are torch reductions on the device.  `disc_factor` and `d_weight` entries are host tensors like the reference's.
    Nothing is downloaded: LPIPS holds its own init until `perceptual_loss` is loaded from local files.
    Refused by name: .train(), disc_conditional=True / cond=, xrec_aux (the reference's own line 96 adds a [B, 3, H, W] tensor in place
    into a [1] tensor and raises), unequal input / reconstruction shapes, CPU tensors."""

    def __init__(self, disc_start, codebook_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3, disc_factor=1.0,
                 disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_ndf=64, disc_loss="hinge",
                 aux_downscale=4., aux_loss_weight=[1., 0], *, precision=None):
        super().__init__()
        assert disc_loss in ["hinge", "vanilla"]
        if disc_conditional:
            raise NotImplementedError("VQLPIPSWithDiscriminator: disc_conditional=True (the conditioning concatenated to the discriminator's "
                                      "input, vqperceptual.py:108-110) is not built; no shipped config sets it")
        self.codebook_weight, self.pixel_weight, self.perceptual_weight = codebook_weight, pixelloss_weight, perceptual_weight
        self.aux_downscale, self.aux_loss_weight = aux_downscale, aux_loss_weight
        self.perceptual_loss = LPIPS(precision=precision).eval()
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers, use_actnorm=use_actnorm, ndf=disc_ndf,
                                                 precision=precision).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss_name = disc_loss
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor, self.discriminator_weight, self.disc_conditional = disc_factor, disc_weight, disc_conditional
        super().train(False)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("VQLPIPSWithDiscriminator.train(): the loss is evaluated without a gradient (the reference asserts "
                                      "`not self.training` on that path, vqperceptual.py:116); there is no backward pass, keep .eval()")
        return super().train(mode)

    @torch.no_grad()
    def evaluate(self, codebook_loss, inputs, reconstructions, global_step, split="train"):
        """((loss, log) of optimizer_idx 0, (d_loss, log) of optimizer_idx 1): vqperceptual.py:85-150 for cond=None, xrec_aux=None."""
        from .patchgan import OUT_NAMES
        for name, t in (("inputs", inputs), ("reconstructions", reconstructions)):
            if not torch.is_tensor(t) or t.dim() != 4:
                raise ValueError(f"VQLPIPSWithDiscriminator: {name} must be a [B, C, H, W] tensor")
        if inputs.shape != reconstructions.shape:
            raise ValueError(f"VQLPIPSWithDiscriminator: inputs {tuple(inputs.shape)} and reconstructions {tuple(reconstructions.shape)} "
                             "differ in shape")
        _on_gpu("VQLPIPSWithDiscriminator", self.discriminator, inputs, reconstructions)
        x, xrec = inputs.contiguous().float(), reconstructions.contiguous().float()
        rec_loss = torch.abs(x - xrec)
        if self.perceptual_weight > 0:
            p_loss = self.perceptual_loss(x, xrec)
            rec_loss = rec_loss + self.perceptual_weight * p_loss
        else:
            p_loss = torch.tensor([0.0])
        rec_aux_loss = torch.tensor([0.0])
        nll_loss = torch.mean(rec_loss)
        out = self.discriminator.pair(x, xrec).out.clone()
        val = dict(zip(OUT_NAMES, out.unbind(0)))
        g_loss = val["g_loss"]
        d_weight = torch.tensor(0.0)          # no gradient: vqperceptual.py:115-117
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        cb = codebook_loss.detach().float().mean()
        loss = nll_loss + d_weight * disc_factor * g_loss + self.codebook_weight * cb
        log0 = {f"{split}/total_loss": loss.clone().detach().mean(), f"{split}/quant_loss": cb, f"{split}/nll_loss": nll_loss.detach().mean(),
                f"{split}/rec_loss": rec_loss.detach().mean(), f"{split}/p_loss": p_loss.detach().mean(),
                f"{split}/rec_aux_loss": rec_aux_loss.detach().mean(), f"{split}/d_weight": d_weight.detach(),
                f"{split}/disc_factor": torch.tensor(disc_factor), f"{split}/g_loss": g_loss.detach().mean()}
        d_loss = disc_factor * val["hinge" if self.disc_loss_name == "hinge" else "vanilla"]
        log1 = {f"{split}/disc_loss": d_loss.clone().detach().mean(), f"{split}/logits_real": val["logits_real"].detach().mean(),
                f"{split}/logits_fake": val["logits_fake"].detach().mean()}
        return (loss, log0), (d_loss, log1)

    def forward(self, codebook_loss, inputs, reconstructions, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                xrec_aux=None):
        if cond is not None:
            raise NotImplementedError("VQLPIPSWithDiscriminator: cond= (a conditional discriminator, vqperceptual.py:108-110, 139-141) is not built")
        if xrec_aux is not None:
            raise NotImplementedError("VQLPIPSWithDiscriminator: xrec_aux= is not built: the reference's own line 96 adds a [B, 3, H, W] tensor "
                                      "in place into a [1] tensor and raises")
        if optimizer_idx not in (0, 1):
            raise ValueError(f"VQLPIPSWithDiscriminator: optimizer_idx must be 0 or 1, got {optimizer_idx!r}")
        return self.evaluate(codebook_loss, inputs, reconstructions, global_step, split)[optimizer_idx]


def _first(cond, n):
    """The conditioning cut to the batch (frido.py:1316-1320, 1429-1433): the first n rows of a tensor, or of every tensor of a list."""
    if cond is None or isinstance(cond, dict):
        return cond
    return [c[:n] for c in cond] if isinstance(cond, list) else cond[:n]


# ---- EMA shadow (frido/modules/ema.py) ---------------------------------------------------------------
class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        self.m_name2s_name = {}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        for name, p in model.named_parameters():
            if p.requires_grad:              # ema.py:16-20: frozen parameters have no shadow (and no `model_ema.*` checkpoint key)
                s_name = name.replace(".", "")
                self.m_name2s_name[name] = s_name
                self.register_buffer(s_name, p.clone().detach().data)
        self.collected_params = []

    def copy_to(self, model):
        shadow = dict(self.named_buffers())
        for key, p in model.named_parameters():
            if p.requires_grad:
                p.data.copy_(shadow[self.m_name2s_name[key]].data)
            else:
                assert key not in self.m_name2s_name

    def store(self, parameters):
        self.collected_params = [p.clone() for p in parameters]

    def restore(self, parameters):
        for c, p in zip(self.collected_params, parameters):
            p.data.copy_(c.data)


# ---- diffusion wrapper + main module (frido/models/diffusion/frido.py) ----------------------------------
class DiffusionWrapper(_Base):
    def __init__(self, diff_model_config, conditioning_key):
        super().__init__()
        self.diffusion_model = instantiate_from_config(diff_model_config)
        self.conditioning_key = conditioning_key
        assert self.conditioning_key in [None, "concat", "crossattn", "hybrid", "adm"]

    def forward(self, x, t, c_concat: list = None, c_crossattn: list = None, stage=None):
        """frido.py:1635-1654, key for key.  Every shipped config uses 'crossattn'; 'hybrid' (channel concat + context) runs on the same
        denoiser plan; None / 'concat' reach a denoiser WITHOUT a context, 'adm' one with class labels -- the denoiser says which of
        those it was built for: an AttentionBlock denoiser (use_spatial_transformer=False) runs without a context and, built with num_classes, takes
        `y`; PyUNetModel.forward raises NotImplementedError for a context-free SpatialTransformer and for `y` on a model without num_classes."""
        key = self.conditioning_key
        if key is None:
            return self.diffusion_model(x, t, stage=stage)
        if key == "concat":
            return self.diffusion_model(torch.cat([x] + list(c_concat), dim=1), t, stage=stage)
        if key == "crossattn":
            return self.diffusion_model(x, t, context=torch.cat(c_crossattn, 1), stage=stage)
        if key == "hybrid":
            return self.diffusion_model(torch.cat([x] + list(c_concat), dim=1), t, context=torch.cat(c_crossattn, 1), stage=stage)
        if key == "adm":
            return self.diffusion_model(x, t, y=c_crossattn[0], stage=stage)
        raise NotImplementedError()


class FridoDiffusion(_Base):
    """frido.py:45-124 (DDPM.__init__) + 478-555 (FridoDiffusion.__init__): sampling, and the objective without a backward pass."""

    def __init__(self, first_stage_config, cond_stage_config, num_timesteps_cond=None, cond_stage_key="image",
                 cond_stage_trainable=False, concat_mode=True, cond_stage_forward=None, conditioning_key=None,
                 scale_factor=1.0, use_prob=False, scale_by_std=False, disable_log_image=False, plot_sample=True,
                 plot_inpaint=True, plot_denoise_rows=True, plot_progressive_rows=True, plot_diffusion_rows=True,
                 plot_quantize_denoised=True, adopted_scale_factor=False, adopted_scale_factor_value=None,
                 noise_mix_ratio=0, stage_loss_ratio=[0.5, 0.5],
                 unet_config=None, timesteps=1000, beta_schedule="linear", loss_type="l2", ckpt_path=None, ignore_keys=[],
                 load_only_unet=False, monitor="val/loss", use_ema=True, first_stage_key="image", image_size=256,
                 channels=3, log_every_t=100, clip_denoised=True, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3,
                 given_betas=None, original_elbo_weight=0., v_posterior=0., l_simple_weight=1., parameterization="eps",
                 scheduler_config=None, use_positional_encodings=False, learn_logvar=False, logvar_init=0.,
                 specify_channels=[], **ignored):
        super().__init__()
        assert parameterization == "eps", "Frido samples in eps-prediction mode"
        unet_config = _plain(unet_config)
        self.parameterization = parameterization
        self.num_timesteps_cond = 1 if num_timesteps_cond is None else num_timesteps_cond
        self.scale_by_std, self.adopted_scale_factor = scale_by_std, adopted_scale_factor
        self.cond_stage_model = None
        self.clip_denoised = False
        self.log_every_t, self.first_stage_key, self.image_size, self.channels = log_every_t, first_stage_key, image_size, channels
        if conditioning_key is None:
            conditioning_key = "concat" if concat_mode else "crossattn"
        if cond_stage_config == "__is_unconditional__":
            conditioning_key = None
        self.model = DiffusionWrapper(unet_config, conditioning_key)
        if specify_channels:
            # ddim.py:207-209,250-251,270-271 / plms.py:216-217,263-264,280-281: the first specify_channels[0] channels of the latent are held
            # fixed through every update (their eps zeroed, pred_x0 and x_prev copied from x) -- an option no shipped config sets (default:
            # the empty list).  The HIP sampler step has no such blend: refusing beats storing the option and ignoring it (r05 verdict).
            raise NotImplementedError("specify_channels: holding the leading channels fixed (ddim.py:207-209,250-251,270-271) is not provided on the HIP path "
                                      "(no shipped Frido config sets it)")
        self.specify_channels = []
        self.unet_config = unet_config
        self.use_split_head = unet_config["params"].get("use_split_head", False)
        self.split_embed_dim_list = unet_config["params"].get("split_embed_dim_list", [])
        self.use_ema = use_ema
        if use_ema:
            self.model_ema = LitEma(self.model)
        self.v_posterior = v_posterior
        # the objective's options (frido.py:105-124, 515-520)
        self.loss_type, self.noise_mix_ratio, self.stage_loss_ratio = loss_type, noise_mix_ratio, list(stage_loss_ratio)
        self.l_simple_weight, self.original_elbo_weight, self.learn_logvar = l_simple_weight, original_elbo_weight, learn_logvar
        if monitor is not None:
            self.monitor = monitor
        self.register_schedule(given_betas=given_betas, beta_schedule=beta_schedule, timesteps=timesteps,
                               linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        # frido.py:120-123: a plain tensor (no state_dict key) unless it is learned
        self.logvar = torch.full(fill_value=logvar_init, size=(self.num_timesteps,))
        if learn_logvar:
            self.logvar = nn.Parameter(self.logvar, requires_grad=True)
        self.shorten_cond_schedule = self.num_timesteps_cond > 1
        self.concat_mode, self.cond_stage_trainable, self.cond_stage_key = concat_mode, cond_stage_trainable, cond_stage_key
        self.cond_stage_forward = cond_stage_forward
        self.use_prob = use_prob
        self.instantiate_first_stage(first_stage_config)
        self.instantiate_cond_stage(cond_stage_config)
        n_scale = len(self.first_stage_model.embed_dim)
        if not scale_by_std:
            self.scale_factor = scale_factor
        elif not adopted_scale_factor:
            self.register_buffer("scale_factor", torch.tensor(scale_factor))
        else:
            self.register_buffer("scale_factor", torch.tensor([scale_factor for _ in range(n_scale)]))
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys)

    # -- schedule buffers (frido.py:127-168) --
    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        betas = given_betas if given_betas is not None else schedules.make_beta_schedule(
            beta_schedule, timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        self.num_timesteps = int(np.asarray(betas).shape[0])
        self.linear_start, self.linear_end = linear_start, linear_end
        for k, v in schedules.ddpm_tables(betas, v_posterior=self.v_posterior).items():
            self.register_buffer(k, torch.from_numpy(v))
        self._anc_tabs = {}      # device coefficient tables of the ancestral update, per (device, clip, with noise)
        # frido.py:169-178 (eps parameterization), float32 torch arithmetic on the registered buffers like the reference's
        alphas = torch.tensor(1. - np.asarray(betas, dtype=np.float64), dtype=torch.float32)
        lvlb_weights = self.betas ** 2 / (2 * self.posterior_variance * alphas * (1 - self.alphas_cumprod))
        lvlb_weights[0] = lvlb_weights[1]
        self.register_buffer("lvlb_weights", lvlb_weights, persistent=False)
        assert not torch.isnan(self.lvlb_weights).all()

    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False):
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd)
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        target = self.model if only_model else self
        return target.load_state_dict(sd, strict=False)

    def instantiate_first_stage(self, cfg):
        model = instantiate_from_config(_plain(cfg))
        self.first_stage_model = model.eval()
        for p in self.first_stage_model.parameters():
            p.requires_grad = False
        self.num_resulotion = len(self.first_stage_model.res_list)
        self.embed_dim_list = self.first_stage_model.embed_dim

    def instantiate_cond_stage(self, cfg):
        if cfg in ("__is_first_stage__",):
            self.cond_stage_model = self.first_stage_model
        elif cfg == "__is_unconditional__":
            self.cond_stage_model = None
        else:
            self.cond_stage_model = instantiate_from_config(_plain(cfg))
            if self.cond_stage_model is not None:
                self.cond_stage_model.eval()

    @contextlib.contextmanager
    def ema_scope(self, context=None, *, keep_runtimes=False):
        """frido.py:181-194: sample with the EMA weights, then restore.  Both swaps drop the denoiser's compiled runtime (plans, engines,
        graphs).  keep_runtimes (validation_step, which enters this scope once per batch): keep one runtime per weight set instead --
        the raw weights' is put back as it was (restore() writes back the very bits it was compiled from), the EMA weights' is reused
        by the next such scope as long as no tensor of the EMA shadow was written since (their version counters).  Costs a second set
        of packed weights and engines on the device."""
        unet = self.model.diffusion_model
        if self.use_ema:
            self.model_ema.store(self.model.parameters())
            self.model_ema.copy_to(self.model)
            if keep_runtimes:
                raw = (unet._rt, unet._rt_key)
                shadow = tuple(b._version for b in self.model_ema.buffers())
                kept = self.__dict__.get("_ema_rt")
                unet._rt, unet._rt_key = kept[1:] if kept is not None and kept[0] == shadow else (None, None)
            else:
                unet.invalidate()
            if context is not None:
                print(f"{context}: Switched to EMA weights")
        try:
            yield None
        finally:
            if self.use_ema:
                self.model_ema.restore(self.model.parameters())
                if keep_runtimes:
                    self.__dict__["_ema_rt"] = (shadow, unet._rt, unet._rt_key)
                    unet._rt, unet._rt_key = raw
                else:
                    unet.invalidate()
                if context is not None:
                    print(f"{context}: Restored training weights")

    def get_learned_conditioning(self, c):
        """frido.py:664-675."""
        if self.cond_stage_forward is None:
            if hasattr(self.cond_stage_model, "encode") and callable(self.cond_stage_model.encode):
                return self.cond_stage_model.encode(c)
            return self.cond_stage_model(c)
        return getattr(self.cond_stage_model, self.cond_stage_forward)(c)

    def get_first_stage_encoding(self, z):
        """frido.py:647-662 (tensor branch)."""
        if not self.adopted_scale_factor:
            return self.scale_factor * z
        start = 0
        for i, e in enumerate(self.first_stage_model.embed_dim):
            if start + e <= z.size(1):
                z[:, start:start + e] *= self.scale_factor[i]
                start += e
        return z.clone()

    def apply_model(self, x_noisy, t, cond, stage=None, return_ids=False):
        """frido.py:1062-1160.  With `split_input_params` set (looked up on every call, like the reference's hasattr) the patch-wise
        branch of :1076-1152 runs: x_noisy is cut into overlapping crops (frido_unfold), the denoiser runs ONCE on the B * L crop batch
        (timesteps, context / labels repeated per crop), and the eps is stitched back with the border-distance weighting (frido_fold)."""
        from . import patching
        patch = patching.params_of(self)
        if patch is not None:
            if return_ids:
                raise ValueError("apply_model(return_ids=True) with split_input_params set: the reference asserts `not return_ids` (frido.py:1078)")
            patching.check_conditioning(self, cond)
            return self._apply_model_patches(x_noisy, t, cond, stage, patch)
        if not isinstance(cond, dict):
            if not isinstance(cond, list):
                cond = [cond]
            cond = {"c_concat" if self.model.conditioning_key == "concat" else "c_crossattn": cond}
        out = self.model(x_noisy, t, stage=stage, **cond)
        return out[0] if isinstance(out, tuple) and not return_ids else out

    def _apply_model_patches(self, x_noisy, t, cond, stage, patch):
        from . import patching
        from .runtime import patch_fold, patch_unfold
        B, _, H, W = x_noisy.shape
        geo = patching.geometry(patch, H, W, patching.MODEL, x_noisy.device)      # raises for a geometry the reference cannot stitch
        _on_gpu("FridoDiffusion.apply_model", x_noisy)
        unet = self.model.diffusion_model
        # the builder only launches layout changes and the two patch kernels, which are the same code in both builds of the library: should
        # the automatic plane selection move the denoiser to another runtime during the forward below, folding on this one is still right
        b = unet.runtime().b
        crops = patch_unfold(b, geo, x_noisy.float())                                  # (B * L, C, kh, kw), crop l of sample b at b * L + l
        per_crop = lambda v: None if v is None else v.repeat_interleave(geo.L, dim=0)
        t = torch.as_tensor(t, device=x_noisy.device, dtype=torch.long).reshape(-1)
        out = self.model(crops, per_crop(t), stage=stage, c_crossattn=[per_crop(cond)])      # cond None: [None], like the whole-latent path
        assert not isinstance(out, tuple), "the patch-wise mode cannot deal with multiple model outputs (frido.py:1144-1145)"
        return patch_fold(b, geo, out, B)

    @torch.no_grad()
    def decode_first_stage(self, z_in, predict_cids=False, force_not_quantize=False, return_code=False, to_uint8=False,
                           force_codes=None):
        """frido.py:823-891: per-scale 1/scale_factor (fused into the VQ kernel) + first-stage decode.  With split_input_params set
        and its patch_distributed_vq true (:840-877): the latent is unfolded (1/scale_factor is per pixel, so it stays in the VQ kernel of
        the crops), all crops are decoded as one batch and folded at vqf x the resolution; to_uint8 converts in the fold kernel."""
        assert not predict_cids
        embed = self.first_stage_model.embed_dim
        if not self.adopted_scale_factor:
            sf = float(self.scale_factor)
            inv = [float(np.float32(1.0) / np.float32(sf))] * len(embed)
        else:
            sfs = self.scale_factor.detach().float().cpu().numpy()
            inv = [float(np.float32(1.0) / np.float32(v)) for v in sfs]
        from . import patching
        patch = patching.params_of(self)
        if patch is not None and patch["patch_distributed_vq"]:
            if return_code or force_codes is not None:
                raise patching.refuse("return_code / force_codes (the reference's patch-wise decode returns the image only)")
            fs = self.first_stage_model
            geo = patching.geometry(patch, z_in.shape[2], z_in.shape[3], patching.DECODE, z_in.device)
            _on_gpu("FridoDiffusion.decode_first_stage", z_in)
            return autoplanes.run(fs, lambda _n: fs.runtime().decode_patches(z_in, geo, inv_scale=inv, to_uint8=to_uint8),
                                  "FridoDiffusion.decode_first_stage")
        return self.first_stage_model.decode(z_in, return_code=return_code, inv_scale=inv, to_uint8=to_uint8,
                                             force_codes=force_codes)

    @torch.no_grad()
    def encode_first_stage(self, x):
        """frido.py:962-1005 (the reference's duplicated encode call is not repeated).  With split_input_params set and its
        patch_distributed_vq true (:963-993): image crops are encoded as one batch and folded at 1 / vqf of the resolution; the image size is
        recorded in split_input_params['original_image_size'] like :968."""
        from . import patching
        patch = patching.params_of(self)
        if patch is not None and patch["patch_distributed_vq"]:
            patch["original_image_size"] = x.shape[-2:]
            fs = self.first_stage_model
            geo = patching.geometry(patch, x.shape[2], x.shape[3], patching.ENCODE, x.device)
            _on_gpu("FridoDiffusion.encode_first_stage", x)
            return autoplanes.run(fs, lambda _n: fs.runtime().encode_patches(x, geo), "FridoDiffusion.encode_first_stage")
        return self.first_stage_model.encode(x)

    @torch.no_grad()
    def get_input(self, batch, k, return_first_stage_outputs=False, force_c_encode=False, cond_key=None,
                  return_original_cond=False, bs=None):
        """frido.py:767-816 for the inference callers (scripts/sample_diffusion.py:236-240): returns [z, c, (x, xrec), (xc)]."""
        x = batch[k]
        if x.dim() == 3:
            x = x[..., None]
        x = x.permute(0, 3, 1, 2).contiguous().float()          # 'b h w c -> b c h w' (frido.py:372-380)
        if bs is not None:
            x = x[:bs]
        x = x.to(self.device)
        sf = self.scale_factor.detach().float().cpu().numpy() if torch.is_tensor(self.scale_factor) else [float(self.scale_factor)]
        n = len(self.first_stage_model.embed_dim)
        scale = [float(sf[i] if len(sf) > 1 else sf[0]) for i in range(n)]
        z = self.first_stage_model.encode(x, scale=scale)        # encode + get_first_stage_encoding fused
        c = None
        if self.model.conditioning_key is not None:
            ck = cond_key or self.cond_stage_key
            xc = batch[ck] if ck != self.first_stage_key else x
            if bs is not None and torch.is_tensor(xc):
                xc = xc[:bs]
            c = self.get_learned_conditioning(xc.to(self.device) if torch.is_tensor(xc) else xc) if force_c_encode or not self.cond_stage_trainable else xc
        out = [z, c]
        if return_first_stage_outputs:
            out.extend([x, self.decode_first_stage(z)])
        if return_original_cond:
            out.append(xc)
        return out

    def get_img_ids(self, batch):
        """frido.py:818-820."""
        return batch["file_name"]

    @torch.no_grad()
    def q_sample(self, x_start, t, ch_start=None, ch_end=None, noise=None, mix_tau=0.):
        """frido.py:302-320: forward diffusion x_t = sqrt(a_t) x_0 + sqrt(1 - a_t) eps, optionally only on the channels
        [ch_start, ...) of a multi-stage latent (coarser channels kept, channels from ch_end on replaced by noise,
        optional noise mixing of the kept ones).  A host-side helper of the callers (mask-guided sampling, logging), not on
        the per-step path: plain tensor arithmetic on whatever device the inputs live on."""
        if noise is None:
            noise = torch.randn_like(x_start)
        shape = (x_start.shape[0],) + (1,) * (x_start.dim() - 1)
        a = self.sqrt_alphas_cumprod.to(x_start.device)[t].reshape(shape)
        s = self.sqrt_one_minus_alphas_cumprod.to(x_start.device)[t].reshape(shape)
        if ch_start is None:
            return a * x_start + s * noise
        out = x_start.clone()
        out[:, ch_start:] = a * x_start[:, ch_start:] + s * noise[:, ch_start:]
        if ch_end is not None:
            out[:, ch_end:] = noise[:, ch_end:]
        if mix_tau != 0.:
            out[:, :ch_start] = (1 - mix_tau) * out[:, :ch_start] + mix_tau * noise[:, :ch_start]
        return out

    # ---- ancestral (DDPM) sampling (frido.py:230-256,1226-1452) ---------------------------------------------------------
    # The reference as shipped cannot run this branch (p_mean_variance reads a flag off the DiffusionWrapper that is not there, and the
    # split head's eps has fewer channels than the latent the loops carry: tests/golden/ancestral_cfg.py).  What is built here is that
    # code with the flag in place and the eps zero-padded to the latent's channels -- the reading under which its own lines are well-formed.
    def _extract(self, name, t, x):
        """extract_into_tensor (frido/modules/diffusionmodules/util.py): buffer[t] shaped (B, 1, 1, ...) for broadcasting against x."""
        t = torch.as_tensor(t, device=x.device, dtype=torch.long)
        return getattr(self, name).to(x.device).gather(-1, t).reshape(t.shape[0], *((1,) * (x.dim() - 1)))

    def predict_start_from_noise(self, x_t, t, noise, ch_start=None, ch_end=None):
        """frido.py:230-242: x_0 from x_t and eps; with ch_start only channels [ch_start, ch_end) are converted, the rest are x_t's.  Plain
        tensor arithmetic on the inputs' device (a helper of the callers; the sampling path has it inside the update kernel)."""
        a, b = self._extract("sqrt_recip_alphas_cumprod", t, x_t), self._extract("sqrt_recipm1_alphas_cumprod", t, x_t)
        if ch_start is None:
            return a * x_t - b * noise
        out = x_t.clone()
        out[:, ch_start:] = a * out[:, ch_start:] - b * noise[:, ch_start:]
        if ch_end is not None:
            out[:, ch_end:] = x_t[:, ch_end:]
        return out

    def q_posterior(self, x_start, x_t, t, ch_start=None, ch_end=None):
        """frido.py:244-256: mean, variance and clipped log variance of q(x_{t-1} | x_t, x_0); outside [ch_start, ch_end) the mean is x_t."""
        mean = self._extract("posterior_mean_coef1", t, x_t) * x_start + self._extract("posterior_mean_coef2", t, x_t) * x_t
        if ch_start is not None:
            mean[:, :ch_start] = x_t[:, :ch_start]
            if ch_end is not None:
                mean[:, ch_end:] = x_t[:, ch_end:]
        return mean, self._extract("posterior_variance", t, x_t), self._extract("posterior_log_variance_clipped", t, x_t)

    def _anc_refuse(self, cond=None, quantize_denoised=False, return_codebook_ids=False, mask=None, x0=None, loop=False):
        if hasattr(self, "split_input_params"):
            from .patching import refuse
            raise refuse("ancestral sampling (p_sample / p_mean_variance / p_sample_loop / progressive_denoising)")
        if quantize_denoised:
            raise NotImplementedError("quantize_denoised: `first_stage_model.quantize` does not exist on the MS-VQGAN (the reference raises an "
                                      "AttributeError at frido.py:1256)")
        if return_codebook_ids:
            raise NotImplementedError("return_codebook_ids: the denoiser has no codebook-id head (predict_codebook_ids) on the HIP path; the "
                                      "reference's p_sample raises 'Support dropped.' (frido.py:1278-1279)")
        if mask is not None or x0 is not None:
            raise NotImplementedError("mask / x0 (inpainting blend, frido.py:1405-1407): the sampler-step descriptor of ABI 7 has no room for the "
                                      "blend's operands")
        if loop and self.num_timesteps_cond > 1:
            raise NotImplementedError("shorten_cond_schedule (num_timesteps_cond > 1, frido.py:1396-1399): the per-step q_sample of the conditioning "
                                      "is not built")
        if isinstance(cond, dict):
            raise NotImplementedError("dict conditionings ('concat' / 'hybrid'): pass the cross-attention conditioning tensor or the class labels")
        if not self.use_split_head:
            raise NotImplementedError("ancestral sampling masks channels per stage, which needs use_split_head=True (every shipped Frido config)")

    def _anc_host_tables(self):
        """The five schedule buffers schedules.ancestral_table reads, as host arrays."""
        return {k: getattr(self, k).detach().float().cpu().numpy() for k in (
            "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
            "posterior_log_variance_clipped")}

    def _anc_table(self, device, clip, with_noise):
        key = (str(device), bool(clip), bool(with_noise))
        if key not in self._anc_tabs:
            tab = schedules.ancestral_table(self._anc_host_tables(), clip_denoised=clip)
            if not with_noise:
                tab[:, 4] = 0.0          # p_mean_variance: x' = the posterior mean
            self._anc_tabs[key] = torch.from_numpy(tab).to(device)
        return self._anc_tabs[key]

    def _anc_update(self, x, c, t, stage, clip_denoised, score_corrector, corrector_kwargs, noise=None, with_noise=False, temperature=1.,
                    seed=0, sample0=0):
        """Denoiser forward + ONE launch of the ancestral update kernel per distinct timestep: (x' or the posterior mean, x0)."""
        _on_gpu("FridoDiffusion.p_sample", x)
        from .runtime import ancestral_step
        stage = int(stage)
        start, end = sum(self.embed_dim_list[:stage]), sum(self.embed_dim_list[:stage + 1])
        assert end <= x.shape[1], f"stage {stage} needs a latent of at least {end} channels"
        tl = [int(v) for v in torch.as_tensor(t).reshape(-1).tolist()]
        assert len(tl) == x.shape[0] and all(0 <= v < self.num_timesteps for v in tl), "t: one timestep in [0, num_timesteps) per sample"
        eps = self.apply_model(x, torch.as_tensor(t, device=x.device, dtype=torch.long), c, stage=stage)      # (B, end - start, H, W)
        if score_corrector is not None:      # frido.py:1233-1241: the corrector sees the eps zero-padded to the latent's channels
            B, C, H, W = x.shape
            pad = torch.cat((x.new_zeros(B, start, H, W), eps, x.new_zeros(B, C - end, H, W)), dim=1)
            eps = score_corrector.modify_score(self, pad, x, t, c, **(corrector_kwargs or {}))[:, start:end].float().contiguous()
        unet = self.model.diffusion_model
        return ancestral_step(unet.runtime().b, x.float(), eps, [self.num_timesteps - 1 - v for v in tl],
                              self._anc_table(x.device, clip_denoised, with_noise), start, noise=noise, temperature=temperature, seed=seed,
                              sample0=sample0, rng_stream=stage + 1)

    @torch.no_grad()
    def p_mean_variance(self, x, c, t, stage, clip_denoised: bool, return_codebook_ids=False, quantize_denoised=False, return_x0=False,
                        score_corrector=None, corrector_kwargs=None):
        """frido.py:1226-1265: (posterior mean, variance, clipped log variance[, x_recon]) -- denoiser forward and update kernel on the HIP
        engine; the two variance factors are (B, 1, 1, 1) buffer lookups like the reference's."""
        self._anc_refuse(c, quantize_denoised, return_codebook_ids)
        mean, x0 = self._anc_update(x, c, t, stage, clip_denoised, score_corrector, corrector_kwargs)
        var, logvar = self._extract("posterior_variance", t, x), self._extract("posterior_log_variance_clipped", t, x)
        return (mean, var, logvar, x0) if return_x0 else (mean, var, logvar)

    @torch.no_grad()
    def p_sample(self, x, c, t, stage, clip_denoised=False, repeat_noise=False, return_codebook_ids=False, quantize_denoised=False,
                 return_x0=False, temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, *, noise="torch", seed=0,
                 sample0=0):
        """frido.py:1267-1305: one ancestral step x_t -> x_{t-1} at `stage` (t may differ per sample: the kernel then goes out per sample).
        noise: "torch" (default) draws like the reference -- one randn of x's shape from torch's CPU generator (repeat_noise: one sample's
        worth, repeated), times temperature, then the dropout mask; a callable shape -> tensor replays a tape; "philox" draws in the kernel,
        keyed by (seed, sample0 + b, num_timesteps - t, stage) -- the loops' key, so this call reproduces their draw at (t, stage)."""
        self._anc_refuse(c, quantize_denoised, return_codebook_ids)
        _on_gpu("FridoDiffusion.p_sample", x)
        nz = None
        if noise == "philox":
            if noise_dropout > 0. or repeat_noise:
                raise NotImplementedError("noise_dropout / repeat_noise act on host noise: use noise='torch' (or a recorded tape)")
        else:
            draw = torch.randn if noise == "torch" else noise
            shape = tuple(x.shape)
            nz = draw((1,) + shape[1:]).repeat(shape[0], *((1,) * (len(shape) - 1))) if repeat_noise else draw(shape)      # noise_like
            nz = torch.as_tensor(nz, dtype=torch.float32) * temperature
            if noise_dropout > 0.:
                nz = torch.nn.functional.dropout(nz, p=noise_dropout)
            nz = nz.to(x.device)
        out, x0 = self._anc_update(x, c, t, stage, clip_denoised, score_corrector, corrector_kwargs, noise=nz, with_noise=True,
                                   temperature=float(temperature) if nz is None else 1.0, seed=seed, sample0=sample0)
        return (out, x0) if return_x0 else out

    def _anc_loop(self, cond, shape, T, what, *, noise, seed, sample0, collect, temperature=1., **kw):
        """The loop on the SamplerEngine (kind="ddpm"): cached per (batch, latent shape, conditioning mode, T, clip, temperature) next to the
        DDIM / PLMS engines of the denoiser, the whole call under the automatic plane selection."""
        from . import samplers
        from .runtime import SamplerEngine
        unet = self.model.diffusion_model
        B, C, H, W = (int(v) for v in shape)
        if isinstance(cond, list):
            raise NotImplementedError("list conditionings: pass the cross-attention conditioning tensor or the class labels")
        _on_gpu(what, cond)
        mode = samplers.check_conditioning(unet, cond, B, name="cond")
        _on_gpu(what, unet)
        clip = bool(self.clip_denoised)
        temp_key = float(temperature) if noise == "philox" else 1.0

        def make(rt):      # only on an engine-cache miss: the posterior tables leave the device once per engine
            return SamplerEngine(rt.builder_for(0), unet.cfg, B=B, C=C, H=H, W=W, nctx=mode if isinstance(mode, int) else 0, S=T, eta=0.,
                                 kind="ddpm", alphas_cumprod=None, embed_dim=self.embed_dim_list, num_stage=self.num_resulotion,
                                 temperature=temp_key, posterior=self._anc_host_tables(), clip=clip)

        def go(noise_src):
            rt = unet.runtime()
            eng = samplers.cached_engine(rt, ("ddpm", B, C, H, W, mode, T, clip, temp_key), lambda: make(rt))
            return eng.run_ancestral(cond, noise=noise_src, seed=seed, sample0=sample0, collect=collect, temperature=temperature,
                                     model=self, **kw)
        return autoplanes.run(unet, go, what, noise=noise)

    @torch.no_grad()
    def progressive_denoising(self, cond, shape, verbose=True, callback=None, quantize_denoised=False, img_callback=None, mask=None, x0=None,
                              temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None, batch_size=None, x_T=None,
                              start_T=None, log_every_t=None, *, noise="torch", seed=0, sample0=0):
        """frido.py:1307-1363: the ancestral loop returning (img, the x0 predictions logged every log_every_t steps); `shape` excludes the
        batch when batch_size is given; temperature: a float or one value per timestep."""
        self._anc_refuse(cond, quantize_denoised, False, mask, x0, loop=True)
        if not log_every_t:
            log_every_t = self.log_every_t
        if batch_size is not None:
            shape = [batch_size] + list(shape)
        else:
            batch_size = shape[0]
        cond = _first(cond, batch_size)
        T = self.num_timesteps if start_T is None else min(self.num_timesteps, start_T)
        return self._anc_loop(cond, shape, T, "FridoDiffusion.progressive_denoising", noise=noise, seed=seed, sample0=sample0, collect="x0",
                              temperature=temperature, x_T=x_T, log_every_t=log_every_t, callback=callback, img_callback=img_callback,
                              noise_dropout=noise_dropout, score_corrector=score_corrector, corrector_kwargs=corrector_kwargs)

    @torch.no_grad()
    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None, log_every_t=None, *, noise="torch", seed=0,
                      sample0=0):
        """frido.py:1365-1418: for every stage, t = timesteps - 1 ... 0, one ancestral step of the full latent; `intermediates` starts with
        x_T and gains the state at t % log_every_t == 0 or t == timesteps - 1, all stages in one list.  noise / seed / sample0: as for the
        DDIM / PLMS samplers (frido_amd/samplers.py)."""
        self._anc_refuse(cond, quantize_denoised, False, mask, x0, loop=True)
        if not log_every_t:
            log_every_t = self.log_every_t
        T = self.num_timesteps if timesteps is None else timesteps
        if start_T is not None:
            T = min(T, start_T)
        img, inter = self._anc_loop(cond, shape, int(T), "FridoDiffusion.p_sample_loop", noise=noise, seed=seed, sample0=sample0, collect="img",
                                    x_T=x_T, log_every_t=log_every_t, callback=callback, img_callback=img_callback)
        return (img, inter) if return_intermediates else img

    @torch.no_grad()
    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None, quantize_denoised=False,
               mask=None, x0=None, shape=None, **kwargs):
        """frido.py:1420-1437.  Like the reference, only the named arguments reach p_sample_loop -- plus noise / seed / sample0 from kwargs."""
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        cond = _first(cond, batch_size)
        extra = {k: kwargs[k] for k in ("noise", "seed", "sample0") if k in kwargs}
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose, timesteps=timesteps,
                                  quantize_denoised=quantize_denoised, mask=mask, x0=x0, **extra)

    @torch.no_grad()
    def sample_log(self, cond, batch_size, ddim, ddim_steps, num_stage=1, **kwargs):
        """frido.py:1439-1452: DDIM through DDIMSampler, otherwise the ancestral loop with its intermediates."""
        if ddim:
            from .samplers import DDIMSampler
            shape = (self.channels, self.image_size, self.image_size)
            return DDIMSampler(self).sample(ddim_steps, batch_size, shape, cond, num_stage=num_stage, verbose=False, **kwargs)
        return self.sample(cond=cond, batch_size=batch_size, return_intermediates=True, **kwargs)

    # ---- the objective (frido.py:196-228, 322-345, 382-419, 1007-1050, 1162-1224) -----------------------------------------------------
    # Evaluating it needs no gradient: it is what test_step / validation_step do.  q_sample, the denoiser and the loss of every stage run
    # as ONE captured graph (frido_amd/objective.py LossEngine); the helpers below are plain tensor arithmetic like q_sample.
    def get_loss(self, pred, target, mean=True):
        """frido.py:322-336."""
        if self.loss_type == "l1":
            loss = (target - pred).abs()
            return loss.mean() if mean else loss
        if self.loss_type == "l2":
            return torch.nn.functional.mse_loss(target, pred, reduction="mean" if mean else "none")
        raise NotImplementedError(f"unknown loss type '{self.loss_type}'")

    def q_mean_variance(self, x_start, t):
        """frido.py:196-207: mean, variance and log variance of q(x_t | x_0), each broadcast against x_start."""
        mean = self._extract("sqrt_alphas_cumprod", t, x_start) * x_start
        shape = (x_start.shape[0],) + (1,) * (x_start.dim() - 1)
        t = torch.as_tensor(t, device=x_start.device, dtype=torch.long)
        variance = (1.0 - self.alphas_cumprod).to(x_start.device).gather(-1, t).reshape(shape)
        return mean, variance, self._extract("log_one_minus_alphas_cumprod", t, x_start)

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """frido.py:1162-1164."""
        return (self._extract("sqrt_recip_alphas_cumprod", t, x_t) * x_t - pred_xstart) / self._extract("sqrt_recipm1_alphas_cumprod", t, x_t)

    def _prior_bpd(self, x_start):
        """frido.py:1166-1178: KL(q(x_T | x_0) || N(0, I)) per sample in bits per dimension (normal_kl + mean_flat of the published
        guided-diffusion losses, against a standard normal)."""
        t = torch.tensor([self.num_timesteps - 1] * x_start.shape[0], device=x_start.device)
        mean1, _, logvar1 = self.q_mean_variance(x_start, t)
        logvar2 = torch.tensor(0.0).to(logvar1)
        kl = 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + ((mean1 - 0.0) ** 2) * torch.exp(-logvar2))
        return kl.mean(dim=list(range(1, kl.dim()))) / np.log(2.0)

    def _objective_refuse(self, cond):
        if hasattr(self, "split_input_params"):
            from .patching import refuse
            raise refuse("the objective (forward / p_losses / validation_step)")
        if self.shorten_cond_schedule:
            raise NotImplementedError("shorten_cond_schedule (num_timesteps_cond > 1, frido.py:1031-1033): the q_sample of the conditioning is not built")
        if isinstance(cond, (dict, list)):
            raise NotImplementedError("dict / list conditionings: pass the cross-attention conditioning tensor or the class labels")
        if self.model.conditioning_key in ("concat", "hybrid"):
            raise NotImplementedError(f"conditioning_key={self.model.conditioning_key!r}: the objective is built for 'crossattn', 'adm' and "
                                      "unconditional denoisers")
        if not self.use_split_head:
            raise NotImplementedError("use_split_head=False: the objective compares the stage's own eps channels, which needs the split head "
                                      "(every shipped Frido config)")

    def _objective(self, x_start, cond, t, noise, seed, sample0, stages=None):
        """Stage rows [num_stage][4] = {loss_simple, loss_gamma, loss_vlb, loss} and per-sample loss_simple [num_stage][B] of ONE engine call
        (device tensors; `stages`: the stages that run and whose rows are valid, default all).
        noise: "philox", or a list with one (B, C, H, W) tensor per stage (None for a stage that does not run).
        The engine is cached per (B, latent shape, conditioning mode, T); the schedule tables and logvar are handed over on every call
        and the objective's scalars key its graphs, so a changed schedule, weight or loss type is in force at the next call."""
        from . import samplers
        from .objective import LossEngine
        unet = self.model.diffusion_model
        _on_gpu("FridoDiffusion.p_losses", x_start, cond, unet)
        B, C, H, W = (int(v) for v in x_start.shape)
        tl = torch.as_tensor(t).reshape(-1)
        assert tl.shape[0] == B, "t: one timestep per sample"
        if not tl.is_cuda:      # (a device t is not read back: the kernels clamp it to the tables)
            assert bool(((tl >= 0) & (tl < self.num_timesteps)).all()), "t: one timestep in [0, num_timesteps) per sample"
        mode = samplers.check_conditioning(unet, cond, B, name="cond")
        assert len(self.stage_loss_ratio) == self.num_resulotion, "Incorrect number of stage_loss_ratio."
        key = ("loss", B, C, H, W, mode, self.num_timesteps)
        tables = (self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, self.lvlb_weights)
        tape = None if isinstance(noise, str) else list(noise)

        def go(_n):
            rt = unet.runtime()
            eng = samplers.cached_engine(rt, key, lambda: LossEngine(
                rt.builder_for(0), unet.cfg, B=B, C=C, H=H, W=W, nctx=mode if isinstance(mode, int) else 0, embed_dim=self.embed_dim_list,
                num_stage=self.num_resulotion, T=self.num_timesteps))
            return eng.run(x_start, cond, tl, tables=tables, tape=tape, seed=seed, sample0=sample0, logvar=self.logvar, stages=stages,
                           loss_type=self.loss_type, mix_tau=self.noise_mix_ratio, l_simple_weight=self.l_simple_weight,
                           original_elbo_weight=self.original_elbo_weight)
        return autoplanes.run(unet, go, "FridoDiffusion.p_losses")

    def _noise_tape(self, noise, shape, stages):
        """_objective's `noise` from p_losses' / forward's: "philox" as it is; else one entry per stage of the model, for the stages of
        `stages` the given tensor or (None / "torch") a randn(shape) of its own from the host generator, in stage order, None elsewhere."""
        if isinstance(noise, str) and noise == "philox":
            return "philox"
        host = noise is None or isinstance(noise, str)
        given = {s: torch.randn(tuple(shape)) if host else noise for s in stages}
        return [given.get(s) for s in range(self.num_resulotion)]

    def _loss_dict(self, row, stage):
        """p_losses' dict of one stage row (frido.py:1188-1222), values as 0-dim device tensors."""
        prefix = "train" if self.training else "val"
        d = {f"{prefix}/loss_simple_stage{stage}": row[0]}
        if self.learn_logvar:
            d[f"{prefix}/loss_gamma"] = row[1]
            d["logvar"] = self.logvar.data.mean()
        d[f"{prefix}/loss_vlb_stage{stage}"] = row[2]
        d[f"{prefix}/loss"] = row[3]
        return row[3], d

    @torch.no_grad()
    def p_losses(self, x_start, cond, t, stage, noise=None, *, seed=0, sample0=0, return_per_sample=False):
        """frido.py:1180-1224: (loss, loss_dict) of one stage -- only that stage's launches run (a graph of its own on the engine that
        forward uses).  noise: None / "torch" draws randn_like(x_start) from the host generator (the reference's draw), a tensor is used
        as it is, "philox" draws in the kernels keyed by (seed, sample0 + b, stage).
        return_per_sample: also the per-sample loss_simple [B]."""
        self._objective_refuse(cond)
        stage = int(stage)
        tape = self._noise_tape(noise, x_start.shape, (stage,))
        assert 0 <= stage < self.num_resulotion, f"stage {stage}: the model has {self.num_resulotion}"
        rows, per = self._objective(x_start, cond, t, tape, seed, sample0, stages=(stage,))
        out = self._loss_dict(rows[stage], stage)
        return out + (per[stage],) if return_per_sample else out

    @torch.no_grad()
    def forward(self, x, c, *args, t=None, noise=None, seed=0, sample0=0, **kwargs):
        """frido.py:1026-1050: t = randint(0, T, (B,)) first (unless given), then per stage one randn_like(x) and p_losses; stage values are
        combined with stage_loss_ratio -- including the reference's quirk that a key shared between stages ('{prefix}/loss', and under
        learn_logvar 'loss_gamma' / 'logvar') accumulates the already-weighted values.  All stages run in ONE engine call.
        noise: None / "torch" (host generator, draw for draw), "philox" (rng_stream = stage), or a tensor (the same noise for every stage,
        the reference's `p_losses(..., noise=)` meaning)."""
        if args or kwargs:
            raise TypeError(f"FridoDiffusion.forward: unexpected arguments {args} {sorted(kwargs)} (p_losses takes noise= only)")
        self._objective_refuse(c)
        if t is None:
            t = torch.randint(0, self.num_timesteps, (x.shape[0],)).long()
        if self.model.conditioning_key is not None:
            assert c is not None
            if self.cond_stage_trainable:
                c = self.get_learned_conditioning(c)
        S = self.num_resulotion
        assert len(self.stage_loss_ratio) == S, "Incorrect number of stage_loss_ratio."
        rows, _ = self._objective(x, c, t, self._noise_tape(noise, x.shape, range(S)), seed, sample0)
        total_loss = torch.zeros((), device=x.device)
        total_loss_dict = dict()
        for s in range(S):
            loss, loss_dict = self._loss_dict(rows[s], s)
            total_loss = total_loss + loss * self.stage_loss_ratio[s]
            for k, v in loss_dict.items():
                total_loss_dict[k] = total_loss_dict[k] + v * self.stage_loss_ratio[s] if k in total_loss_dict else v * self.stage_loss_ratio[s]
        return total_loss, total_loss_dict

    def shared_step(self, batch, **kwargs):
        """frido.py:1007-1009."""
        x, c = self.get_input(batch, self.first_stage_key)
        return self(x, c, **kwargs)

    def training_step(self, batch, batch_idx):
        raise FridoHipError("training_step: no backward pass exists on the HIP path (the objective is evaluated without gradients: "
                            "forward / p_losses / validation_step / test_step)")

    @torch.no_grad()
    def validation_step(self, batch, batch_idx, **kwargs):
        """frido.py:401-411: the raw weights' dict, then the EMA weights' with '_ema' key suffixes; both are logged and the merged dict is
        returned.  The scope keeps one compiled runtime per weight set (ema_scope(keep_runtimes=True)), so from the second batch on
        both passes replay their captured graphs."""
        _, loss_dict_no_ema = self.shared_step(batch, **kwargs)
        with self.ema_scope(keep_runtimes=True):
            _, loss_dict_ema = self.shared_step(batch, **kwargs)
            loss_dict_ema = {key + "_ema": loss_dict_ema[key] for key in loss_dict_ema}
        self.log_dict(loss_dict_no_ema, prog_bar=False, logger=True, on_step=False, on_epoch=True)
        self.log_dict(loss_dict_ema, prog_bar=False, logger=True, on_step=False, on_epoch=True)
        return {**loss_dict_no_ema, **loss_dict_ema}

    @torch.no_grad()
    def test_step(self, batch, batch_idx, **kwargs):
        """frido.py:413-417."""
        return self.shared_step(batch, **kwargs)


MSLatentDiffusion = FridoDiffusion   # stale alias `ldm.models.diffusion.msldm.MSLatentDiffusion` in two shipped configs

"""Configurations of the AttentionBlock denoiser fixtures (plain dicts, our own): UNET_SMALL of golden_cfg.py with the attention family
switched from the SpatialTransformer to the reference's AttentionBlock (pyunet.py:303-358), which is the family that runs without a
cross-attention context.  Shared by tests/golden/make_golden_attnblock.py and the tests."""
from golden_cfg import UNET_SMALL, UNET_FULL

# two stages + split head + SPADE, legacy=True (the default) with num_head_channels=32: 64 / 96 channels -> 2 / 3 heads of 32,
# heads split before q / k / v (QKVAttentionLegacy)
AB_SMALL = dict(UNET_SMALL, use_spatial_transformer=False, context_dim=None)
# head dimension 64, heads from num_head_channels, q / k / v split before the heads (QKVAttention): 128 / 192 channels -> 2 / 3 heads
AB_D64 = dict(AB_SMALL, model_channels=64, num_head_channels=64, legacy=False, use_new_attention_order=True)
# legacy=True with num_heads=4 and no num_head_channels: ONE head in every block of the input path and the middle -- and, by the
# reference's own rule (pyunet.py:764: the output path hands num_heads_upsample to the block), num_heads_upsample heads on the
# output path, so one head everywhere needs num_heads_upsample=1
AB_LEGACY4 = dict(AB_SMALL, num_head_channels=-1, num_heads=4, num_heads_upsample=1)
# class-conditional: label_emb as nn.Embedding (y int64 [B]) and as nn.Linear (y float [B, num_classes])
AB_CLS_EMB = dict(AB_SMALL, num_classes=10, use_embed=True)
AB_CLS_LIN = dict(AB_SMALL, num_classes=10, use_embed=False)
# Sampler fixtures: the same small two-stage split-head models WITHOUT SPADE.  Measured on the reference itself (CPU, make_golden_attnblock.py
# records it as *_ref_sens): with SPADE an AttentionBlock of stage 1 sees its input scaled by gamma maps computed from the UN-normalised
# stage-0 latent (|z| up to 35 - 160 under the synthetic weights) with nothing between that norm and the qkv projection, its softmax
# becomes a near-argmax, and the reference's OWN sampling run moves by 1.2e-3 (DDIM, S 4) / 1.0e-1 (PLMS, S 6) of the latent maximum when
# every eps it computes is perturbed by 1e-6 relative -- no fp32 implementation, the reference on another BLAS included, reproduces such a
# golden to the samplers' 1e-3 bound.  (The SpatialTransformer has a LayerNorm in front of its attention: the existing fixtures amplify 1x.)
# Without SPADE the same perturbation moves the result by 1.3e-6 / 4.7e-7.  SPADE-fed AttentionBlocks are pinned by the forward fixtures
# above (both stages, eps to 2e-4).
AB_SMP = dict(AB_SMALL, use_SPADE_norm=False)
AB_SMP_EMB = dict(AB_SMP, num_classes=10, use_embed=True)
AB_SMP_LIN = dict(AB_SMP, num_classes=10, use_embed=False)
# the shipped f8f4 denoiser with the attention family switched: 12 / 18 / 30 heads of 32 over 1024 / 256 / 64 tokens
AB_FULL = dict(UNET_FULL, use_spatial_transformer=False, context_dim=None)

FORWARD = {"ab_small": AB_SMALL, "ab_d64": AB_D64, "ab_legacy4": AB_LEGACY4, "ab_cls_emb": AB_CLS_EMB, "ab_cls_lin": AB_CLS_LIN}

"""Configurations of the patch-wise (split_input_params) fixtures, shared by tests/golden/make_golden_patch.py and the tests.

The models are the small two-stage split-head denoiser with and without SPADE and the small two-scale first stage; the conditioning is
a [2, 5, 64] tensor fed directly (cond_stage_key="caption": none of the keys for which the reference unfolds the conditioning itself).
Under a 1e-6 relative perturbation of every eps the reference's own patch-wise sampler results move by ~1e-6 of the latent maximum (the
generator measures and stores it per run as *_ref_sens and refuses to write a fixture above 1e-4).
"""
from golden_cfg import UNET_SMALL, VQ_SMALL  # noqa: F401

MODELS = {"spade": UNET_SMALL, "plain": dict(UNET_SMALL, use_SPADE_norm=False)}
COND_SHAPE = (2, 5, 64)
COND_STAGE_KEY = "caption"

# latent 16 x 16, 3 x 3 crops of 8 x 8: up to 4 crops over one pixel
SPLIT = dict(ks=(8, 8), stride=(4, 4), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01, clip_max_weight=0.5,
             clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
SPLIT_TIE = dict(SPLIT, tie_braker=True)
# latent 12 x 20, 3 x 4 crops of 4 x 8: rows do not overlap, columns do
SPLIT_RECT = dict(SPLIT, ks=(4, 8), stride=(4, 4))
RECT_HW = (12, 20)
# image 64 x 64, 3 x 3 crops of 32 x 32 -> latent crops of 8 x 8
SPLIT_ENC = dict(SPLIT, ks=(32, 32), stride=(16, 16))

# sampler runs: name -> (model, sampler, S, eta, guidance scale, split params)
RUNS = {"ddim_eta1": ("spade", "ddim", 4, 1.0, 1.0, SPLIT),
        "plms": ("spade", "plms", 5, 0.0, 1.0, SPLIT),
        "ddim_eta0_cfg": ("plain", "ddim", 4, 0.0, 1.5, SPLIT_TIE)}

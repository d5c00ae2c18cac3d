"""Records the exact bits of the DDIM / PLMS samplers (FridoSamplerStep.hist_mode 0, 1 and 3) on an MI355X, from whichever checkout
--repo names, into an .npz -- the fixture of tests/test_ancestral_gpu.py::test_ddim_and_plms_bits_are_those_of_the_library_before_the_mode.

    python tests/golden/record_sampler_bits.py --repo <built checkout of the commit to pin> --out tests/golden/sampler_step_bits_abi7.npz

tests/golden/sampler_step_bits_abi7.npz was recorded this way from a built checkout of ea2b9b2, the last commit before
FRIDO_STEP_ANCESTRAL: `frido_sampler_step` there has one kernel and no mode branch.  The small two-stage SpatialTransformer model of
smoke(), B = 2, latent 6 x 16 x 16, Philox noise (no host generator involved):
  ddim      DDIM-5, eta = 1 (hist_mode 0, noise every step), logged every 2 steps
  ddim_cfg  the same with classifier-free guidance 2.0 (the eps_uncond mix of the same kernel)
  plms      PLMS-6 (hist_mode 3 on the first step's second half, 1 afterwards)
Every GEMM runs on the library's static tile (FRIDO_TUNE = 0 here, tune.ENABLED = False in the test), so the bits do not depend on
what a tile cache holds.  `runs(model, c)` is shared with the test: only frido_amd names that exist on both sides of the change.
"""
import argparse
import os
import sys

import numpy as np

SEED, B, SHAPE, CTX = 11, 2, (6, 16, 16), (2, 5, 64)


def build_model():
    from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg
    from frido_amd.models import instantiate_from_config
    from frido_amd.synth import fill_module, seeded_normal
    import torch
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["conditioning_key"] = "__is_unconditional__", "crossattn"
    model = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    fill_module(model.model, "model.")
    fill_module(model.first_stage_model, "first_stage_model.")
    c = torch.from_numpy(seeded_normal("sampler_bits:c", CTX))
    return model.cuda().eval(), c.cuda()


def runs(model, c):
    """{name: float32 array}: final latents, plus the last logged state and x0 prediction of the DDIM run."""
    from frido_amd.samplers import DDIMSampler, PLMSSampler
    kw = dict(batch_size=B, shape=SHAPE, conditioning=c, num_stage=2, verbose=False, noise="philox", seed=SEED, log_every_t=2)
    out = {}
    z, inter = DDIMSampler(model).sample(S=5, eta=1.0, **kw)
    out["ddim"], out["ddim_x_inter_last"], out["ddim_pred_x0_last"] = z, inter["x_inter"][-1], inter["pred_x0"][-1]
    out["ddim_cfg"], _ = DDIMSampler(model).sample(S=5, eta=1.0, unconditional_guidance_scale=2.0, unconditional_conditioning=-c, **kw)
    out["plms"], _ = PLMSSampler(model).sample(S=6, eta=0.0, **kw)
    return {k: v.detach().float().cpu().numpy() for k, v in out.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repo", required=True, help="built checkout whose frido_amd is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["FRIDO_TUNE"] = "0"
    repo = os.path.abspath(a.repo)
    sys.path[:0] = [repo, os.path.join(repo, "tests", "golden")]
    import frido_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(frido_amd.__file__))) == repo, frido_amd.__file__
    res = runs(*build_model())
    assert all(np.isfinite(v).all() for v in res.values())
    np.savez_compressed(a.out, **res)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in res.items()})

"""Diffusion-objective fixtures: configurations, the run list and the shared input recipes.  Shared by tests/golden/make_golden_loss.py
(captures loss_*.npz from the reference's own FridoDiffusion.forward / validation_step on CPU) and the tests.

Two models on VQ_SMALL at B = 4, 16 x 16: the two-stage SPADE cross-attention denoiser (UNET_SMALL, key 'crossattn', a (B, 5, 64) context)
and the class-conditional AttentionBlock denoiser (AB_SMP_EMB, key 'adm').  Every run starts from torch.manual_seed(SEED) and lets the
model draw: t = randint first, then one randn_like(x) per stage -- the reference's order, which the tests replay from the host generator.

A validation_step run reads its inputs through `get_input`; both sides replace that ONE method on the instance with
`lambda batch, k: [batch["z"], batch["c"]]` (the first-stage encode of an image batch is pinned by other fixtures), everything after it --
shared_step, forward, ema_scope, the key suffixes -- is the code under test.
"""
import numpy as np

from attnblock_cfg import AB_SMP_EMB  # noqa: F401
from golden_cfg import UNET_SMALL, VQ_SMALL  # noqa: F401

SEED = 23
B = 4
SHAPE = (B, 6, 16, 16)
T = 1000

MODELS = {"unet_small": ("UNET_SMALL", "crossattn"), "ab_smp_emb": ("AB_SMP_EMB", "adm")}

# name -> constructor options of the run; `validation`: the run goes through validation_step (raw weights, then the EMA shadow)
_COMBOS = [("l1_mix", dict(loss_type="l1", original_elbo_weight=0., noise_mix_ratio=0.1)),
           ("l2_elbo", dict(loss_type="l2", original_elbo_weight=0.5, noise_mix_ratio=0.)),
           ("l1_elbo", dict(loss_type="l1", original_elbo_weight=0.5, noise_mix_ratio=0.)),
           ("l2_mix", dict(loss_type="l2", original_elbo_weight=0., noise_mix_ratio=0.1))]
RUNS = {
    "unet_small": dict(_COMBOS + [("l2_logvar", dict(loss_type="l2", original_elbo_weight=0.5, noise_mix_ratio=0.1, learn_logvar=True)),
                                  ("l1_val", dict(loss_type="l1", original_elbo_weight=0.5, noise_mix_ratio=0.1, validation=True))]),
    "ab_smp_emb": dict(_COMBOS + [("l1_logvar", dict(loss_type="l1", original_elbo_weight=0.5, noise_mix_ratio=0., learn_logvar=True)),
                                  ("l2_val", dict(loss_type="l2", original_elbo_weight=0., noise_mix_ratio=0.1, validation=True))]),
}
STAGE_LOSS_RATIO = [0.4, 0.6]
L_SIMPLE_WEIGHT = 0.75


def ctor_options(run):
    """FridoDiffusion keywords of a run."""
    o = {k: v for k, v in run.items() if k != "validation"}
    return dict(o, stage_loss_ratio=list(STAGE_LOSS_RATIO), l_simple_weight=L_SIMPLE_WEIGHT)


def logvar_ramp():
    """The learned log variance of the learn_logvar runs: a ramp over [-1, 1] with a seeded jitter, so that both the division by
    exp(logvar[t]) and the added term are exercised at every drawn t."""
    r = np.linspace(-1.0, 1.0, T) + 0.05 * np.random.default_rng(SEED).standard_normal(T)
    return np.clip(r, -1.0, 1.0).astype(np.float32)


def ema_shadow(name, weight):
    """The EMA shadow of parameter `name` (a numpy array `weight`): the weight under a seeded 2 % relative perturbation -- different
    from the weights, as well conditioned as they are."""
    import zlib
    g = np.random.default_rng(zlib.crc32(("ema:" + name).encode()))
    return (weight * (1.0 + 0.02 * g.standard_normal(weight.shape))).astype(np.float32)

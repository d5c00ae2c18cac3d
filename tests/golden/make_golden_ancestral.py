#!/usr/bin/env python3
"""Generate the ancestral-sampling fixtures (tests/golden/anc_*.npz) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixtures hold inputs and results only.  Weights are never stored: both sides
regenerate them with frido_amd.synth.fill_tensor keyed by state_dict name (make_golden_attnblock.build_frido).

    python tests/golden/make_golden_ancestral.py [anc_tables anc_uncond anc_cond]

Reference entry points exercised (frido/models/diffusion/frido.py): register_schedule :127-168, predict_start_from_noise / q_posterior
:230-256, p_mean_variance / p_sample :1226-1305, progressive_denoising :1308-1363, p_sample_loop :1366-1418, sample / sample_log
:1421-1452, decode_first_stage :823-891.  ancestral_cfg.py says why two shims on the model instance are needed to run them at all.
"""
import os
import sys
import inspect

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_attnblock as A  # noqa: E402  (reference harness, build_frido, NoiseTape, save, T, labels_for)
from golden_cfg import VQ_SMALL  # noqa: E402
from ancestral_cfg import (AB_SMP, AB_SMP_EMB, UNET_SMALL, SEED, B, SHAPE, TABLES, LINEAR, POSTERIOR_KEYS, FULL_T_CANDIDATES,  # noqa: E402
                           SIGNATURES)
from frido_amd.synth import seeded_normal  # noqa: E402

REF_SENS_MAX, REF_SENS_PERT = A.REF_SENS_MAX, A.REF_SENS_PERT


def build_frido(ucfg, vcfg, key, **over):
    """make_golden_attnblock.build_frido with top-level config overrides (timesteps=...): the same construction, weights and stream hooks."""
    fr = A.H.import_ref("frido.models.diffusion.frido")
    A.H.patch_samplers()
    cfg = dict(A.frido_cfg(ucfg, vcfg, dict()), **over)
    cfg["first_stage_config"]["params"]["lossconfig"] = {"target": "torch.nn.Identity"}
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    model = fr.FridoDiffusion(**cfg)
    model.model.conditioning_key = key
    A.fill_module(model.model, "model.")
    A.fill_module(model.first_stage_model, "first_stage_model.")
    model.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    net = model.model.diffusion_model
    for blk in list(net.input_blocks) + [net.middle_block] + list(net.output_blocks):
        blk.register_forward_hook(lambda m, i, o: A._STREAM_MAX.__setitem__(0, max(A._STREAM_MAX[0], float(o.detach().abs().max()))))
    return model.eval()


def shim(model, pad=True):
    """The two instance-level shims of ancestral_cfg.py; each is applied only after the unshimmed reference has been SEEN to fail."""
    x = torch.zeros(SHAPE)
    t = torch.zeros(SHAPE[0], dtype=torch.long)
    c = getattr(model, "_probe_cond", None)
    try:
        model.p_mean_variance(x, c, t, 0, clip_denoised=False)
        raise SystemExit("the reference's p_mean_variance runs unshimmed: the fixtures' premise changed, regenerate without shim()")
    except AttributeError as e:
        print(f"  reference, unshimmed: AttributeError: {e}")
    model.model.use_split_head = model.use_split_head
    if not pad:
        return model
    try:
        model.p_mean_variance(x, c, t, 0, clip_denoised=False)
        raise SystemExit("stage 0 of the reference's p_mean_variance runs on the full latent: regenerate without the padding shim")
    except RuntimeError as e:
        print(f"  reference, flag set, stage 0 on the full latent: RuntimeError: {e}")
    orig, embed = model.apply_model, list(model.embed_dim_list)

    def padded(x_noisy, t, cond, stage=None, return_ids=False):
        out = orig(x_noisy, t, cond, stage=stage, return_ids=return_ids)
        n = x_noisy.shape[1] - sum(embed[:stage + 1])
        return torch.cat((out, out.new_zeros(out.shape[0], n, *out.shape[2:])), dim=1) if n > 0 else out
    model.apply_model = padded
    return model


def gen_tables():
    fr = A.H.import_ref("frido.models.diffusion.frido")

    class Host(nn.Module):
        parameterization = "eps"
    out = {}
    for tag, (sched, T, v) in TABLES.items():
        h = Host()
        h.v_posterior = v
        fr.DDPM.register_schedule(h, beta_schedule=sched, timesteps=T, **LINEAR)
        for k in POSTERIOR_KEYS + ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"):
            out[f"{tag}_{k}"] = getattr(h, k).numpy()
    A.save("anc_tables", **out)


def with_sens(out, model, name, go, decode=True):
    """go() -> (samples, intermediates list or None); records the run, its decode and the reference's own movement under a perturbed eps."""
    samples, inter = go()
    gen = torch.Generator().manual_seed(99)
    hook = model.model.diffusion_model.register_forward_hook(
        lambda m, i, o: o * (1 + REF_SENS_PERT * torch.empty_like(o).normal_(generator=gen)))
    pert = go()[0]
    hook.remove()
    sens = float((pert - samples).abs().max() / samples.abs().max())
    print(f"  {name}: max |z| {float(samples.abs().max()):.4g}; under a {REF_SENS_PERT:g} eps perturbation the reference moves by {sens:.3g}")
    out[f"{name}_ref_sens"] = np.float64(sens)
    out[f"{name}_samples"] = samples.numpy()
    if inter is not None:
        out[f"{name}_n_inter"] = np.int64(len(inter))
        for tag, idx in (("first", 0), ("mid", len(inter) // 2), ("last", len(inter) - 1)):
            out[f"{name}_inter_{tag}"] = inter[idx].numpy()
    if decode:
        with torch.no_grad():
            out[f"{name}_img"] = model.decode_first_stage(samples).numpy()
    return sens


def seeded(fn):
    def go():
        torch.manual_seed(SEED)
        with torch.no_grad():
            r = fn()
        return r if isinstance(r, tuple) else (r, None)
    return go


def gen_uncond():
    A._STREAM_MAX[0] = 0.0
    model = shim(build_frido(AB_SMP, VQ_SMALL, None))
    assert model.clip_denoised is False and model.num_resulotion == 2
    out = {}
    sens = []
    sens.append(with_sens(out, model, "loop", seeded(lambda: model.p_sample_loop(
        None, SHAPE, timesteps=12, return_intermediates=True, log_every_t=5, verbose=False))))
    model.clip_denoised = True
    sens.append(with_sens(out, model, "loop_clip", seeded(lambda: model.p_sample_loop(
        None, SHAPE, timesteps=12, return_intermediates=True, log_every_t=5, verbose=False))))
    model.clip_denoised = False
    sens.append(with_sens(out, model, "prog", seeded(lambda: model.progressive_denoising(
        None, SHAPE[1:], batch_size=B, start_T=12, temperature=0.8, verbose=False))))
    sens.append(with_sens(out, model, "drop", seeded(lambda: model.progressive_denoising(
        None, SHAPE[1:], batch_size=B, start_T=12, noise_dropout=0.25, verbose=False))))
    # one p_sample at t = [500, 0] (per-sample timesteps; sample 1 gets no noise), both stages, on the full latent
    x = A.T(seeded_normal("anc:step_x", SHAPE))
    out["step_x"], out["step_t"] = x.numpy(), np.array([500, 0], dtype=np.int64)
    for s in (0, 1):
        for clip in (False, True):
            name = f"step_s{s}" + ("_clip" if clip else "")
            sens.append(with_sens(out, model, name, seeded(lambda s=s, clip=clip: tuple(
                (r[0], [r[1]]) for r in [model.p_sample(x.clone(), None, torch.tensor([500, 0]), s, clip_denoised=clip, return_x0=True)])[0]),
                decode=False))
    # p_mean_variance's own outputs at stage 1
    with torch.no_grad():
        mean, var, logvar, x0 = model.p_mean_variance(x.clone(), None, torch.tensor([500, 0]), 1, clip_denoised=False, return_x0=True)
    out["pmv_mean"], out["pmv_var"], out["pmv_logvar"], out["pmv_x0"] = mean.numpy(), var.numpy(), logvar.numpy(), x0.numpy()
    # predict_start_from_noise / q_posterior as plain functions (no shim involved)
    e = A.T(seeded_normal("anc:step_e", SHAPE))
    with torch.no_grad():
        out["psfn"] = model.predict_start_from_noise(x, torch.tensor([500, 0]), e).numpy()
        out["psfn_ch"] = model.predict_start_from_noise(x, torch.tensor([500, 0]), e, ch_start=3, ch_end=6).numpy()
        qm, qv, ql = model.q_posterior(e, x, torch.tensor([999, 1]), ch_start=0, ch_end=3)
    out["step_e"], out["qp_mean"], out["qp_var"], out["qp_logvar"] = e.numpy(), qm.numpy(), qv.numpy(), ql.numpy()
    out["stream_absmax"] = np.float64(A._STREAM_MAX[0])
    # the full chain: sample(None, batch_size=2) on a model built with timesteps = T, the longest candidate that is well conditioned
    for T in FULL_T_CANDIDATES:
        full = {}
        m2 = shim(build_frido(AB_SMP, VQ_SMALL, None, timesteps=T))
        assert m2.num_timesteps == T
        s_full = with_sens(full, m2, "full", seeded(lambda: m2.sample(None, batch_size=B, return_intermediates=True, verbose=False)))
        if s_full < REF_SENS_MAX:
            out.update(full)
            out["full_T"] = np.int64(T)
            sens.append(s_full)
            break
        print(f"  full chain T = {T}: ill conditioned ({s_full:.3g}), trying a shorter one")
    else:
        raise SystemExit("no full chain is well conditioned")
    assert max(sens) < REF_SENS_MAX, sens
    out["stream_absmax"] = np.float64(max(float(out["stream_absmax"]), A._STREAM_MAX[0]))
    A.save("anc_uncond", **out)


def gen_cond():
    A._STREAM_MAX[0] = 0.0
    out = {}
    c = A.T(np.load(os.path.join(HERE, "sampler_small.npz"))["c"])
    model = build_frido(UNET_SMALL, VQ_SMALL, "crossattn")
    model._probe_cond = c
    shim(model)
    out["c"] = c.numpy()
    sens = [with_sens(out, model, "ctx_sample", seeded(lambda: model.sample(
        cond=c, batch_size=B, timesteps=10, return_intermediates=True, verbose=False)))]
    sens.append(with_sens(out, model, "ctx_sample_log", seeded(lambda: model.sample_log(
        c, B, ddim=False, ddim_steps=None, timesteps=10, verbose=False))))
    model = build_frido(AB_SMP_EMB, VQ_SMALL, "adm")
    y = A.labels_for(AB_SMP_EMB, "anc_adm_emb", B)
    model._probe_cond = y
    shim(model)
    out["emb_y"] = y.numpy()
    sens.append(with_sens(out, model, "emb_sample", seeded(lambda: model.sample(
        cond=y, batch_size=B, timesteps=10, return_intermediates=True, verbose=False))))
    assert max(sens) < REF_SENS_MAX, sens
    out["stream_absmax"] = np.float64(A._STREAM_MAX[0])
    A.save("anc_cond", **out)


def check_signatures():
    fr = A.H.import_ref("frido.models.diffusion.frido")
    for name, want in SIGNATURES.items():
        got = [p for p in inspect.signature(getattr(fr.FridoDiffusion, name)).parameters if p not in ("self", "kwargs")]
        assert got == want, (name, got, want)
    print("  ancestral_cfg.SIGNATURES equal the reference's")


GENS = {"anc_tables": gen_tables, "anc_uncond": gen_uncond, "anc_cond": gen_cond}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    check_signatures()
    for name in (sys.argv[1:] or list(GENS)):
        print(f"[{name}]")
        GENS[name]()

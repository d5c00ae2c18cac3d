#!/usr/bin/env python3
"""Generate the AttentionBlock-denoiser fixtures (tests/golden/ab_*.npz) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixtures it writes are data (inputs + expected outputs) and are committed.
Weights are never stored: both sides regenerate them with frido_amd.synth.fill_tensor keyed by state_dict name.

    python tests/golden/make_golden_attnblock.py [names...]

Reference entry points exercised:
  frido/modules/diffusionmodules/pyunet.py:303-358,381-440   AttentionBlock, QKVAttentionLegacy / QKVAttention
  frido/modules/diffusionmodules/pyunet.py:867-950           PyUNetModel.forward (no context; class labels)
  frido/models/diffusion/ddim.py:56-273, plms.py:57-303      DDIM / PLMS sampling loops (conditioning None / labels)
  frido/models/diffusion/frido.py:823-891                    decode_first_stage
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from frido_amd.synth import fill_tensor, seeded_normal  # noqa: E402
from frido_amd.configs import frido_cfg  # noqa: E402
sys.path.remove(REPO)
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("_ref_harness", os.path.join(REPO, "oracle", "_ref_harness.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

sys.path.insert(0, HERE)
from golden_cfg import VQ_SMALL  # noqa: E402
from attnblock_cfg import FORWARD, AB_SMP, AB_SMP_EMB, AB_SMP_LIN, AB_FULL  # noqa: E402


def fill_module(mod, prefix=""):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(prefix + name, p.shape)))
    return mod


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def labels_for(cfg, tag, B):
    """Class labels in the form the model's label_emb takes: int64 [B] (nn.Embedding) or float [B, num_classes] (nn.Linear)."""
    n = cfg["num_classes"]
    if cfg["use_embed"]:
        return torch.from_numpy(np.random.default_rng(11).integers(0, n, (B,)))
    return T(seeded_normal(f"{tag}:y", (B, n)))


def attention_sites(net):
    """(heads, new order?) of every AttentionBlock in forward order, read off the reference's modules."""
    heads, order = [], []
    for blk in list(net.input_blocks) + [net.middle_block] + list(net.output_blocks):
        for m in blk:
            if type(m).__name__ == "AttentionBlock":
                heads.append(m.num_heads)
                order.append(type(m.attention).__name__ == "QKVAttention")
    return np.array(heads, dtype=np.int64), np.array(order)


def gen_unet(tag, cfg, B=2, hw=None, store_x=True):
    m = H.import_ref("frido.modules.diffusionmodules.pyunet")
    net = fill_module(m.PyUNetModel(**cfg), "model.diffusion_model.").eval()
    hw = hw or cfg["image_size"]
    x = T(seeded_normal(f"{tag}:x", (B, cfg["in_channels"], hw, hw)))
    out = {"x": x.numpy()} if store_x else {}
    y = labels_for(cfg, tag, B) if cfg.get("num_classes") else None
    if y is not None:
        out["y"] = y.numpy()
    splits = cfg["split_embed_dim_list"]
    for s in range(cfg.get("num_stage", 1)):
        t = torch.tensor([996 - 37 * i for i in range(B)], dtype=torch.long)
        smax, hooks = [0.0], []
        for blk in list(net.input_blocks) + [net.middle_block] + list(net.output_blocks):
            hooks.append(blk.register_forward_hook(lambda mod, i, o, smax=smax: smax.__setitem__(0, max(smax[0], float(o.detach().abs().max())))))
        with torch.no_grad():
            e = net(x[:, :sum(splits[:s + 1])].contiguous(), t, y=y, stage=s)
        for h in hooks:
            h.remove()
        out[f"stream_absmax_{s}"] = np.float64(smax[0])
        print(f"  {tag} stage {s}: residual stream max |x| = {smax[0]:.4g}, eps max {float(e.abs().max()):.4g}")
        out[f"t_{s}"], out[f"eps_{s}"] = t.numpy(), e.numpy()
    out["nparam"] = np.int64(sum(p.numel() for p in net.parameters()))
    out["keys"] = np.array(sorted(k for k, _ in net.named_parameters()))
    out["heads"], out["new_order"] = attention_sites(net)
    save(tag, **out)


class NoiseTape:
    """Records every torch.randn draw."""

    def __init__(self):
        self.draws = []
        self._orig = torch.randn

    def __enter__(self):
        def rec(*a, **k):
            r = self._orig(*a, **k)
            self.draws.append(r.detach().numpy().copy())
            return r
        torch.randn = rec
        return self

    def __exit__(self, *a):
        torch.randn = self._orig


_STREAM_MAX = [0.0]


def build_frido(ucfg, vcfg, key):
    fr = H.import_ref("frido.models.diffusion.frido")
    H.patch_samplers()
    cfg = frido_cfg(ucfg, vcfg, dict())
    cfg["first_stage_config"]["params"]["lossconfig"] = {"target": "torch.nn.Identity"}
    cfg["cond_stage_config"] = "__is_unconditional__"       # labels are fed directly; needs cond_stage_trainable=False
    cfg["cond_stage_trainable"] = False
    cfg["conditioning_key"] = key
    model = fr.FridoDiffusion(**cfg)
    model.model.conditioning_key = key      # ('__is_unconditional__' resets the wrapper's key to None: frido.py, DDPM.__init__)
    fill_module(model.model, "model.")
    fill_module(model.first_stage_model, "first_stage_model.")
    model.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    net = model.model.diffusion_model
    for blk in list(net.input_blocks) + [net.middle_block] + list(net.output_blocks):
        blk.register_forward_hook(lambda m, i, o: _STREAM_MAX.__setitem__(0, max(_STREAM_MAX[0], float(o.detach().abs().max()))))
    return model.eval()


REF_SENS_MAX = 1e-4      # a fixture is kept only if the reference's own result moves by less than this (10x under the samplers' bound) ...
REF_SENS_PERT = 1e-6     # ... when every eps of the run is perturbed by this much (relative, seeded normal): fp32-class forward error


def run_sampler(out, model, name, sampler_cls, S, eta, scale, c, uc, ucfg, B, log_every_t=2):
    hw, C = ucfg["image_size"], ucfg["in_channels"]

    def go():
        torch.manual_seed(23)
        smp = sampler_cls(model)
        with NoiseTape() as tape, torch.no_grad():
            samples, inter = smp.sample(S=S, batch_size=B, shape=(C, hw, hw), conditioning=c, num_stage=ucfg["num_stage"], eta=eta,
                                        verbose=False, log_every_t=log_every_t, unconditional_guidance_scale=scale,
                                        unconditional_conditioning=uc if scale != 1.0 else None)
        return samples, inter, tape
    samples, inter, tape = go()
    with torch.no_grad():
        img = model.decode_first_stage(samples)
    # conditioning of the fixture: the reference's own run with every eps perturbed by REF_SENS_PERT
    gen = torch.Generator().manual_seed(99)
    hook = model.model.diffusion_model.register_forward_hook(
        lambda m, i, o: o * (1 + REF_SENS_PERT * torch.empty_like(o).normal_(generator=gen)))
    pert = go()[0]
    hook.remove()
    sens = float((pert - samples).abs().max() / samples.abs().max())
    print(f"  {name}: reference run under a {REF_SENS_PERT:g} eps perturbation moves by {sens:.3g} of max |z| = {float(samples.abs().max()):.4g}")
    assert sens < REF_SENS_MAX, f"{name}: ill-conditioned fixture (the reference itself moves by {sens:.3g})"
    out[f"{name}_ref_sens"] = np.float64(sens)
    out[f"{name}_samples"] = samples.numpy()
    out[f"{name}_img"] = img.numpy()
    out[f"{name}_noise_sum"] = np.float64(sum(float(d.astype(np.float64).sum()) for d in tape.draws))
    out[f"{name}_nx"] = np.int64(len(inter["x_inter"]))
    out[f"{name}_x_inter_last"] = inter["x_inter"][-1].numpy()
    out[f"{name}_pred_x0_1"] = inter["pred_x0"][1].numpy()
    out[f"{name}_args"] = np.array([S, eta, scale, log_every_t], dtype=np.float64)


def gen_sampler_uncond():
    DDIM, PLMS = H.patch_samplers()
    _STREAM_MAX[0] = 0.0
    model = build_frido(AB_SMP, VQ_SMALL, None)
    out = {}
    run_sampler(out, model, "ddim_eta1", DDIM, 4, 1.0, 1.0, None, None, AB_SMP, 2)
    run_sampler(out, model, "plms", PLMS, 6, 0.0, 1.0, None, None, AB_SMP, 2)
    out["stream_absmax"] = np.float64(_STREAM_MAX[0])
    print(f"  ab_sampler_uncond: residual stream max |x| = {_STREAM_MAX[0]:.4g}")
    save("ab_sampler_uncond", **out)


def gen_sampler_adm():
    DDIM, PLMS = H.patch_samplers()
    _STREAM_MAX[0] = 0.0
    out = {}
    B = 2
    model = build_frido(AB_SMP_EMB, VQ_SMALL, "adm")
    y = labels_for(AB_SMP_EMB, "ab_adm_emb", B)
    uy = torch.full_like(y, AB_SMP_EMB["num_classes"] - 1)       # a "null class" index as unconditional labels
    out["emb_y"], out["emb_uy"] = y.numpy(), uy.numpy()
    run_sampler(out, model, "emb_ddim_eta0_cfg", DDIM, 5, 0.0, 1.5, y, uy, AB_SMP_EMB, B)
    run_sampler(out, model, "emb_plms_cfg", PLMS, 5, 0.0, 1.5, y, uy, AB_SMP_EMB, B, log_every_t=3)
    model = build_frido(AB_SMP_LIN, VQ_SMALL, "adm")
    y = labels_for(AB_SMP_LIN, "ab_adm_lin", B)
    out["lin_y"] = y.numpy()
    run_sampler(out, model, "lin_ddim_eta1", DDIM, 4, 1.0, 1.0, y, None, AB_SMP_LIN, B)
    out["stream_absmax"] = np.float64(_STREAM_MAX[0])
    print(f"  ab_sampler_adm: residual stream max |x| = {_STREAM_MAX[0]:.4g}")
    save("ab_sampler_adm", **out)


GENS = {**{tag: (lambda tag=tag, cfg=cfg: gen_unet(tag, cfg)) for tag, cfg in FORWARD.items()},
        # full width at B = 2, 64 x 64: x is regenerated by the test from its seed tag (not stored), eps only
        "ab_full": lambda: gen_unet("ab_full", AB_FULL, B=2, store_x=False),
        "ab_sampler_uncond": gen_sampler_uncond, "ab_sampler_adm": gen_sampler_adm}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    for name in (sys.argv[1:] or list(GENS)):
        print(f"[{name}]")
        GENS[name]()

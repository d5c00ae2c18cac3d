#!/usr/bin/env python3
"""Generate the patch-wise fixtures (tests/golden/patch_*.npz) by IMPORTING THE REFERENCE on CPU and setting `split_input_params`.

Runs only where the reference checkout exists; the fixtures it writes are data (inputs + expected outputs) and are committed.
Weights are never stored: both sides regenerate them with frido_amd.synth.fill_tensor keyed by state_dict name.

    python tests/golden/make_golden_patch.py [names...]

Reference entry points exercised (frido/models/diffusion/frido.py):
  :677-764    meshgrid / delta_border / get_weighting / get_fold_unfold   (the `weighting` and `normalization` tensors)
  :1062-1160  apply_model with split_input_params                         (both stages, tie_braker both ways, a rectangular latent)
  :823-891    decode_first_stage, :962-1005 encode_first_stage            (patch_distributed_vq)
  ddim.py:56-273, plms.py:57-303                                          (the samplers inherit the mode through apply_model)
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
from patch_cfg import (MODELS, VQ_SMALL, COND_SHAPE, COND_STAGE_KEY, SPLIT, SPLIT_TIE, SPLIT_RECT, RECT_HW, SPLIT_ENC, RUNS)  # noqa: E402

REF_SENS_MAX = 1e-4      # a sampler fixture is kept only if the reference's own result moves by less than this ...
REF_SENS_PERT = 1e-6     # ... when every eps of the run is perturbed by this much (relative, seeded normal)


def fill_module(mod, prefix=""):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(prefix + name, p.shape)))
    return mod


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrs.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")
    assert os.path.getsize(path) < 1 << 20


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build_frido(ucfg, scale_factor=(0.9, 1.1)):
    fr = H.import_ref("frido.models.diffusion.frido")
    H.patch_samplers()
    cfg = frido_cfg(ucfg, VQ_SMALL, dict())
    cfg["first_stage_config"]["params"]["lossconfig"] = {"target": "torch.nn.Identity"}
    cfg["cond_stage_config"] = {"target": "torch.nn.Identity"}      # the conditioning tensor is fed directly
    cfg["cond_stage_trainable"] = False
    cfg["cond_stage_key"] = COND_STAGE_KEY
    model = fr.FridoDiffusion(**cfg)
    fill_module(model.model, "model.")
    fill_module(model.first_stage_model, "first_stage_model.")
    model.scale_factor.copy_(torch.tensor(scale_factor))
    return model.eval()


def tables(model, split, hw, **kw):
    """The reference's own `weighting` ([kh * kw][L]) and `normalization` ([H][W]) for a tensor of spatial size hw."""
    model.split_input_params = dict(split)
    ks, stride = split["ks"], split["stride"]
    _, _, normalization, weighting = model.get_fold_unfold(torch.zeros(1, 1, *hw), ks, stride, **kw)
    L = weighting.shape[-1]
    return weighting.reshape(-1, L).numpy(), normalization.reshape(normalization.shape[-2:]).numpy()


def gen_apply():
    out = {}
    c = T(seeded_normal("patch:c", COND_SHAPE))
    x = T(seeded_normal("patch:x", (2, 6, 16, 16)))
    xr = T(seeded_normal("patch:xr", (2, 6) + RECT_HW))
    t = torch.tensor([996, 959], dtype=torch.long)
    out.update(c=c.numpy(), x=x.numpy(), xr=xr.numpy(), t=t.numpy())
    for mname, ucfg in MODELS.items():
        model = build_frido(ucfg)
        for tname, split in (("notie", SPLIT), ("tie", SPLIT_TIE)):
            model.split_input_params = dict(split)
            for s in range(2):
                with torch.no_grad():
                    e = model.apply_model(x[:, :3 * (s + 1)].contiguous(), t, c, stage=s)
                out[f"{mname}_{tname}_eps_{s}"] = e.numpy()
            if mname == "spade":
                out[f"{tname}_weighting"], out[f"{tname}_normalization"] = tables(model, split, (16, 16))
        del model.split_input_params
        with torch.no_grad():
            whole = model.apply_model(x, t, c, stage=1)
        d = float((whole - T(out[f"{mname}_notie_eps_1"])).abs().max())
        print(f"  {mname}: patch-wise eps differs from the whole-latent eps by {d:.3g}")
        out[f"{mname}_whole_minus_patch"] = np.float64(d)
        if mname == "spade":
            model.split_input_params = dict(SPLIT_RECT)
            for s in range(2):
                with torch.no_grad():
                    e = model.apply_model(xr[:, :3 * (s + 1)].contiguous(), t, c, stage=s)
                out[f"rect_eps_{s}"] = e.numpy()
            out["rect_weighting"], out["rect_normalization"] = tables(model, SPLIT_RECT, RECT_HW)
    save("patch_apply", **out)


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


def gen_sampler():
    DDIM, PLMS = H.patch_samplers()
    c = T(seeded_normal("patch:c", COND_SHAPE))
    uc = torch.zeros_like(c)
    out = {"c": c.numpy()}
    models = {}
    for name, (mname, kind, S, eta, scale, split) in RUNS.items():
        if mname not in models:
            models[mname] = build_frido(MODELS[mname])
        model = models[mname]
        model.split_input_params = dict(split)
        cls = PLMS if kind == "plms" else DDIM

        def go():
            torch.manual_seed(23)
            with NoiseTape() as tape, torch.no_grad():
                samples, inter = cls(model).sample(S=S, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=eta, verbose=False,
                                                   log_every_t=2, unconditional_guidance_scale=scale,
                                                   unconditional_conditioning=uc if scale != 1.0 else None)
            return samples, inter, tape
        samples, inter, tape = go()
        gen = torch.Generator().manual_seed(99)
        hook = model.model.diffusion_model.register_forward_hook(
            lambda m, i, o: o * (1 + REF_SENS_PERT * torch.empty_like(o).normal_(generator=gen)))
        pert = go()[0]
        hook.remove()
        sens = float((pert - samples).abs().max() / samples.abs().max())
        print(f"  {name}: reference run under a {REF_SENS_PERT:g} eps perturbation moves by {sens:.3g} of max |z| = {float(samples.abs().max()):.4g}")
        assert sens < REF_SENS_MAX, f"{name}: ill-conditioned fixture (the reference itself moves by {sens:.3g})"
        del model.split_input_params
        torch.manual_seed(23)
        with torch.no_grad():
            whole, _ = cls(model).sample(S=S, batch_size=2, shape=(6, 16, 16), conditioning=c, num_stage=2, eta=eta, verbose=False,
                                         log_every_t=2, unconditional_guidance_scale=scale,
                                         unconditional_conditioning=uc if scale != 1.0 else None)
        out[f"{name}_whole_minus_patch"] = np.float64(float((whole - samples).abs().max() / samples.abs().max()))
        print(f"  {name}: the whole-latent run differs by {float(out[f'{name}_whole_minus_patch']):.3g} (relative)")
        out[f"{name}_ref_sens"] = np.float64(sens)
        out[f"{name}_samples"] = samples.numpy()
        out[f"{name}_noise_sum"] = np.float64(sum(float(d.astype(np.float64).sum()) for d in tape.draws))
        out[f"{name}_nx"] = np.int64(len(inter["x_inter"]))
        out[f"{name}_x_inter_last"] = inter["x_inter"][-1].numpy()
        out[f"{name}_pred_x0_1"] = inter["pred_x0"][1].numpy()
        out[f"{name}_args"] = np.array([S, eta, scale, 2], dtype=np.float64)
    save("patch_sampler", **out)


def gen_vq():
    """Patch-wise decode of vq_small.npz's own latent `h` and encode of its `img` (scale_factor 1: the fixture's codes stay the ones the
    whole decode is pinned with)."""
    g = np.load(os.path.join(HERE, "vq_small.npz"))
    model = build_frido(MODELS["spade"], scale_factor=(1.0, 1.0))
    h, img = T(g["h"]), T(g["img"])
    out = {}
    model.split_input_params = dict(SPLIT)
    with torch.no_grad():
        dec = model.decode_first_stage(h)
    out["dec"] = dec.numpy()
    out["dec_weighting"], out["dec_normalization"] = tables(model, SPLIT, tuple(h.shape[2:]), uf=SPLIT["vqf"])
    print(f"  patch decode differs from the whole decode by {float((dec - T(g['dec'])).abs().max()):.3g}")
    model.split_input_params = dict(SPLIT_ENC)
    with torch.no_grad():
        enc = model.encode_first_stage(img)
    out["enc"] = enc.numpy()
    assert tuple(model.split_input_params["original_image_size"]) == tuple(img.shape[2:])      # frido.py:968
    out["enc_weighting"], out["enc_normalization"] = tables(model, SPLIT_ENC, tuple(img.shape[2:]), df=SPLIT_ENC["vqf"])
    print(f"  patch encode differs from the whole encode by {float((enc - T(g['enc'])).abs().max()):.3g}")
    save("patch_vq", **out)


GENS = {"patch_apply": gen_apply, "patch_sampler": gen_sampler, "patch_vq": gen_vq}

if __name__ == "__main__":
    torch.set_grad_enabled(False)
    for name in (sys.argv[1:] or list(GENS)):
        print(f"[{name}]")
        GENS[name]()

#!/usr/bin/env python3
"""Generate the editing fixture (tests/golden/edit_ref.npz) by IMPORTING THE REFERENCE on CPU.

Runs only where the reference checkout exists; the fixture it writes is data (inputs + recorded noise + expected outputs) and is committed.
Weights are never stored: both sides regenerate them with frido_amd.synth.fill_tensor keyed by state_dict name.

    python tests/golden/make_golden_edit.py

Reference entry point exercised: frido/models/diffusion/ddim.py:56-186 DDIMSampler.sample(mask=, x0=, x_T=) on the two-stage UNET_SMALL
model -- the blend of :158-161 with FridoDiffusion.q_sample (frido.py:302-307).  x_T is given, so stage 0 is adopted and stage 1 runs with
x0's 6 channels: the one place the shipped lines execute.  Every torch.randn AND torch.randn_like draw is recorded in call order
(q_sample draws with randn_like, the update with randn).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from frido_amd.synth import fill_tensor, seeded_normal  # noqa: E402
sys.path.remove(REPO)
import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("_ref_harness", os.path.join(REPO, "oracle", "_ref_harness.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

sys.path.insert(0, HERE)
from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg  # noqa: E402
from edit_cfg import B, SHAPE, S, NUM_STAGE, RUNS  # noqa: E402

REF_SENS_MAX = 1e-4      # kept only if the reference's own result moves by less than this (10x under the samplers' 1e-3 bound) ...
REF_SENS_PERT = 1e-6     # ... when every eps of the run is perturbed by this much (relative, seeded normal)


def fill_module(mod, prefix=""):
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(torch.from_numpy(fill_tensor(prefix + name, p.shape)))
    return mod


class NoiseTape:
    """Records every torch.randn and torch.randn_like draw, in call order."""

    def __init__(self):
        self.draws = []
        self._randn, self._like = torch.randn, torch.randn_like

    def __enter__(self):
        def rec(orig):
            def f(*a, **k):
                r = orig(*a, **k)
                self.draws.append(r.detach().numpy().copy())
                return r
            return f
        torch.randn, torch.randn_like = rec(self._randn), rec(self._like)
        return self

    def __exit__(self, *a):
        torch.randn, torch.randn_like = self._randn, self._like


def build_frido():
    fr = H.import_ref("frido.models.diffusion.frido")
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    cfg["first_stage_config"]["params"]["lossconfig"] = {"target": "torch.nn.Identity"}
    cfg["cond_stage_config"]["params"]["device"] = "cpu"
    model = fr.FridoDiffusion(**cfg)
    fill_module(model.model, "model.")
    fill_module(model.first_stage_model, "first_stage_model.")
    fill_module(model.cond_stage_model, "cond_stage_model.")
    model.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    return model.eval()


def masks():
    """(B, 1, H, W): a binary mask that keeps the left half and one block on the right; a soft one with a linear ramp across the columns."""
    H_, W_ = SHAPE[1:]
    binary = torch.zeros(B, 1, H_, W_)
    binary[:, :, :, :W_ // 2] = 1.0
    binary[1, :, 4:8, 10:14] = 1.0
    soft = torch.linspace(0.0, 1.0, W_).reshape(1, 1, 1, W_).expand(B, 1, H_, W_).clone()
    soft[1] = soft[1].flip(-1) * 0.75
    return {"binary": binary, "soft": soft}


def main():
    DDIM, _ = H.patch_samplers()
    model = build_frido()
    c = torch.from_numpy(np.load(os.path.join(HERE, "sampler_small.npz"))["c"])
    x0 = torch.from_numpy(seeded_normal("edit:x0", (B,) + SHAPE))
    x_T = torch.from_numpy(seeded_normal("edit:xT", (B,) + SHAPE))
    m = masks()
    out = {"x0": x0.numpy(), "x_T": x_T.numpy(), **{f"mask_{k}": v.numpy() for k, v in m.items()}}
    for name, (eta, kind) in RUNS.items():
        def go():
            torch.manual_seed(23)
            with NoiseTape() as tape, torch.no_grad():
                samples, inter = DDIM(model).sample(S=S, batch_size=B, shape=SHAPE, conditioning=c, num_stage=NUM_STAGE, eta=eta, verbose=False,
                                                    log_every_t=2, mask=m[kind], x0=x0, x_T=x_T)
            return samples, inter, tape
        samples, inter, tape = go()
        assert len(tape.draws) == 2 * S and all(d.shape == (B,) + SHAPE for d in tape.draws), [d.shape for d in tape.draws]
        gen = torch.Generator().manual_seed(99)
        hook = model.model.diffusion_model.register_forward_hook(
            lambda mod, i, o: o * (1 + REF_SENS_PERT * torch.empty_like(o).normal_(generator=gen)))
        pert = go()[0]
        hook.remove()
        sens = float((pert - samples).abs().max() / samples.abs().max())
        print(f"  {name}: reference run under a {REF_SENS_PERT:g} eps perturbation moves by {sens:.3g} of max |z| = {float(samples.abs().max()):.4g}")
        assert sens < REF_SENS_MAX, f"{name}: ill-conditioned fixture (the reference itself moves by {sens:.3g})"
        out[f"{name}_ref_sens"] = np.float64(sens)
        out[f"{name}_samples"] = samples.numpy()
        out[f"{name}_noise"] = np.concatenate([d.reshape(-1) for d in tape.draws])
        out[f"{name}_nx"] = np.int64(len(inter["x_inter"]))
    path = os.path.join(HERE, "edit_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    main()

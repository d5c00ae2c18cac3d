"""Records the exact bits of every path through runtime.SamplerEngine on an MI355X, from whichever checkout --repo names, into an .npz --
the fixture of tests/test_engine_bits_gpu.py::test_engine_bits_are_those_of_the_engine_before_the_refactor.

    python tests/golden/record_engine_bits.py --repo <built checkout of the commit to pin> --out tests/golden/sampler_engine_bits.npz

tests/golden/sampler_engine_bits.npz was recorded this way from a built checkout of ac11453, the last commit before SamplerEngine got one
step-body builder and one replay loop.  record_sampler_bits.py pins Philox DDIM / PLMS without K-step units; this one walks the engine's
other branches.  The small two-stage SpatialTransformer model of record_sampler_bits.build_model() (the class-conditional run: the
AttentionBlock denoiser AB_SMP_EMB with conditioning_key 'adm'), B = 2, latent 6 x 16 x 16, S = 10 steps logged every 5, GRAPH_STEPS = 4
(FRIDO_GRAPH_STEPS here, runtime.GRAPH_STEPS in the test), so every stage replays the units [1, 4, 4, 1]:
  ddim   ddim_tape (eta 1, host noise from a tape), ddim_philox_cfg (guidance 2.0), ddim_dropout (noise_dropout 0.3 on ddim_tape's tape),
         ddim_xT (x_T given: stage 0 skipped), ddim_callbacks (single steps; what img_callback received), ddim_corrector_cfg (the eager loop)
  plms   plms_tape_cfg, plms_corrector
  dpm    dpm2_logsnr_cfg (order 2), dpm1_uniform (order 1, time_uniform)
  ddpm   anc_loop_tape (p_sample_loop), anc_prog_philox (progressive_denoising), anc_temps_dropout (a per-timestep temperature list and
         noise_dropout), anc_corrector -- the last two through progressive_denoising: p_sample_loop, like the reference's, takes neither
  patch  patch_ddim (ddim_tape's tape, patch_cfg.SPLIT), patch_plms
  labels labels_ddim_cfg (class labels, guidance 1.5)
Host noise is a tape over synth.seeded_normal; torch.manual_seed only where a dropout mask is drawn.  The score corrector returns
e_t - 0.1 * x.  Every GEMM runs on the library's static tile (FRIDO_TUNE = 0 here, tune.ENABLED = False in the test).

Per run the file holds the final latent in full ("<run>") and, as "<run>.<what><k>", the SHA-256 of the bytes of every logged intermediate
and of every tensor a callback received (32 uint8 each: ~150 float arrays of 6 - 12 KB would be 1.6 MB, and a committed file stays under
1 MiB); the recorder checks that every array is finite before it hashes it.  `runs(group)` is shared with the test: only names that exist on
both sides of the change.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

SEED, B, SHAPE, S, LOG = 11, 2, (6, 16, 16), 10, 5
GROUPS = ("ddim", "plms", "dpm", "ddpm", "patch", "labels")
# runs that differ in one option must differ in bits
DIFFERENT = (("ddim_tape", "ddim_dropout"), ("ddim_tape", "ddim_xT"), ("ddim_tape", "patch_ddim"), ("plms_tape_cfg", "plms_corrector"),
             ("dpm2_logsnr_cfg", "dpm1_uniform"), ("anc_loop_tape", "anc_temps_dropout"), ("anc_prog_philox", "anc_corrector"))
_MODELS = {}


class Tape:
    """shape -> the next values of a seeded normal stream."""

    def __init__(self, tag, n=1 << 17):
        from frido_amd.synth import seeded_normal
        self.buf, self.pos = seeded_normal(f"engine_bits:{tag}", (n,)), 0

    def __call__(self, shape):
        import torch
        n = int(np.prod(shape))
        assert self.pos + n <= self.buf.size
        out = torch.from_numpy(self.buf[self.pos:self.pos + n].reshape(shape).copy())
        self.pos += n
        return out


class Corrector:
    def modify_score(self, model, e_t, x, t, c):
        return e_t - 0.1 * x


def model_of(name):
    """"small": (record_sampler_bits.build_model()'s model, its context); "labels": (the class-conditional AttentionBlock denoiser, labels)."""
    if name not in _MODELS:
        import torch
        if name == "small":
            import record_sampler_bits
            _MODELS[name] = record_sampler_bits.build_model()
        else:
            from attnblock_cfg import AB_SMP_EMB
            from golden_cfg import VQ_SMALL, BERT_SMALL, frido_cfg
            from frido_amd.models import instantiate_from_config
            from frido_amd.synth import fill_module
            cfg = frido_cfg(AB_SMP_EMB, VQ_SMALL, BERT_SMALL)
            cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, "adm"
            m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
            m.model.conditioning_key = "adm"
            fill_module(m.model, "model.")
            fill_module(m.first_stage_model, "first_stage_model.")
            _MODELS[name] = m.cuda().eval(), torch.tensor([1, 7], device="cuda")
    return _MODELS[name]


def _digest(t):
    a = np.ascontiguousarray(t.detach().float().cpu().numpy())
    assert np.isfinite(a).all()
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


def _put(out, run, z, **lists):
    out[run] = z.detach().float().cpu().numpy()
    for what, tensors in lists.items():
        assert len(tensors) > 0, (run, what)
        for k, t in enumerate(tensors):
            out[f"{run}.{what}{k}"] = _digest(t)


def runs(group):
    """{name: array} of one group of GROUPS."""
    import torch
    from frido_amd.samplers import DDIMSampler, PLMSSampler, DPMSolverSampler
    out = {}
    model, c = model_of("labels" if group == "labels" else "small")
    kw = dict(S=S, batch_size=B, shape=SHAPE, conditioning=c, num_stage=2, verbose=False, log_every_t=LOG)
    cfg = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=-c)
    philox = dict(noise="philox", seed=SEED)

    def sampler(run, cls, received=None, **more):
        z, inter = cls(model).sample(**dict(kw, **more))
        assert len(inter["x_inter"]) == len(inter["pred_x0"]) >= 1 + 3      # x_T, then steps 0, 4 and 9 of every stage that ran
        _put(out, run, z, x_inter=inter["x_inter"], pred_x0=inter["pred_x0"], **(received or {}))

    if group == "ddim":
        sampler("ddim_tape", DDIMSampler, eta=1.0, noise=Tape("a"))
        sampler("ddim_philox_cfg", DDIMSampler, eta=1.0, **philox, **cfg)
        torch.manual_seed(SEED)
        sampler("ddim_dropout", DDIMSampler, eta=1.0, noise=Tape("a"), noise_dropout=0.3)
        sampler("ddim_xT", DDIMSampler, eta=1.0, noise=Tape("a"), x_T=Tape("xT")((B,) + SHAPE))
        steps, imgs = [], []
        sampler("ddim_callbacks", DDIMSampler, dict(img_callback=imgs), eta=1.0, noise=Tape("b"), callback=steps.append,
                img_callback=lambda x0, i: imgs.append(x0))
        assert steps == 2 * list(range(S)) and len(imgs) == 2 * S
        sampler("ddim_corrector_cfg", DDIMSampler, eta=1.0, noise=Tape("b"), score_corrector=Corrector(), **cfg)
    elif group == "plms":
        sampler("plms_tape_cfg", PLMSSampler, eta=0.0, noise=Tape("c"), **cfg)
        sampler("plms_corrector", PLMSSampler, eta=0.0, noise=Tape("c"), score_corrector=Corrector(), **cfg)
    elif group == "dpm":
        sampler("dpm2_logsnr_cfg", DPMSolverSampler, order=2, skip_type="logSNR", **philox, **cfg)
        sampler("dpm1_uniform", DPMSolverSampler, order=1, skip_type="time_uniform", **philox, **cfg)
    elif group == "ddpm":
        full = (B,) + SHAPE
        z, inter = model.p_sample_loop(c, full, timesteps=S, return_intermediates=True, log_every_t=LOG, verbose=False, noise=Tape("d"))
        assert len(inter) == 1 + 2 * 3
        _put(out, "anc_loop_tape", z, inter=inter)
        prog = dict(start_T=S, log_every_t=LOG, verbose=False)
        z, inter = model.progressive_denoising(c, full, **prog, **philox)
        _put(out, "anc_prog_philox", z, inter=inter)
        torch.manual_seed(SEED)
        z, inter = model.progressive_denoising(c, full, **prog, noise=Tape("d"), temperature=[0.5 + 0.05 * t for t in range(S)], noise_dropout=0.3)
        _put(out, "anc_temps_dropout", z, inter=inter)
        z, inter = model.progressive_denoising(c, full, **prog, **philox, score_corrector=Corrector())
        _put(out, "anc_corrector", z, inter=inter)
    elif group == "patch":
        from patch_cfg import SPLIT
        model.split_input_params = dict(SPLIT)
        try:
            sampler("patch_ddim", DDIMSampler, eta=1.0, noise=Tape("a"))
            sampler("patch_plms", PLMSSampler, eta=0.0, **philox)
        finally:
            del model.split_input_params
    elif group == "labels":
        sampler("labels_ddim_cfg", DDIMSampler, eta=1.0, **philox, unconditional_guidance_scale=1.5,
                unconditional_conditioning=torch.full_like(c, 9))
    else:
        raise KeyError(group)
    assert all(np.isfinite(v).all() for v in out.values())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repo", required=True, help="built checkout whose frido_amd is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.environ["FRIDO_TUNE"] = "0"
    os.environ["FRIDO_GRAPH_STEPS"] = "4"
    repo = os.path.abspath(a.repo)
    sys.path[:0] = [repo, os.path.join(repo, "tests", "golden")]
    import frido_amd
    from frido_amd import runtime
    assert os.path.dirname(os.path.dirname(os.path.abspath(frido_amd.__file__))) == repo, frido_amd.__file__
    assert runtime.GRAPH_STEPS == 4
    res = {}
    for group in GROUPS:
        res.update(runs(group))
    for a_, b_ in DIFFERENT:
        assert not np.array_equal(res[a_], res[b_]), (a_, b_)
    np.savez_compressed(a.out, **res)
    print({k: (v.shape, float(np.abs(v).max())) for k, v in res.items() if "." not in k})

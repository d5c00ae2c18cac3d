"""Records the exact bits of the paths whose step bodies hold the unfold / fold, q_sample / loss, codebook-loss, DPM, blend, inversion and
guidance launches, on an MI355X, from whichever checkout --repo names, into an .npz -- the fixture of tests/test_opkind_bits_gpu.py.

    python tests/golden/record_opkind_bits.py --repo <built checkout of the commit to pin> --out tests/golden/opkind_bits.npz

tests/golden/opkind_bits.npz was recorded this way, twice with identical results, from a built checkout of 2a5108f, the last commit on which
those nine launches were side launchers next to the executor (ABI 7).  Public API only, so the same file runs on both sides of the change.
record_engine_bits.py already pins the patch-wise DDIM / PLMS loops and DPM-Solver++ under classifier-free guidance (patch_ddim, patch_plms,
dpm2_logsnr_cfg, dpm1_uniform); this one walks the rest.  The small two-stage model of record_sampler_bits.build_model(), B = 2, latent
6 x 16 x 16, GRAPH_STEPS = 4 (FRIDO_GRAPH_STEPS here, runtime.GRAPH_STEPS in the test), static GEMM tiles (FRIDO_TUNE = 0 here,
tune.ENABLED = False in the test):
  edit     edit_philox, edit_tape: DDIMSampler.edit, S = 10, the last 9 rows, a keep mask, init "z0", eta 1 -- the start blend, one plain
           step, then the masked body in the units [4, 4], then the noise-free blend
  invert   invert_cfg: DDIMSampler.invert, 9 of 10 rows ([4, 4, 1]), guidance 2.0
  compose  compose_ddim, compose_dpm: .sample with compose= of two entries at scale 1.5 and guidance_rescale = 0.5, S = 10
  dpm      dpm2_plain: DPMSolverSampler.sample, order 2, time_uniform, no guidance (one evaluation per step)
  loss     loss_philox, loss_tape: FridoDiffusion.forward's total and p_losses' dict and per-sample rows for both stages
  msvq     msvq_plain, msvq_aux: MSFPNVQModel.forward on msvq_small.npz's image, use_aux_loss off and on
Host noise is a tape over synth.seeded_normal.  Final tensors only: per run the main result in full ("<run>") and, as "<run>.<what>", every
other returned tensor -- small ones in full, images as the SHA-256 of their bytes (32 uint8); every array is checked to be finite first.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

SEED, B, SHAPE, S = 11, 2, (6, 16, 16), 10
GROUPS = ("edit", "invert", "compose", "dpm", "loss", "msvq")
# runs that differ in one option must differ in bits
DIFFERENT = (("edit_philox", "edit_tape"), ("compose_ddim", "compose_dpm"), ("compose_dpm", "dpm2_plain"), ("loss_philox", "loss_tape"))
_MODELS = {}


def _small():
    if "small" not in _MODELS:
        import record_sampler_bits
        _MODELS["small"] = record_sampler_bits.build_model()
    return _MODELS["small"]


def _normal(tag, shape):
    import torch
    from frido_amd.synth import seeded_normal
    return torch.from_numpy(seeded_normal(f"opkind_bits:{tag}", tuple(shape)))


class Tape:
    """shape -> the next values of a seeded normal stream."""

    def __init__(self, tag, n=1 << 17):
        self.buf, self.pos = _normal(tag, (n,)).numpy(), 0

    def __call__(self, shape):
        import torch
        n = int(np.prod(shape))
        assert self.pos + n <= self.buf.size
        out = torch.from_numpy(self.buf[self.pos:self.pos + n].reshape(shape).copy())
        self.pos += n
        return out


def _np(t):
    a = np.ascontiguousarray(t.detach().float().cpu().numpy())
    assert np.isfinite(a).all()
    return a


def _digest(t):
    return np.frombuffer(hashlib.sha256(_np(t).tobytes()).digest(), dtype=np.uint8).copy()


def runs(group):
    """{name: array} of one group of GROUPS."""
    import torch
    from frido_amd.samplers import DDIMSampler, DPMSolverSampler
    out = {}
    if group == "msvq":
        from golden_cfg import VQ_SMALL
        from frido_amd.models import MSFPNVQModel
        from frido_amd.synth import fill_module
        img = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "msvq_small.npz"))["img"]).cuda()
        for run, aux in (("msvq_plain", False), ("msvq_aux", True)):
            cfg = dict(VQ_SMALL, lossconfig=dict(target="taming.modules.losses.DummyLoss"), use_aux_loss=aux)
            m = fill_module(MSFPNVQModel(**cfg), "first_stage_model.").cuda().eval()
            res = m(img)
            again = m(img)                    # the captured graph, replayed
            dec, diff = res[0], res[-2]
            assert torch.equal(dec, again[0]) and torch.equal(diff, again[-2])
            out[run], out[f"{run}.dec"] = _np(diff).reshape(-1), _digest(dec)
            if aux:
                out[f"{run}.aux"], out[f"{run}.aux2"] = _digest(res[1][0]), _digest(res[1][1])
        return out
    model, c = _small()
    full = (B,) + SHAPE
    kw = dict(num_stage=2, verbose=False)
    cfg = dict(unconditional_guidance_scale=2.0, unconditional_conditioning=-c)
    philox = dict(noise="philox", seed=SEED)
    if group == "edit":
        z0 = _normal("z0", full).cuda()
        mask = (_normal("mask", (B, 1) + SHAPE[1:]) > 0).float().cuda()
        for run, noise in (("edit_philox", philox), ("edit_tape", dict(noise=Tape("edit")))):
            z, _ = DDIMSampler(model).edit(S, z0, c, t_start=S - 1, keep_mask=mask, init="z0", eta=1.0, **kw, **noise)
            out[run] = _np(z)
    elif group == "invert":
        z, _ = DDIMSampler(model).invert(S, _normal("z0", full).cuda(), c, t_start=S - 1, **kw, **cfg)
        out["invert_cfg"] = _np(z)
    elif group == "compose":
        comp = dict(compose=[(_normal("c1", c.shape).cuda(), -0.75), (_normal("c2", c.shape).cuda(), 0.5)], guidance_rescale=0.5,
                    unconditional_guidance_scale=1.5, unconditional_conditioning=-c)
        common = dict(S=S, batch_size=B, shape=SHAPE, conditioning=c, **kw, **philox, **comp)
        out["compose_ddim"] = _np(DDIMSampler(model).sample(eta=1.0, **common)[0])
        out["compose_dpm"] = _np(DPMSolverSampler(model).sample(order=2, skip_type="logSNR", **common)[0])
    elif group == "dpm":
        z, _ = DPMSolverSampler(model).sample(S=S, batch_size=B, shape=SHAPE, conditioning=c, order=2, skip_type="time_uniform", **kw, **philox)
        out["dpm2_plain"] = _np(z)
    elif group == "loss":
        x, t = _normal("x", full).cuda(), torch.tensor([5, 700])
        for run, noise in (("loss_philox", philox), ("loss_tape", dict(noise=_normal("noise", full)))):
            total, _ = model(x, c, t=t, **noise)
            out[run] = _np(total).reshape(-1)
            for s in range(2):
                _, d, per = model.p_losses(x, c, t, s, return_per_sample=True, **noise)
                out[f"{run}.per{s}"] = _np(per)
                for k in sorted(d):
                    out[f"{run}.s{s}:{k}"] = _np(d[k]).reshape(-1)
    else:
        raise KeyError(group)
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

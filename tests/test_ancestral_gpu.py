"""Ancestral (DDPM) sampling on the MI355X: the update kernel against a float64 restatement, its Philox stream against frido_randn, every fixture run of tests/golden/make_golden_ancestral.py
against the reference's result, and the replay machinery (graph units vs eager steps, shards, graph reuse, score corrector, the vanilla
call sequence of scripts/sample_diffusion.py).

Bounds: the kernel at 2e-6 absolute, what tests/test_kernels_gpu.py::test_sampler_step_and_handoff_match_oracle uses for the DDIM step;
latents, intermediates and x0 predictions at the samplers' 1e-3 max-relative (tests/test_model_gpu.py::test_sampler_matches_reference_golden).
The fixtures are well conditioned (their *_ref_sens: the reference's own movement under a 1e-6 perturbation of every eps, asserted below
1e-4) and stay inside the fp16 planes' range, so a FridoNumericsWarning is an error here.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from golden_cfg import VQ_SMALL, BERT_SMALL, UNET_SMALL, frido_cfg  # noqa: E402
from ancestral_cfg import AB_SMP, AB_SMP_EMB, SEED, B, SHAPE, TABLES, LINEAR  # noqa: E402
from frido_amd.synth import fill_module, seeded_normal  # noqa: E402


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    from frido_amd import _lib
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _frido(ucfg, key, **over):
    from frido_amd.models import instantiate_from_config
    cfg = dict(frido_cfg(ucfg, VQ_SMALL, BERT_SMALL), **over)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    return m.cuda().eval()


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def _launch(**kw):
    from frido_amd.engine import Prog, require_gpu
    dev = require_gpu("cuda")
    p = Prog(dev, 2)
    for kind, args in kw.pop("before", []):
        p.emit(kind, **args)
    p.emit("FRIDO_OP_SAMPLER_STEP", **kw)
    p.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _row(t, clip):
    from frido_amd import schedules
    tabs = schedules.ddpm_tables(schedules.make_beta_schedule("linear", 1000, **LINEAR))
    return schedules.ancestral_table(tabs, clip_denoised=clip)[1000 - 1 - t]


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("tape", ["flat", "tail"])
def test_update_kernel_matches_float64_restatement(stage, clip, tape):
    """Steps 1-4 of the update (x0 on the active channels, clamp on all, posterior mean on the active channels, noise zeroed on [0, start)
    only) in float64 on the kernel's own float32 inputs, so that only the kernel's fp32 roundings remain: with |x|, |eps| <= ~2.2 and the
    t = 100 row (c_recip 1.08, c_recipm1 0.41) every product and sum stays below 4, five roundings of at most 2.4e-7 each."""
    from frido_amd import _lib
    Bk, H, W, Cx, temp = 2, 8, 8, 6, 0.8
    start, nch = 3 * stage, 3
    f = lambda tag, c: torch.from_numpy(seeded_normal(f"anck:{tag}", (Bk, H, W, c))) * 0.5
    x, eps, nz = f("x", Cx), f("e", nch), f("n", Cx) * 2
    row = _row(100, clip)
    assert 1.0 < row[0] < 1.2 and row[4] > 0
    coef = torch.from_numpy(np.stack([np.zeros_like(row), row])).cuda()
    step = torch.ones(1, dtype=torch.int32, device="cuda")
    xd, ed = x.cuda(), eps.cuda()
    c0 = 0 if tape == "flat" else start
    nd = nz[..., c0:].contiguous().cuda()
    out, p0 = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    _launch(x=xd.data_ptr(), B=Bk, HW=H * W, Cx=Cx, start=start, nch=nch, eps_cond=ed.data_ptr(), coef=coef.data_ptr(), step=step.data_ptr(),
            temperature=temp, x_out=out.data_ptr(), pred_x0=p0.data_ptr(), write_x=1, noise=nd.data_ptr(), noise_stride=0, noise_C=Cx - c0,
            noise_c0=c0, hist_mode=_lib.STEP_ANCESTRAL)
    r = [float(v) for v in row]
    X, E, N = x.double(), eps.double(), nz.double()
    act = slice(start, start + nch)
    x0 = X.clone()
    x0[..., act] = r[0] * X[..., act] - r[1] * E
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    mean = X.clone()
    mean[..., act] = r[2] * x0[..., act] + r[3] * X[..., act]
    N[..., :start] = 0.0
    ref = mean + r[4] * (N * float(np.float32(temp)))
    e_x, e_0 = float((out.cpu().double() - ref).abs().max()), float((p0.cpu().double() - x0).abs().max())
    print(f"stage {stage} clip {clip} tape {tape}: x' max-abs error {e_x:.2e}, x0 {e_0:.2e}")
    assert e_x < 2e-6 and e_0 < 2e-6
    assert stage == 0 or torch.equal(out[..., :start], xd[..., :start])       # frozen channels pass through untouched
    assert stage == 1 or float((out[..., nch:] - xd[..., nch:]).abs().max()) > 0.1      # stage 0: the channels above the stage's random-walk
    # pred_x0 alone (write_x = 0) leaves the state alone
    out2 = torch.full_like(xd, 7.0)
    _launch(x=xd.data_ptr(), B=Bk, HW=H * W, Cx=Cx, start=start, nch=nch, eps_cond=ed.data_ptr(), coef=coef.data_ptr(), step=step.data_ptr(),
            temperature=temp, x_out=out2.data_ptr(), pred_x0=p0.data_ptr(), write_x=0, hist_mode=_lib.STEP_ANCESTRAL)
    assert bool((out2 == 7.0).all()) and float((p0.cpu().double() - x0).abs().max()) < 2e-6


@pytest.mark.parametrize("stage", [0, 1])
def test_philox_noise_is_frido_randn_for_the_same_keys(stage):
    """x = eps = 0 with the row {0, 0, 0, 0, sigma = 1}: x' IS the noise.  Draw index = step + coef_row_offset + 1 = 0 here, frido_randn's."""
    from frido_amd import _lib
    Bk, HW, Cx, seed, s0 = 3, 64, 6, 77, 5
    start = 3 * stage
    coef = torch.zeros(2, 12, device="cuda")
    coef[0, 4] = 1.0
    x, eps = torch.zeros(Bk, HW, Cx, device="cuda"), torch.zeros(Bk, HW, 3, device="cuda")
    out, want = torch.empty_like(x), torch.empty_like(x)
    _launch(before=[("FRIDO_OP_RANDN", dict(dst=want.data_ptr(), n=want.numel(), per_sample=HW * Cx, seed=seed, sample0=s0, rng_stream=stage + 1))],
            x=x.data_ptr(), B=Bk, HW=HW, Cx=Cx, start=start, nch=3, eps_cond=eps.data_ptr(), coef=coef.data_ptr() + 48, coef_row_offset=-1,
            temperature=1.0, x_out=out.data_ptr(), write_x=1, seed=seed, sample0=s0, rng_stream=stage + 1, hist_mode=_lib.STEP_ANCESTRAL)
    assert torch.equal(out[..., start:], want[..., start:]) and float(out[..., start:].std()) > 0.9
    assert stage == 0 or bool((out[..., :start] == 0).all())


def test_nonfinite_state_raises_the_status_bit():
    from frido_amd import _lib
    coef = torch.from_numpy(_row(100, False)[None]).cuda()
    x = torch.zeros(1, 16, 4, device="cuda")
    x[0, 3, 2] = float("inf")
    eps = torch.zeros(1, 16, 4, device="cuda")
    _launch(x=x.data_ptr(), B=1, HW=16, Cx=4, start=0, nch=4, eps_cond=eps.data_ptr(), coef=coef.data_ptr(), temperature=1.0,
            x_out=x.data_ptr(), write_x=1, hist_mode=_lib.STEP_ANCESTRAL)
    assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE


def test_ddim_and_plms_bits_are_those_of_the_library_before_the_mode(monkeypatch):
    """hist_mode 0 (DDIM, with and without guidance) and 1 / 3 (PLMS) through the launcher that now branches on FRIDO_STEP_ANCESTRAL:
    bit for bit the latents tests/golden/record_sampler_bits.py recorded on an MI355X from the commit before the mode existed (static
    GEMM tiles on both sides, so the tile cache has no say)."""
    from frido_amd import tune
    import record_sampler_bits as rec
    monkeypatch.setattr(tune, "ENABLED", False)
    g = golden("sampler_step_bits_abi7")
    got = rec.runs(*rec.build_model())
    assert sorted(got) == sorted(g.files) and {"ddim", "ddim_cfg", "plms"} <= set(got)
    for k in sorted(got):
        same = np.array_equal(got[k], g[k])
        print(f"{k}: {'identical' if same else 'max-abs difference %.3e' % float(np.abs(got[k] - g[k]).max())}")
        assert same, k
    assert not np.array_equal(g["ddim"], g["ddim_cfg"]) and not np.array_equal(g["ddim"], g["plms"])


# ---- fixture runs against the reference --------------------------------------------------------------------------------
def _check(g, run, samples, inter, model, decode=True):
    assert float(g[f"{run}_ref_sens"]) < 1e-4
    err = _rel(samples, g[f"{run}_samples"])
    print(f"{run}: latent max-relative error {err:.2e}")
    assert err < 1e-3
    if inter is not None:
        assert len(inter) == int(g[f"{run}_n_inter"])
        for tag, idx in (("first", 0), ("mid", len(inter) // 2), ("last", len(inter) - 1)):
            e = _rel(inter[idx], g[f"{run}_inter_{tag}"])
            print(f"{run}: intermediate {tag} ({idx}) {e:.2e}")
            assert e < 1e-3, (run, tag)
    if decode:
        img = model.decode_first_stage(samples)
        bad = float(((img.cpu() - torch.from_numpy(g[f"{run}_img"])).abs().amax(1) > 1e-3).float().mean())
        print(f"{run}: decoded pixels off by > 1e-3: {100 * bad:.3f} %")
        assert img.shape == g[f"{run}_img"].shape and torch.isfinite(img).all()


@pytest.mark.parametrize("run", [pytest.param("loop", marks=pytest.mark.gate), "loop_clip", "prog", "drop"])
def test_unconditional_loops_match_the_reference(run):
    g = golden("anc_uncond")
    assert float(g["stream_absmax"]) < 1000.0
    model = _frido(AB_SMP, None)
    torch.manual_seed(SEED)
    if run.startswith("loop"):
        model.clip_denoised = run == "loop_clip"
        z, inter = model.p_sample_loop(None, SHAPE, timesteps=12, return_intermediates=True, log_every_t=5, verbose=False)
        assert len(inter) == 1 + 2 * 4        # x_T, then t = 11, 10, 5, 0 of both stages
    elif run == "prog":
        z, inter = model.progressive_denoising(None, SHAPE[1:], batch_size=B, start_T=12, temperature=0.8, verbose=False)
    else:
        z, inter = model.progressive_denoising(None, SHAPE[1:], batch_size=B, start_T=12, noise_dropout=0.25, verbose=False)
    _check(g, run, z, inter, model)


def test_full_chain_through_sample_matches_the_reference():
    g = golden("anc_uncond")
    T = int(g["full_T"])
    model = _frido(AB_SMP, None, timesteps=T)
    torch.manual_seed(SEED)
    z, inter = model.sample(None, batch_size=B, return_intermediates=True, verbose=False)
    _check(g, "full", z, inter, model)
    eng = next(iter(model.model.diffusion_model.runtime()._sampler_engines.values()))
    assert eng.kind == "ddpm" and eng.n_steps == T and getattr(eng, "multi_step_launches", 0) > 0       # replayed in multi-step units


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("clip", [False, True])
def test_p_sample_with_per_sample_timesteps_matches_the_reference(stage, clip):
    g = golden("anc_uncond")
    model = _frido(AB_SMP, None)
    run = f"step_s{stage}" + ("_clip" if clip else "")
    x, t = torch.from_numpy(g["step_x"]).cuda(), torch.from_numpy(g["step_t"]).cuda()
    torch.manual_seed(SEED)
    out, x0 = model.p_sample(x, None, t, stage, clip_denoised=clip, return_x0=True)
    _check(g, run, out, [x0], model, decode=False)
    assert not clip or float(x0.abs().max()) <= 1.0
    if stage == 1 and not clip:
        mean, var, logvar, x0m = model.p_mean_variance(x, None, t, 1, clip_denoised=False, return_x0=True)
        assert _rel(mean, g["pmv_mean"]) < 1e-3 and _rel(x0m, g["pmv_x0"]) < 1e-3
        assert torch.equal(var.cpu(), torch.from_numpy(g["pmv_var"])) and torch.equal(logvar.cpu(), torch.from_numpy(g["pmv_logvar"]))
        assert torch.equal(out[1], mean[1])          # t = 0: no noise, the sample is the posterior mean


@pytest.mark.parametrize("run", ["ctx_sample", "ctx_sample_log", "emb_sample"])
def test_conditional_loops_match_the_reference(run):
    g = golden("anc_cond")
    assert float(g["stream_absmax"]) < 1000.0
    if run.startswith("ctx"):
        model, c = _frido(UNET_SMALL, "crossattn"), torch.from_numpy(g["c"]).cuda()
    else:
        model, c = _frido(AB_SMP_EMB, "adm"), torch.from_numpy(g["emb_y"]).cuda()
    torch.manual_seed(SEED)
    if run == "ctx_sample_log":
        z, inter = model.sample_log(c, B, ddim=False, ddim_steps=None, timesteps=10, verbose=False)
    else:
        z, inter = model.sample(cond=c, batch_size=B, timesteps=10, return_intermediates=True, verbose=False)
    _check(g, run, z, inter, model)


def test_sample_log_ddim_goes_to_the_ddim_sampler():
    from frido.models.diffusion.ddim import DDIMSampler
    model = _frido(AB_SMP, None)
    a, ia = model.sample_log(None, 2, ddim=True, ddim_steps=4, num_stage=2, eta=1.0, noise="philox", seed=3)
    b, _ = DDIMSampler(model).sample(4, 2, (6, 16, 16), None, num_stage=2, verbose=False, eta=1.0, noise="philox", seed=3)
    assert torch.equal(a, b) and "x_inter" in ia


# ---- replay machinery -----------------------------------------------------------------------------------------------------
class _Identity:
    def modify_score(self, model, e_t, x, t, c):
        assert e_t.shape == x.shape and bool((e_t[:, 3:] == 0).all() or (e_t[:, :3] == 0).all())      # zero-padded to the latent's channels
        return e_t


@pytest.mark.parametrize("noise", ["philox", "torch"])
def test_graph_units_single_graph_steps_and_eager_steps_are_bit_identical(noise, monkeypatch):
    """T = 10, log_every_t = 5: with GRAPH_STEPS = 4 the steps t = 8 ... 5 and 4 ... 1 of each stage are 4-step replays and the logged ones
    single steps; GRAPH_STEPS = 1 replays one body per step; an identity score corrector runs every step eagerly (forward program, hook,
    update kernel).  Same kernels in the same order: latents and intermediates must agree bit for bit."""
    from frido_amd import runtime
    outs = []
    for K, hook in ((4, None), (1, None), (4, _Identity())):
        monkeypatch.setattr(runtime, "GRAPH_STEPS", K)
        model = _frido(AB_SMP, None)
        torch.manual_seed(SEED)
        z, inter = model.progressive_denoising(None, SHAPE, start_T=10, log_every_t=5, verbose=False, noise=noise, seed=5, score_corrector=hook)
        torch.manual_seed(SEED)
        z2, inter2 = model.p_sample_loop(None, SHAPE, timesteps=10, log_every_t=5, return_intermediates=True, verbose=False, noise=noise, seed=5)
        eng = next(iter(model.model.diffusion_model.runtime()._sampler_engines.values()))
        multi = getattr(eng, "multi_step_launches", 0)
        assert multi == ((4 if hook is None else 0) + 4 if K == 4 else 0), multi      # two 4-step units per stage and loop
        assert torch.equal(z, z2) and len(inter) == 6 and len(inter2) == 7      # t = 9, 5, 0 of both stages (+ x_T)
        outs.append([t.cpu() for t in [z] + inter + inter2])
    for other in outs[1:]:
        assert len(other) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(outs[0], other))


def test_philox_shards_reproduce_the_single_process_batch_and_graphs_are_reused():
    model = _frido(AB_SMP, None)
    kw = dict(timesteps=8, verbose=False, noise="philox")
    full = model.p_sample_loop(None, (4, 6, 16, 16), seed=9, sample0=0, **kw)
    lo = model.p_sample_loop(None, (2, 6, 16, 16), seed=9, sample0=0, **kw)
    eng = model.model.diffusion_model.runtime()._sampler_engines[next(reversed(model.model.diffusion_model.runtime()._sampler_engines))]
    ncap = eng.graph_captures
    hi = model.p_sample_loop(None, (2, 6, 16, 16), seed=9, sample0=2, **kw)
    other = model.p_sample_loop(None, (2, 6, 16, 16), seed=10, sample0=0, **kw)
    assert eng.graph_captures == ncap and len(model.model.diffusion_model.runtime()._sampler_engines) == 2      # nothing was captured again
    assert torch.equal(full, torch.cat((lo, hi))) and not torch.equal(other, lo) and torch.isfinite(full).all()


def test_pipeline_routes_ddpm_with_philox_noise():
    from frido_amd.pipeline import sample_images
    model = _frido(AB_SMP_EMB, "adm")
    y = torch.tensor([1, 7], device="cuda")
    a = sample_images(model, y, S=6, sampler="ddpm", seed=4, gather=False)
    b = sample_images(model, y, S=6, sampler="ddpm", seed=4, gather=False)
    assert a.shape == (2, 3, 64, 64) and torch.equal(a, b) and torch.isfinite(a).all()
    for bad, word in ((dict(num_stage=1), "num_stage"), (dict(eta=0.0), "eta"), (dict(scale=2.0), "guidance")):
        with pytest.raises(ValueError, match=word):      # what the ancestral loop cannot honour is refused, not ignored
            sample_images(model, y, S=6, sampler="ddpm", seed=4, gather=False, **bad)


def test_p_sample_reproduces_the_loops_philox_draw_on_a_short_chain():
    """Both entry points key the Philox draw by (seed, sample, num_timesteps - t, stage) -- also when the chain is shorter than the schedule
    (timesteps = 3 of 1000).  p_sample from each logged state of the loop must land on the loop's next state.  The two run the same fp32
    arithmetic through different programs (per-call forward and layout changes vs the engine's plan), so the bound is the samplers' 1e-3
    max-relative.  Another draw is far outside it: sigma is 0.027 / 0.032 at t = 1 / 2, two independent draws differ by more than 3 somewhere
    among 3072 values and the state stays below 5, so a wrong key moves the result by more than 1.6e-2 (asserted at 5e-3)."""
    model = _frido(AB_SMP, None)
    z, inter = model.p_sample_loop(None, SHAPE, timesteps=3, return_intermediates=True, log_every_t=1, verbose=False, noise="philox", seed=21,
                                   sample0=4)
    assert len(inter) == 1 + 2 * 3 and torch.equal(inter[-1], z)
    k = 0
    for stage in (0, 1):
        for t in (2, 1, 0):
            tt = torch.full((B,), t, device="cuda", dtype=torch.long)
            nxt = model.p_sample(inter[k], None, tt, stage, noise="philox", seed=21, sample0=4)
            other = model.p_sample(inter[k], None, tt, stage, noise="philox", seed=22, sample0=4)
            e, eo = _rel(nxt, inter[k + 1].cpu()), _rel(other, inter[k + 1].cpu())
            print(f"stage {stage} t {t}: p_sample vs loop {e:.2e}; with another seed {eo:.2e}")
            assert e < 1e-3 and (t == 0 or eo > 5e-3)
            k += 1


def test_vanilla_sampling_script_call_sequence():
    """scripts/sample_diffusion.py:141-153,187-200 (--vanilla_sample): ema_scope, progressive_denoising(None, shape, verbose=True) or
    p_sample_loop(None, shape, return_intermediates=..., verbose=...), decode_first_stage -- on a 20-step schedule."""
    from frido_amd.models import LitEma
    model = _frido(AB_SMP, None, timesteps=20)
    model.model_ema = LitEma(model.model).cuda()
    unet = model.model.diffusion_model
    shape = [2, unet.in_channels, unet.image_size, unet.image_size]
    for prog in (True, False):
        with model.ema_scope("Plotting"):
            if prog:
                sample, progrow = model.progressive_denoising(None, shape, verbose=True)
            else:
                sample, progrow = model.p_sample_loop(None, shape, return_intermediates=True, verbose=True)
        x_sample = model.decode_first_stage(sample)
        assert x_sample.shape == (2, 3, 64, 64) and bool(torch.isfinite(x_sample).all()) and len(progrow) >= 2

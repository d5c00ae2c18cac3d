"""The diffusion objective on the MI355X: the two kernels (frido_qsample, frido_diffusion_loss) against torch on the same device, the
public surface (forward / p_losses / validation_step) against goldens captured from the reference's own FridoDiffusion
(tests/golden/make_golden_loss.py), and the LossEngine's graph replay.

Bounds.
  kernels: q_sample is the reference's expression rounding for rounding, so torch.equal; the loss sums exact fp32 elements in f64 and
    rounds once (<= 6e-8), against float64 torch: relative error <= 1e-6 (a factor of 16 on top).
  model: x_noisy <= 1e-6 relative.  Losses: the forward bound of tests/test_attnblock_gpu.py (eps within 2e-4 of max |eps|) carried
    through | |a - p| - |a - p'| | <= |p - p'|:  E = 2e-4 * max|eps| for l1 and 2e-4 * max|eps| * (2 * max|target - eps| + 2e-4 * max|eps|)
    for l2, per stage, both maxima from the fixture.  The dict values are linear in the per-sample losses, so E goes through the same
    coefficients: a stage entry carries stage_loss_ratio[s] (x max lvlb_weights[t] for the vlb entries), '{prefix}/loss_gamma' and
    '{prefix}/loss' sum over the stages with max exp(-logvar[t]) and l_simple_weight / original_elbo_weight as p_losses applies them.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from golden_cfg import UNET_SMALL, VQ_SMALL, BERT_SMALL, frido_cfg  # noqa: E402
import attnblock_cfg  # noqa: E402
import golden_cfg  # noqa: E402
import loss_cfg as LC  # noqa: E402
from frido_amd import _lib  # noqa: E402
from frido_amd.synth import fill_module  # noqa: E402

T = LC.T


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _frido(ucfg, key, **over):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(ucfg, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    cfg.update(over)
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key       # ('__is_unconditional__' resets the wrapper's key to None, like the reference)
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    return m.cuda().eval()


_MODELS = {}


def _model(tag):
    """One model per fixture for the whole module (the objective's options are plain attributes read at call time)."""
    if tag not in _MODELS:
        cfg_name, key = LC.MODELS[tag]
        _MODELS[tag] = _frido(getattr(attnblock_cfg, cfg_name, None) or getattr(golden_cfg, cfg_name), key)
    return _MODELS[tag]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(shape, seed, sample0, stream):
    """frido_randn over [B][HW][Cx] with per_sample = HW * Cx."""
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    kind, st = _lib.make_op("FRIDO_OP_RANDN", dst=out.data_ptr(), n=out.numel(), per_sample=out[0].numel(), seed=seed, sample0=sample0,
                            rng_stream=stream)
    _lib.check(_lib.lib().frido_randn(C.byref(st), _stream()), "frido_randn")
    return out


# ---- frido_qsample --------------------------------------------------------------------------------------------------------------------
def _qsample(m, x0, t, ch, mix, noise=None, seed=0, sample0=0, stream=0):
    from frido_amd.objective import launch_qsample
    B, HW, Cx = x0.shape
    out = torch.full((B, HW, ch[1]), float("nan"), dtype=torch.float32, device="cuda")
    d = _lib.STRUCTS["FridoQSample"](x0=x0.data_ptr(), x_noisy=out.data_ptr(), t=t.data_ptr(), sqrt_ac=m.sqrt_alphas_cumprod.data_ptr(),
                                     sqrt_1mac=m.sqrt_one_minus_alphas_cumprod.data_ptr(), noise=noise.data_ptr() if noise is not None else None,
                                     seed=seed, sample0=sample0, mix_tau=mix, B=B, HW=HW, Cx=Cx, ch_start=ch[0], ch_end=ch[1], T=T, rng_stream=stream)
    launch_qsample(d, _stream())
    return out


@pytest.mark.gate
@pytest.mark.parametrize("mix", [0.0, 0.1])
@pytest.mark.parametrize("Cx,ch", [(6, (0, 3)), (6, (3, 6)), (8, (0, 4)), (8, (4, 8))])      # Cx = 8: the 16-byte path
def test_qsample_is_bit_equal_to_torch_and_philox_to_its_own_tape(Cx, ch, mix):
    m = _model("unet_small")
    B, H, W = 3, 4, 5
    g = torch.Generator(device="cuda").manual_seed(5)
    x0 = torch.randn(B, H * W, Cx, device="cuda", generator=g)
    noise = torch.randn(B, H * W, Cx, device="cuda", generator=g)
    t = torch.tensor([0, 500, T - 1], device="cuda")
    got = _qsample(m, x0, t, ch, mix, noise=noise)
    nchw = lambda v: v.view(B, H, W, -1).permute(0, 3, 1, 2).contiguous()
    ref = m.q_sample(nchw(x0), t, ch_start=ch[0], ch_end=ch[1], noise=nchw(noise), mix_tau=mix)
    assert torch.equal(nchw(got), ref[:, :ch[1]])
    # Philox: the kernel's own draw is frido_randn's with the same key
    tape = _randn((B, H * W, Cx), seed=77, sample0=5, stream=1)
    assert torch.equal(_qsample(m, x0, t, ch, mix, seed=77, sample0=5, stream=1), _qsample(m, x0, t, ch, mix, noise=tape))
    assert not torch.equal(_qsample(m, x0, t, ch, mix, seed=77, sample0=5, stream=0), _qsample(m, x0, t, ch, mix, noise=tape))


@pytest.mark.gate
def test_qsample_philox_does_not_depend_on_the_sharding():
    m = _model("unet_small")
    g = torch.Generator(device="cuda").manual_seed(6)
    x0 = torch.randn(4, 20, 6, device="cuda", generator=g)
    t = torch.tensor([3, 999, 250, 0], device="cuda")
    whole = _qsample(m, x0, t, (3, 6), 0.1, seed=9, sample0=0, stream=1)
    halves = [_qsample(m, x0[b:b + 2].contiguous(), t[b:b + 2].contiguous(), (3, 6), 0.1, seed=9, sample0=b, stream=1) for b in (0, 2)]
    assert torch.equal(whole, torch.cat(halves))


# ---- frido_diffusion_loss -------------------------------------------------------------------------------------------------------------
def _loss(pred, t, Cx, ch_start, loss_type, logvar, lvlb, noise=None, seed=0, sample0=0, stream=0, lsw=0.75, elbo=0.5):
    from frido_amd.objective import launch_loss
    B, HW, nch = pred.shape
    per, row = torch.full((B,), float("nan"), device="cuda"), torch.full((4,), float("nan"), device="cuda")
    d = _lib.STRUCTS["FridoDiffusionLoss"](pred=pred.data_ptr(), t=t.data_ptr(), noise=noise.data_ptr() if noise is not None else None,
                                           logvar=logvar.data_ptr(), lvlb_weights=lvlb.data_ptr(), per_sample=per.data_ptr(), out=row.data_ptr(),
                                           seed=seed, sample0=sample0, B=B, HW=HW, Cx=Cx, ch_start=ch_start, nch=nch, T=T, rng_stream=stream,
                                           loss_type=loss_type, l_simple_weight=lsw, original_elbo_weight=elbo)
    launch_loss(d, _stream())
    return per, row


@pytest.mark.gate
@pytest.mark.parametrize("loss_type", [0, 1], ids=["l1", "l2"])
@pytest.mark.parametrize("nch", [3, 4])
@pytest.mark.parametrize("HW", [20, 1028])
def test_diffusion_loss_against_float64_torch(HW, nch, loss_type):
    m = _model("unet_small")
    B, Cx, ch_start = 3, 2 * nch, nch
    g = torch.Generator(device="cuda").manual_seed(7)
    pred = torch.randn(B, HW, nch, device="cuda", generator=g)
    t = torch.tensor([0, 500, T - 1], device="cuda")
    logvar = torch.from_numpy(LC.logvar_ramp()).cuda()
    noise = _randn((B, HW, Cx), seed=3, sample0=11, stream=1)
    per, row = _loss(pred, t, Cx, ch_start, loss_type, logvar, m.lvlb_weights, noise=noise)
    df = noise[:, :, ch_start:ch_start + nch].double() - pred.double()
    ls = (df.abs() if loss_type == 0 else df * df).mean(dim=(1, 2))
    lv, w = logvar.double()[t], m.lvlb_weights.double()[t]
    gamma, vlb = (ls / lv.exp() + lv).mean(), (w * ls).mean()
    want = torch.stack([ls.mean(), gamma, vlb, 0.75 * gamma + 0.5 * vlb])
    e_per, e_row = float(((per.double() - ls) / ls).abs().max()), float(((row.double() - want) / want).abs().max())
    print(f"HW {HW} nch {nch} type {loss_type}: per-sample rel err {e_per:.2e}, row rel err {e_row:.2e}")
    assert e_per <= 1e-6 and e_row <= 1e-6
    # two runs are bit-identical; the Philox form regenerates the same target; a row of the batch is the single-sample call's
    per2, row2 = _loss(pred, t, Cx, ch_start, loss_type, logvar, m.lvlb_weights, noise=noise)
    assert torch.equal(per, per2) and torch.equal(row, row2)
    per3, row3 = _loss(pred, t, Cx, ch_start, loss_type, logvar, m.lvlb_weights, seed=3, sample0=11, stream=1)
    assert torch.equal(per, per3) and torch.equal(row, row3)
    for b in range(B):
        one, _ = _loss(pred[b:b + 1].contiguous(), t[b:b + 1].contiguous(), Cx, ch_start, loss_type, logvar, m.lvlb_weights,
                       noise=noise[b:b + 1].contiguous())
        assert torch.equal(one, per[b:b + 1]), b


# ---- the model against the reference's goldens -----------------------------------------------------------------------------------------
def _inputs(tag):
    g = golden(f"loss_{tag}")
    return g, torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["c"]).cuda()


def _configure(m, run):
    for k, v in LC.ctor_options(run).items():
        setattr(m, k, v)
    m._parameters.pop("logvar", None)      # (a plain tensor cannot be assigned over a Parameter)
    m.logvar = torch.nn.Parameter(torch.from_numpy(LC.logvar_ramp())) if run.get("learn_logvar") else torch.zeros(T)
    m.learn_logvar = bool(run.get("learn_logvar"))


def _engine(m):
    return list(m.model.diffusion_model.runtime()._sampler_engines.values())[-1]


def _bounds(g, name, run, sfx, t, m):
    """Per key of the loss dict: the bound of the module docstring."""
    ratio, lsw, elbo = LC.STAGE_LOSS_RATIO, LC.L_SIMPLE_WEIGHT, run["original_elbo_weight"]
    E = []
    for s in range(2):
        me, md = float(g[f"{name}_max_eps{sfx}_{s}"]), float(g[f"{name}_max_diff{sfx}_{s}"])
        E.append(2e-4 * me if run["loss_type"] == "l1" else 2e-4 * me * (2 * md + 2e-4 * me))
    w = float(m.lvlb_weights.cpu()[t].max())
    iv = float(torch.exp(-m.logvar.detach().cpu()[t]).max())
    b = {f"val/loss_simple_stage{s}{sfx}": ratio[s] * E[s] for s in range(2)}
    b.update({f"val/loss_vlb_stage{s}{sfx}": ratio[s] * w * E[s] for s in range(2)})
    b[f"val/loss_gamma{sfx}"] = sum(ratio[s] * iv * E[s] for s in range(2))
    b[f"val/loss{sfx}"] = sum(ratio[s] * (lsw * iv + elbo * w) * E[s] for s in range(2))
    b[f"logvar{sfx}"] = 1e-6
    return E, b


def _check_pass(g, name, run, sfx, m, eng, d):
    t = torch.from_numpy(g[f"{name}_t{sfx}"])
    assert torch.equal(eng.t.cpu(), t), "t is drawn first, from the host generator"
    E, bounds = _bounds(g, name, run, sfx, t, m)
    for s in range(2):
        ref = torch.from_numpy(g[f"{name}_x_noisy{sfx}_{s}"])[:, :3 * (s + 1)]
        got = eng.x_noisy[s].view(LC.B, 16, 16, -1).permute(0, 3, 1, 2).cpu()
        ex = float((got - ref).abs().max() / ref.abs().max())
        el = float((eng.per_sample[s].cpu().double() - torch.from_numpy(g[f"{name}_loss_simple{sfx}"][s]).double()).abs().max())
        print(f"{name}{sfx} stage {s}: x_noisy rel err {ex:.2e}; per-sample loss_simple abs err {el:.2e} (bound {E[s]:.2e})")
        assert ex <= 1e-6 and el <= E[s]
    for k, v in zip(g[f"{name}_keys"].tolist(), g[f"{name}_values"].tolist()):
        if not k.endswith(sfx) or (sfx == "" and k.endswith("_ema")):
            continue
        err = abs(float(d[k]) - v)
        print(f"  {k}: {float(d[k]):.7g} (reference {v:.7g}), abs err {err:.2e} (bound {bounds[k]:.2e})")
        assert err <= bounds[k], k


@pytest.mark.parametrize("tag,name", [pytest.param(t, n, marks=pytest.mark.gate) if (t, n) == ("unet_small", "l2_logvar") else (t, n)
                                       for t in LC.MODELS for n, r in LC.RUNS[t].items() if not r.get("validation")])
def test_forward_matches_reference_golden(tag, name):
    run = LC.RUNS[tag][name]
    g, x, c = _inputs(tag)
    m = _model(tag)
    _configure(m, run)
    torch.manual_seed(LC.SEED)
    total, d = m(x, c)
    assert sorted(d) == g[f"{name}_keys"].tolist()
    assert all(v.is_cuda and v.dim() == 0 for k, v in d.items() if k != "logvar")
    _check_pass(g, name, run, "", m, _engine(m), d)
    _, bounds = _bounds(g, name, run, "", torch.from_numpy(g[f"{name}_t"]), m)
    err = abs(float(total) - float(g[f"{name}_total"]))
    print(f"  total: {float(total):.7g} (reference {float(g[f'{name}_total']):.7g}), abs err {err:.2e}")
    assert err <= bounds["val/loss"]
    assert float(g[f"{name}_ref_sens"]) < 1e-6


@pytest.mark.parametrize("tag", list(LC.MODELS))
def test_validation_step_matches_reference_golden(tag):
    name, run = next((n, r) for n, r in LC.RUNS[tag].items() if r.get("validation"))
    g, x, c = _inputs(tag)
    m = _model(tag)
    _configure(m, run)
    params = dict(m.model.named_parameters())
    before = {k: v.detach().clone() for k, v in params.items()}
    names = {s: k for k, s in m.model_ema.m_name2s_name.items()}
    for s_name, buf in m.model_ema.named_buffers():
        if s_name in names:
            buf.copy_(torch.from_numpy(LC.ema_shadow(names[s_name], before[names[s_name]].cpu().numpy())))
    m.get_input = lambda batch, k: [batch["z"], batch["c"]]
    seen = []
    fwd = m.forward
    m.forward = lambda *a, **k: (lambda out: (seen.append((_engine(m).t.clone(), [v.clone() for v in _engine(m).x_noisy],
                                                            _engine(m).per_sample.clone())), out)[1])(fwd(*a, **k))
    unet = m.model.diffusion_model
    try:
        torch.manual_seed(LC.SEED)
        d = m.validation_step(dict(z=x, c=c), 0)
        # the second batch replays both passes' graphs: one runtime is kept per weight set
        rts = unet.runtime(), m._ema_rt[1]
        engs = [list(rt._sampler_engines.values())[-1] for rt in rts]
        caps = [e.graph_captures for e in engs]
        torch.manual_seed(LC.SEED)
        d_again = m.validation_step(dict(z=x, c=c), 1)
        assert rts[0] is not rts[1] and unet.runtime() is rts[0] and m._ema_rt[1] is rts[1]
        assert [e.graph_captures for e in engs] == caps
        assert sorted(d_again) == sorted(d) and all(torch.equal(d[k], d_again[k]) for k in d)
        del seen[2:]
    finally:
        del m.forward, m.get_input
    assert sorted(d) == g[f"{name}_keys"].tolist()
    assert all(torch.equal(v, before[k]) for k, v in params.items()), "ema_scope restores the weights"

    class Snap:
        pass
    for (t, xn, per), sfx in zip(seen, ("", "_ema")):
        snap = Snap()
        snap.t, snap.x_noisy, snap.per_sample = t, xn, per
        _check_pass(g, name, run, sfx, m, snap, d)
    for s in range(2):
        assert float(d[f"val/loss_simple_stage{s}"]) != float(d[f"val/loss_simple_stage{s}_ema"])


# ---- the engine -----------------------------------------------------------------------------------------------------------------------
SCALARS = dict(loss_type="l2", mix_tau=0.1, l_simple_weight=0.75, original_elbo_weight=0.5)
SC_KEY = (1, 0.1, 0.75, 0.5)


def _new_engine(m, B, use_graph=True, nctx=5):
    from frido_amd.objective import LossEngine
    unet = m.model.diffusion_model
    rt = unet.runtime()
    return LossEngine(rt.builder_for(0), unet.cfg, B=B, C=6, H=16, W=16, nctx=nctx, embed_dim=m.embed_dim_list, num_stage=2, T=T,
                      use_graph=use_graph)


def _run(eng, m, x, c, t, **kw):
    return eng.run(x, c, t, tables=(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, m.lvlb_weights), **dict(SCALARS, **kw))


def test_replayed_graph_equals_the_eager_launches_and_serves_other_batches():
    g, x, c = _inputs("unet_small")
    m = _model("unet_small")
    graph, eager = _new_engine(m, LC.B), _new_engine(m, LC.B, use_graph=False)
    gen = torch.Generator().manual_seed(1)
    lv = torch.from_numpy(LC.logvar_ramp())
    key = ("tape", (0, 1), SC_KEY)
    for i in range(2):                                  # the second call: other t, other noise, the same graph
        t = torch.randint(0, T, (LC.B,), generator=gen)
        tape = [torch.randn(LC.SHAPE, generator=gen) for _ in range(2)]
        a = _run(graph, m, x, c, t, tape=tape, logvar=lv)
        handle = graph.graphs[key]
        b = _run(eager, m, x, c, t, tape=tape, logvar=lv)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), i
        assert all(torch.equal(p, q) for p, q in zip(graph.x_noisy, eager.x_noisy))
    assert list(graph.graphs) == [key] and graph.graphs[key] is handle and graph.graph_captures == 1
    fresh = _run(_new_engine(m, LC.B), m, x, c, t, tape=tape, logvar=lv)
    assert torch.equal(a[0], fresh[0]) and torch.equal(a[1], fresh[1])
    assert bool(torch.isfinite(a[0]).all()) and float(a[0][:, 0].min()) > 0


@pytest.mark.parametrize("tag", ["ab_smp_emb", "unet_small"])
def test_philox_rows_do_not_depend_on_the_sharding(tag):
    """The per-sample rows of a B = 4 call EQUAL those of two B = 2 calls with sample0 0 and 2, bit for bit, and so does the noise
    (x_noisy): the Philox key names the global sample, the loss kernel's sum does not depend on B, and the suite's GEMM tiles are
    pinned or static (tests/conftest.py), with a summation order that does not depend on the row count."""
    g, x, c = _inputs(tag)
    m = _model(tag)
    nctx = 5 if tag == "unet_small" else 0
    t = torch.tensor([10, 400, 700, 999])
    whole = _new_engine(m, 4, nctx=nctx)
    rows, per = _run(whole, m, x, c, t, seed=21, sample0=0)
    xn = [v.clone() for v in whole.x_noisy]
    half = _new_engine(m, 2, nctx=nctx)
    for b0 in (0, 2):
        _, p2 = _run(half, m, x[b0:b0 + 2], c[b0:b0 + 2], t[b0:b0 + 2], seed=21, sample0=b0)
        for s in range(2):
            assert torch.equal(half.x_noisy[s], xn[s][b0:b0 + 2]), (b0, s)      # the noise itself: bit for bit
        err = float((p2 - per[:, b0:b0 + 2]).abs().max())
        print(f"{tag} samples {b0}..{b0 + 1}: per-sample loss differs by {err:.2e} from the B = 4 call")
        assert torch.equal(p2, per[:, b0:b0 + 2]), b0
    assert list(whole.graphs) == [("philox", (0, 1), SC_KEY)]
    assert bool(torch.isfinite(per).all()) and float(per.min()) > 0


def test_public_philox_noise_and_p_losses_agree_with_forward():
    g, x, c = _inputs("ab_smp_emb")
    m = _model("ab_smp_emb")
    _configure(m, LC.RUNS["ab_smp_emb"]["l2_elbo"])
    t = torch.tensor([5, 300, 600, 900])
    total, d = m(x, c, t=t, noise="philox", seed=4)
    total2, d2 = m(x, c, t=t, noise="philox", seed=4)
    assert torch.equal(total, total2) and all(torch.equal(d[k], d2[k]) for k in d)
    assert not torch.equal(total, m(x, c, t=t, noise="philox", seed=5)[0])
    parts = [m.p_losses(x, c, t, s, noise="philox", seed=4) for s in range(2)]
    want = sum(p[0] * r for p, r in zip(parts, m.stage_loss_ratio))
    assert torch.equal(total, want)
    # a noise tensor: the same noise for every stage
    n = torch.randn(LC.SHAPE)
    tot_n, _ = m(x, c, t=t, noise=n)
    parts = [m.p_losses(x, c, t, s, noise=n) for s in range(2)]
    assert torch.equal(tot_n, sum(p[0] * r for p, r in zip(parts, m.stage_loss_ratio)))
    # p_losses runs its own stage only: graphs of one stage on the engine that forward uses
    engines = m.model.diffusion_model.runtime()._sampler_engines
    eng, n_eng = _engine(m), len(engines)
    assert {k[:2] for k in eng.graphs} == {(kind, st) for kind in ("philox", "tape") for st in ((0, 1), (0,), (1,))}
    # the weights and the schedule are per call: no new engine, no stale table.  Doubling is exact in binary.
    _, d0 = m(x, c, t=t, noise="philox", seed=4)
    plans = list(eng.stages)
    m.original_elbo_weight, m.l_simple_weight = 0.25, 0.5
    m.lvlb_weights.mul_(2.0)
    try:
        _, d1 = m(x, c, t=t, noise="philox", seed=4)
    finally:
        m.lvlb_weights.mul_(0.5)
    assert len(engines) == n_eng and _engine(m) is eng and all(p is q for p, q in zip(plans, eng.stages))
    for s in range(2):
        assert torch.equal(d1[f"val/loss_simple_stage{s}"], d0[f"val/loss_simple_stage{s}"])
        assert torch.equal(d1[f"val/loss_vlb_stage{s}"], 2 * d0[f"val/loss_vlb_stage{s}"])
    want = sum(r * (0.5 * float(d0[f"val/loss_simple_stage{s}"]) / r + 0.25 * float(d1[f"val/loss_vlb_stage{s}"]) / r)
               for s, r in enumerate(m.stage_loss_ratio))
    assert abs(float(d1["val/loss"]) - want) <= 1e-6 * abs(want)

"""DPM-Solver++(2M) on the MI355X: the update kernel bit for bit against an eager torch fp32 restatement, the engine (captured graphs, the
K-step graph, the eager path, repeatability), the sampler against the same loop composed from `apply_model` per step plus the restated
update in torch, its first-order / uniform-grid form against DDIM at eta = 0, and the pipeline route.

The solver is not in the reference, so there is no golden: the kernel is pinned by the restatement, the loop by the composed route.
Bounds of the two route comparisons: the samplers' 1e-3 max-relative (tests/test_attnblock_gpu.py `_check_run`), and 4 x the error DDIM
eta = 0, S = 6 shows between the same two routes (engine vs apply_model per step) on the same model: the update combines two x0
predictions with weights summing to at most 3 in magnitude for r >= 1/4.  Measured on an MI355X (UNET_SMALL, B = 2, S = 6; also in
profiles/dpm_sampling.txt), without / with guidance 1.5: DPM-Solver++(2M) engine vs composed route 8.2e-7 / 8.3e-7; DDIM eta = 0 between the
same two routes 8.0e-7 / 1.04e-6; order 1 on the uniform grid vs DDIMSampler(eta = 0) 6.3e-7 / 7.3e-7.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_cfg import VQ_SMALL, BERT_SMALL, UNET_SMALL, frido_cfg  # noqa: E402
from attnblock_cfg import AB_SMP_EMB  # noqa: E402
from frido_amd.synth import fill_module, seeded_normal  # noqa: E402

SHAPE, B, S, EMBED = (6, 16, 16), 2, 6, [3, 3]


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    from frido_amd import _lib
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _rel(got, ref):
    ref = ref.detach().cpu().double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


# ---- 5. the kernel ------------------------------------------------------------------------------------------------------------------
def _table():
    """Rows of the shipped schedule's 2M table, S = 20 on the logSNR grid: row 0 first-order, rows 1 .. second-order."""
    from frido_amd import schedules
    ac = np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0155))
    _, tab = schedules.dpm_solver_table(ac, 20)
    assert tab[0, 5] == 0 and tab[7, 5] < 0
    return tab


def _restate(x, e_c, e_u, s, row, hist, start, nch):
    """The update in eager elementwise torch fp32 ops on the GPU, expression for expression (every op rounds on its own).
    Returns (x', pred_x0 with NaN where the kernel does not write, new history)."""
    inv_alpha, sigma, c_x, c_d, w_cur, w_last = (float(v) for v in row[:6])
    xa = x[..., start:start + nch]
    e = e_c if e_u is None else e_u + s * (e_c - e_u)
    x0 = (xa - sigma * e) * inv_alpha
    D = x0 if w_last == 0 else w_cur * x0 + w_last * hist.reshape(x0.shape)
    xn = c_x * xa + c_d * D
    out, p0 = x.clone(), torch.full_like(x, float("nan"))
    out[..., start:start + nch] = xn
    p0[..., :start] = x[..., :start]
    p0[..., start:start + nch] = x0
    return out, p0, x0.reshape(-1, nch).clone()


def _launch(planes, **kw):
    from frido_amd import _lib
    from frido_amd.engine import require_gpu
    with _lib.use_planes(planes):
        require_gpu("cuda")
        d = _lib.STRUCTS["FridoDpmStep"](**kw)
        _lib.check(_lib.lib().frido_dpm_step(C.byref(d), torch.cuda.current_stream().cuda_stream), "frido_dpm_step")
    torch.cuda.synchronize()


GEOMETRIES = {"scalar_s3n3": (2, 15, 6, 3, 3), "scalar_s0n6": (2, 15, 6, 0, 6), "vec_s4n4": (2, 64, 8, 4, 4)}


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("second", [False, True], ids=["first_order", "second_order"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_kernel_matches_the_torch_restatement_bit_for_bit(geo, guided, second, planes):
    """Scalar path (HW = 5 x 3, Cx = 6) and 16-byte path (HW = 8 x 8, Cx = 8, (4, 4)); cfg_dev overrides cfg_scale; a step counter of 2 with
    coef_row_offset picks the row; x_out aliases x in a second launch; pred_x0 on all written channels; a first-order row finds the
    history full of NaN and must not read it."""
    Bk, HW, Cx, start, nch = GEOMETRIES[geo]
    tab = _table()
    f = lambda tag, c: torch.from_numpy(seeded_normal(f"dpmk:{geo}:{tag}", (Bk, HW, c))).cuda()
    x, e_c, e_u, h0 = f("x", Cx), f("ec", nch), f("eu", nch) if guided else None, f("h", nch).reshape(-1, nch)
    row_i = 7 if second else 0
    step = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    coef = torch.from_numpy(np.concatenate([np.full((3, 8), np.nan, np.float32), tab])).cuda()      # row = step + offset = 3 + row_i
    cfg_dev = torch.full((1,), 2.25, device="cuda")
    hist = h0.clone() if second else torch.full_like(h0, float("nan"))
    out, p0 = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    kw = dict(x=x.data_ptr(), B=Bk, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=e_c.data_ptr(), eps_uncond=e_u.data_ptr() if guided else None,
              cfg_scale=1.5, cfg_dev=cfg_dev.data_ptr(), coef=coef.data_ptr(), step=step.data_ptr(), coef_row_offset=1 + row_i,
              x_out=out.data_ptr(), pred_x0=p0.data_ptr(), x0_hist=hist.data_ptr())
    _launch(planes, **kw)
    want, want_p0, want_h = _restate(x, e_c, e_u, 2.25, tab[row_i], h0, start, nch)
    end = start + nch
    assert torch.isfinite(out[..., :end]).all() and torch.equal(out[..., :end], want[..., :end])
    assert bool(torch.isnan(out[..., end:]).all()) and bool(torch.isnan(p0[..., end:]).all())      # channels above the stage: not written
    assert torch.equal(p0[..., :end], want_p0[..., :end]) and torch.equal(hist, want_h) and torch.isfinite(hist).all()
    assert not guided or not torch.equal(want, _restate(x, e_c, e_u, 1.5, tab[row_i], h0, start, nch)[0])      # the device scalar, not cfg_scale
    assert not second or not torch.equal(want, _restate(x, e_c, e_u, 2.25, tab[0], h0, start, nch)[0])         # the history did enter
    # cfg_scale without the device scalar; x_out aliasing x; no pred_x0
    x2, hist2 = x.clone(), (h0.clone() if second else torch.full_like(h0, float("nan")))
    _launch(planes, **dict(kw, cfg_dev=None, x=x2.data_ptr(), x_out=x2.data_ptr(), pred_x0=None, x0_hist=hist2.data_ptr()))
    want2, _, want_h2 = _restate(x, e_c, e_u, 1.5, tab[row_i], h0, start, nch)
    assert torch.equal(x2, want2) and torch.equal(hist2, want_h2)


def test_unaligned_bases_take_the_scalar_path():
    """Cx, start and nch multiples of 4 but eps 4 bytes off a 16-byte boundary: scalar accesses, the same bits."""
    Bk, HW, Cx, start, nch = GEOMETRIES["vec_s4n4"]
    tab = _table()
    f = lambda tag, c: torch.from_numpy(seeded_normal(f"dpmk:una:{tag}", (Bk, HW, c))).cuda()
    x, h0 = f("x", Cx), f("h", nch).reshape(-1, nch)
    buf = torch.zeros(Bk * HW * nch + 1, device="cuda")
    e_c = buf[1:].view(Bk, HW, nch)
    e_c.copy_(f("ec", nch))
    assert e_c.data_ptr() % 16 == 4
    out, hist, coef = torch.empty_like(x), h0.clone(), torch.from_numpy(tab).cuda()
    _launch("f16", x=x.data_ptr(), B=Bk, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=e_c.data_ptr(), coef=coef.data_ptr(), coef_row_offset=7, x_out=out.data_ptr(), x0_hist=hist.data_ptr())
    want, _, want_h = _restate(x, e_c, None, 1.0, tab[7], h0, start, nch)
    assert torch.equal(out[..., :start + nch], want[..., :start + nch]) and torch.equal(hist, want_h)


def test_nonfinite_state_raises_the_status_bit():
    from frido_amd import _lib
    coef = torch.from_numpy(_table()).cuda()
    x, eps, hist = torch.zeros(1, 16, 4, device="cuda"), torch.zeros(1, 16, 4, device="cuda"), torch.zeros(16, 4, device="cuda")
    _launch("f16", x=x.data_ptr(), B=1, HW=16, Cx=4, start=0, nch=4, eps_cond=eps.data_ptr(), coef=coef.data_ptr(), x_out=x.data_ptr(),
            x0_hist=hist.data_ptr())
    assert _lib.status_flags(clear=True) == 0
    x[0, 3, 2] = float("inf")
    _launch("f16", x=x.data_ptr(), B=1, HW=16, Cx=4, start=0, nch=4, eps_cond=eps.data_ptr(), coef=coef.data_ptr(), x_out=x.data_ptr(),
            x0_hist=hist.data_ptr())
    assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_captured_graph_replayed_twice_equals_two_eager_launches(planes):
    """[frido_dpm_step, counter add] captured once and replayed twice: the device counter moves the replays from the first-order row 0 to
    the second-order row 1, which reads the history the first replay wrote."""
    from frido_amd import _lib
    from frido_amd.engine import Prog, require_gpu
    Bk, HW, Cx, start, nch = GEOMETRIES["vec_s4n4"]
    tab = _table()
    f = lambda tag, c: torch.from_numpy(seeded_normal(f"dpmk:graph:{tag}", (Bk, HW, c))).cuda()
    x_init, e_c = f("x", Cx), f("ec", nch)
    coef = torch.from_numpy(tab).cuda()
    results = []
    with _lib.use_planes(planes):
        dev = require_gpu("cuda")
        for graph in (False, True):
            x, hist = x_init.clone(), torch.full((Bk * HW, nch), float("nan"), device="cuda")
            step = torch.zeros(1, dtype=torch.int32, device="cuda")
            d = _lib.STRUCTS["FridoDpmStep"](x=x.data_ptr(), B=Bk, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=e_c.data_ptr(), coef=coef.data_ptr(),
                                              step=step.data_ptr(), x_out=x.data_ptr(), x0_hist=hist.data_ptr())
            p = Prog(dev, 2)
            p.ops = [_lib.op_of("FRIDO_OP_DPM_STEP", d)]
            p.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=1)
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                g = p.capture(stream.cuda_stream) if graph else None
                for _ in range(2):
                    g.launch(stream.cuda_stream) if graph else p.run(stream.cuda_stream)
            stream.synchronize()
            assert int(step) == 2
            results.append((x, hist))
    want1, _, h1 = _restate(x_init, e_c, None, 1.0, tab[0], None, start, nch)
    want2, _, h2 = _restate(want1, e_c, None, 1.0, tab[1], h1, start, nch)
    for x, hist in results:
        assert torch.equal(x, want2) and torch.equal(hist, h2)


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _frido(ucfg, key):
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(ucfg, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, key
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = key
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    return m.cuda().eval()


@pytest.fixture(scope="module")
def ctx_model():
    m = _frido(UNET_SMALL, "crossattn")
    c = torch.from_numpy(seeded_normal("dpm:c", (B, 5, 64))).cuda()
    uc = torch.from_numpy(seeded_normal("dpm:uc", (B, 5, 64))).cuda()
    return m, c, uc


@pytest.fixture(scope="module")
def label_model():
    m = _frido(AB_SMP_EMB, "adm")
    return m, torch.tensor([1, 7], device="cuda"), torch.tensor([0, 0], device="cuda")


def _dpm(model, c, uc=None, scale=1.0, **kw):
    from frido.models.diffusion.dpm_solver import DPMSolverSampler
    kw = dict(dict(noise="philox", seed=11, log_every_t=10 ** 9), **kw)
    return DPMSolverSampler(model).sample(S=S, batch_size=c.shape[0], shape=SHAPE, conditioning=c, num_stage=2, verbose=False,
                                          unconditional_guidance_scale=scale, unconditional_conditioning=uc if scale != 1.0 else None, **kw)


def _engines(model, kind="dpm"):
    return [e for e in model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).values() if e.kind == kind]


def _clear_engines(model):
    model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).clear()


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ctx", "ctx_cfg", "labels"])
def test_graph_path_eager_path_and_a_second_run_agree_bit_for_bit(case, ctx_model, label_model, monkeypatch):
    from frido_amd import runtime
    monkeypatch.setattr(runtime, "GRAPH_STEPS", 2)
    model, c, uc = label_model if case == "labels" else ctx_model
    scale = 1.5 if case == "ctx_cfg" else 1.0
    _clear_engines(model)
    z, inter = _dpm(model, c, uc, scale)
    eng, = _engines(model)
    assert eng.n_steps == 6 and eng.xrep == (2 if scale != 1.0 else 1)
    assert eng.multi_step_launches == 4 and ("dpm", 0, "x2") in eng.graphs and ("dpm", 1, "x2") in eng.graphs      # steps 1-2 and 3-4 of both stages
    assert z.shape == (B,) + SHAPE and torch.isfinite(z).all() and set(inter) == {"x_inter", "pred_x0"}
    assert len(inter["x_inter"]) == 1 + 2 * 2 and torch.equal(inter["x_inter"][-1], z)      # x_T, then the first and the last step of each stage
    z2, _ = _dpm(model, c, uc, scale)
    assert torch.equal(z, z2) and len(_engines(model)) == 1 and eng.multi_step_launches == 8
    eng.use_graph, eng.graphs = False, {}
    try:
        eager, _ = _dpm(model, c, uc, scale)
    finally:
        eng.use_graph, eng.graphs = True, {}
    assert eng.multi_step_launches == 8 and torch.equal(eager, z)
    other, _ = _dpm(model, c, uc, scale, seed=12)
    assert not torch.equal(other, z)


def test_solver_options_key_the_engine_cache_and_callbacks_see_every_step(ctx_model):
    model, c, uc = ctx_model
    _clear_engines(model)
    a, _ = _dpm(model, c)
    b, _ = _dpm(model, c, order=1)
    d, _ = _dpm(model, c, skip_type="time_uniform")
    e, _ = _dpm(model, c, lower_order_final=False)
    assert len(_engines(model)) == 4 and len({t.cpu().numpy().tobytes() for t in (a, b, d, e)}) == 4
    seen, imgs = [], []
    f, inter = _dpm(model, c, callback=seen.append, img_callback=lambda p0, i: imgs.append((i, tuple(p0.shape))), log_every_t=2)
    assert torch.equal(f, a) and len(_engines(model)) == 4
    assert seen == list(range(6)) * 2 and [i for i, _ in imgs] == seen and imgs[0][1] == (B, 3, 16, 16) and imgs[-1][1] == (B, 6, 16, 16)
    assert len(inter["x_inter"]) == 1 + 2 * 4 and len(inter["pred_x0"]) == 1 + 2 * 4      # index 5, 4, 2, 0 of each stage
    # a supplied x_T is the finished stage 0: only stage 1 runs, the coarse channels stay as given
    x_T = torch.from_numpy(seeded_normal("dpm:xT", (B,) + SHAPE))
    g, _ = _dpm(model, c, x_T=x_T)
    assert torch.equal(g[:, :3].cpu(), x_T[:, :3]) and not torch.equal(g[:, 3:].cpu(), x_T[:, 3:])


# ---- 7. / 8. against the composed path and against DDIM ------------------------------------------------------------------------------
def _handoff(img, s, num_stage=2):
    c0, c1 = sum(EMBED[:s]), sum(EMBED[:s + 1])
    tmp = img[:, c0:c1].clone()
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.avg_pool2d(tmp, 2, 2)
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.interpolate(tmp, scale_factor=2, mode="nearest")
    img[:, c0:c1] = tmp
    return img


def _composed(model, c, uc, scale, x_T, t_loop, update):
    """The multi-stage loop of ddim.py:116-186 driven from here: model.apply_model per step (twice under guidance), the CFG mix and
    `update(i, x_active, e, hist) -> (x', x0)` in eager torch fp32 on the GPU, the hand-off between the stages."""
    img_tmp = x_T.cuda()
    img = None
    for s in range(2):
        img = img_tmp[:, :EMBED[0]].clone() if s == 0 else torch.cat((img, img_tmp[:, sum(EMBED[:s]):sum(EMBED[:s + 1])]), dim=1)
        start, hist = sum(EMBED[:s]), None
        for i, t in enumerate(t_loop):
            tt = torch.full((img.shape[0],), int(t), device="cuda", dtype=torch.long)
            e = model.apply_model(img, tt, c, stage=s)
            if scale != 1.0:
                e_u = model.apply_model(img, tt, uc, stage=s)
                e = e_u + scale * (e - e_u)
            xn, hist = update(i, img[:, start:], e, hist)
            img = torch.cat((img[:, :start], xn), dim=1)
        img = _handoff(img, s)
    return img


def _dpm_update(tab):
    def update(i, xa, e, hist):
        inv_alpha, sigma, c_x, c_d, w_cur, w_last = (float(v) for v in tab[i, :6])
        x0 = (xa - sigma * e) * inv_alpha
        D = x0 if w_last == 0 else w_cur * x0 + w_last * hist
        return c_x * xa + c_d * D, x0
    return update


def _ddim_update(tab):
    """sampler_step_kernel's DDIM expressions at eta = 0 (ddim.py:237-268) on the engine's own float32 table."""
    def update(i, xa, e, hist):
        a_t, a_prev, sq1m = (torch.tensor(float(v), device="cuda") for v in (tab[i, 0], tab[i, 1], tab[i, 3]))
        x0 = (xa - sq1m * e) / a_t.sqrt()
        return a_prev.sqrt() * x0 + (1.0 - a_prev).sqrt() * e, x0
    return update


@pytest.fixture(scope="module")
def routes(ctx_model):
    """Per guidance scale: x_T (Philox, seed 11), DDIM eta = 0, S = 6 through the engine and composed from apply_model, and their distance --
    the yardstick of tests 7 and 8, computed once."""
    from frido.models.diffusion.ddim import DDIMSampler
    from frido_amd import schedules
    model, c, uc = ctx_model
    ac = model.alphas_cumprod.detach().float().cpu().numpy()
    tab, t_loop = schedules.sampler_coef_table(ac, S, 0.0)
    out = {}
    for scale in (1.0, 1.5):
        z, inter = DDIMSampler(model).sample(S=S, batch_size=B, shape=SHAPE, conditioning=c, num_stage=2, eta=0.0, verbose=False, noise="philox",
                                             seed=11, log_every_t=10 ** 9, unconditional_guidance_scale=scale,
                                             unconditional_conditioning=uc if scale != 1.0 else None)
        x_T = inter["x_inter"][0]
        zc = _composed(model, c, uc, scale, x_T, t_loop, _ddim_update(tab))
        out[scale] = dict(x_T=x_T, ddim=z, ddim_err=_rel(z, zc))
    return out


@pytest.mark.parametrize("scale", [1.0, 1.5], ids=["plain", "cfg1.5"])
def test_sampler_matches_the_loop_composed_from_apply_model(scale, ctx_model, routes):
    from frido_amd import schedules
    model, c, uc = ctx_model
    r = routes[scale]
    z, inter = _dpm(model, c, uc, scale)
    assert torch.equal(inter["x_inter"][0], r["x_T"])      # the same Philox x_T as the DDIM run
    t_loop, tab = schedules.dpm_solver_table(model.alphas_cumprod.detach().double().cpu().numpy(), S)
    assert len(t_loop) == 6 and np.all(tab[1:-1, 5] < 0)
    zc = _composed(model, c, uc, scale, r["x_T"], t_loop, _dpm_update(tab))
    err = _rel(z, zc)
    print(f"scale {scale}: DPM-Solver++(2M) engine vs composed route {err:.3e}; DDIM eta 0 S 6 between the same routes {r['ddim_err']:.3e} "
          f"(ratio {err / max(r['ddim_err'], 1e-30):.2f})")
    assert err <= 1e-3
    assert err <= 4 * r["ddim_err"]


@pytest.mark.parametrize("scale", [1.0, 1.5], ids=["plain", "cfg1.5"])
def test_first_order_on_the_uniform_grid_is_ddim_eta0(scale, ctx_model, routes):
    model, c, uc = ctx_model
    r = routes[scale]
    z, inter = _dpm(model, c, uc, scale, order=1, skip_type="time_uniform")
    assert torch.equal(inter["x_inter"][0], r["x_T"])
    err = _rel(z, r["ddim"])
    print(f"scale {scale}: DPM order 1 / time_uniform vs DDIMSampler(eta = 0) {err:.3e}; yardstick {r['ddim_err']:.3e} "
          f"(ratio {err / max(r['ddim_err'], 1e-30):.2f})")
    assert err <= 1e-3
    assert err <= 4 * r["ddim_err"]
    second, _ = _dpm(model, c, uc, scale, skip_type="time_uniform")
    assert not torch.equal(second, z)      # the second-order rows are another solver


# ---- 9. the pipeline ----------------------------------------------------------------------------------------------------------------
def test_pipeline_routes_dpm_and_is_shard_invariant(ctx_model):
    from frido_amd.pipeline import sample_images
    model, c, _ = ctx_model
    c4 = torch.cat((c, torch.from_numpy(seeded_normal("dpm:c2", (B, 5, 64))).cuda()))
    kw = dict(S=S, sampler="dpm", seed=4, gather=False, gather_dtype="uint8")
    full = sample_images(model, c4, sample0=0, **kw)
    lo, hi = sample_images(model, c4[:2], sample0=0, **kw), sample_images(model, c4[2:], sample0=2, **kw)
    assert full.dtype == torch.uint8 and full.shape == (4, 64, 64, 3)
    assert torch.equal(full, torch.cat((lo, hi))) and not torch.equal(lo, hi)
    z4, _ = _dpm(model, c4, seed=4)
    z2, _ = _dpm(model, c4[2:], seed=4, sample0=2)
    assert torch.equal(z4[2:], z2)      # the latents too, not only their rounding to uint8
    assert len(_engines(model)) >= 1 and _engines(model)[-1].kind == "dpm"

"""DDIM inversion on the MI355X: the update kernel (frido_invert_step) through the C ABI against float64, the engine against a loop composed
in this file from model.apply_model and the same table, the engine's exact properties, the round trip invert -> edit(init="noise", eta=0)
and pipeline.invert_images.

Kernel bound, per element: 8 * 2^-24 * (|c0 x| + |c1| (|e_u| + |s| (|e_c| + |e_u|))) -- at most eight fp32 roundings of partial results of
that magnitude (the subtraction, the product with s, the sum, the two products with the coefficients, the final sum; without guidance
e_u = 0 and e_c = e).  Engine bound: 5e-5 relative to the maximum, the bound the project uses for the same arithmetic run through
different plans (E2E_X3 latent_rel).
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_cfg import VQ_SMALL, BERT_SMALL, UNET_SMALL, frido_cfg  # noqa: E402
from helpers import golden  # noqa: E402
from frido_amd.synth import fill_module, seeded_normal  # noqa: E402

SHAPE, B, EMBED = (6, 16, 16), 2, [3, 3]
ENGINE_BOUND = 5e-5
SCALE = 1.5


@pytest.fixture(autouse=True)
def _no_numerics_warning():
    from frido_amd import _lib
    _lib.status_flags(clear=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", _lib.FridoNumericsWarning)
        yield
    assert _lib.status_flags(clear=True) == 0


def _rel(got, ref):
    ref = torch.as_tensor(ref).detach().cpu().double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
def _launch(planes="f16", **kw):
    from frido_amd import _lib
    from frido_amd.engine import require_gpu
    with _lib.use_planes(planes):
        require_gpu("cuda")
        d = _lib.STRUCTS["FridoInvertStep"](**kw)
        _lib.check(_lib.lib().frido_invert_step(C.byref(d), torch.cuda.current_stream().cuda_stream), "frido_invert_step")
    torch.cuda.synchronize()


def _table():
    """The S = 6 table of the shipped schedule: 7 rows, neighbours far apart."""
    from frido_amd import schedules
    ac = np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0155)).astype(np.float32)
    ts = schedules.make_ddim_timesteps("uniform", 6, 1000)
    _, al, alp = schedules.make_ddim_sampling_parameters(ac, ts, 0.0)
    return schedules.ddim_inversion_table(al, alp)


# the grid is capped at 2048 workgroups of 256 (csrc/invert.hip): 524 289 units need the second trip of the grid-stride loop
GEOMETRIES = {"b2_hw256_c6_w36": (2, 256, 6, 3, 6), "b3_hw35_c9_w36": (3, 35, 9, 3, 6), "b1_hw174763_c6_w36": (1, 174763, 6, 3, 6)}
STEP, ROW_OFFSET = 2, 1       # the device counter holds 2: coefficients from row 3


def _f64(x, ec, eu, s, c0, c1, lo, hi):
    """(x' in float64 on the whole state, the per-element bound on the window [lo, hi))."""
    x, ec = x.double(), ec.double()
    eu = torch.zeros_like(ec) if eu is None else eu.double()
    e = eu + s * (ec - eu) if s is not None else ec
    s = 1.0 if s is None else s          # without guidance e = 0 + 1 * (e - 0)
    out = x.clone()
    out[..., lo:hi] = c0 * x[..., lo:hi] + c1 * e
    bound = 8 * 2.0 ** -24 * ((c0 * x[..., lo:hi]).abs() + abs(c1) * (eu.abs() + abs(s) * (ec.abs() + eu.abs())))
    return out, bound


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_kernel_matches_float64_and_wrong_variants_do_not(geo, guided, planes):
    Bk, HW, Cx, lo, hi = GEOMETRIES[geo]
    wn = hi - lo
    f = lambda tag, *shape: torch.from_numpy(seeded_normal(f"invk:{geo}:{tag}", shape))
    x, ec, eu = f("x", Bk, HW, Cx), f("ec", Bk, HW, wn), f("eu", Bk, HW, wn) if guided else None
    x[0, 0, 0] = float("nan")          # outside the window: never read, stays where it is, raises nothing
    tab = _table()
    row = STEP + ROW_OFFSET
    c0, c1 = float(tab[row, 0]), float(tab[row, 1])
    s = float(np.float32(SCALE)) if guided else None
    xd, ecd, eud, td = x.cuda(), ec.cuda(), eu.cuda() if guided else None, torch.from_numpy(tab).cuda()
    step, cfg = torch.full((1,), STEP, dtype=torch.int32, device="cuda"), torch.full((1,), SCALE, device="cuda")
    kw = dict(x=xd.data_ptr(), eps_cond=ecd.data_ptr(), coef=td.data_ptr(), step=step.data_ptr(), coef_row_offset=ROW_OFFSET, B=Bk, HW=HW, Cx=Cx,
              c_lo=lo, c_hi=hi, cfg_scale=99.0)       # cfg_dev overrides the field
    if guided:
        kw.update(eps_uncond=eud.data_ptr(), cfg_dev=cfg.data_ptr())
    _launch(planes, **kw)
    got = xd.cpu()
    want, bound = _f64(x, ec, eu, s, c0, c1, lo, hi)
    worst = float(((got[..., lo:hi].double() - want[..., lo:hi]).abs() / bound).max())
    print(f"{geo} {'guided' if guided else 'plain'} {planes}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    # channels outside the window keep their bits
    outside = [c for c in range(Cx) if not lo <= c < hi]
    assert torch.equal(_bits(got[..., outside]), _bits(x[..., outside]))
    # wrong variants, each at least 10 x over the bound somewhere on the window
    miss = lambda other: float(((got[..., lo:hi].double() - other[..., lo:hi]).abs() / bound).max())
    for r in (row - 1, row + 1):
        assert miss(_f64(x, ec, eu, s, float(tab[r, 0]), float(tab[r, 1]), lo, hi)[0]) >= 10
    if guided:
        assert miss(_f64(x, ec, None, None, c0, c1, lo, hi)[0]) >= 10 and miss(_f64(x, eu, None, None, c0, c1, lo, hi)[0]) >= 10
    for sh in (-1, 1):
        if hi + sh <= Cx:
            assert miss(_f64(x, ec, eu, s, c0, c1, lo + sh, hi + sh)[0]) >= 10


@pytest.mark.gate
def test_nonfinite_result_raises_the_status_bit():
    from frido_amd import _lib
    x, e, tab = torch.zeros(1, 16, 6, device="cuda"), torch.zeros(1, 16, 3, device="cuda"), torch.ones(1, 2, device="cuda")
    kw = dict(x=x.data_ptr(), eps_cond=e.data_ptr(), coef=tab.data_ptr(), B=1, HW=16, Cx=6, c_lo=3, c_hi=6, cfg_scale=1.0)
    x[0, 2, 1] = float("inf")            # outside the window: never read
    _launch(**kw)
    assert _lib.status_flags(clear=True) == 0
    e[0, 3, 1] = float("inf")
    _launch(**kw)
    assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE


# ---- models -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_model():
    from frido_amd.models import instantiate_from_config
    cfg = frido_cfg(UNET_SMALL, VQ_SMALL, BERT_SMALL)
    cfg["cond_stage_config"], cfg["cond_stage_trainable"], cfg["conditioning_key"] = "__is_unconditional__", False, "crossattn"
    m = instantiate_from_config(dict(target="frido.models.diffusion.frido.FridoDiffusion", params=cfg))
    m.model.conditioning_key = "crossattn"
    fill_module(m.model, "model.")
    fill_module(m.first_stage_model, "first_stage_model.")
    m.scale_factor.copy_(torch.tensor([0.9, 1.1]))
    m = m.cuda().eval()
    c = torch.from_numpy(golden("sampler_small")["c"]).cuda()
    uc = torch.from_numpy(seeded_normal("invert:uc", tuple(c.shape))).cuda()
    return m, c, uc


def _sampler(model):
    from frido.models.diffusion.ddim import DDIMSampler
    return DDIMSampler(model)


def _engines(model, kind="invert"):
    return [e for e in model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).values() if e.kind == kind]


def _clear_engines(model):
    model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).clear()


def _z0(tag, Bk=B):
    """A latent shaped like an encoded one: the coarse channels [0, 3) constant over 2 x 2 blocks, their values multiples of 2^-8 so that
    the hand-off's block mean of four equal floats returns them exactly."""
    z = torch.from_numpy(seeded_normal(f"invert:{tag}", (Bk,) + SHAPE))
    coarse = torch.round(z[:, :3, ::2, ::2] * 256) / 256
    z[:, :3] = coarse.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return z.cuda()


def _invert(model, c, uc, z0, S=6, scale=SCALE, **kw):
    kw = dict(dict(num_stage=2, verbose=False, log_every_t=10 ** 9), **kw)
    return _sampler(model).invert(S, z0, c, unconditional_guidance_scale=scale, unconditional_conditioning=uc if scale != 1.0 else None, **kw)


def _grid(model, S):
    from frido_amd import schedules
    ac = model.alphas_cumprod.detach().float().cpu().numpy()
    ts = schedules.make_ddim_timesteps("uniform", S, len(ac))
    _, al, alp = schedules.make_ddim_sampling_parameters(ac, ts, 0.0)
    return ts, al, alp


def _eps(model, x, t_value, c, uc, scale, s):
    t = torch.full((x.shape[0],), int(t_value), device="cuda", dtype=torch.long)
    e_c = model.apply_model(x, t, c, stage=s)
    if scale == 1.0:
        return e_c
    e_u = model.apply_model(x, t, uc, stage=s)
    return e_u + torch.tensor(scale, device="cuda") * (e_c - e_u)


def _composed_invert(model, c, uc, z0, S, k, scale=SCALE, first_stage=0):
    """Per stage, per row: model.apply_model on HIP (conditional and unconditional), the guidance mix and x' = c0 x + c1 e in eager torch
    fp32 from the same float32 table."""
    from frido_amd import schedules
    ts, al, alp = _grid(model, S)
    tab = torch.from_numpy(schedules.ddim_inversion_table(al, alp)).cuda()
    out = z0.clone()
    for s in range(first_stage, 2):
        a, e = sum(EMBED[:s]), sum(EMBED[:s + 1])
        x = z0[:, :e].clone()
        for i in range(k):
            x = torch.cat((x[:, :a], tab[i, 0] * x[:, a:e] + tab[i, 1] * _eps(model, x, ts[i], c, uc, scale, s)), dim=1)
        out[:, a:e] = x[:, a:e]
    return out


def _composed_back(model, c, uc, x_T, S, k, scale=SCALE):
    """The last k rows of DDIM at eta = 0 from x_T, two stages with the hand-off: the update restated from ddim.py:237-268 on the sampler's
    own float32 schedule, like tests/test_edit_gpu.py's composed loop."""
    from frido_amd import schedules
    ac = model.alphas_cumprod.detach().float().cpu().numpy()
    tab, t_loop = schedules.sampler_coef_table(ac, S, 0.0)
    n = tab.shape[0]
    full = lambda v: torch.full((x_T.shape[0], 1, 1, 1), float(v), device="cuda")
    img = x_T.clone()
    for s in range(2):
        a, e = sum(EMBED[:s]), sum(EMBED[:s + 1])
        x = img[:, :e].clone()
        for row in range(n - k, n):
            e_t = _eps(model, x, t_loop[row], c, uc, scale, s)
            a_t, a_prev, _, sq1m = (full(v) for v in tab[row, :4])
            pred_x0 = (x[:, a:e] - sq1m * e_t) / a_t.sqrt()
            x = torch.cat((x[:, :a], a_prev.sqrt() * pred_x0 + (1. - a_prev).sqrt() * e_t), dim=1)
        if s == 0:      # the hand-off: stage 0's result block-averaged (avg_pool2d, nearest back)
            x = torch.nn.functional.interpolate(torch.nn.functional.avg_pool2d(x, 2, 2), scale_factor=2, mode="nearest")
        img = torch.cat((x, img[:, e:]), dim=1)
    return img


@pytest.mark.gate
def test_invert_matches_the_loop_composed_from_apply_model(ctx_model):
    """UNET_SMALL (two stages, split head, SPADE), B = 2, 16 x 16, S = 6 (7 rows), t_start = 4, guidance 1.5."""
    model, c, uc = ctx_model
    z0 = _z0("composed:z0")
    got, inter = _invert(model, c, uc, z0, t_start=4)
    want = _composed_invert(model, c, uc, z0, 6, 4)
    err = _rel(got, want)
    moved = _rel(got, z0)
    print(f"invert S 6 k 4 guidance {SCALE} vs its composed loop {err:.3e} (bound {ENGINE_BOUND:.0e}); distance from z0 {moved:.3e}")
    assert got.shape == z0.shape and torch.isfinite(got).all()
    assert err <= ENGINE_BOUND and moved > 1e3 * ENGINE_BOUND
    last = inter["x_inter"][-1]                  # stage 1's last state: z0's coarse channels, its own window inverted
    assert torch.equal(inter["x_inter"][0], z0) and torch.equal(last[:, :3], z0[:, :3]) and torch.equal(last[:, 3:], got[:, 3:])
    assert len(inter["x_inter"]) == 1 + 2 * 2    # z0, then steps 0 and k - 1 of both stages
    eng, = _engines(model)
    assert set(k for k in eng.graphs) == {("invert", 0), ("invert", 1)} and eng.n_steps == 7


@pytest.mark.gate
def test_engine_edges(ctx_model):
    """t_start = 1 and t_start = the number of rows run (S = 5 divides the model's 1000 timesteps: exactly 5 rows); first_stage = 1 keeps
    stage 0's bits; the intermediates and the callback count k steps per stage that runs; the host generator is left alone."""
    model, c, uc = ctx_model
    z0 = _z0("edges:z0")
    rng = torch.get_rng_state()
    one, _ = _invert(model, c, uc, z0, t_start=1)
    assert torch.isfinite(one).all() and _rel(one, _composed_invert(model, c, uc, z0, 6, 1)) <= ENGINE_BOUND
    whole, _ = _invert(model, c, uc, z0, S=5, t_start=5)
    assert torch.isfinite(whole).all() and _rel(whole, _composed_invert(model, c, uc, z0, 5, 5)) <= ENGINE_BOUND
    seen = []
    upper, inter = _invert(model, c, uc, z0, t_start=4, first_stage=1, callback=seen.append, log_every_t=2)
    assert torch.equal(_bits(upper[:, :3]), _bits(z0[:, :3])) and not torch.equal(upper[:, 3:], z0[:, 3:])
    assert seen == list(range(4)) and len(inter["x_inter"]) == 1 + 3        # steps 0, 1 and 3 of k = 4 are logged at log_every_t = 2
    both, _ = _invert(model, c, uc, z0, t_start=4)
    assert torch.equal(_bits(both[:, 3:]), _bits(upper[:, 3:]))             # the stages do not depend on one another
    assert torch.equal(torch.get_rng_state(), rng)


@pytest.mark.gate
def test_a_second_call_replays_the_graphs_and_equals_a_fresh_engine(ctx_model):
    """z0, k and the guidance scale are device state or loop bounds: other values replay the same graphs."""
    model, c, uc = ctx_model
    _clear_engines(model)
    z1, z2 = _z0("again:z1"), _z0("again:z2")
    first, _ = _invert(model, c, uc, z1, t_start=4)
    eng, = _engines(model)
    captures = eng.graph_captures
    second, _ = _invert(model, c, uc, z2, t_start=3, scale=2.0)
    assert eng.graph_captures == captures and len(_engines(model)) == 1
    _clear_engines(model)
    fresh, _ = _invert(model, c, uc, z2, t_start=3, scale=2.0)
    assert torch.equal(_bits(second), _bits(fresh)) and not torch.equal(second, first)
    _clear_engines(model)
    again, _ = _invert(model, c, uc, z1, t_start=4)
    assert torch.equal(_bits(again), _bits(first))


def test_a_chain_longer_than_one_graph_unit_equals_single_steps(ctx_model):
    """S = 25, k = 23: one 20-step unit and three single steps; a callback forces single steps -- the same bits."""
    model, c, uc = ctx_model
    _clear_engines(model)
    z0 = _z0("long:z0")
    out, _ = _invert(model, c, uc, z0, S=25, t_start=23)
    eng, = _engines(model)
    assert eng.multi_step_launches >= 1 and ("invert", 0, "x20") in eng.graphs and ("invert", 1, "x20") in eng.graphs
    launches = eng.multi_step_launches
    single, _ = _invert(model, c, uc, z0, S=25, t_start=23, callback=lambda i: None)
    assert eng.multi_step_launches == launches and torch.equal(_bits(single), _bits(out)) and torch.isfinite(out).all()


def test_round_trip_through_edit_from_noise(ctx_model):
    """x_inv = invert(S = 50, t_start = 5); edit(init='noise', x_T = x_inv, t_start = 5, eta = 0, reimpose = False) comes back closer to z0
    than edit(init='z0') with the same arguments does (that one re-noises the start with a random draw), and its error is the composed
    torch loop's own round-trip error to 1e-3 relative.  The absolute error depends on the synthetic weights: printed, recorded in
    profiles/invert_sampling.txt, not asserted."""
    model, c, uc = ctx_model
    z0 = _z0("trip:z0")
    kw = dict(t_start=5, eta=0., reimpose=False, num_stage=2, verbose=False, noise="philox", seed=11, log_every_t=10 ** 9,
              unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    x_inv, _ = _invert(model, c, uc, z0, S=50, t_start=5)
    back, _ = _sampler(model).edit(50, z0, c, init="noise", x_T=x_inv, **kw)
    sdedit, _ = _sampler(model).edit(50, z0, c, init="z0", **kw)
    err, err_sdedit = float((back - z0).abs().max()), float((sdedit - z0).abs().max())
    want_inv = _composed_invert(model, c, uc, z0, 50, 5)
    err_composed = float((_composed_back(model, c, uc, want_inv, 50, 5) - z0).abs().max())
    print(f"round trip S 50 k 5 guidance {SCALE}: max |back - z0| {err:.6e} (composed loop {err_composed:.6e}, relative difference "
          f"{abs(err - err_composed) / err_composed:.2e}); edit(init='z0') {err_sdedit:.6e}; max |z0| {float(z0.abs().max()):.3f}")
    assert err < err_sdedit
    assert abs(err - err_composed) <= 1e-3 * err_composed


def test_invert_images_is_encode_then_invert(ctx_model):
    from frido_amd.pipeline import invert_images
    model, c, uc = ctx_model
    images = torch.from_numpy(seeded_normal("invert:images", (B, 3, 64, 64))).clamp(-1, 1).cuda()
    z0 = model.get_first_stage_encoding(model.encode_first_stage(images))
    want, _ = _invert(model, c, None, z0, t_start=4, scale=1.0)
    got = invert_images(model, images, c, S=6, t_start=4, gather=False)
    assert got.shape == (B,) + SHAPE and torch.equal(_bits(got), _bits(want))
    guided = invert_images(model, images, c, S=6, strength=0.7, scale=SCALE, uncond=uc, first_stage=1, gather=False)
    assert torch.equal(_bits(guided[:, :3]), _bits(z0[:, :3])) and torch.equal(_bits(guided), _bits(_invert(model, c, uc, z0, strength=0.7, first_stage=1)[0]))
    # a shard equals the same rows of the whole batch
    im4, c4 = torch.cat((images, images.flip(-1))), torch.cat((c, c.flip(0)))
    whole = invert_images(model, im4, c4, S=6, t_start=4, gather=False)
    assert torch.equal(_bits(whole), _bits(torch.cat((invert_images(model, im4[:2], c4[:2], S=6, t_start=4, gather=False),
                                                      invert_images(model, im4[2:], c4[2:], S=6, t_start=4, sample0=2, gather=False)))))

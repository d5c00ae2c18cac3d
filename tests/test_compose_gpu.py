"""Composed guidance on the MI355X: the kernel (frido_guidance_compose) through the C ABI -- the plain form bit for bit against a torch
fp32 restatement, the rescaled form against float64 --, the engine against loops composed in this file from model.apply_model, the
restated composition and a restated update, the existing classifier-free path as an oracle, the engine's exact properties, a
class-conditional denoiser and pipeline.sample_images.

Rescaled-form bound, per element: (3 n + 2) * 2^-24 * f_b * (|e_u| + sum |w_i| (|e_i| + |e_u|)) -- three fp32 roundings per term, the
rounding of f_b and the final product.  Engine bound: 5e-5 relative to the maximum, the bound the project uses for the same arithmetic run
through different plans (E2E_X3 latent_rel).  The eta = 1 case replays a recorded tape (the composed loop has to see the update's draws);
every other run draws x_T with Philox and the loops start from the engine's own logged x_T.
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

SHAPE, B, EMBED, S = (6, 16, 16), 2, [3, 3], 5
ENGINE_BOUND = 5e-5
SCALE, W1, W2, PHI = 1.5, -0.75, 0.5, 0.7


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
def _call(name, struct, planes="f16", **kw):
    from frido_amd import _lib
    from frido_amd.engine import require_gpu
    with _lib.use_planes(planes):
        require_gpu("cuda")
        d = _lib.STRUCTS[struct](**kw)
        _lib.check(getattr(_lib.lib(), name)(C.byref(d), torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()


def _launch(planes="f16", **kw):
    _call("frido_guidance_compose", "FridoGuidanceCompose", planes, **kw)


# (n, B, per_sample).  The grid is capped at 2048 workgroups of 256 (csrc/guidance.hip): 524 289 scalar units (an odd total), or as many
# 16-byte units (a total of 4 * 524 289), need the second trip of the grid-stride loop.
GEOMETRIES = {"n1_b2_p768": (1, 2, 768), "n3_b3_p105": (3, 3, 105), "n8_b1_p48": (8, 1, 48), "n1_b1_p524289": (1, 1, 524289),
              "n1_b1_p2097156": (1, 1, 2097156)}
WEIGHTS = {1: [1.5], 3: [1.5, -0.75, 0.0], 8: [1.5, -0.75, 0.0, 0.5, 2.0, -0.25, 1.0, 0.3]}      # above 1, negative, zero


def _slots(geo, Bk=None, scales=None):
    """eps [n + 1][Bk][per_sample] from seeded_normal; scales: a factor per sample."""
    n, Bg, per = GEOMETRIES[geo]
    Bk = Bg if Bk is None else Bk
    e = torch.from_numpy(seeded_normal(f"guide:{geo}:{Bk}", (n + 1, Bk, per)))
    if scales is not None:
        e = e * torch.tensor(scales, dtype=torch.float32).view(1, Bk, 1)
    return n, Bk, per, e.contiguous()


def _restate(e, w):
    """acc = e_u; acc = acc + w_i (e_i - e_u) in order, every product and sum an fp32 torch op of its own."""
    n = e.shape[0] - 1
    acc = e[n].clone()
    for i in range(n):
        acc = acc + torch.tensor(w[i], dtype=torch.float32) * (e[i] - e[n])
    return acc


def _wdev(w, phi=0.0):
    return torch.tensor(list(w) + [phi], dtype=torch.float32, device="cuda")


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("alias", [True, False], ids=["in_place", "apart"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_plain_form_is_the_torch_restatement_bit_for_bit(geo, alias, planes):
    n, Bk, per, e = _slots(geo)
    w = WEIGHTS[n]
    ed, wd = e.cuda(), _wdev(w, phi=float("nan"))      # the plain form never reads phi
    out = ed[0] if alias else torch.full((Bk, per), 7.0, device="cuda")
    _launch(planes, eps=ed.data_ptr(), out=out.data_ptr(), weights=wd.data_ptr(), n=n, B=Bk, per_sample=per, rescale=0)
    want = _restate(e, w)
    assert torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(ed[1:]), _bits(e[1:]))                        # the slots other than 0 keep their bits
    assert alias or torch.equal(_bits(ed[0]), _bits(e[0]))
    # the wrong readings are not what it computes
    assert not torch.equal(out.cpu(), _restate(e.flip(0), w))
    if n > 1:
        assert not torch.equal(out.cpu(), _restate(e, [w[1], w[0]] + w[2:]))


@pytest.mark.gate
def test_unaligned_bases_take_the_scalar_path_with_the_same_bits():
    n, Bk, per, e = _slots("n1_b2_p768")
    w = WEIGHTS[n]
    pad = torch.zeros(e.numel() + 1, device="cuda")
    pad[1:] = e.reshape(-1).cuda()                    # slot 0 starts 4 bytes past a 16-byte boundary
    out, wd = torch.zeros(Bk * per + 1, device="cuda"), _wdev(w)
    _launch(eps=pad.data_ptr() + 4, out=out.data_ptr() + 4, weights=wd.data_ptr(), n=n, B=Bk, per_sample=per, rescale=0)
    assert torch.equal(_bits(out[1:].view(Bk, per)), _bits(_restate(e, w))) and float(out[0]) == 0.0


UPDATE_GEOMETRIES = {"vec_c8_s4n4": (2, 64, 8, 4, 4), "scalar_c6_s3n3": (2, 35, 6, 3, 3)}


@pytest.mark.gate
@pytest.mark.parametrize("geo", sorted(UPDATE_GEOMETRIES))
@pytest.mark.parametrize("kernel", ["sampler_step", "dpm_step", "invert_step"])
def test_n1_composed_eps_drives_every_update_kernel_to_the_bits_of_its_own_mix(kernel, geo):
    """n = 1 is sampler_step_kernel's expression: an update kernel fed the composed eps with eps_uncond = NULL writes what the same launch
    fed both halves and cfg_dev writes."""
    from frido_amd import schedules
    Bk, HW, Cx, start, nch = UPDATE_GEOMETRIES[geo]
    f = lambda tag, *shape: torch.from_numpy(seeded_normal(f"guide:upd:{geo}:{tag}", shape)).cuda()
    x, eps, hist = f("x", Bk, HW, Cx), f("eps", 2, Bk * HW, nch), f("hist", Bk * HW, nch)
    cfg, step = torch.full((1,), SCALE, device="cuda"), torch.full((1,), 1, dtype=torch.int32, device="cuda")
    mixed, wd = torch.empty(Bk * HW, nch, device="cuda"), _wdev([SCALE])
    _launch(eps=eps.data_ptr(), out=mixed.data_ptr(), weights=wd.data_ptr(), n=1, B=Bk, per_sample=HW * nch, rescale=0)
    ac = np.cumprod(1.0 - schedules.make_beta_schedule("linear", 1000, linear_start=0.0015, linear_end=0.0155))
    results = []
    for ec, eu in ((eps[0], eps[1]), (mixed, None)):
        xo, p0, h = x.clone(), torch.zeros_like(x), hist.clone()
        kw = dict(x=xo.data_ptr(), B=Bk, HW=HW, Cx=Cx, eps_cond=ec.data_ptr(), eps_uncond=eu.data_ptr() if eu is not None else None,
                  cfg_scale=99.0, cfg_dev=cfg.data_ptr(), step=step.data_ptr())
        if kernel == "sampler_step":
            tab = torch.from_numpy(schedules.sampler_coef_table(ac.astype(np.float32), 6, 0.0)[0]).cuda()
            _call("frido_sampler_step", "FridoSamplerStep", start=start, nch=nch, coef=tab.data_ptr(), x_out=xo.data_ptr(), pred_x0=p0.data_ptr(),
                  write_x=1, temperature=1.0, **kw)
        elif kernel == "dpm_step":
            tab = torch.from_numpy(schedules.dpm_solver_table(ac, 6)[1]).cuda()      # row 1: second order, reads the history
            _call("frido_dpm_step", "FridoDpmStep", start=start, nch=nch, coef=tab.data_ptr(), x_out=xo.data_ptr(), pred_x0=p0.data_ptr(),
                  x0_hist=h.data_ptr(), **kw)
        else:
            ts = schedules.make_ddim_timesteps("uniform", 6, 1000)
            _, al, alp = schedules.make_ddim_sampling_parameters(ac.astype(np.float32), ts, 0.0)
            tab = torch.from_numpy(schedules.ddim_inversion_table(al, alp)).cuda()
            _call("frido_invert_step", "FridoInvertStep", c_lo=start, c_hi=start + nch, coef=tab.data_ptr(), **kw)
        results.append((xo, p0, h))
    (xa, pa, ha), (xb, pb, hb) = results
    assert torch.equal(_bits(xa), _bits(xb)) and torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ha), _bits(hb))
    assert not torch.equal(xa, x)


def _f64(e, w, phi, per_batch=False):
    """(out, f [Bk], bound) in float64: the composition, the rescale factor per sample (per_batch: the wrong one, over the whole batch) and
    the per-element bound."""
    e = e.double()
    n = e.shape[0] - 1
    acc, mag = e[n].clone(), e[n].abs()
    for i in range(n):
        acc = acc + w[i] * (e[i] - e[n])
        mag = mag + abs(w[i]) * (e[i].abs() + e[n].abs())
    if per_batch:
        sd = lambda t: t.std(unbiased=False).expand(t.shape[0], 1)
    else:
        sd = lambda t: t.std(dim=1, unbiased=False, keepdim=True)
    f = phi * sd(e[0]) / sd(acc) + (1 - phi)
    return acc * f, f.reshape(-1), (3 * n + 2) * 2.0 ** -24 * f * mag


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_rescaled_form_matches_float64_and_wrong_variants_do_not(geo, planes):
    n, Bk, per, e = _slots(geo, Bk=max(GEOMETRIES[geo][1], 2), scales=[4.0 ** b for b in range(max(GEOMETRIES[geo][1], 2))])
    w = WEIGHTS[n]
    ed = e.cuda()

    def run(phi, src=ed):
        buf, wd = src.clone(), _wdev(w, phi)
        _launch(planes, eps=buf.data_ptr(), out=buf.data_ptr(), weights=wd.data_ptr(), n=n, B=Bk, per_sample=per, rescale=1)
        assert torch.equal(_bits(buf[1:]), _bits(src[1:]))
        return buf[0].cpu()
    got = run(PHI)
    want, f, bound = _f64(e, w, PHI)
    worst = float(((got.double() - want).abs() / bound).max())
    print(f"{geo} {planes}: rescaled form, worst error / bound {worst:.3f}; f_b {[round(float(v), 4) for v in f]}")
    assert worst <= 1.0
    assert torch.equal(_bits(run(PHI)), _bits(got))                      # two launches, equal bits
    # phi = 1: every sample's output has its e_0's standard deviation; phi = 0: the plain form's bits
    one = run(1.0).double()
    sd_rel = float(((one.std(dim=1, unbiased=False) - e[0].double().std(dim=1, unbiased=False)).abs() / e[0].double().std(dim=1, unbiased=False)).max())
    print(f"{geo} {planes}: phi = 1, output std vs e_0's, worst relative {sd_rel:.2e}")
    assert sd_rel <= 1e-6
    assert torch.equal(_bits(run(0.0)), _bits(_restate(e, w)))
    # the named wrong variants, each at least 10 x over the bound somewhere
    miss = lambda other: float(((got.double() - other).abs() / bound).max())
    wrong = {"slot 0 as the unconditional one": _f64(torch.cat((e[n:], e[1:n], e[:1])), w, PHI)[0],
             "statistics over the whole batch": _f64(e, w, PHI, per_batch=True)[0], "phi ignored": _f64(e, w, 0.0)[0]}
    if n > 1:
        wrong["two weights swapped"] = _f64(e, [w[1], w[0]] + w[2:], PHI)[0]
    for name, other in wrong.items():
        assert miss(other) >= 10, (name, miss(other))
    # ... and, where the variant changes it, the standard deviation check at phi = 1 rejects them by 10 x too
    sd_of = lambda t: t.std(dim=1, unbiased=False)
    for name, other in (("slot 0 as the unconditional one", _f64(torch.cat((e[n:], e[1:n], e[:1])), w, 1.0)[0]),
                        ("statistics over the whole batch", _f64(e, w, 1.0, per_batch=True)[0]), ("phi ignored", _f64(e, w, 0.0)[0])):
        assert float(((sd_of(other) - sd_of(e[0].double())).abs() / sd_of(e[0].double())).max()) >= 1e-5, name


@pytest.mark.gate
@pytest.mark.parametrize("rescale", [0, 1])
def test_an_inf_in_a_read_slot_raises_the_status_bit(rescale):
    from frido_amd import _lib
    e, wd = torch.from_numpy(seeded_normal("guide:inf", (3, 2, 48))).cuda(), _wdev([1.5, -0.75], 0.5)
    out = torch.empty(2, 48, device="cuda")
    kw = dict(eps=e.data_ptr(), out=out.data_ptr(), weights=wd.data_ptr(), n=2, B=2, per_sample=48, rescale=rescale)
    _launch(**kw)
    assert _lib.status_flags(clear=True) == 0
    e[1, 1, 7] = float("inf")
    _launch(**kw)
    assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE


@pytest.mark.gate
def test_a_constant_composition_rescales_by_one():
    """sigma(acc) == 0: f_b = 1."""
    e = torch.ones(2, 2, 48, device="cuda") * torch.tensor([2.0, 0.5], device="cuda").view(2, 1, 1)
    wd, out = _wdev([1.5], 1.0), torch.empty(2, 48, device="cuda")
    _launch(eps=e.data_ptr(), out=out.data_ptr(), weights=wd.data_ptr(), n=1, B=2, per_sample=48, rescale=1)
    assert torch.equal(out, torch.full_like(out, 0.5 + 1.5 * (2.0 - 0.5)))


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
    c, uc, c1, c2 = (torch.from_numpy(seeded_normal(f"guide:{tag}", (B, 5, 64))).cuda() for tag in ("c", "uc", "c1", "c2"))
    return m, c, uc, c1, c2


@pytest.fixture(scope="module")
def label_model():
    m = _frido(AB_SMP_EMB, "adm")
    return m, torch.tensor([1, 7], device="cuda"), torch.tensor([0, 0], device="cuda"), torch.tensor([3, 4], device="cuda"), \
        torch.tensor([5, 2], device="cuda")


def _cls(kind):
    from frido.models.diffusion.ddim import DDIMSampler
    from frido.models.diffusion.plms import PLMSSampler
    from frido.models.diffusion.dpm_solver import DPMSolverSampler
    return dict(ddim=DDIMSampler, plms=PLMSSampler, dpm=DPMSolverSampler)[kind]


def _sample(model, kind, c, uc, scale=SCALE, **kw):
    kw = dict(dict(noise="philox", seed=11, log_every_t=10 ** 9, num_stage=2, verbose=False), **kw)
    return _cls(kind)(model).sample(S=S, batch_size=c.shape[0], shape=SHAPE, conditioning=c, unconditional_guidance_scale=scale,
                                    unconditional_conditioning=uc, **kw)


def _cache(model):
    return model.model.diffusion_model.runtime().__dict__.setdefault("_sampler_engines", {})


def _engines(model, composed=True):
    return [e for e in _cache(model).values() if getattr(e, "composed", False) == composed]


class _Tape:
    def __init__(self, flat):
        self.flat, self.pos = flat, 0

    def __call__(self, shape):
        n = int(np.prod(shape))
        out = torch.from_numpy(self.flat[self.pos:self.pos + n].reshape(shape).copy())
        self.pos += n
        return out


# ---- the loops composed here --------------------------------------------------------------------------------------------------------
def _mix(es, eu, w, phi):
    """Section 1 restated in torch on the GPU: fp32 terms in order; the rescale factor per sample from float64 statistics, rounded once."""
    acc = eu
    for e, wi in zip(es, w):
        acc = acc + torch.tensor(wi, device="cuda") * (e - eu)
    if phi:
        sd = lambda t: t.double().flatten(1).std(dim=1, unbiased=False)
        f = (phi * sd(es[0]) / sd(acc) + (1 - phi)).float().view(-1, 1, 1, 1)
        acc = acc * f
    return acc


def _eps_fn(model, conds, uc, w, phi):
    def eps(x, t_value, s):
        t = torch.full((x.shape[0],), int(t_value), device="cuda", dtype=torch.long)
        return _mix([model.apply_model(x, t, c, stage=s) for c in conds], model.apply_model(x, t, uc, stage=s), w, phi)
    return eps


def _handoff(img, s, num_stage=2):
    c0, c1 = sum(EMBED[:s]), sum(EMBED[:s + 1])
    tmp = img[:, c0:c1].clone()
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.avg_pool2d(tmp, 2, 2)
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.interpolate(tmp, scale_factor=2, mode="nearest")
    img[:, c0:c1] = tmp
    return img


def _x_prev(tab, row, xa, e, nz=None):
    """The DDIM update restated from ddim.py:237-268 on the engine's own float32 table row."""
    a_t, a_prev, sigma, sq1m = (torch.tensor(float(v), device="cuda") for v in tab[row, :4])
    x0 = (xa - sq1m * e) / a_t.sqrt()
    out = a_prev.sqrt() * x0 + (1.0 - a_prev - sigma ** 2).sqrt() * e
    return out + sigma * nz if nz is not None else out


def _loop(model, kind, eps, x_T, eta=0.0, draw=None, k=None):
    """The two-stage loop driven from here: per step eps(x, t, stage) -- apply_model per conditioning and the restated composition --, the
    restated update of `kind` in eager torch fp32, the hand-off.  draw: the tape (x_T first, then per step one (B, e_s, H, W) draw).
    k: only the LAST k rows of every stage, from x_T's channels (DDIMSampler.edit(init="noise"))."""
    from frido_amd import schedules
    if kind == "dpm":
        t_loop, tab = schedules.dpm_solver_table(model.alphas_cumprod.detach().double().cpu().numpy(), S)
    else:
        tab, t_loop = schedules.sampler_coef_table(model.alphas_cumprod.detach().float().cpu().numpy(), S, eta, plms=(kind == "plms"))
    n = len(t_loop)
    rows = range(n - k, n) if k is not None else range(n)
    img = draw((B,) + SHAPE).cuda() if draw is not None else x_T.clone()
    for s in range(2):
        a, e_hi = sum(EMBED[:s]), sum(EMBED[:s + 1])
        x = img[:, :e_hi].clone()
        old, hist = [], None
        for i in rows:
            nz = draw((B, e_hi, 16, 16)).cuda()[:, a:] if draw is not None else None
            e_t = eps(x, t_loop[i], s)
            xa = x[:, a:]
            if kind == "ddim":
                xn = _x_prev(tab, i, xa, e_t, nz)
            elif kind == "dpm":
                inv_alpha, sigma, c_x, c_d, w_cur, w_last = (float(v) for v in tab[i, :6])
                x0 = (xa - sigma * e_t) * inv_alpha
                D = x0 if w_last == 0 else w_cur * x0 + w_last * hist
                xn, hist = c_x * xa + c_d * D, x0
            else:       # plms.py:156-194,285-303
                if not old:
                    x_p = torch.cat((x[:, :a], _x_prev(tab, i, xa, e_t)), dim=1)
                    e_p = (e_t + eps(x_p, t_loop[min(i + 1, n - 1)], s)) / 2
                elif len(old) == 1:
                    e_p = (3 * e_t - old[-1]) / 2
                elif len(old) == 2:
                    e_p = (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
                else:
                    e_p = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
                xn = _x_prev(tab, i, xa, e_p)
                old = (old + [e_t])[-3:]
            x = torch.cat((x[:, :a], xn), dim=1)
        img = torch.cat((_handoff(x, s), img[:, e_hi:]), dim=1)
    return img


CASES = {"ddim_eta0": ("ddim", 0.0), "ddim_eta1": ("ddim", 1.0), "plms": ("plms", 0.0), "dpm": ("dpm", 0.0), "edit": ("edit", 0.0)}


@pytest.mark.parametrize("phi", [0.0, PHI], ids=["plain", "rescale0.7"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_samplers_match_the_loop_composed_from_apply_model(case, phi, ctx_model):
    """compose=[(c1, -0.75), (c2, 0.5)] at scale 1.5, S = 5, two stages, B = 2; the loop with one term dropped and the loop with two
    weights swapped miss the right loop by at least 10 x the bound."""
    model, c, uc, c1, c2 = ctx_model
    kind, eta = CASES[case]
    compose, conds, w = [(c1, W1), (c2, W2)], [c, c1, c2], [SCALE, W1, W2]
    kw, tape, k = dict(compose=compose, guidance_rescale=phi), None, None
    if eta:
        flat = seeded_normal("guide:tape", (B * 6 * 256 * (1 + 2 * S),))
        tape, kw["noise"] = _Tape(flat), _Tape(flat)
    if kind == "edit":
        k = 3
        x_T = torch.from_numpy(seeded_normal("guide:edit:xT", (B,) + SHAPE)).cuda()
        z0 = torch.from_numpy(seeded_normal("guide:edit:z0", (B,) + SHAPE)).cuda()
        got, _ = _cls("ddim")(model).edit(S, z0, c, t_start=k, init="noise", x_T=x_T, eta=0.0, num_stage=2, verbose=False, noise="philox",
                                          seed=11, log_every_t=10 ** 9, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, **kw)
        kind = "ddim"
    else:
        got, inter = _sample(model, kind, c, uc, eta=eta, **kw)
        x_T = inter["x_inter"][0]
    eng = _engines(model)[-1]
    assert eng.composed and eng.ncond == 3 and eng.xrep == 4 and eng.rescale == bool(phi) and torch.isfinite(got).all()
    run = lambda cs, ws: _loop(model, kind, _eps_fn(model, cs, uc, ws, phi), x_T, eta, _Tape(tape.flat) if tape else None, k)
    want = run(conds, w)
    err = _rel(got, want)
    dropped, swapped = _rel(run(conds[:2], w[:2]), want), _rel(run(conds, [w[0], w[2], w[1]]), want)
    print(f"{case} phi {phi}: engine vs its composed loop {err:.3e} (bound {ENGINE_BOUND:.0e}); the loop with c2 dropped {dropped:.3e}, with "
          f"w1 / w2 swapped {swapped:.3e}")
    assert err <= ENGINE_BOUND
    assert dropped >= 10 * ENGINE_BOUND and swapped >= 10 * ENGINE_BOUND


def test_the_same_conditioning_twice_is_the_existing_path_at_the_summed_scale(ctx_model):
    """sample(c, u, scale = s, compose = [(c, a)]) against sample(c, u, scale = s + a): the existing classifier-free path is the oracle."""
    model, c, uc, _, _ = ctx_model
    for kind in ("ddim", "plms", "dpm"):
        old, _ = _sample(model, kind, c, uc, scale=SCALE + 0.5)
        new, _ = _sample(model, kind, c, uc, scale=SCALE, compose=[(c, 0.5)])
        err = _rel(new, old)
        print(f"{kind}: scale 1.5 + compose (c, 0.5) vs the existing path at scale 2.0: {err:.3e} (bound {ENGINE_BOUND:.0e})")
        assert err <= ENGINE_BOUND and not torch.equal(new, _sample(model, kind, c, uc, scale=SCALE)[0])


@pytest.mark.gate
def test_replay_other_weights_and_a_plain_call_in_between(ctx_model):
    """A second run gives the same bits; other weights and another phi replay the same graphs and equal a fresh engine's result bit for
    bit; a call without the keywords returns the bits it returned before the composed calls, from the engine under the key it always had."""
    model, c, uc, c1, c2 = ctx_model
    _cache(model).clear()
    plain_before, _ = _sample(model, "ddim", c, uc)
    assert list(_cache(model)) == [("ddim", B, 6, 16, 16, 5, S, 0.0, True, 2, 1.0, 0)]
    kw = dict(compose=[(c1, W1), (c2, W2)], guidance_rescale=PHI)
    first, _ = _sample(model, "ddim", c, uc, **kw)
    eng, = _engines(model)
    assert list(_cache(model))[-1] == ("ddim", B, 6, 16, 16, 5, S, 0.0, True, 2, 1.0, 0, ("compose", 3, True))
    captures = eng.graph_captures
    from frido_amd import _lib
    mix = _lib.OP_KINDS["FRIDO_OP_GUIDANCE_COMPOSE"]
    assert captures == 2 and all(any(op[0] == mix for op in g.keep[1].ops) for g in eng.graphs.values())
    second, _ = _sample(model, "ddim", c, uc, **kw)
    assert torch.equal(_bits(second), _bits(first)) and eng.graph_captures == captures
    kw2 = dict(compose=[(c1, 0.25), (c2, -1.25)], guidance_rescale=0.3)
    other, _ = _sample(model, "ddim", c, uc, scale=2.5, **kw2)
    assert eng.graph_captures == captures and len(_engines(model)) == 1 and not torch.equal(other, first)
    plain_after, _ = _sample(model, "ddim", c, uc)
    assert torch.equal(_bits(plain_after), _bits(plain_before)) and len(_cache(model)) == 2
    plain_eng, = _engines(model, composed=False)
    assert plain_eng.xrep == 2 and not any(op[0] == mix for g in plain_eng.graphs.values() for op in g.keep[1].ops)
    _cache(model).clear()
    fresh, _ = _sample(model, "ddim", c, uc, scale=2.5, **kw2)
    assert torch.equal(_bits(fresh), _bits(other))


def test_rescale_alone_and_a_unit_scale_are_weights_like_any_other(ctx_model):
    """guidance_rescale without compose (one conditioning, composed engine), and scale 1.0 inside a composition: against the composed loop."""
    model, c, uc, c1, _ = ctx_model
    got, inter = _sample(model, "ddim", c, uc, guidance_rescale=PHI)
    eng = _engines(model)[-1]
    assert eng.ncond == 1 and eng.xrep == 2 and eng.rescale
    err = _rel(got, _loop(model, "ddim", _eps_fn(model, [c], uc, [SCALE], PHI), inter["x_inter"][0]))
    got1, inter1 = _sample(model, "ddim", c, uc, scale=1.0, compose=[(c1, W1)])
    err1 = _rel(got1, _loop(model, "ddim", _eps_fn(model, [c, c1], uc, [1.0, W1], 0.0), inter1["x_inter"][0]))
    print(f"rescale alone vs its composed loop {err:.3e}; scale 1.0 with one extra term {err1:.3e} (bound {ENGINE_BOUND:.0e})")
    assert err <= ENGINE_BOUND and err1 <= ENGINE_BOUND
    assert not torch.equal(got, _sample(model, "ddim", c, uc)[0])


def test_class_labels_compose_through_the_same_code(label_model):
    model, y, uy, y1, y2 = label_model
    got, inter = _sample(model, "ddim", y, uy, compose=[(y1, W1), (y2, W2)], guidance_rescale=PHI)
    eng = _engines(model)[-1]
    assert eng.labels and eng.xrep == 4
    want = _loop(model, "ddim", _eps_fn(model, [y, y1, y2], uy, [SCALE, W1, W2], PHI), inter["x_inter"][0])
    swapped = _loop(model, "ddim", _eps_fn(model, [y, y1, y2], uy, [SCALE, W2, W1], PHI), inter["x_inter"][0])
    err = _rel(got, want)
    print(f"class-conditional AttentionBlock denoiser, labels in compose: engine vs its composed loop {err:.3e}; weights swapped {_rel(swapped, want):.3e}")
    assert err <= ENGINE_BOUND and _rel(swapped, want) >= 10 * ENGINE_BOUND


def test_sample_images_and_edit_images_pass_the_keywords_through(ctx_model):
    from frido_amd.pipeline import edit_images, sample_images
    model, c, uc, c1, c2 = ctx_model
    kw = dict(compose=[(c1, W1), (c2, W2)], guidance_rescale=PHI)
    for sampler, eta in (("ddim", 1.0), ("plms", 0.0), ("dpm", 0.0)):
        img = sample_images(model, c, S=S, sampler=sampler, eta=eta, scale=SCALE, uncond=uc, seed=4, sample0=6, num_stage=2, gather=False, **kw)
        z, _ = _sample(model, sampler, c, uc, eta=eta, seed=4, sample0=6, **kw)
        assert torch.equal(_bits(img), _bits(model.decode_first_stage(z))), sampler
        plain = sample_images(model, c, S=S, sampler=sampler, eta=eta, scale=SCALE, uncond=uc, seed=4, sample0=6, num_stage=2, gather=False)
        assert not torch.equal(img, plain), sampler
    images = torch.from_numpy(seeded_normal("guide:images", (B, 3, 64, 64))).clamp(-1, 1).cuda()
    z0 = model.get_first_stage_encoding(model.encode_first_stage(images))
    out = edit_images(model, images, c, S=S, strength=0.6, eta=0.0, scale=SCALE, uncond=uc, seed=4, num_stage=2, gather=False, **kw)
    z, _ = _cls("ddim")(model).edit(S, z0, c, strength=0.6, eta=0.0, num_stage=2, verbose=False, noise="philox", seed=4, log_every_t=10 ** 9,
                                    unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, **kw)
    assert torch.equal(_bits(out), _bits(model.decode_first_stage(z)))

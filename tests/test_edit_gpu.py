"""DDIM editing on the MI355X: the blend kernel (frido_keep_blend) bit for bit against the torch fp32 expression evaluated op by op on the
CPU, its Philox draws, the reference's own mask / x0 blend (tests/golden/edit_ref.npz, recorded from the reference's DDIMSampler.sample) at
the samplers' bound, the default per-stage semantics against a loop composed in this file, and the exact properties of the engine.

Bound of the composed-loop comparison (EDIT_COMPOSED_BOUND): 10 x the distance between the SAME composed loop without any edit
(apply_model per step + the DDIM update restated in torch + the hand-off) and DDIMSampler.sample on this model (UNET_SMALL, two stages,
S = 6) -- the margin covers the extra blend roundings per step and the eager-versus-captured difference.  That distance is on record for
the commit before editing existed: 8.046e-07 (profiles/dpm_sampling.txt, "DDIM eta 0 S 6 between the same routes", scale 1.0; 1.04e-06
under guidance, which this test does not use).  The test prints the same distance at its own setting (eta = 1, tape noise) next to the
edit's, and tools/edit_step_bench.py copies both lines into profiles/edit_sampling.txt.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_cfg import VQ_SMALL, BERT_SMALL, UNET_SMALL, frido_cfg  # noqa: E402
from attnblock_cfg import AB_SMP_EMB  # noqa: E402
import edit_cfg  # noqa: E402
from helpers import golden  # noqa: E402
from frido_amd.synth import fill_module, seeded_normal  # noqa: E402

SHAPE, B, EMBED = (6, 16, 16), 2, [3, 3]
PLAIN_COMPOSED_ERR = 8.046e-7     # composed loop (apply_model per step + the update in torch) vs DDIMSampler.sample, S = 6, on the commit before: see the module docstring
EDIT_COMPOSED_BOUND = 10 * PLAIN_COMPOSED_ERR


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


# ---- the kernel: tape noise ------------------------------------------------------------------------------------------------------------
def _launch(planes="f16", stream=None, **kw):
    from frido_amd import _lib
    from frido_amd.engine import require_gpu
    with _lib.use_planes(planes):
        require_gpu("cuda")
        d = _lib.STRUCTS["FridoKeepBlend"](**kw)
        _lib.check(_lib.lib().frido_keep_blend(C.byref(d), torch.cuda.current_stream().cuda_stream if stream is None else stream), "frido_keep_blend")
    torch.cuda.synchronize()


def _restate(x, z0, m, n, sa, sb, c0, c1, clean):
    """x' on the CPU in eager elementwise torch fp32 ops, expression for expression (every op rounds on its own):
    q = sa * z0 + sb * n (frido.py:306-307), x' = q * m + (1 - m) * x (ddim.py:161); m None: x' = q; clean: q = z0."""
    q = z0[..., c0:c1] if clean else torch.tensor(sa) * z0[..., c0:c1] + torch.tensor(sb) * n[..., c0:c1]
    out = x.clone()
    out[..., c0:c1] = q if m is None else q * m[..., None] + (1. - m[..., None]) * x[..., c0:c1]
    return out


GEOMETRIES = {"b2_4x4_c6_w36": (2, 16, 6, 3, 6), "b3_5x7_c6_w36": (3, 35, 6, 3, 6), "b3_5x7_c6_w03": (3, 35, 6, 0, 3), "b2_4x4_c9_w36": (2, 16, 9, 3, 6)}
STEP, ROW_OFFSET, ROWS = 2, 1, 5       # the device counter holds 2: coefficients from row 3, tape from row 2


def _mask(kind, Bk, HW, tag):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(Bk, HW)
    u = torch.from_numpy(seeded_normal(f"editk:{tag}:m", (Bk, HW))).sigmoid()
    return (u > 0.5).float() if kind == "binary" else u


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("clean", [0, 1], ids=["noised", "clean"])
@pytest.mark.parametrize("mask", ["soft", "binary", "none", "zero"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_kernel_matches_the_torch_expression_bit_for_bit(geo, mask, clean, planes):
    """Every shape of the issue (210 floats per sample at 5 x 7 x 6: odd sizes, a window at offset 3 and at 0, channels on both sides of
    the window at Cx = 9), soft / binary / absent / all-zero masks, the noised and the clean form, a row offset and a step counter > 0.
    The WHOLE state is compared as bits: channels outside the window keep theirs, and m = 0 leaves x bit-identical."""
    Bk, HW, Cx, c0, c1 = GEOMETRIES[geo]
    f = lambda tag, *shape: torch.from_numpy(seeded_normal(f"editk:{geo}:{tag}", shape))
    x, z0, m = f("x", Bk, HW, Cx), f("z0", Bk, HW, Cx), _mask(mask, Bk, HW, geo)
    x[0, 0, c1 if c1 < Cx else 0] = float("nan")          # outside the window: a NaN there stays where it is and raises nothing (never read)
    tape = f("tape", ROWS, Bk, HW, c1)                                             # the channels reached so far
    qtab = torch.from_numpy(np.stack([np.linspace(0.9, 0.1, ROWS), np.linspace(0.3, 0.95, ROWS)], 1).astype(np.float32))
    sa, sb = float(qtab[STEP + ROW_OFFSET, 0]), float(qtab[STEP + ROW_OFFSET, 1])
    want = _restate(x, z0, m, tape[STEP], sa, sb, c0, c1, clean)
    xd, zd, md, td, qd = x.cuda(), z0.cuda(), None if m is None else m.cuda(), tape.cuda(), qtab.cuda()
    step = torch.full((1,), STEP, dtype=torch.int32, device="cuda")
    kw = dict(x=xd.data_ptr(), z0=zd.data_ptr(), mask=None if md is None else md.data_ptr(), B=Bk, HW=HW, Cx=Cx, c0=c0, c1=c1, clean=clean)
    if not clean:
        kw.update(qtab=qd.data_ptr(), step=step.data_ptr(), row_offset=ROW_OFFSET, noise=td.data_ptr(), noise_stride=Bk * HW * c1, noise_C=c1)
    _launch(planes, **kw)
    assert torch.equal(_bits(xd), _bits(want))
    if mask == "zero":
        assert torch.equal(_bits(xd), _bits(x))
    if mask == "none" and not clean:
        assert not torch.equal(_bits(xd[..., c0:c1]), _bits(x[..., c0:c1]))


def test_nonfinite_result_raises_the_status_bit():
    from frido_amd import _lib
    x, z0, qtab = torch.zeros(1, 16, 6, device="cuda"), torch.zeros(1, 16, 6, device="cuda"), torch.ones(1, 2, device="cuda")
    tape = torch.zeros(1, 1, 16, 6, device="cuda")
    kw = dict(x=x.data_ptr(), z0=z0.data_ptr(), qtab=qtab.data_ptr(), B=1, HW=16, Cx=6, c0=3, c1=6, noise=tape.data_ptr(), noise_C=6, noise_stride=96)
    x[0, 2, 1] = float("inf")            # outside the window: never read
    _launch(**kw)
    assert _lib.status_flags(clear=True) == 0
    z0[0, 3, 4] = float("inf")
    _launch(**kw)
    assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE


# ---- the kernel: Philox ---------------------------------------------------------------------------------------------------------------
def _philox_draws(Bk, HW, Cx, c0, c1, *, seed, sample0, row, stream, rng_dev=False):
    """The kernel's own draws: z0 = 0, {sa, sb} = {0, 1}, no mask -> x' = 0 * 0 + 1 * n = n on the window."""
    x, z0 = torch.full((Bk, HW, Cx), 7.0, device="cuda"), torch.zeros(Bk, HW, Cx, device="cuda")
    qtab = torch.tensor([[0.0, 1.0]] * (row + 1), device="cuda")
    kw = dict(x=x.data_ptr(), z0=z0.data_ptr(), qtab=qtab.data_ptr(), B=Bk, HW=HW, Cx=Cx, c0=c0, c1=c1, row_offset=row, rng_stream=stream)
    if rng_dev:
        rng = torch.tensor([seed, sample0], dtype=torch.int64, device="cuda")
        kw.update(rng_dev=rng.data_ptr(), seed=999, sample0=999)
    else:
        kw.update(seed=seed, sample0=sample0)
    _launch(**kw)
    assert bool((x[..., :c0] == 7.0).all()) and bool((x[..., c1:] == 7.0).all())
    return x[..., c0:c1].clone()


@pytest.mark.gate
def test_philox_draws_depend_on_the_global_sample_only():
    """B = 4 against two B = 2 launches with sample0 = 0, 2: the same (seed, global sample) gives the same bits whatever B and the
    position in the batch are; rng_dev overrides the fields; another seed / row / stream gives other draws."""
    kw = dict(seed=31, row=3, stream=65)
    full = _philox_draws(4, 35, 6, 3, 6, sample0=0, **kw)
    lo, hi = _philox_draws(2, 35, 6, 3, 6, sample0=0, **kw), _philox_draws(2, 35, 6, 3, 6, sample0=2, **kw)
    assert torch.equal(_bits(full), _bits(torch.cat((lo, hi)))) and not torch.equal(lo, hi)
    assert torch.equal(_bits(_philox_draws(2, 35, 6, 3, 6, sample0=2, rng_dev=True, **kw)), _bits(hi))
    # the numbering is the window's: the same draws whatever channels surround it
    assert torch.equal(_bits(_philox_draws(2, 35, 9, 3, 6, sample0=2, **kw)), _bits(hi))
    for other in (dict(kw, seed=32), dict(kw, row=4), dict(kw, stream=64)):
        assert not torch.equal(_philox_draws(2, 35, 6, 3, 6, sample0=2, **other), hi)


@pytest.mark.gate
def test_philox_draws_differ_from_the_ddim_updates():
    """The DDIM update's own draws at the same (seed, sample, row, stage) -- sampler_step_kernel with x = 0, eps = 0 and a coefficient row
    {a_t, a_prev, sigma} = {1, 0, 1}, so that x' = sigma * noise -- against the blend's on stream 64 + stage: other bits; on the update's own
    stream (stage + 1) the blend would repeat them, which is why the engine keeps the streams apart."""
    from frido_amd import runtime
    from frido_amd.engine import Prog, require_gpu
    dev = require_gpu("cuda")
    Bk, HW, stage, row, seed = 2, 35, 1, 3, 31
    x, eps = torch.zeros(Bk, HW, 6, device="cuda"), torch.zeros(Bk, HW, 3, device="cuda")
    coef = torch.zeros(row + 1, 12, device="cuda")
    coef[row, :9] = torch.tensor([1.0, 0, 1.0, 0, 1, 0, 0, 0, 1])
    p = Prog(dev, 2)
    p.emit("FRIDO_OP_SAMPLER_STEP", x=x.data_ptr(), B=Bk, HW=HW, Cx=6, start=3, nch=3, eps_cond=eps.data_ptr(), coef=coef.data_ptr(),
           coef_row_offset=row, x_out=x.data_ptr(), write_x=1, temperature=1.0, seed=seed, sample0=0, rng_stream=stage + 1, cfg_scale=1.0)
    p.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    upd = x[..., 3:6]
    assert float(upd.abs().max()) > 0
    assert runtime.EDIT_RNG_STREAM + stage not in range(0, 2 + 1)
    mine = _philox_draws(Bk, HW, 6, 3, 6, seed=seed, sample0=0, row=row, stream=runtime.EDIT_RNG_STREAM + stage)
    assert not torch.equal(mine, upd) and float((mine - upd).abs().min()) > 0
    assert torch.equal(_bits(_philox_draws(Bk, HW, 6, 3, 6, seed=seed, sample0=0, row=row, stream=stage + 1)), _bits(upd))


@pytest.mark.gate
def test_philox_draws_are_standard_normal():
    """B = 4, 32 x 32, 3 channels: n = 12 288 draws; |mean| <= 4 / sqrt(n) and |var - 1| <= 4 sqrt(2 / n) (four standard errors)."""
    d = _philox_draws(4, 1024, 6, 3, 6, seed=5, sample0=0, row=0, stream=65).double().cpu()
    n = d.numel()
    mean, var = float(d.mean()), float(d.var(unbiased=False))
    print(f"n = {n}: mean {mean:+.4f} (bound {4 / n ** 0.5:.4f}), var - 1 {var - 1:+.4f} (bound {4 * (2 / n) ** 0.5:.4f})")
    assert n == 12288 and abs(mean) <= 4 / n ** 0.5 and abs(var - 1) <= 4 * (2 / n) ** 0.5


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_captured_body_with_the_device_counter_and_rng_equals_eager(planes):
    """[blend, counter add] captured once and replayed three times from row 1: the device counter moves every replay to its own
    coefficient row and Philox draw, rng_dev carries the key; the replay equals the eager run bit for bit, and rows differ."""
    from frido_amd import _lib
    from frido_amd.engine import Prog, require_gpu
    Bk, HW, Cx, c0, c1 = GEOMETRIES["b3_5x7_c6_w36"]
    f = lambda tag, *shape: torch.from_numpy(seeded_normal(f"editk:graph:{tag}", shape)).cuda()
    x_init, z0, m = f("x", Bk, HW, Cx), f("z0", Bk, HW, Cx), f("m", Bk, HW).sigmoid()
    qtab = torch.tensor([[0.9, 0.2], [0.8, 0.4], [0.6, 0.6], [0.3, 0.9]], device="cuda")
    rng = torch.tensor([77, 4], dtype=torch.int64, device="cuda")
    results = []
    with _lib.use_planes(planes):
        dev = require_gpu("cuda")
        for graph in (False, True):
            x, step = x_init.clone(), torch.full((1,), 1, dtype=torch.int32, device="cuda")
            d = _lib.STRUCTS["FridoKeepBlend"](x=x.data_ptr(), z0=z0.data_ptr(), mask=m.data_ptr(), qtab=qtab.data_ptr(), step=step.data_ptr(),
                                                rng_dev=rng.data_ptr(), rng_stream=65, B=Bk, HW=HW, Cx=Cx, c0=c0, c1=c1)
            p = Prog(dev, 2)
            p.ops = [_lib.op_of("FRIDO_OP_KEEP_BLEND", d)]
            p.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=1)
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                g = p.capture(stream.cuda_stream) if graph else None
                for _ in range(3):
                    g.launch(stream.cuda_stream) if graph else p.run(stream.cuda_stream)
            stream.synchronize()
            assert int(step) == 4
            results.append(x)
    assert torch.equal(_bits(results[0]), _bits(results[1])) and torch.isfinite(results[0]).all()
    # the same three rows one by one with the key in the descriptor's fields
    x = x_init.clone()
    for row in (1, 2, 3):
        _launch(planes, x=x.data_ptr(), z0=z0.data_ptr(), mask=m.data_ptr(), qtab=qtab.data_ptr(), row_offset=row, seed=77, sample0=4, rng_stream=65,
                B=Bk, HW=HW, Cx=Cx, c0=c0, c1=c1)
    assert torch.equal(_bits(x), _bits(results[1]))


# ---- models ---------------------------------------------------------------------------------------------------------------------------
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
    c = torch.from_numpy(golden("sampler_small")["c"]).cuda()
    uc = torch.from_numpy(seeded_normal("edit:uc", tuple(c.shape))).cuda()
    return m, c, uc


@pytest.fixture(scope="module")
def label_model():
    m = _frido(AB_SMP_EMB, "adm")
    return m, torch.tensor([1, 7], device="cuda"), torch.tensor([0, 0], device="cuda")


def _sampler(model):
    from frido.models.diffusion.ddim import DDIMSampler
    return DDIMSampler(model)


def _engines(model, kind="ddim"):
    return [e for e in model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).values() if e.kind == kind]


def _clear_engines(model):
    model.model.diffusion_model.runtime().__dict__.get("_sampler_engines", {}).clear()


class _Tape:
    def __init__(self, flat):
        self.t, self.pos = torch.from_numpy(np.asarray(flat, dtype=np.float32)), 0

    def __call__(self, shape):
        n = int(np.prod(shape))
        out = self.t[self.pos:self.pos + n].reshape(shape).clone()
        assert out.numel() == n
        self.pos += n
        return out


def _z0(tag, Bk=B):
    """A latent shaped like an encoded one: the coarse channels [0, 3) constant over 2 x 2 blocks.  Their values are multiples of 2^-8, so
    the hand-off's block mean ((v + v) + v) + v) * 0.25 returns v exactly; with full mantissas 3 v would round, in the reference's
    avg_pool2d as well."""
    z = torch.from_numpy(seeded_normal(f"edit:{tag}", (Bk,) + SHAPE))
    coarse = torch.round(z[:, :3, ::2, ::2] * 256) / 256
    z[:, :3] = coarse.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return z.cuda()


def _keep_mask(tag, Bk=B):
    """(Bk, 1, 16, 16): sample 0 binary (keeps the left half and a 4 x 4 block), the others a soft ramp."""
    m = torch.zeros(Bk, 1, 16, 16)
    m[0, :, :, :8] = 1.0
    m[0, :, 4:8, 10:14] = 1.0
    m[1:] = torch.linspace(0.0, 1.0, 16).reshape(1, 1, 1, 16)
    return m.cuda()


def _edit(model, c, z0, uc=None, scale=1.0, S=6, **kw):
    kw = dict(dict(num_stage=2, verbose=False, noise="philox", seed=11, log_every_t=10 ** 9), **kw)
    return _sampler(model).edit(S, z0, c, unconditional_guidance_scale=scale, unconditional_conditioning=uc if scale != 1.0 else None, **kw)


# ---- pinned to the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.gate
@pytest.mark.parametrize("run", sorted(edit_cfg.RUNS))
def test_reference_form_matches_the_references_own_masked_sampling(run, ctx_model):
    """The reference's DDIMSampler.sample(mask=, x0=, x_T=) on the two-stage model (x_T adopted as stage 0, stage 1 blends all 6 channels
    before every evaluation, ddim.py:158-161), its recorded randn / randn_like tape replayed through edit(): the samplers' 1e-3 bound of
    tests/test_model_gpu.py.  The fixture's own sensitivity (eps perturbed by 1e-6) is at least 10 x under it."""
    g = golden("edit_ref")
    model, c, _ = ctx_model
    eta, kind = edit_cfg.RUNS[run]
    assert float(g[f"{run}_ref_sens"]) < 1e-4
    tape = _Tape(g[f"{run}_noise"])
    x0, x_T, m = (torch.from_numpy(g[k]).cuda() for k in ("x0", "x_T", f"mask_{kind}"))
    out, inter = _edit(model, c, x0, S=edit_cfg.S, t_start=edit_cfg.S, x_T=x_T, first_stage=1, init="noise", blend="reference", reimpose=False,
                       keep_mask=m, noise=tape, eta=eta, log_every_t=2)
    err = _rel(out, g[f"{run}_samples"])
    print(f"{run}: edit(blend='reference') vs the reference's masked DDIM {err:.3e} (fixture sensitivity {float(g[f'{run}_ref_sens']):.2e})")
    assert tape.pos == tape.t.numel() and len(inter["x_inter"]) == int(g[f"{run}_nx"])
    assert err < 1e-3


# ---- the default semantics against a loop composed here ----------------------------------------------------------------------------------
def _handoff(img, s, num_stage=2):
    c0, c1 = sum(EMBED[:s]), sum(EMBED[:s + 1])
    tmp = img[:, c0:c1].clone()
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.avg_pool2d(tmp, 2, 2)
    for _ in range(num_stage - s - 1):
        tmp = torch.nn.functional.interpolate(tmp, scale_factor=2, mode="nearest")
    img[:, c0:c1] = tmp
    return img


def _composed(model, c, draw, S, eta, k=None, z0=None, mask=None, reimpose=True):
    """The two-stage loop driven from here in eager torch on the GPU: per step the blend (edits only), model.apply_model on HIP, the DDIM
    update restated from oracle/samplers.py `_x_prev` (ddim.py:237-268) on the sampler's own float32 schedule, then the hand-off.
    k None: plain sampling from a drawn x_T.  Else the default edit: init 'z0', blend 'stage', the draws in the engine's host order."""
    from frido_amd import runtime, schedules
    ac = model.alphas_cumprod.detach().float().cpu().numpy()
    tab, t_loop = schedules.sampler_coef_table(ac, S, eta)
    n = tab.shape[0]          # the uniform grid has range(0, T, T // S) rows: 7 at S = 6
    k = n if k is None else k
    row0 = n - k
    dev = lambda shape: draw(shape).cuda()
    full = lambda v: torch.full((B, 1, 1, 1), float(v), device="cuda")
    masks = runtime.stage_masks(mask, 2) if mask is not None else None
    img = dev((B,) + SHAPE) if z0 is None else z0.clone()
    for s in range(2):
        a, e = sum(EMBED[:s]), sum(EMBED[:s + 1])
        x = img[:, :e].clone()
        q = lambda row, n: (full(model.sqrt_alphas_cumprod[int(t_loop[row])]) * z0[:, a:e]
                            + full(model.sqrt_one_minus_alphas_cumprod[int(t_loop[row])]) * n[:, a:e])
        if z0 is not None:
            x[:, a:e] = q(row0, dev((B, e, 16, 16)))
        for i in range(k):
            row = row0 + i
            if masks is not None and i > 0:
                x[:, a:e] = q(row, dev((B, e, 16, 16))) * masks[s] + (1. - masks[s]) * x[:, a:e]
            nz = dev((B, e, 16, 16))
            t = torch.full((B,), int(t_loop[row]), device="cuda", dtype=torch.long)
            e_t = model.apply_model(x, t, c, stage=s)
            a_t, a_prev, sigma, sq1m = (full(v) for v in tab[row, :4])
            xa = x[:, a:e]
            pred_x0 = (xa - sq1m * e_t) / a_t.sqrt()
            x = torch.cat((x[:, :a], a_prev.sqrt() * pred_x0 + (1. - a_prev - sigma ** 2).sqrt() * e_t + sigma * nz[:, a:e] * 1.0), dim=1)
        if masks is not None and reimpose:
            x[:, a:e] = z0[:, a:e] * masks[s] + (1. - masks[s]) * x[:, a:e]
        img = torch.cat((_handoff(x, s), img[:, e:]), dim=1)
    return img


def test_default_edit_matches_the_loop_composed_from_apply_model(ctx_model):
    """Two stages, S = 6, k = 4, eta = 1, tape noise, a soft + binary keep mask, reimpose: within EDIT_COMPOSED_BOUND = 10 x the distance
    between the same composed loop WITHOUT an edit and DDIMSampler.sample (also measured here, for the record)."""
    model, c, _ = ctx_model
    flat = seeded_normal("edit:composed:noise", (40 * B * 6 * 256,))
    plain, _ = _sampler(model).sample(S=6, batch_size=B, shape=SHAPE, conditioning=c, num_stage=2, eta=1.0, verbose=False, noise=_Tape(flat),
                                      log_every_t=10 ** 9)
    base = _rel(plain, _composed(model, c, _Tape(flat), 6, 1.0))
    z0, m = _z0("composed:z0"), _keep_mask("composed")
    t1, t2 = _Tape(flat), _Tape(flat)
    out, _ = _edit(model, c, z0, t_start=4, keep_mask=m, eta=1.0, noise=t1)
    want = _composed(model, c, t2, 6, 1.0, k=4, z0=z0, mask=m)
    err = _rel(out, want)
    print(f"plain composed loop vs DDIMSampler.sample (eta 1, tape) {base:.3e} (on record, eta 0: {PLAIN_COMPOSED_ERR:.3e}); edit k = 4 vs its composed "
          f"loop {err:.3e} (bound {EDIT_COMPOSED_BOUND:.3e})")
    assert t1.pos == t2.pos
    assert err <= EDIT_COMPOSED_BOUND


# ---- exact properties --------------------------------------------------------------------------------------------------------------------
class _Interleaved:
    """sample()'s tape for an edit from noise: x_T first, then per step the blend's draw (taken from `junk`) before the update's."""

    def __init__(self, base, junk):
        self.base, self.junk, self.calls = base, junk, 0

    def __call__(self, shape):
        self.calls += 1
        return self.junk(shape) if self.calls > 1 and self.calls % 2 == 0 else self.base(shape)


@pytest.mark.gate
@pytest.mark.parametrize("noise", ["tape", "philox"])
def test_an_all_zero_mask_from_noise_is_sample_bit_for_bit(noise, ctx_model):
    """keep_mask = 0 everywhere, init 'noise', k = S: every blend is q * 0 + (1 - 0) * x = x, so the edit is sample() with the same tape
    (the blend draws are taken and thrown away) and with the same Philox seed.  S = 5 divides the model's 1000 timesteps, so the grid has
    exactly S rows and k = S is the whole chain."""
    model, c, _ = ctx_model
    flat, junk = seeded_normal("edit:zero:noise", (14 * B * 6 * 256,)), seeded_normal("edit:zero:junk", (14 * B * 6 * 256,))
    src = (lambda: _Tape(flat)) if noise == "tape" else (lambda: "philox")
    want, winter = _sampler(model).sample(S=5, batch_size=B, shape=SHAPE, conditioning=c, num_stage=2, eta=1.0, verbose=False, noise=src(),
                                          seed=11, log_every_t=2)
    n_e = _Interleaved(_Tape(flat), _Tape(junk)) if noise == "tape" else "philox"
    z0 = _z0("zero:z0")
    got, ginter = _edit(model, c, z0, S=5, t_start=5, init="noise", keep_mask=torch.zeros(B, 1, 16, 16, device="cuda"), reimpose=False, eta=1.0,
                        noise=n_e, log_every_t=2)
    assert torch.equal(_bits(got), _bits(want))
    assert len(ginter["x_inter"]) == len(winter["x_inter"]) and all(torch.equal(a, b) for a, b in zip(ginter["x_inter"], winter["x_inter"]))


def test_keeping_everything_returns_z0_exactly(ctx_model):
    """keep_mask = 1, reimpose: after each stage z0 * 1 + (1 - 1) * x = z0 goes back, and the hand-off's block mean of the block-constant
    coarse channels is z0 again."""
    model, c, _ = ctx_model
    z0 = _z0("keepall:z0")
    out, _ = _edit(model, c, z0, strength=0.7, keep_mask=torch.ones(B, 1, 16, 16, device="cuda"), eta=1.0)
    assert torch.equal(out, z0)
    moved, _ = _edit(model, c, z0, strength=0.7, eta=1.0)
    assert not torch.equal(moved, z0) and torch.isfinite(moved).all()


def test_a_stage_1_edit_keeps_stage_0s_bits_and_counts_its_steps(ctx_model):
    """first_stage = 1: channels [0, 3) come back with z0's bits, with and without a mask; k steps per stage that runs: callbacks,
    img_callback shapes and the intermediates (index 3, 2, 0 of k = 4 are logged at log_every_t = 2)."""
    model, c, _ = ctx_model
    z0, m = _z0("stage1:z0"), _keep_mask("stage1")
    for mask in (None, m):
        seen = []
        out, inter = _edit(model, c, z0, t_start=4, first_stage=1, keep_mask=mask, eta=1.0, callback=seen.append, log_every_t=2)
        assert torch.equal(_bits(out[:, :3]), _bits(z0[:, :3])) and not torch.equal(out[:, 3:], z0[:, 3:])
        assert seen == list(range(4)) and len(inter["x_inter"]) == 1 + 3 and len(inter["pred_x0"]) == 1 + 3
    seen, imgs = [], []
    out, inter = _edit(model, c, z0, t_start=4, keep_mask=m, eta=1.0, callback=seen.append, img_callback=lambda p0, i: imgs.append((i, tuple(p0.shape))),
                       log_every_t=2)
    assert seen == list(range(4)) * 2 and [i for i, _ in imgs] == seen and imgs[0][1] == (B, 3, 16, 16) and imgs[-1][1] == (B, 6, 16, 16)
    assert len(inter["x_inter"]) == 1 + 2 * 3 and torch.equal(inter["x_inter"][0], z0)


def test_a_chain_longer_than_one_graph_unit_equals_single_steps(ctx_model):
    """S = 24, k = 23 with a mask from z0: step 0 runs the plain body, the 22 steps left are one 20-step unit and two single steps; a
    callback forces single steps -- the same bits."""
    model, c, _ = ctx_model
    _clear_engines(model)
    z0, m = _z0("long:z0"), _keep_mask("long")
    out, _ = _edit(model, c, z0, S=24, t_start=23, keep_mask=m, eta=1.0)
    eng, = _engines(model)
    assert eng.multi_step_launches >= 1 and ("edit", 0, "x20") in eng.graphs and ("edit", 1, "x20") in eng.graphs
    launches = eng.multi_step_launches
    single, _ = _edit(model, c, z0, S=24, t_start=23, keep_mask=m, eta=1.0, callback=lambda i: None)
    assert eng.multi_step_launches == launches and torch.equal(_bits(single), _bits(out)) and torch.isfinite(out).all()


def test_a_second_call_captures_nothing_new_and_equals_a_fresh_engine(ctx_model):
    """z0, the masks, the seed, sample0 and the start row are device state or fixed buffers: other values replay the same graphs."""
    model, c, _ = ctx_model
    _clear_engines(model)
    z1, m1 = _z0("again:z1"), _keep_mask("again")
    z2, m2 = _z0("again:z2"), _keep_mask("again").flip(-1).contiguous()
    first, _ = _edit(model, c, z1, t_start=4, keep_mask=m1, eta=1.0, seed=3)
    eng, = _engines(model)
    captures = eng.graph_captures
    second, _ = _edit(model, c, z2, t_start=3, keep_mask=m2, eta=1.0, seed=4, sample0=6)
    assert eng.graph_captures == captures and len(_engines(model)) == 1
    _clear_engines(model)
    fresh, _ = _edit(model, c, z2, t_start=3, keep_mask=m2, eta=1.0, seed=4, sample0=6)
    assert torch.equal(_bits(second), _bits(fresh)) and not torch.equal(second, first)
    _clear_engines(model)
    again, _ = _edit(model, c, z1, t_start=4, keep_mask=m1, eta=1.0, seed=3)
    assert torch.equal(_bits(again), _bits(first))


def test_a_batch_of_four_equals_two_batches_of_two_under_philox(ctx_model):
    model, c, _ = ctx_model
    c4 = torch.cat((c, torch.from_numpy(seeded_normal("edit:c2", tuple(c.shape))).cuda()))
    z4, m4 = _z0("b4:z0", 4), _keep_mask("b4", 4)
    kw = dict(t_start=4, eta=1.0, seed=9)
    full, _ = _edit(model, c4, z4, keep_mask=m4, **kw)
    lo, _ = _edit(model, c4[:2], z4[:2], keep_mask=m4[:2], sample0=0, **kw)
    hi, _ = _edit(model, c4[2:], z4[2:], keep_mask=m4[2:], sample0=2, **kw)
    assert torch.equal(_bits(full), _bits(torch.cat((lo, hi))))
    assert not torch.equal(hi, _edit(model, c4[2:], z4[2:], keep_mask=m4[2:], sample0=0, **kw)[0])


def test_guidance_and_a_class_label_model_run_and_stay_finite(ctx_model, label_model):
    model, c, uc = ctx_model
    z0, m = _z0("cfg:z0"), _keep_mask("cfg")
    plain, _ = _edit(model, c, z0, t_start=4, keep_mask=m, eta=1.0)
    guided, _ = _edit(model, c, z0, uc, 2.0, t_start=4, keep_mask=m, eta=1.0)
    assert torch.isfinite(guided).all() and not torch.equal(guided, plain)
    lm, y, uy = label_model
    out, _ = _edit(lm, y, z0, t_start=4, keep_mask=m, eta=1.0)
    out_g, _ = _edit(lm, y, z0, uy, 2.0, t_start=4, keep_mask=m, eta=1.0)
    assert out.shape == z0.shape and torch.isfinite(out).all() and torch.isfinite(out_g).all() and not torch.equal(out, out_g)
    # everything kept under the binary half of the mask came back with z0's bits (reimpose)
    keep = (m[0, 0] == 1.0)
    assert torch.equal(out[0, 3:][:, keep], z0[0, 3:][:, keep])


def test_edit_images_with_everything_kept_is_the_plain_reconstruction(ctx_model):
    from frido_amd.pipeline import edit_images
    model, c, _ = ctx_model
    images = torch.from_numpy(seeded_normal("edit:images", (B, 3, 64, 64))).clamp(-1, 1).cuda()
    rec = model.decode_first_stage(model.get_first_stage_encoding(model.encode_first_stage(images)))
    kept = edit_images(model, images, c, S=6, strength=0.7, keep_mask=torch.ones(B, 1, 64, 64, device="cuda"), seed=2, gather=False)
    assert kept.shape == rec.shape == (B, 3, 64, 64) and torch.equal(kept, rec)
    edited = edit_images(model, images, c, S=6, strength=0.7, seed=2, gather=False)
    assert torch.isfinite(edited).all() and not torch.equal(edited, rec)
    # sharded: four images as one batch and as two shards keyed by the global sample index
    im4, c4 = torch.cat((images, images.flip(-1))), torch.cat((c, c.flip(0)))
    half = torch.ones(4, 1, 64, 64, device="cuda")
    half[..., 32:] = 0
    kw = dict(S=6, strength=0.7, seed=2, gather=False)
    lo = edit_images(model, im4[:2], c4[:2], keep_mask=half[:2], sample0=0, **kw)
    hi = edit_images(model, im4[2:], c4[2:], keep_mask=half[2:], sample0=2, **kw)
    both = edit_images(model, im4, c4, keep_mask=half, **kw)
    assert torch.equal(both, torch.cat((lo, hi)))
    with pytest.raises(ValueError, match="keep_mask must be"):
        edit_images(model, images, c, S=6, strength=0.7, keep_mask=torch.ones(B, 1, 16, 16, device="cuda"))

"""The small fp32 kernels of the sampling loop (csrc/misc.hip, the row normalisation of csrc/norm.hip) on the MI355X, each launched directly
against a plain statement of its operation: the DDIM / PLMS update on every path of its descriptor (explicit history, the device ring,
hist_mode 3, cfg_dev, write_x = 0, x_out aliasing x, a non-zero step counter, more pixels than the launch has threads), the stage hand-off
on a channel slice of a non-square plane, and TIME_EMB / CONVT / PLACE / RELAYOUT / EMBED / L2NORM / COPY / FILL / TO_U8.

References are float64 statements on the kernel's own fp32 inputs (or exact fp32 / integer operations, compared with torch.equal).  Where a
comparison has a tolerance, named WRONG variants of the operation are evaluated on the host from the same data and must lie at least 10x
outside it (_tells_apart), so that a bound which could not see a near miss fails here rather than pass quietly.  Buffers around every
written range hold a sentinel.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frido_amd.synth import seeded_normal  # noqa: E402

SENTINEL = -777.25
STEP_TOL = 2e-6          # tests/test_kernels_gpu.py::test_sampler_step_and_handoff_match_oracle: absolute, on unit-normal data


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _builder():
    from frido_amd.builder import Builder
    return Builder(_dev(), 2, {})


def _run(b):
    b.prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _t(tag, *shape):
    return torch.from_numpy(seeded_normal("small:" + tag, shape))


def _tells_apart(got, wrong, tol, what):
    """Every wrong variant lies >= 10x outside the bound `tol` (scalar or per-element tensor) on the same data."""
    got = got.double()
    for name, w in wrong.items():
        far = float(((got - w.double()).abs() / tol).max())
        assert far >= 10.0, (what, name, f"only {far:.1f}x the bound away: the bound would not see it")


# ---- the DDIM / PLMS update ------------------------------------------------------------------------------------------------------------
PLMS = {0: ([1.0], 1.0), 1: ([3.0, -1.0], 2.0), 2: ([23.0, -16.0, 5.0], 12.0), 3: ([55.0, -59.0, 37.0, -9.0], 24.0)}      # plms.py:285-301


def _row(a_t, a_prev, sigma, nhist, junk=5.0):
    """One 12-float coefficient row {a_t, a_prev, sigma, sqrt(1 - a_t), ab0..3, den, pad}: the Adams-Bashforth weights of `nhist` older
    eps; the weights of history the kernel must NOT read hold `junk`, so a history pointer switched on too early shows."""
    ab, den = PLMS[nhist]
    ab = ab + [junk] * (4 - len(ab))
    return [a_t, a_prev, sigma, float(np.sqrt(np.float32(1.0) - np.float32(a_t))), *ab, den, 0.0, 0.0, 0.0]


def _step_ref(x, e_c, e_u, cfg, hist, row, start, noise=None, temperature=1.0):
    """float64 statement of the update on fp32 inputs (NHWC; ddim.py:211-268, plms.py:285-301): CFG mix, Adams-Bashforth combine with the
    older eps in `hist` (newest first), x0 and x' on channels [start, start + nch), frozen channels passed through.
    -> (x', x0, mixed eps), the first two with all Cx channels."""
    cf = torch.as_tensor(row, dtype=torch.float32).double()
    a_t, a_prev, sigma, sq1m, den = cf[0], cf[1], cf[2], cf[3], cf[8]
    e = e_c.double()
    if e_u is not None:
        e = e_u.double() + float(np.float32(cfg)) * (e - e_u.double())
    mixed = e
    if hist:
        acc = cf[4] * e
        for k, h in enumerate(hist):
            acc = acc + cf[5 + k] * h.double()
        e = acc / den
    nch = e.shape[-1]
    xa = x[..., start:start + nch].double()
    x0a = (xa - sq1m * e) / a_t.sqrt()
    xpa = a_prev.sqrt() * x0a + (1.0 - a_prev - sigma * sigma).sqrt() * e
    if noise is not None:
        xpa = xpa + sigma * noise.double() * temperature
    x0, xp = x.double().clone(), x.double().clone()
    x0[..., start:start + nch] = x0a
    xp[..., start:start + nch] = xpa
    return xp, x0, mixed


def _err(got, ref):
    return float((got.double() - ref).abs().max())


@pytest.mark.parametrize("nhist", [1, 2, 3])
def test_sampler_step_explicit_history(nhist):
    """hist1..3 / ab0..3 / den, with CFG, eps_out, pred_x0, a noise tape indexed by the device step counter (step 2, coef_row_offset 1: row 3
    of the table, tape entry 2) and x_out apart from x.  Data: unit normal; row a_t 0.95, a_prev 0.97, sigma 0.1 (late in a run, where the
    combined eps -- up to ~15 here, the weights 55 -59 37 -9 over 24 on independent histories -- enters x0 with sqrt(1 - a_t) / sqrt(a_t) =
    0.23: the combine's roundings, ~2^-24 * 100 * sqrt(7) / 24 = 7e-7 in e, then stay under STEP_TOL in x0 and x')."""
    B, HW, start, nch = 2, 61, 2, 4
    Cx, N = start + nch, B * HW * nch
    x, e_c, e_u = _t("eh:x", B, HW, Cx), _t("eh:ec", B, HW, nch), _t("eh:eu", B, HW, nch)
    hist = [_t(f"eh:h{k}", B, HW, nch) for k in range(3)]
    tape = _t("eh:tape", 4, B, HW, nch)
    cfg, step0, off = 1.5, 2, 1
    table = torch.tensor([_row(0.5, 0.4, 0.3, 0)] * 3 + [_row(0.95, 0.97, 0.1, nhist)] + [_row(0.5, 0.4, 0.3, 0)], dtype=torch.float32)
    xd, ecd, eud, taped, coef = x.cuda(), e_c.cuda(), e_u.cuda(), tape.cuda(), table.cuda()
    hd = [h.cuda() for h in hist]
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    xo, x0, eo = (torch.full(s, SENTINEL, device="cuda") for s in ((B, HW, Cx), (B, HW, Cx), (N + 8,)))
    b = _builder()
    b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=ecd.data_ptr(),
                eps_uncond=eud.data_ptr(), cfg_scale=cfg, eps_out=eo.data_ptr(), hist1=hd[0].data_ptr(),
                hist2=hd[1].data_ptr() if nhist >= 2 else None, hist3=hd[2].data_ptr() if nhist >= 3 else None,
                coef=coef.data_ptr(), step=step.data_ptr(), coef_row_offset=off, noise=taped.data_ptr(), noise_stride=N, noise_C=nch,
                noise_c0=0, temperature=0.75, x_out=xo.data_ptr(), pred_x0=x0.data_ptr(), write_x=1)
    _run(b)
    row = table[step0 + off]
    ref = lambda h: _step_ref(x, e_c, e_u, cfg, h, row, start, tape[step0], 0.75)
    xp_ref, x0_ref, mixed = ref(hist[:nhist])
    errs = _err(xo.cpu(), xp_ref), _err(x0.cpu(), x0_ref), _err(eo[:N].cpu().view(B, HW, nch), mixed)
    print(f"explicit history {nhist}: |x' - ref| {errs[0]:.2e}, |x0 - ref| {errs[1]:.2e}, |eps_out - mixed| {errs[2]:.2e} (bound {STEP_TOL:.0e})")
    assert max(errs) < STEP_TOL, errs
    assert torch.equal(xd.cpu(), x) and bool((eo[N:] == SENTINEL).all())                       # x itself is read only; eps_out ends at N
    assert torch.equal(xo.cpu()[..., :start], x[..., :start]) and torch.equal(x0.cpu()[..., :start], x[..., :start])
    wrong = {1: {"no combine": ref([])[0], "tape entry 0": _step_ref(x, e_c, e_u, cfg, hist[:1], row, start, tape[0], 0.75)[0]},
             2: {"hist1 / hist2 swapped": ref([hist[1], hist[0]])[0], "hist2 ignored": ref(hist[:1])[0]},
             3: {"hist2 / hist3 swapped": ref([hist[0], hist[2], hist[1]])[0], "hist3 ignored": ref(hist[:2])[0]}}[nhist]
    _tells_apart(xo.cpu(), wrong, STEP_TOL, f"explicit history {nhist}")


def test_sampler_step_history_ring_over_six_steps():
    """hist_mode 1 driven by FRIDO_OP_STEP_ADD over steps 0..5: the (CFG-mixed) eps of step i goes to slot i & 3, so slots 0 and 1 are
    written twice, and min(i, 3) older slots are combined: h2 and h3 switch on at steps 2 and 3 (the rows of steps 0..2 hold junk in the
    weights of history that must not be read yet).  x is updated in place (x_out aliases x) with a noise tape indexed by the counter.
    Each step is checked on its own: the reference takes the state as the device held it before the step and the older eps as the device
    stored them when they were new (each checked against the float64 mix at that time), so nothing accumulates against STEP_TOL and the
    reference never asks the kernel which slot is which.  Then hist_mode 3 at the counter of step 5: eps is combined with slot 5 & 3 by
    ab0 / ab1 alone, and the ring must not change."""
    B, HW, start, nch = 2, 37, 2, 3
    Cx, N, steps = start + nch, B * HW * nch, 6
    stride = N + 6
    x0_host = _t("ring:x", B, HW, Cx)
    e_c, e_u, tape = _t("ring:ec", steps + 1, B, HW, nch), _t("ring:eu", steps + 1, B, HW, nch), _t("ring:tape", steps, B, HW, nch)
    cfg = 1.5
    table = torch.tensor([_row(0.93 + 0.008 * i, 0.938 + 0.008 * i, 0.05, min(i, 3)) for i in range(steps)], dtype=torch.float32)
    xd, ecd, eud, taped, coef = x0_host.cuda(), e_c.cuda(), e_u.cuda(), tape.cuda(), table.cuda()
    ring = torch.full((4, stride), SENTINEL, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    stored = []

    def launch(i, mode, add):
        b = _builder()
        b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=ecd[i].data_ptr(),
                    eps_uncond=eud[i].data_ptr(), cfg_scale=cfg, coef=coef.data_ptr(), step=step.data_ptr(), noise=taped.data_ptr(),
                    noise_stride=N, noise_C=nch, noise_c0=0, temperature=1.0, x_out=xd.data_ptr(), write_x=1,
                    hist_ring=ring.data_ptr(), hist_stride=stride, hist_mode=mode)
        if add:
            b.prog.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=add)
        _run(b)

    worst = 0.0
    for i in range(steps):
        x_before, ring_before = xd.cpu(), ring.cpu()
        launch(i, 1, 1)
        assert int(step.item()) == i + 1
        ring_now = ring.cpu()
        older = stored[::-1][:3]                                                            # newest first: steps i-1, i-2, i-3
        xp_ref, _, mixed = _step_ref(x_before, e_c[i], e_u[i], cfg, older, table[i], start, tape[i])
        new = ring_now[i & 3, :N].view(B, HW, nch)
        e_err, x_err = _err(new, mixed), _err(xd.cpu(), xp_ref)
        worst = max(worst, e_err, x_err)
        print(f"ring step {i}: |slot - mixed| {e_err:.2e}, |x' - ref| {x_err:.2e} (bound {STEP_TOL:.0e})")
        assert e_err < STEP_TOL and x_err < STEP_TOL, (i, e_err, x_err)
        keep = [s for s in range(4) if s != (i & 3)]
        assert torch.equal(ring_now[keep], ring_before[keep]) and bool((ring_now[:, N:] == SENTINEL).all()), i
        assert torch.equal(xd.cpu()[..., :start], x0_host[..., :start])
        stored.append(new.clone())
        if i >= 1:      # the ring read one slot off: h_k from step i - k + 1 (h1 = this step's own eps) -- and history switched on late
            off_by_one = _step_ref(x_before, e_c[i], e_u[i], cfg, stored[::-1][:min(i, 3)], table[i], start, tape[i])[0]
            late = _step_ref(x_before, e_c[i], e_u[i], cfg, older[:-1], table[i], start, tape[i])[0]
            _tells_apart(xd.cpu(), {"ring offset by one slot": off_by_one, "oldest slot not read": late}, STEP_TOL, f"ring step {i}")
    # hist_mode 3 (second half of the Heun-style first step) at the counter of step 5
    b = _builder()
    b.prog.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=-1)
    _run(b)
    assert int(step.item()) == steps - 1
    x_before, ring_before = xd.cpu(), ring.cpu()
    launch(steps, 3, 0)
    i = steps - 1
    xp_ref, _, _ = _step_ref(x_before, e_c[steps], e_u[steps], cfg, [stored[i]], table[i], start, tape[i])
    x_err = _err(xd.cpu(), xp_ref)
    print(f"ring hist_mode 3: |x' - ref| {x_err:.2e}")
    assert x_err < STEP_TOL and torch.equal(ring.cpu(), ring_before) and int(step.item()) == i
    wrong = {"combined with the slot before": _step_ref(x_before, e_c[steps], e_u[steps], cfg, [stored[i - 1]], table[i], start, tape[i])[0],
             "older slots read too": _step_ref(x_before, e_c[steps], e_u[steps], cfg, stored[::-1][:3], table[i], start, tape[i])[0]}
    _tells_apart(xd.cpu(), wrong, STEP_TOL, "ring hist_mode 3")


def test_sampler_step_cfg_dev_and_write_x_zero():
    """write_x = 0: only pred_x0 and eps_out are produced, x is not touched and no x_out is needed; the device guidance scale (2.5)
    overrides the descriptor's (1.0).  One older eps, so pred_x0 is the x0 of the COMBINED eps while eps_out is the mixed one."""
    B, HW, start, nch = 2, 37, 3, 3
    Cx, N = start + nch, B * HW * nch
    x, e_c, e_u, h1 = _t("w0:x", B, HW, Cx), _t("w0:ec", B, HW, nch), _t("w0:eu", B, HW, nch), _t("w0:h", B, HW, nch)
    row = _row(0.9, 0.93, 0.1, 1)
    xd, ecd, eud, hd = x.cuda(), e_c.cuda(), e_u.cuda(), h1.cuda()
    coef = torch.tensor([row], dtype=torch.float32, device="cuda")
    cfg_dev = torch.tensor([2.5], dtype=torch.float32, device="cuda")
    x0, eo = torch.full((B, HW, Cx), SENTINEL, device="cuda"), torch.full((N,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=ecd.data_ptr(),
                eps_uncond=eud.data_ptr(), cfg_scale=1.0, cfg_dev=cfg_dev.data_ptr(), eps_out=eo.data_ptr(), hist1=hd.data_ptr(),
                coef=coef.data_ptr(), temperature=1.0, pred_x0=x0.data_ptr(), write_x=0)
    _run(b)
    _, x0_ref, mixed = _step_ref(x, e_c, e_u, 2.5, [h1], row, start)
    errs = _err(x0.cpu(), x0_ref), _err(eo.cpu().view(B, HW, nch), mixed)
    print(f"write_x = 0 / cfg_dev: |x0 - ref| {errs[0]:.2e}, |eps_out - mixed| {errs[1]:.2e}")
    assert max(errs) < STEP_TOL and torch.equal(xd.cpu(), x)
    _tells_apart(x0.cpu(), {"cfg_scale field used": _step_ref(x, e_c, e_u, 1.0, [h1], row, start)[1]}, STEP_TOL, "cfg_dev")


def test_sampler_step_more_pixels_than_threads():
    """B * HW = 600002 pixels > 2048 * 256 (the launch's grid cap): the second trip of the pixel loop, Cx = nch = 3 with x updated in place
    from a noise tape.  Plain eps (no mix, no history), so that the 1.8e6 elements' extremes (|x| ~ 5) are not amplified: an output is
    about ten fp32 roundings (the products, sums and the fp32 square roots of a_t, a_prev) of values that reach 8 only in the far tail
    (2.4e-7 each there, 1.2e-7 below 4), which keeps the worst of them under the sampler tests' STEP_TOL.  Wrong variants held 10x outside
    it: the second trip skipped (pixels from 2048 * 256 on left equal to x), the noise not added; the second trip's pixels are also
    compared on their own."""
    B, HW, C = 2, 300001, 3
    x, e, nz = _t("big:x", B, HW, C), _t("big:e", B, HW, C), _t("big:n", B, HW, C)
    row = _row(0.9, 0.93, 0.1, 0)
    xd, ed, nd = x.cuda(), e.cuda(), nz.cuda()
    coef = torch.tensor([row], dtype=torch.float32, device="cuda")
    x0 = torch.empty_like(xd)
    b = _builder()
    b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=HW, Cx=C, start=0, nch=C, eps_cond=ed.data_ptr(), coef=coef.data_ptr(),
                noise=nd.data_ptr(), noise_stride=0, noise_C=C, noise_c0=0, temperature=1.0, x_out=xd.data_ptr(), pred_x0=x0.data_ptr(),
                write_x=1)
    _run(b)
    xp_ref, x0_ref, _ = _step_ref(x, e, None, 1.0, [], row, 0, nz)
    errs = _err(xd.cpu(), xp_ref), _err(x0.cpu(), x0_ref)
    print(f"600002 pixels: |x' - ref| {errs[0]:.2e}, |x0 - ref| {errs[1]:.2e}")
    assert max(errs) < STEP_TOL, errs
    assert torch.equal(ed.cpu(), e) and torch.equal(nd.cpu(), nz)
    skipped = xp_ref.clone().view(B * HW, C)
    skipped[2048 * 256:] = x.double().view(B * HW, C)[2048 * 256:]
    wrong = {"second trip skipped (pixels from 2048 * 256 on left as x)": skipped.view(B, HW, C),
             "noise not added": _step_ref(x, e, None, 1.0, [], row, 0, None)[0]}
    _tells_apart(xd.cpu(), wrong, STEP_TOL, "600002 pixels")
    tail = xd.cpu().view(B * HW, C)[2048 * 256:]                    # and the second trip on its own, not hidden in a maximum over all
    assert _err(tail, xp_ref.view(B * HW, C)[2048 * 256:]) < STEP_TOL and not torch.equal(tail, x.view(B * HW, C)[2048 * 256:])


# ---- stage hand-off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2])
def test_handoff_channel_slice_of_a_non_square_plane(levels):
    """Channels [3, 7) of 9 on an 8 x 12 plane: 2 x 2 and 4 x 4 block means (avg_pool2d `levels` times, nearest expand) in float64 at the
    existing test's 1e-6; the channels outside the slice keep their bits."""
    B, H, W, Cx, c0, c1 = 2, 8, 12, 9, 3, 7
    img = _t("ho:x", B, H, W, Cx)
    d = img.cuda()
    b = _builder()
    b.prog.emit("FRIDO_OP_HANDOFF", x=d.data_ptr(), B=B, H=H, W=W, Cx=Cx, c0=c0, c1=c1, levels=levels)
    _run(b)
    got = d.cpu()
    t = img[..., c0:c1].double().permute(0, 3, 1, 2)
    for _ in range(levels):
        t = F.avg_pool2d(t, 2, 2)
    ref = F.interpolate(t, scale_factor=2 ** levels, mode="nearest").permute(0, 2, 3, 1)
    assert _err(got[..., c0:c1], ref) < 1e-6
    assert torch.equal(got[..., :c0], img[..., :c0]) and torch.equal(got[..., c1:], img[..., c1:])
    bs = 2 ** levels          # W-major blocks (H and W exchanged in the block walk) would average other pixels
    tw = img[..., c0:c1].double().reshape(B, H * W // (bs * bs), bs * bs, c1 - c0).mean(2, keepdim=True).expand(-1, -1, bs * bs, -1)
    _tells_apart(got[..., c0:c1], {"blocks of the flat pixel index": tw.reshape(B, H, W, c1 - c0)}, 1e-6, f"handoff levels {levels}")


# ---- timestep embedding ----------------------------------------------------------------------------------------------------------------
def _time_emb_ref(t, dim, max_period, variant=None):
    """The kernel's fp32 steps mirrored in numpy float32 with exp / cos / sin in float64 -> (out float64 [n][dim], tolerance [n][dim]).

    Tolerance, from the fp32 rounding of the phase a = t * f_k, f_k = exp(arg_k), arg_k = -ln(max_period) * k / half: expf is good to an
    ulp (2^-23 f_k) and f_k, then a, are rounded (2 * 2^-24), so |a - a_ref| <= |a| 2^-22, and cos / sin move by no more than the phase
    does; cosf / sinf themselves add a few ulp of a value <= 1: 4 * 2^-24.
        tol = (|t| f_k + 1) * 2^-22       (2.4e-4 at t = 999, k = 0; 2.4e-7 at t = 0)
    This takes logf(max_period) as the correctly rounded fp32 logarithm, which the mirror uses: a device logf one ulp off would move
    arg_k by 2^-23 |arg_k| and ask for |arg_k| + 1 in place of 1 in the first term.  It is not granted here."""
    half = dim // 2
    neg_log = -np.float32(np.log(np.float64(np.float32(max_period))))
    k = np.arange(half, dtype=np.float32)
    arg = (neg_log * k) / np.float32(max(half - 1, 1) if variant == "half-1" else half)
    assert arg.dtype == np.float32
    f = np.exp(arg.astype(np.float64)).astype(np.float32)
    a = (np.asarray(t, dtype=np.float32)[:, None] * f[None, :]).astype(np.float32)
    c, s = np.cos(a.astype(np.float64)), np.sin(a.astype(np.float64))
    out = np.zeros((len(t), dim))
    out[:, :half], out[:, half:2 * half] = (s, c) if variant == "swap" else (c, s)
    tol = np.full((len(t), dim), 2.0 ** -22)
    ta = (np.abs(a.astype(np.float64)) + 1.0) * 2.0 ** -22
    tol[:, :half], tol[:, half:2 * half] = ta, ta
    return torch.from_numpy(out), torch.from_numpy(tol)


@pytest.mark.parametrize("dim", [2, 8, 7, 192])
def test_time_emb(dim):
    """t in {0, 1, 500, 999} (int64), max_period 10000; the odd dim has a zero last column.  Per-element tolerance: _time_emb_ref (the fp32
    rounding of the phase, (|t| f_k + 1) 2^-22).  Wrong variants: k / (half - 1) in the frequency table, sin and cos exchanged.
    Measured on the MI355X, worst |got - ref| / tol: 0.061 (dim 2), 0.097 (dim 8), 0.111 (dim 7), 0.405 (dim 192); printed by the test."""
    t = [0, 1, 500, 999]
    td = torch.tensor(t, dtype=torch.int64, device="cuda")
    pad = torch.full((len(t) * dim + 4,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_TIME_EMB", t=td.data_ptr(), n=len(t), dim=dim, max_period=10000.0, out=pad.data_ptr())
    _run(b)
    assert bool((pad[len(t) * dim:] == SENTINEL).all())
    got = pad[:len(t) * dim].view(len(t), dim).cpu()
    ref, tol = _time_emb_ref(t, dim, 10000.0)
    ratio = float(((got.double() - ref).abs() / tol).max())
    print(f"time_emb dim {dim}: worst |got - ref| / tol {ratio:.3f}, max abs err {float((got.double() - ref).abs().max()):.2e}")
    assert ratio <= 1.0
    if dim & 1:
        assert bool((got[:, dim - 1] == 0).all())
    wrong = {"sin / cos swapped": _time_emb_ref(t, dim, 10000.0, "swap")[0]}
    if dim // 2 > 1:            # with one frequency (k = 0, f = 1) the divisor does not enter
        wrong["k / (half - 1)"] = _time_emb_ref(t, dim, 10000.0, "half-1")[0]
    _tells_apart(got, wrong, tol, f"time_emb dim {dim}")


# ---- transposed convolution ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,h,w,Cin,Cout", [(2, 3, 5, 3, 4), (1, 1, 1, 4, 3), (2, 8, 8, 8, 8)])
def test_convt(B, h, w, Cin, Cout, bias):
    """ConvTranspose2d(k = 4, stride 2, padding 1) against F.conv_transpose2d in float64.  An output sums at most 4 Cin products (2 x 2 of
    the 16 taps land on it) and the bias in one fma chain: |err| <= (4 Cin + 1) 2^-24 sum |terms|, the sum from the same convolution of
    the absolute values.  Wrong variants: padding 0 (outputs one pixel off), a flipped kernel."""
    x, wt = _t("ct:x", B, Cin, h, w), _t("ct:w", Cin, Cout, 4, 4) / np.sqrt(4.0 * Cin)
    bs = _t("ct:b", Cout) if bias else None
    xd, wd = x.permute(0, 2, 3, 1).contiguous().cuda(), wt.cuda()
    bd = bs.cuda() if bias else None
    n = B * 2 * h * 2 * w * Cout
    out = torch.full((n + 4,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_CONVT", src=xd.data_ptr(), dst=out.data_ptr(), weight=wd.data_ptr(), bias=bd.data_ptr() if bias else None,
                B=B, h=h, w=w, Cin=Cin, Cout=Cout)
    _run(b)
    assert bool((out[n:] == SENTINEL).all())
    got = out[:n].view(B, 2 * h, 2 * w, Cout).cpu().permute(0, 3, 1, 2)
    bd64 = bs.double() if bias else None
    ref = F.conv_transpose2d(x.double(), wt.double(), bd64, stride=2, padding=1)
    mag = F.conv_transpose2d(x.double().abs(), wt.double().abs(), bd64.abs() if bias else None, stride=2, padding=1)
    tol = (4 * Cin + 1) * 2.0 ** -24 * mag
    ratio = float(((got.double() - ref).abs() / tol).max())
    print(f"convt {(B, h, w, Cin, Cout)} bias {bias}: worst |got - ref| / tol {ratio:.3f}")
    assert ratio <= 1.0
    wrong = {"padding 0": F.conv_transpose2d(x.double(), wt.double(), bd64, stride=2, padding=0)[..., :2 * h, :2 * w],
             "flipped kernel": F.conv_transpose2d(x.double(), wt.double().flip(2, 3), bd64, stride=2, padding=1)}
    _tells_apart(got, wrong, tol, "convt")


# ---- PLACE / RELAYOUT / EMBED: exact data movement ---------------------------------------------------------------------------------------
def _place_ref(x, c0, Cuse, Cdst, d0, up, scale):
    B, h, w, _ = x.shape
    ref = torch.full((B, Cdst, h << up, w << up), SENTINEL)
    v = x[..., c0:c0 + Cuse].permute(0, 3, 1, 2)
    ref[:, d0:d0 + Cuse] = v.repeat_interleave(1 << up, 2).repeat_interleave(1 << up, 3) * scale
    return ref


@pytest.mark.parametrize("up", [0, 1, 2])
def test_place(up):
    """Nearest 2^up up-sampling of an NHWC channel slice into an NCHW channel slice, scaled by 0.5 (exact): bit-equal, and the other
    channels of dst keep the sentinel."""
    B, h, w, Csrc, c0, Cuse, Cdst, d0 = 2, 3, 5, 7, 2, 3, 6, 1
    x = _t("pl:x", B, h, w, Csrc)
    xd = x.cuda()
    dst = torch.full((B, Cdst, h << up, w << up), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_PLACE", src=xd.data_ptr(), dst=dst.data_ptr(), B=B, h=h, w=w, Csrc=Csrc, c0=c0, Cuse=Cuse, Cdst=Cdst, d0=d0,
                up_shift=up, scale=0.5)
    _run(b)
    assert torch.equal(dst.cpu(), _place_ref(x, c0, Cuse, Cdst, d0, up, 0.5))


def test_place_second_trip_of_the_grid_stride_loop():
    """3 * (4 * 211) * (4 * 209) = 2116752 outputs > 8192 * 256: the launch's threads each take a second element."""
    B, h, w, Csrc, c0, Cuse, Cdst, d0, up = 1, 211, 209, 4, 1, 3, 5, 1, 2
    assert B * Cuse * (h << up) * (w << up) > 8192 * 256
    x = _t("pl2:x", B, h, w, Csrc)
    xd = x.cuda()
    dst = torch.full((B, Cdst, h << up, w << up), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_PLACE", src=xd.data_ptr(), dst=dst.data_ptr(), B=B, h=h, w=w, Csrc=Csrc, c0=c0, Cuse=Cuse, Cdst=Cdst, d0=d0,
                up_shift=up, scale=0.5)
    _run(b)
    assert torch.equal(dst.cpu(), _place_ref(x, c0, Cuse, Cdst, d0, up, 0.5))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_relayout_channel_slice(mode):
    """A proper slice on both sides (c0 = 2, Cuse = 3 of Csrc = 7 -> d0 = 1 of Cdst = 6), odd HW.  mode 0: NCHW -> NHWC, 1: NHWC -> NCHW,
    2: NHWC -> NHWC column block.  Bit-equal inside the slice, sentinel outside."""
    B, HW, Csrc, c0, Cuse, Cdst, d0 = 2, 35, 7, 2, 3, 6, 1
    if mode == 0:
        x = _t("rl:x", B, Csrc, HW)
        ref = torch.full((B, HW, Cdst), SENTINEL)
        ref[..., d0:d0 + Cuse] = x[:, c0:c0 + Cuse].permute(0, 2, 1)
    else:
        x = _t("rl:x", B, HW, Csrc)
        if mode == 1:
            ref = torch.full((B, Cdst, HW), SENTINEL)
            ref[:, d0:d0 + Cuse] = x[..., c0:c0 + Cuse].permute(0, 2, 1)
        else:
            ref = torch.full((B, HW, Cdst), SENTINEL)
            ref[..., d0:d0 + Cuse] = x[..., c0:c0 + Cuse]
    xd = x.cuda()
    dst = torch.full(tuple(ref.shape), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_RELAYOUT", src=xd.data_ptr(), dst=dst.data_ptr(), B=B, HW=HW, Csrc=Csrc, c0=c0, Cuse=Cuse, Cdst=Cdst, d0=d0,
                to_nchw=mode)
    _run(b)
    assert torch.equal(dst.cpu(), ref)


@pytest.mark.parametrize("D", [4, 64])
@pytest.mark.parametrize("with_pos", [True, False])
def test_embed(D, with_pos):
    """out[r] = tok[clamp(tokens[r], 0, vocab - 1)] + pos[r % n]: tokens below 0 and at / above vocab clamp, three sequences of n = 5 share
    the position table; bit-equal to the fp32 add (or to the plain gather without pos)."""
    n, nseq, vocab = 5, 3, 11
    rows = n * nseq
    tokens = torch.tensor([0, 10, -1, 11, 3, -(2 ** 40), 2 ** 40, 7, 7, 1, 100, -3, 5, 9, 10], dtype=torch.int64)
    tok, pos = _t("em:tok", vocab, D), _t("em:pos", n, D)
    td, tokd, posd = tokens.cuda(), tok.cuda(), pos.cuda()
    out = torch.full((rows * D + 4,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_EMBED", tokens=td.data_ptr(), tok=tokd.data_ptr(), pos=posd.data_ptr() if with_pos else None,
                out=out.data_ptr(), rows=rows, n=n, D=D, vocab=vocab)
    _run(b)
    ref = tok[tokens.clamp(0, vocab - 1)]
    if with_pos:
        ref = ref + pos[torch.arange(rows) % n]
    assert torch.equal(out[:rows * D].cpu().view(rows, D), ref) and bool((out[rows * D:] == SENTINEL).all())


# ---- row L2 normalisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 5, 7])
@pytest.mark.parametrize("C", [1, 63, 65, 512, 768])
def test_l2norm(rows, C):
    """x / ||x||_2 per row (one wave per row, four rows per workgroup: 5 and 7 rows leave a partly filled workgroup) in float64.  The sum
    of squares takes ceil(C / 64) fused steps per lane and 6 butterfly steps, each rounding a partial sum no larger than the total: it is
    off by at most (ceil(C / 64) + 6) 2^-24 of itself, the inverse root by half of that, plus sqrtf and the division (an ulp, 2^-23, each
    where they are not correctly rounded) and the final product (2^-24):  |err| <= ((ceil(C / 64) + 6) / 2 + 5) 2^-24 |ref|."""
    x = _t("l2:x", rows, C) * 3 + 0.5
    xd = x.cuda()
    out = torch.full((rows * C + 4,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_L2NORM", x=xd.data_ptr(), out=out.data_ptr(), rows=rows, C=C)
    _run(b)
    got = out[:rows * C].cpu().view(rows, C)
    assert bool((out[rows * C:] == SENTINEL).all())
    ref = x.double() / x.double().pow(2).sum(1, keepdim=True).sqrt()
    tol = (((C + 63) // 64 + 6) / 2 + 5) * 2.0 ** -24 * ref.abs()
    ratio = float(((got.double() - ref).abs() / tol.clamp_min(1e-300)).max())
    print(f"l2norm rows {rows} C {C}: worst |got - ref| / tol {ratio:.3f}")
    assert ratio <= 1.0
    wrong = {"normalised by the sum of squares": x.double() / x.double().pow(2).sum(1, keepdim=True)}
    if C > 1:                   # (with one column there is no norm without the last column)
        wrong["last column left out of the norm"] = x.double() / x.double()[:, :-1].pow(2).sum(1, keepdim=True).sqrt()
    _tells_apart(got, wrong, tol.clamp_min(1e-300), f"l2norm C {C}")


# ---- COPY / FILL / TO_U8 -------------------------------------------------------------------------------------------------------------------
def _bytes(tag, n):
    return torch.from_numpy(seeded_normal("small:" + tag, ((n + 3) // 4,))).view(torch.uint8)[:n].clone()


@pytest.mark.parametrize("n", [16, 2048 * 256 * 16 + 48])
def test_copy(n):
    """n bytes, 16-byte units: one unit, and three units more than the launch's 2048 * 256 threads move in their first trip.  Byte-equal
    inside, the 16 bytes before and after keep their pattern."""
    src = _bytes(f"cp{n}", n)
    sd = src.cuda()
    dst = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_COPY", src=sd.data_ptr(), dst=dst.data_ptr() + 16, n=n)
    _run(b)
    got = dst.cpu()
    assert torch.equal(got[16:16 + n], src)
    assert bool((got[:16] == 0xA5).all()) and bool((got[16 + n:] == 0xA5).all())


@pytest.mark.parametrize("n", [1, 7, 8192 * 256 + 5])
def test_fill(n):
    """n 32-bit words of a pattern from a 4-byte-aligned (not 16-byte-aligned) start; three words before and after keep theirs."""
    value, keep = 0xDEADBEEF, 0x01234567
    buf = torch.full((n + 6,), keep, dtype=torch.int32, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_FILL", dst=buf.data_ptr() + 12, n=n, value=value)
    _run(b)
    got = buf.cpu()
    assert bool((got[3:3 + n] == value - 2 ** 32).all())
    assert bool((got[:3] == keep).all()) and bool((got[3 + n:] == keep).all())


def test_to_u8():
    """((x + 1) * 127.5) clamped to [0, 255] and truncated, in fp32 like the statement in torch: every truncation boundary k / 127.5 - 1
    with its two fp32 neighbours, values below -1 and above 1, signed zero.  Equal to the torch expression on the same fp32 values."""
    k = torch.arange(0, 257, dtype=torch.float64)
    edge = (k / 127.5 - 1.0).float()
    inf = torch.tensor(float("inf"))
    vals = torch.cat([edge, torch.nextafter(edge, inf), torch.nextafter(edge, -inf),
                      torch.tensor([-2.0, -1.5, -1.0000001, -1.0, -0.0, 0.0, 1.0, 1.0000001, 1.5, 2.0, 1e30, -1e30, 0.9999999, -0.9999999])])
    ref = ((vals + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    assert int(ref.min()) == 0 and int(ref.max()) == 255 and len(ref.unique()) == 256
    vd = vals.cuda()
    n = vals.numel()
    out = torch.full((n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_TO_U8", src=vd.data_ptr(), dst=out.data_ptr(), n=n)
    _run(b)
    got = out.cpu()
    assert torch.equal(got[:n], ref), (vals[got[:n] != ref], got[:n][got[:n] != ref], ref[got[:n] != ref])
    assert bool((got[n:] == 0xA5).all())

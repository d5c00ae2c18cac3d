"""The noise generator on the MI355X against an independent host reference (tests/philox_ref.py: Philox4x32-10 in plain integers, whose
rounds reproduce the published known answers in tests/test_philox_host.py; fp32 uniforms as csrc/philox.h forms them; float64 log / sqrt /
sin / cos).  frido_randn anchors every other "Philox" test of the suite (the ancestral, edit and loss kernels are compared with it); this
file anchors frido_randn, and the draws inside sampler_step_kernel, whose numbering (grp = p * ngrp + g, draw = step + coef_row_offset + 1)
nothing else states independently.

The bound.  What separates the kernel from the reference is the error of the device's logf, sqrtf, sincosf and the rounding of r * cos:
MEASURED on the MI355X over every comparison of this file (311029 values): worst |got - ref| / max(1, |ref|) = 2.181e-07 (worst absolute
error 4.70e-07, worst relative error 2.31e-07 among |v| > 1e-3).  NOISE_BOUND = 4 x that figure = 8.72e-07, scaled by max(1, |v|) -- 4x
because the device functions are not correctly rounded and other words hit other arguments; the ceiling it may never exceed is 2e-5.
Under `pytest -s` the module prints its worst figures after its last test, next to the recorded one.
An error in the integer part moves values by O(1): each comparison also evaluates two wrong generators on the host (nine rounds; grp and
draw exchanged) and asserts that they lie at least 10x outside the bound on the same data.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import philox_ref as P  # noqa: E402
from frido_amd.synth import seeded_normal  # noqa: E402

NOISE_MEASURED = 2.181e-07                       # worst |got - ref| / max(1, |ref|) measured on the MI355X (module docstring)
NOISE_BOUND = 4 * NOISE_MEASURED
assert NOISE_BOUND <= 2e-5                       # the ceiling the bound may never exceed
SENTINEL = -777.25

_WORST = {"scaled": 0.0, "abs": 0.0, "rel": 0.0, "n": 0}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _builder():
    from frido_amd.builder import Builder
    return Builder(_dev(), 2, {})


def _run(b):
    b.prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _scaled_err(got, ref):
    """max |got - ref| / max(1, |ref|) of float64 arrays, recording the module's worst figures (printed at the end)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    e = float((d / np.maximum(1.0, np.abs(ref))).max())
    _WORST["scaled"] = max(_WORST["scaled"], e)
    _WORST["abs"] = max(_WORST["abs"], float(d.max()))
    big = np.abs(ref) > 1e-3
    if big.any():
        _WORST["rel"] = max(_WORST["rel"], float((d[big] / np.abs(ref[big])).max()))
    _WORST["n"] += got.size
    return e


def _check_noise(got, ref, wrong, what):
    """got within NOISE_BOUND of ref; finite and inside the Box-Muller range; every wrong variant >= 10x outside the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    assert float(np.abs(got).max()) <= P.VMAX * (1 + 2.0 ** -22), (what, float(np.abs(got).max()))    # fp32 sqrtf / product on top of 6.6604
    e = _scaled_err(got, ref)
    print(f"noise {what}: scaled err {e:.3e} (bound {NOISE_BOUND:.1e})")
    assert e <= NOISE_BOUND, (what, e)
    for name, w in wrong.items():
        d = np.abs(got - w) / np.maximum(1.0, np.abs(w))
        assert float(d.max()) >= 10 * NOISE_BOUND and float(np.median(d)) >= 10 * NOISE_BOUND, (what, name, "not told apart")


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the module's worst figures after its last test (visible with `pytest -s`)."""
    yield
    if _WORST["n"]:
        print(f"\ntest_philox_gpu: {_WORST['n']} values, worst |got - ref| / max(1, |ref|) {_WORST['scaled']:.3e} "
              f"(recorded {NOISE_MEASURED:.2e}, bound {NOISE_BOUND:.2e}), worst abs {_WORST['abs']:.3e}, "
              f"worst rel on |v| > 1e-3 {_WORST['rel']:.3e}")


# ---- frido_randn ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1234, 2 ** 32 + 5, 2 ** 64 - 1])
def test_randn_matches_host_reference(seed):
    """Every (sample0, rng_stream, per_sample) of {0, 3, 2^32 + 1} x {0, 1, 65} x {4, 12, 4096} under one seed, 27 launches of one program.
    sample0 = 2^32 + 1 puts a bit into the counter's high sample word, where stream << 20 is folded in.  Each launch covers two whole
    samples and 6 floats of a third (n = 2 per_sample + 6, not a multiple of 4): the last group is partial, and the floats after n keep
    a sentinel.  Measured on the MI355X: worst |got - ref| / max(1, |ref|) 1.98e-07 over the four seeds; bound NOISE_BOUND = 8.72e-07
    (4 x the module's worst measured figure, 2.181e-07)."""
    cases = [(s0, st, per) for s0 in (0, 3, 2 ** 32 + 1) for st in (0, 1, 65) for per in (4, 12, 4096)]
    b = _builder()
    bufs = []
    for s0, st, per in cases:
        n = 2 * per + 6
        buf = torch.full((n + 10,), SENTINEL, device="cuda")
        bufs.append(buf)
        b.prog.emit("FRIDO_OP_RANDN", dst=buf.data_ptr(), n=n, per_sample=per, seed=seed, sample0=s0, rng_stream=st)
    _run(b)
    for (s0, st, per), buf in zip(cases, bufs):
        n = 2 * per + 6
        got = buf.cpu().numpy()
        assert (got[n:] == np.float32(SENTINEL)).all(), ("wrote past n", s0, st, per)
        groups = np.arange((n + 3) // 4)
        ref = P.randn_fill(seed, s0, st, per, groups).reshape(-1)[:n]
        wrong = {"nine rounds": P.randn_fill(seed, s0, st, per, groups, rounds=9).reshape(-1)[:n],
                 "grp / draw swapped": P.randn_fill(seed, s0, st, per, groups, swap_grp_draw=True).reshape(-1)[:n]}
        if per == 4:            # draw 0 and the only group 0 exchange to the same counter: no such variant at this size
            del wrong["grp / draw swapped"]
        _check_noise(got[:n], ref, wrong, f"seed {seed} sample0 {s0} stream {st} per_sample {per}")


def test_randn_streams_samples_and_seeds_are_distinct_keys():
    """The key fields are all live: changing any one of seed lo / seed hi / sample lo / sample hi / stream changes the draw (the same
    launches as above would also pass a kernel that ignored a field the REFERENCE ignores; the reference's layout is pinned on the host,
    this pins that the five fields do not collide with each other in the cases used here)."""
    keys = [(1234, 3, 0), (1235, 3, 0), (1234 + 2 ** 32, 3, 0), (1234, 4, 0), (1234, 3 + 2 ** 32, 0), (1234, 3, 1), (1234, 3 + (1 << 52), 0)]
    b = _builder()
    out = torch.empty(len(keys), 64, device="cuda")
    for i, (seed, s0, st) in enumerate(keys):
        b.prog.emit("FRIDO_OP_RANDN", dst=out[i].data_ptr(), n=64, per_sample=64, seed=seed, sample0=s0, rng_stream=st)
    _run(b)
    got = out.cpu().numpy()
    for i, (seed, s0, st) in enumerate(keys):
        g = np.arange(16)
        wrong = {"nine rounds": P.randn_fill(seed, s0, st, 64, g, rounds=9).reshape(-1),
                 "grp / draw swapped": P.randn_fill(seed, s0, st, 64, g, swap_grp_draw=True).reshape(-1)}
        _check_noise(got[i], P.randn_fill(seed, s0, st, 64, g).reshape(-1), wrong, f"key {keys[i]}")
    # Deliberate documentation of the layout, not a wish: the stream is folded into the counter's high sample word as stream << 20, so
    # stream 1 at sample 3 and stream 0 at sample 3 + 2^52 are the SAME counter (hi = 1 << 20).  Sample indices stay far below 2^52, so
    # the collision is out of reach; if the layout is ever changed to remove it, this line (and philox_ref.counter) change with it.
    assert np.array_equal(got[5], got[6])
    for i in range(5):
        for j in range(i + 1, 6):
            assert np.abs(got[i] - got[j]).max() > 1.0, (keys[i], keys[j])


def test_randn_second_trip_of_the_grid_stride_loop():
    """More groups than the launch has threads (the grid is capped at 8192 blocks of 256): 8192 * 256 + 1000 whole groups and a partial one.
    Every value is checked for range on the device; a strided subset (every 997th group, which walks through every residue of the
    group-in-sample index), the groups either side of the first trip's end and the tail are compared with the reference.  Measured on
    the MI355X: worst |got - ref| / max(1, |ref|) 2.181e-07 over the 12019 values compared (the module's worst); bound NOISE_BOUND = 8.72e-07."""
    per = 4096
    first_trip = 8192 * 256
    n = 4 * (first_trip + 1000) + 3
    buf = torch.full((n + 5,), SENTINEL, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_RANDN", dst=buf.data_ptr(), n=n, per_sample=per, seed=2 ** 32 + 5, sample0=3, rng_stream=1)
    _run(b)
    body = buf[:n]
    assert bool(torch.isfinite(body).all()) and float(body.abs().max()) <= P.VMAX * (1 + 2.0 ** -22)
    assert bool((buf[n:] == SENTINEL).all())
    ngroups = (n + 3) // 4
    groups = np.unique(np.concatenate([np.arange(0, ngroups, 997), np.arange(first_trip - 300, first_trip + 300),
                                       np.arange(ngroups - 300, ngroups)]))
    idx = (groups[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
    keep = idx < n
    got = body[torch.from_numpy(idx[keep]).cuda()].cpu().numpy()
    kw = dict(seed=2 ** 32 + 5, sample0=3, stream=1, per_sample=per, groups=groups)
    ref = P.randn_fill(**kw).reshape(-1)[keep]
    wrong = {"nine rounds": P.randn_fill(**kw, rounds=9).reshape(-1)[keep],
             "grp / draw swapped": P.randn_fill(**kw, swap_grp_draw=True).reshape(-1)[keep]}
    _check_noise(got, ref, wrong, f"second trip, {len(groups)} of {ngroups} groups")
    v = body.double()
    assert abs(float(v.mean())) < 0.005 and abs(float(v.std()) - 1.0) < 0.005          # 8.4e6 draws: sigma of the mean 3.5e-4


# ---- the draws inside sampler_step_kernel --------------------------------------------------------------------------------------------
STEP0, OFFSET = 2, 3                             # device step counter and coef_row_offset: row 5 of the table, draw 6
NOISE_ROW = [0.5, 0.0, 1.0, float(np.sqrt(np.float32(0.5))), 1, 0, 0, 0, 1, 0, 0, 0]      # a_t, a_prev, sigma: x' = noise when x = eps = 0


def _coef_table(row, at=STEP0 + OFFSET, rows=8):
    """A coefficient table whose every OTHER row would give something else (sigma 0.3 on a_prev 0.6), so a wrong row index shows."""
    t = torch.tensor([[0.9, 0.6, 0.3, float(np.sqrt(0.1)), 1, 0, 0, 0, 1, 0, 0, 0]] * rows, dtype=torch.float32)
    t[at] = torch.tensor(row, dtype=torch.float32)
    return t.cuda()


def _noise_launch(nch, start, B, HW, *, seed, sample0, stream, temperature=1.0, rng_dev=None, row=NOISE_ROW, x=None, eps=None):
    Cx = start + nch
    xd = (torch.zeros(B, HW, Cx) if x is None else x).cuda()
    ed = (torch.zeros(B, HW, nch) if eps is None else eps).cuda()
    out = torch.full((B, HW, Cx), SENTINEL, device="cuda")
    coef = _coef_table(row)
    step = torch.full((1,), STEP0, dtype=torch.int32, device="cuda")
    b = _builder()
    b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=ed.data_ptr(),
                coef=coef.data_ptr(), step=step.data_ptr(), coef_row_offset=OFFSET, seed=seed, sample0=sample0, rng_stream=stream,
                rng_dev=rng_dev.data_ptr() if rng_dev is not None else None, temperature=temperature, x_out=out.data_ptr(), write_x=1)
    _run(b)
    assert int(step.item()) == STEP0
    return out.cpu()


@pytest.mark.parametrize("nch", [3, 4, 6, 12])
def test_sampler_step_draws_match_host_reference(nch):
    """x = eps = 0 on the active channels and the row {a_t 0.5, a_prev 0, sigma 1}: x' IS the in-kernel draw (sqrt(a_prev) x0 = 0,
    sqrt(1 - 0 - 1) e = 0, 1 * noise * 1 exact).  Two frozen channels in front (start = 2) carry data and must come back as they were; the
    device step counter holds 2 and coef_row_offset is 3, so the row is 5 and the draw 6; B = 2 samples from sample0 = 2^32 + 1 on stream
    65, HW = 37 pixels.  ngrp = ceil(nch / 4) = 1, 1, 2, 3 groups per pixel, the last one partial for nch = 3 and 6.  Measured on the
    MI355X: worst |got - ref| / max(1, |ref|) 1.53e-07 (nch 12); bound NOISE_BOUND = 8.72e-07, the one measured for frido_randn."""
    B, HW, start = 2, 37, 2
    seed, s0, st = 2 ** 64 - 1, 2 ** 32 + 1, 65
    x = torch.zeros(B, HW, start + nch)
    x[..., :start] = torch.from_numpy(seeded_normal("phx:frozen", (B, HW, start)))
    out = _noise_launch(nch, start, B, HW, seed=seed, sample0=s0, stream=st, x=x)
    assert torch.equal(out[..., :start], x[..., :start])
    draw = STEP0 + OFFSET + 1
    ref = P.sampler_noise(seed, s0, st, draw, B, HW, nch)
    wrong = {"nine rounds": P.sampler_noise(seed, s0, st, draw, B, HW, nch, rounds=9),
             "grp / draw swapped": P.sampler_noise(seed, s0, st, draw, B, HW, nch, swap_grp_draw=True),
             "draw = step + offset (no + 1)": P.sampler_noise(seed, s0, st, draw - 1, B, HW, nch)}
    ngrp = (nch + 3) // 4
    if ngrp > 1:                # groups numbered p + g instead of p * ngrp + g (the same thing when a pixel has one group)
        smp = s0 + np.arange(B)[:, None, None]
        v = P.randn4(seed, smp, draw, st, np.arange(HW)[None, :, None] + np.arange(ngrp)[None, None, :])
        wrong["grp = p + g"] = v.reshape(B, HW, ngrp * 4)[..., :nch]
    _check_noise(out[..., start:].numpy(), ref, wrong, f"sampler_step nch {nch}")
    # the device key {seed, sample0} overrides the descriptor's fields and gives the same bits as the fields did
    rng = torch.tensor([seed - 2 ** 64, s0], dtype=torch.int64, device="cuda")          # uint64 seed as the int64 holding its bits
    out_dev = _noise_launch(nch, start, B, HW, seed=99, sample0=7, stream=st, rng_dev=rng, x=x)
    assert torch.equal(out_dev, out)
    # temperature scales the draw: 1 * noise * 0.5 is exact in fp32
    out_t = _noise_launch(nch, start, B, HW, seed=seed, sample0=s0, stream=st, temperature=0.5, x=x)
    assert torch.equal(out_t[..., start:], out[..., start:] * 0.5) and torch.equal(out_t[..., :start], x[..., :start])


def test_sampler_step_sigma_zero_row_draws_nothing():
    """A row with sigma = 0 leaves x' equal to the noise-free update sqrt(a_prev) x0 + sqrt(1 - a_prev) e, x0 = (x - sqrt(1 - a_t) e) /
    sqrt(a_t), here in float64 on unit-normal x and eps at the sampler test's 2e-6 -- and bit-equal whatever the key and temperature.
    Wrong variants held 10x outside the 2e-6: a_t and a_prev exchanged, eps not subtracted in x0."""
    B, HW, start, nch = 2, 37, 2, 6
    a_t, a_prev = 0.5, 0.7
    row = [a_t, a_prev, 0.0, float(np.sqrt(np.float32(1 - a_t))), 1, 0, 0, 0, 1, 0, 0, 0]
    x = torch.from_numpy(seeded_normal("phx:x", (B, HW, start + nch)))
    eps = torch.from_numpy(seeded_normal("phx:e", (B, HW, nch)))
    out = _noise_launch(nch, start, B, HW, seed=5, sample0=0, stream=0, row=row, x=x, eps=eps)
    cf = torch.tensor(row, dtype=torch.float32).double()
    x0 = (x[..., start:].double() - cf[3] * eps.double()) / cf[0].sqrt()
    ref = cf[1].sqrt() * x0 + (1 - cf[1]).sqrt() * eps.double()
    err = float((out[..., start:].double() - ref).abs().max())
    print(f"sigma = 0 row: max abs err {err:.2e}")
    assert err < 2e-6 and torch.equal(out[..., :start], x[..., :start])
    # wrong variants, at least 10x outside the 2e-6 on the same data: a_t and a_prev exchanged; eps not subtracted in x0
    x0_swap = (x[..., start:].double() - (1 - cf[1]).sqrt() * eps.double()) / cf[1].sqrt()
    wrong = {"a_t / a_prev exchanged": cf[0].sqrt() * x0_swap + (1 - cf[0]).sqrt() * eps.double(),
             "eps not subtracted": cf[1].sqrt() * (x[..., start:].double() / cf[0].sqrt()) + (1 - cf[1]).sqrt() * eps.double()}
    for name, w in wrong.items():
        far = float((out[..., start:].double() - w).abs().max()) / 2e-6
        assert far >= 10.0, (name, f"only {far:.1f}x the bound away")
    out2 = _noise_launch(nch, start, B, HW, seed=6, sample0=9, stream=3, temperature=0.5, row=row, x=x, eps=eps)
    assert torch.equal(out2, out)

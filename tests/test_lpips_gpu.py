"""LPIPS on the MI355X against the float64 restatement of tests/lpips_ref.py: the four kernels of csrc/lpips.hip at kernel level, the
LPIPS module in both builds of the library, graph replay, re-planning, and pipeline.reconstruction_metrics.

Bounds (none of them is taken from what the code under test returns):
  scale    2 x the error of the SAME formula evaluated in float32 on the host against float64, per shape.
  maxpool  bit-equal to F.max_pool2d on the same float32 data (distinct values: a wrong window or a ceil-mode pool differs).
  layer    |hip - f64| <= 2 x L32 x |f64| per sample.  L32 is the largest relative float32-vs-float64 difference of the host evaluation of
           the same formula over ALL layer cases and samples of this file: one sample's own float32 error is a single draw of a random
           sign sum and can sit far below the typical one, so it cannot scale a bound (for the tower the issue measured a factor of
           70 between such draws).  Five wrong variants of the formula are shown, in float64 on the host, to lie >= 10 x outside.
  tower    the five feature maps relative to each layer's max |f|: 8 x the difference between the restatement run in float32 and in
           float64 on the same inputs (the factor allows for the kernels' other summation order; tests/test_clip_image_gpu.py's rule).
           The per-layer values and the total: |hip - f64| <= 8 x E32 x |f64|, E32 the largest relative float32-vs-float64 difference of
           the restatement over ALL tower cases, samples and layers.  The bf16-pair build gets 10 x these bounds, the ratio
           tests/test_model_gpu.py and tests/test_clip_image_gpu.py give that build.  The conditioning the bound rests on (every layer
           contributes; no pixel's feature norm is small beside its layer's mean) is asserted on the float64 side first.
  metrics  see test_reconstruction_metrics_are_the_float64_composition.
Measured errors: profiles/lpips.txt."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from frido_amd import _lib, lpips
from frido_amd.engine import require_gpu

pytestmark = pytest.mark.gpu

BF16_PAIR_RATIO = 10.0      # the bf16-pair build's allowance over the default build's bound: see the module docstring
PAD = 64                    # NaN floats behind every kernel output: the kernel must leave them alone


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n):
    """n floats for a kernel to write, NaN-filled, with PAD NaNs behind them."""
    require_gpu("cuda")
    return torch.full((n + PAD,), float("nan"), device="cuda")


def _take(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), f"{what} wrote behind its output"
    out = buf[:n].cpu()
    assert not bool(torch.isnan(out).any()), f"{what} left output elements unwritten"
    return out


# ---- frido_lpips_scale ---------------------------------------------------------------------------------
SCALE_SHAPES = [pytest.param(2, 5, 7, id="2x5x7-scalar-path", marks=pytest.mark.gate), pytest.param(1, 16, 16, id="1x16x16-vector-path", marks=pytest.mark.gate),
                pytest.param(1, 363, 365, id="second-trip-scalar"),      # 264990 pixels, one per thread: the launch caps at 1024 x 256 threads
                pytest.param(2, 512, 516, id="second-trip-vector")]      # 264192 units of four pixels


@pytest.mark.parametrize("B,H,W", SCALE_SHAPES)
def test_scale_kernel_matches_float64(B, H, W):
    x, y = R.images(B, H, W, 31)
    shift = torch.tensor(R.SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    both = torch.cat([x, y])
    ref = ((both.double() - shift.double()) / scale.double()).permute(0, 2, 3, 1).reshape(-1, 3)
    host32 = ((both - shift) / scale).permute(0, 2, 3, 1).reshape(-1, 3)
    bound = 2.0 * float((host32.double() - ref).abs().max())
    xg, yg = x.cuda(), y.cuda()
    n = 2 * B * H * W * 3
    dst = _out(n)
    lpips.launch("frido_lpips_scale", lpips.scale_desc(xg.data_ptr(), yg.data_ptr(), dst.data_ptr(), B, H, W), _stream())
    got = _take(dst, n, "frido_lpips_scale").view(-1, 3)
    err = float((got.double() - ref).abs().max())
    print(f"lpips_scale B={B} {H}x{W}: max abs err {err:.3e}, bound (2 x float32 on the host) {bound:.3e}")
    assert bound > 0 and err <= bound
    assert torch.equal(got, host32)      # subtraction and a REAL division, each correctly rounded: the host's bits (a reciprocal multiply differs)
    # another channel's constants are not this formula
    assert float((((both.double() - shift.double().roll(1, 1)) / scale.double().roll(1, 1)).permute(0, 2, 3, 1).reshape(-1, 3) - ref).abs().max()) >= 10 * bound


# ---- frido_maxpool2 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 64, 516])
@pytest.mark.parametrize("H,W", [pytest.param(6, 6, marks=pytest.mark.gate), (5, 4), (9, 10)], ids=["6x6", "5x4", "9x10"])
def test_maxpool_is_torchs_bit_for_bit(H, W, C):
    _check_pool(2, H, W, C)


def test_maxpool_second_trip_of_the_grid_stride_loop():
    _check_pool(4, 130, 130, 64)      # 4 x 65 x 65 x 16 = 270400 units, the launch caps at 1024 x 256 threads


def _check_pool(B, H, W, C):
    n_in = B * H * W * C
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
    src = (torch.randperm(n_in, generator=g).float() - n_in // 2).view(B, H, W, C)      # distinct values, both signs, exact in float32
    ref = F.max_pool2d(src.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    assert ref.shape == (B, H // 2, W // 2, C)
    sg = src.cuda()
    dst = _out(ref.numel())
    lpips.launch("frido_maxpool2", lpips.maxpool_desc(sg.data_ptr(), dst.data_ptr(), B, H, W, C), _stream())
    got = _take(dst, ref.numel(), "frido_maxpool2").view(ref.shape)
    assert torch.equal(got, ref)
    if H % 2 or W % 2:      # what a ceil-mode pool would have kept differs from the floor-mode result
        ceil = F.max_pool2d(src.permute(0, 3, 1, 2), 2, 2, ceil_mode=True)
        assert ceil.shape[2:] != ref.shape[1:3]


# ---- frido_lpips_layer + frido_lpips_finish ------------------------------------------------------------
LAYER_CASES = [(B, C, HW, None) for C in (64, 512) for HW in (1, 4, 90, 1024) for B in (1, 3)] + [
    (3, 64, 90, 89),       # per = 2: workgroups 45 .. 88 own no pixel and write 0
    (2, 128, 90, 4),       # the 32-lane form; per = 23, the last workgroup owns 21 pixels
    (2, 256, 33, 2),       # the one-pixel-per-wave form with one register set
    (1, 516, 7, 7),        # C > 512: the form that reads the row twice
    (2, 12, 9, 3)]         # a row shorter than the 16 lanes it gets
OTHER = (64, 4)            # (C, HW) of the four further layers the finish kernel adds in these tests


def _layer_data(B, C, HW, seed):
    """(f0, f1 [B, C, HW, 1] float32, w [C]).  With HW >= 4: pixel 0 of sample 0 is all zero on BOTH sides (it must contribute exactly 0),
    pixel 1 is zero in f0 only, pixel 2 has tiny features in f0 (norm ~ 1e-5 and below: where eps inside the root differs from eps outside)."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.rand(B, C, HW, 1, generator=g, dtype=torch.float32)
    f1 = (0.8 * f0 + 0.4 * torch.rand(B, C, HW, 1, generator=g, dtype=torch.float32))
    f0 = f0 * (torch.rand(B, C, HW, 1, generator=g) > 0.3)      # post-ReLU features: many exact zeros
    if HW >= 4:
        f0[0, :, 0] = 0
        f1[0, :, 0] = 0
        f0[0, :, 1] = 0
        f0[0, :, 2] *= 1e-6
    return f0, f1, torch.rand(C, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _layer_case(case):
    """(data of the five layers, float64 per_layer [B, 5], float64 total [B], float32 host per_layer): computed once, shared, never changed."""
    B, C, HW, _ = case
    data = [_layer_data(B, C, HW, 7 * C + HW + B)] + [_layer_data(B, *OTHER, 50 + l) for l in range(1, 5)]
    per64 = torch.stack([R.layer_ref(f0.double(), f1.double(), w.double()) for f0, f1, w in data], dim=1)
    per32 = torch.stack([R.layer_ref(f0, f1, w) for f0, f1, w in data], dim=1)
    return data, per64, per64.sum(1), per32


@functools.lru_cache(maxsize=None)
def _L32():
    worst = 0.0
    for case in LAYER_CASES:
        _, per64, _, per32 = _layer_case(case)
        worst = max(worst, float(((per32.double() - per64) / per64).abs().max()))
    return worst


def _run_layers(case):
    """(per_layer [B, 5], out [B]) of the kernels on the case's data."""
    B, C, HW, nblk0 = case
    data = _layer_case(case)[0]
    nblk = [nblk0 or lpips.layer_blocks(HW)] + [lpips.layer_blocks(OTHER[1])] * 4
    hws = [HW] + [OTHER[1]] * 4
    require_gpu("cuda")
    partials = torch.full((B * sum(nblk) + 8,), float("nan"), dtype=torch.float64, device="cuda")
    keep, off = [], 0
    for l, (f0, f1, w) in enumerate(data):
        rows = lambda f: f.squeeze(-1).permute(0, 2, 1).contiguous().cuda()      # noqa: E731  [B * HW][C]
        a, b, wg = rows(f0), rows(f1), w.cuda()
        keep += [a, b, wg]
        lpips.launch("frido_lpips_layer", lpips.layer_desc(a.data_ptr(), b.data_ptr(), wg.data_ptr(), partials.data_ptr() + 8 * off, B, hws[l],
                                                           a.shape[-1], nblk[l]), _stream())
        off += B * nblk[l]
    res = _out(B * 6)
    lpips.launch("frido_lpips_finish", lpips.finish_desc(partials.data_ptr(), res.data_ptr(), res.data_ptr() + 4 * 5 * B, B, nblk, hws), _stream())
    got = _take(res, B * 6, "frido_lpips_finish")
    assert bool(torch.isnan(partials[off:]).all()) and not bool(torch.isnan(partials[:off]).any()), "frido_lpips_layer: its partial sums"
    return got[:5 * B].view(B, 5), got[5 * B:], partials[:off].cpu()


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.gate) if c in ((3, 64, 90, None), (1, 512, 1024, None)) else c for c in LAYER_CASES],
                         ids=lambda c: f"B{c[0]}-C{c[1]}-HW{c[2]}" + (f"-nblk{c[3]}" if c[3] else ""))
def test_layer_and_finish_match_float64(case):
    B, C, HW, _ = case
    data, per64, tot64, per32 = _layer_case(case)
    bound = 2.0 * _L32()
    per, out, partials = _run_layers(case)
    e_per = float(((per.double() - per64) / per64).abs().max())
    e_tot = float(((out.double() - tot64) / tot64).abs().max())
    own = float(((per32.double() - per64) / per64).abs().max())
    print(f"lpips_layer B={B} C={C} HW={HW}: rel err per layer {e_per:.3e}, total {e_tot:.3e}; float32 on the host: this case {own:.3e}, "
          f"all cases {_L32():.3e}; bound {bound:.3e}")
    assert 0 < bound < 1e-5 and e_per <= bound
    # the total is the float32 sum of five float32 values in the reference's order: exactly
    assert torch.equal(out, (((per[:, 0] + per[:, 1]) + per[:, 2]) + per[:, 3]) + per[:, 4])
    per2, out2, partials2 = _run_layers(case)                       # no atomics, a fixed order: the same bits
    assert torch.equal(per, per2) and torch.equal(out, out2) and torch.equal(partials, partials2)
    if HW >= 4:
        # the near misses, in float64 on the host, each at least 10 x outside the bound (relative, on layer 0 of the sample that has the
        # zero and tiny pixels)
        f0, f1, w = (t.double() for t in data[0])
        ref = R.layer_ref(f0, f1, w)
        for kw in (dict(eps_inside=True), dict(normalise=False), dict(diff_first=True), dict(unit_weights=True), dict(pad_count=2)):
            d = float(((R.layer_ref(f0, f1, w, **kw) - ref) / ref).abs()[0])
            assert d >= 10.0 * bound, (kw, d, bound)


def test_zero_pixels_contribute_zero_not_nan():
    """One pixel, all zero on both sides: 0 / 1e-10 - 0 / 1e-10 = 0 exactly.  Zero on one side only: the other side's sum w f1^2 / n1^2."""
    require_gpu("cuda")
    C = 64
    w = torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.1
    f1 = torch.rand(1, C, generator=torch.Generator().manual_seed(4)) + 0.1
    zero = torch.zeros(1, C)
    for a, b, want in ((zero, zero, 0.0), (zero, f1, float((w.double() * (f1.double() / f1.double().norm()) ** 2).sum()))):
        partials = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        ag, bg, wg = a.cuda(), b.cuda(), w.cuda()
        lpips.launch("frido_lpips_layer", lpips.layer_desc(ag.data_ptr(), bg.data_ptr(), wg.data_ptr(), partials.data_ptr(), 1, 1, C, 1), _stream())
        torch.cuda.synchronize()
        got = float(partials[0])
        # float32 on C-term sums: at most (C + 8) roundings of 2^-24 each, all terms non-negative
        assert (got == 0.0) if want == 0.0 else (abs(got - want) <= (C + 8) * 2.0 ** -24 * want), (got, want)


# ---- the tower ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sd():
    from frido_amd.models import LPIPS
    return R.filled_state_dict(LPIPS())


@functools.lru_cache(maxsize=None)
def _tower_case(case):
    """(x, y, float64 (total, per_layer, fx, fy), float32 restatement (total, per_layer, fx, fy)): computed once, shared, never changed."""
    x, y = R.images(*case, R.case_seed(case))
    return x, y, R.lpips_ref(_sd(), x, y), R.lpips_ref(_sd(), x, y, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _E32():
    """The largest relative float32-vs-float64 difference of the restatement over all tower cases, samples, layers and totals -- after
    the conditioning it rests on was checked on the float64 side."""
    worst = 0.0
    for case in R.CASES:
        _, _, (tot64, per64, fx, fy), (tot32, per32, _, _) = _tower_case(case)
        assert float(per64.min()) > 0.02 * float(tot64.max()), (case, per64)               # every layer contributes
        for k in range(5):
            for f in (fx[k], fy[k]):
                n = torch.sqrt((f ** 2).sum(1))
                assert float(n.min()) >= 0.3 * float(n.mean()), (case, k)                     # the normalisation is well conditioned
        worst = max(worst, float(((per32.double() - per64) / per64).abs().max()), float(((tot32.double() - tot64) / tot64).abs().max()))
    return worst


def _module(precision=None):
    from taming.modules.losses.lpips import LPIPS
    return R.fill(LPIPS(precision=precision)).cuda()


_SHARED = {}


def _shared(precision):
    if precision not in _SHARED:
        _SHARED[precision] = _module(precision)
    return _SHARED[precision]


def _rows(f):
    return f.permute(0, 2, 3, 1).reshape(-1, f.shape[1])


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_bf16"], ids=["f16-pairs", "bf16-pairs"])
@pytest.mark.parametrize("case", [pytest.param(R.CASES[0], marks=pytest.mark.gate), R.CASES[1], pytest.param(R.CASES[2], marks=pytest.mark.gate)],
                         ids=[str(c) for c in R.CASES])
def test_tower_matches_float64_and_the_reference_golden(case, precision):
    import os
    import numpy as np
    B, H, W = case
    x, y, (tot64, per64, fx64, fy64), (_, _, fx32, fy32) = _tower_case(case)
    ratio = BF16_PAIR_RATIO if precision == "bf16x3_bf16" else 1.0
    e32 = _E32()
    _lib.status_flags(clear=True)
    m = _shared(precision)
    plan = m._run(x.cuda(), y.cuda())
    assert (B, H, W) in m._plans and plan.planes_hw == lpips.plane_sizes(H, W)
    torch.cuda.synchronize()
    for k in range(5):
        ref = torch.cat([_rows(fx64[k]), _rows(fy64[k])])
        r32 = torch.cat([_rows(fx32[k]), _rows(fy32[k])])
        got = plan.feats[k].view().cpu()
        assert got.shape == ref.shape
        scale = float(ref.abs().max())
        d32 = float((r32.double() - ref).abs().max()) / scale
        err = float((got.double() - ref).abs().max()) / scale
        print(f"lpips tower {case} {precision} relu{k + 1}: rel err {err:.3e}, float32 restatement {d32:.3e}, bound {8 * d32 * ratio:.3e}")
        assert d32 > 0 and err <= 8.0 * d32 * ratio, (k, err, d32)
    per = m.per_layer(x.cuda(), y.cuda())
    out = m(x.cuda(), y.cuda())
    assert per.shape == (B, 5) and out.shape == (B, 1, 1, 1) and out.dtype == per.dtype == torch.float32 and out.is_cuda
    assert _lib.status_flags() == 0
    per, out = per.cpu(), out.cpu().flatten()
    e_per = ((per.double() - per64) / per64).abs()
    e_tot = float(((out.double() - tot64) / tot64).abs().max())
    print(f"lpips tower {case} {precision}: per-layer rel err {[f'{float(v):.2e}' for v in e_per.max(0).values]}, total {e_tot:.3e}, "
          f"E32 {e32:.3e}, bound {8 * e32 * ratio:.3e}")
    assert float(e_per.max()) <= 8.0 * e32 * ratio and e_tot <= 8.0 * e32 * ratio
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_ref.npz"))
    ci = R.CASES.index(case)
    g_per, g_out = torch.from_numpy(gold[f"per_layer_{ci}"]).double(), torch.from_numpy(gold[f"out_{ci}"]).double()
    assert float(((per.double() - g_per) / g_per).abs().max()) <= 8.0 * e32 * ratio
    assert float(((out.double() - g_out) / g_out).abs().max()) <= 8.0 * e32 * ratio


def test_replay_returns_the_same_bits_and_a_new_shape_replans():
    from frido_amd.models import PLAN_CACHE_SIZE
    x, y, (tot64, _, _, _), _ = _tower_case(R.CASES[0])
    _lib.status_flags(clear=True)
    m = _module()
    xg, yg = x.cuda(), y.cuda()
    a = m(xg, yg)
    b = m(xg, yg)
    assert torch.equal(a, b) and m.graph_captures == 1 and list(m._plans) == [(2, 32, 32)]
    p = m.per_layer(xg, yg)                                      # the same graph: no capture
    assert m.graph_captures == 1 and torch.equal((((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]) + p[:, 4], a.flatten())
    c = m(xg[:1], yg[:1])                                        # another batch size: another plan, another graph
    assert m.graph_captures == 2 and list(m._plans) == [(2, 32, 32), (1, 32, 32)]
    assert c.shape == (1, 1, 1, 1) and abs(float(c) - float(tot64[0])) <= 8.0 * _E32() * float(tot64[0])
    d = m(yg, xg)                                                # the first plan again, sides swapped: squares of the negated differences
    assert m.graph_captures == 2 and torch.equal(d, a)
    e = m(xg[:, :, :16, :24], yg[:, :, :16, :24])                # another image size: a third plan
    assert m.graph_captures == 3 and e.shape == a.shape and list(m._plans)[-1] == (2, 16, 24)
    z = m(xg, xg)                                                # both halves of the batch of 2B see the same rows: exactly 0
    assert torch.equal(z, torch.zeros_like(z)) and torch.equal(m.per_layer(yg, yg), torch.zeros(2, 5, device="cuda"))
    assert len(m._plans) <= PLAN_CACHE_SIZE and _lib.status_flags() == 0


# ---- pipeline.reconstruction_metrics -------------------------------------------------------------------
def test_reconstruction_metrics_are_the_float64_composition():
    """Every entry against float64 on the host, composed from the SAME reconstruction `dec` the first stage returned.
    l1, mse: a float32 mean of N = 3 H W non-negative terms -- at most 3 roundings per term and log2 N <= 14 levels of a tree sum, 19
    x 2^-24 relative; the bound is 32 x 2^-24.  psnr = 10 log10(4 / mse): d psnr = (10 / ln 10) x the relative error of mse, plus the
    float32 rounding of the logarithm and the product, 4 x 2^-24 |psnr|.  lpips: the tower bound, 8 x the restatement's relative
    float32-vs-float64 difference (the larger of E32 and this input's own).  nll_loss: the sum of its parts' bounds.  quant_loss: the
    same number forward returned."""
    import math
    from golden_cfg import VQ_SMALL
    from frido_amd.models import MSFPNVQModel, VQModelInterface
    from frido_amd.pipeline import reconstruction_metrics
    from frido_amd.synth import fill_module
    from helpers import golden
    dummy = dict(target="taming.modules.losses.DummyLoss")
    fs = fill_module(MSFPNVQModel(**dict(VQ_SMALL, lossconfig=dummy)), "first_stage_model.").cuda().eval()
    img = torch.from_numpy(golden("msvq_small")["img"]).cuda()
    lp = _shared("bf16x3")
    _lib.status_flags(clear=True)
    dec, diff, _ = fs(img)
    got = reconstruction_metrics(fs, img, lp, perceptual_weight=0.5)
    assert set(got) == {"l1", "mse", "psnr", "lpips", "quant_loss", "nll_loss"}
    assert all(v.shape == (img.shape[0],) and v.dtype == torch.float32 and v.is_cuda for v in got.values())
    x64, d64 = img.cpu().double(), dec.cpu().double()
    l1 = (x64 - d64).abs().mean((1, 2, 3))
    mse = ((x64 - d64) ** 2).mean((1, 2, 3))
    psnr = 10.0 * torch.log10(4.0 / mse)
    lp64, per64, _, _ = R.lpips_ref(_sd(), img.cpu(), dec.cpu())
    lp32, per32, _, _ = R.lpips_ref(_sd(), img.cpu(), dec.cpu(), dtype=torch.float32)
    e_lp = 8.0 * max(_E32(), float(((per32.double() - per64) / per64).abs().max()), float(((lp32.double() - lp64) / lp64).abs().max()))
    u = 2.0 ** -24
    rel = lambda k, ref: float(((got[k].cpu().double() - ref) / ref).abs().max())      # noqa: E731
    print(f"reconstruction_metrics: l1 {rel('l1', l1):.2e} mse {rel('mse', mse):.2e} lpips {rel('lpips', lp64):.2e} (bound {e_lp:.2e}) "
          f"psnr abs {float((got['psnr'].cpu().double() - psnr).abs().max()):.2e}; values l1 {l1.tolist()} psnr {psnr.tolist()} lpips {lp64.tolist()}")
    assert rel("l1", l1) <= 32 * u and rel("mse", mse) <= 32 * u
    assert float((got["psnr"].cpu().double() - psnr).abs().max()) <= 10.0 / math.log(10.0) * 32 * u + 4 * u * float(psnr.abs().max())
    assert rel("lpips", lp64) <= e_lp
    nll = l1 + 0.5 * lp64
    assert float((got["nll_loss"].cpu().double() - nll).abs().max()) <= float((32 * u * l1 + 0.5 * e_lp * lp64 + 2 * u * nll).max())
    assert torch.equal(got["quant_loss"], diff.reshape(1).expand(img.shape[0]))
    assert _lib.status_flags() == 0
    # a VQModelInterface goes through encode -> decode and has no codebook loss to report
    vq = fill_module(VQModelInterface(**VQ_SMALL, lossconfig=dummy), "first_stage_model.").cuda().eval()
    got2 = reconstruction_metrics(vq, img, lp)
    assert set(got2) == {"l1", "mse", "psnr", "lpips", "nll_loss"}
    rec = vq.decode(vq.encode(img))
    assert torch.equal(got2["l1"], (img - rec).abs().mean(dim=(1, 2, 3))) and torch.equal(got2["lpips"], lp(img, rec).flatten())
    assert torch.equal(got2["nll_loss"], got2["l1"] + got2["lpips"])

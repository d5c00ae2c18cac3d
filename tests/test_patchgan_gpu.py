"""The PatchGAN discriminator and the tokenizer's loss on the MI355X against the float64 restatement of tests/patchgan_ref.py: the five
kernels of csrc/patchgan.hip at kernel level, the 4 x 4 convolution on the implicit GEMM alone, the NLayerDiscriminator and
VQLPIPSWithDiscriminator modules in both builds of the library, graph replay, re-planning, MSFPNVQModel.validation_step and
pipeline.reconstruction_metrics(discriminator=).

Bounds (none of them is taken from what the code under test returns):
  stem, affine, head   max |hip - f64| <= 2 x max |host32 - f64|: the SAME formula evaluated in float32 on the host, per case.  The
           named wrong variants (pad 0, the other stride, ky <-> kx, no bias, slope 0.01; the variance without its root, the
           activation first, a / b by pixel) are shown, in float64 on the host, to lie >= 10 x outside.
  terms + finish       every output relative to its own scale (a mean of logits: the mean |logit|; hinge, vanilla: the value):
           <= 2 x T32, the largest such float32-vs-float64 difference of the host evaluation over ALL cases of this file (one case's
           own difference is a single draw and can be 0: a mean of one logit is exact).  Swapped hinge signs, a mean over Ho Wo
           instead of B Ho Wo and a missing 0.5 lie >= 10 x outside.
  conv on the GEMM     tests/test_kernels_gpu.py's bounds for the two-plane GEMM: 2e-5 of max |y| on the fp16-pair build, 1e-4 on
           the bf16-pair build, against float64.
  net, loss            logits relative to max |logits|, loss / log entries relative to themselves: 8 x E32, the largest
           float32-vs-float64 difference of the restatement over all cases (for the net: over every hidden map and the logits); the
           bf16-pair build gets 10 x that bound (tests/test_lpips_gpu.py's rule).  Against the reference's fixture: that bound plus
           the 4 x E32 tests/test_patchgan_host.py allows between the fixture and the float64 restatement.
Measured errors: profiles/patchgan.txt."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as L
import patchgan_ref as R
from frido_amd import _lib
from frido_amd import patchgan as pg
from frido_amd.engine import require_gpu

pytestmark = pytest.mark.gpu

BF16_PAIR_RATIO = 10.0      # the bf16-pair build's allowance over the default build's bound
PAD = 64                    # NaN floats behind every kernel output: the kernel must leave them alone
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patchgan_ref.npz"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, dtype=torch.float32):
    require_gpu("cuda")
    return torch.full((n + PAD,), float("nan"), device="cuda", dtype=dtype)


def _take(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), f"{what} wrote behind its output"
    out = buf[:n].cpu()
    assert not bool(torch.isnan(out).any()), f"{what} left output elements unwritten"
    return out


def _rows(f):
    """NCHW -> NHWC rows [B * H * W, C]."""
    return f.permute(0, 2, 3, 1).reshape(-1, f.shape[1])


# ---- frido_disc_stem -----------------------------------------------------------------------------------
STEM_CASES = [pytest.param(2, 3, 24, 24, 16, True, id="2x3x24x24-ndf16", marks=pytest.mark.gate),
              pytest.param(1, 3, 40, 36, 16, True, id="1x3x40x36-ndf16"),
              pytest.param(2, 5, 21, 23, 12, True, id="odd-planes-Cin5-ndf12"),      # 3 lanes per pixel: 85 pixel slots, one idle thread
              pytest.param(1, 3, 32, 32, 64, True, id="ndf64", marks=pytest.mark.gate),
              pytest.param(2, 8, 8, 6, 64, True, id="Cin8-ndf64-full-lds"),
              pytest.param(2, 3, 24, 24, 16, False, id="y-null"),
              pytest.param(1, 3, 364, 364, 64, True, id="second-trip")]              # 66248 pixels in tiles of 4 x 16: 1036 tiles, the grid caps at 1024


@pytest.mark.parametrize("B,Cin,H,W,ndf,pair", STEM_CASES)
def test_stem_kernel_matches_float64(B, Cin, H, W, ndf, pair):
    g = torch.Generator().manual_seed(H * 100 + W + ndf)
    x, y = R.images(B, H, W, 17 + H, C=Cin)
    w = torch.randn(ndf, Cin, 4, 4, generator=g) * 0.3
    bias = torch.randn(ndf, generator=g)
    both = torch.cat([x, y]) if pair else x
    ref = _rows(R.stem_ref(both, w, bias))
    host32 = _rows(R.stem_ref(both, w, bias, dtype=torch.float32))
    bound = 2.0 * float((host32.double() - ref).abs().max())
    xg, yg, wg, bg = x.cuda(), y.cuda(), pg.repack_stem_weight(w).cuda(), bias.cuda()
    dst = _out(ref.numel())
    pg.launch("frido_disc_stem", pg.stem_desc(xg.data_ptr(), yg.data_ptr() if pair else None, wg.data_ptr(), bg.data_ptr(), dst.data_ptr(),
                                              B, Cin, H, W, ndf), _stream())
    got = _take(dst, ref.numel(), "frido_disc_stem").view(ref.shape)
    err = float((got.double() - ref).abs().max())
    print(f"disc_stem B={B} Cin={Cin} {H}x{W} ndf={ndf} pair={pair}: max abs err {err:.3e}, bound (2 x float32 on the host) {bound:.3e}")
    assert bound > 0 and err <= bound
    for kw in (dict(pad=0), dict(stride=1), dict(transpose=True), dict(drop_bias=True), dict(slope=0.01)):
        assert float((_rows(R.stem_ref(both, w, bias, **kw)) - ref).abs().max()) >= 10 * bound, kw


# ---- frido_affine_leaky --------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [pytest.param(50, 16, marks=pytest.mark.gate), (77, 128), (3, 4), pytest.param(4100, 256, id="second-trip")])
def test_affine_leaky_matches_float64_in_place_and_out_of_place(rows, C):
    """4100 x 256: 262400 units of four floats, the grid caps at 1024 x 256 threads."""
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g) * 2
    gam, bet, mu = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) * 1.5 + 0.5                  # per-channel distinct statistics
    a, b = pg.fold_batchnorm(gam, bet, mu, var)
    ref = R.affine_ref(x, a, b)
    host32 = R.affine_ref(x, a, b, dtype=torch.float32)
    bound = 2.0 * float((host32.double() - ref).abs().max())
    ag, bg = a.cuda(), b.cuda()
    xg = x.cuda()
    dst = _out(rows * C)
    pg.launch("frido_affine_leaky", pg.affine_desc(xg.data_ptr(), ag.data_ptr(), bg.data_ptr(), dst.data_ptr(), rows, C), _stream())
    got = _take(dst, rows * C, "frido_affine_leaky").view(rows, C)
    buf = _out(rows * C)
    buf[:rows * C] = xg.flatten()
    pg.launch("frido_affine_leaky", pg.affine_desc(buf.data_ptr(), ag.data_ptr(), bg.data_ptr(), buf.data_ptr(), rows, C), _stream())
    inplace = _take(buf, rows * C, "frido_affine_leaky in place").view(rows, C)
    err = float((got.double() - ref).abs().max())
    print(f"affine_leaky {rows}x{C}: max abs err {err:.3e}, bound {bound:.3e}")
    assert bound > 0 and err <= bound and torch.equal(inplace, got)
    # what BatchNorm2d itself computes, and the wrong variants
    bn = F.batch_norm(x.double().t().reshape(1, C, rows, 1), mu.double(), var.double(), gam.double(), bet.double(), False, 0.0, 1e-5)
    # a and b are rounded to float32 once each: 2^-24 of |a x| and of |b|, the latter a difference of terms up to |beta| + |mean a|
    assert float((R.leaky(bn).reshape(C, rows).t() - ref).abs().max()) <= 2.0 ** -23 * float(a.abs().max() * x.abs().max() + bet.abs().max() + (mu.abs() * a.abs()).max())
    wrong = [R.affine_ref(x, *R.fold_bn(gam, bet, mu, var, no_root=True)), R.affine_ref(x, a, b, act_first=True)]
    if rows > 4:
        wrong.append(R.affine_ref(x, a, b, by_pixel=True))
    for wv in wrong:
        assert float((wv - ref).abs().max()) >= 10 * bound


# ---- frido_disc_head -----------------------------------------------------------------------------------
HEAD_CASES = [pytest.param(2, 5, 4, 128, id="2x5x4-C128", marks=pytest.mark.gate), pytest.param(3, 2, 2, 16, id="one-logit-C16"),
              pytest.param(2, 6, 7, 512, id="C512"), pytest.param(1, 4, 4, 260, id="C260-second-column-trip"),
              pytest.param(2, 47, 47, 8, id="second-trip")]      # 2 x 46 x 46 = 4232 logits, the grid caps at 1024 x 4 waves


@pytest.mark.parametrize("S,H,W,C", HEAD_CASES)
def test_head_kernel_matches_float64(S, H, W, C):
    g = torch.Generator().manual_seed(S + 10 * H + C)
    f = torch.randn(S, C, H, W, generator=g)
    w = torch.randn(1, C, 4, 4, generator=g) / np.sqrt(16 * C) * 3
    bias = torch.tensor([0.75])
    ref = R.head_ref(f, w, bias)
    host32 = R.head_ref(f, w, bias, dtype=torch.float32)
    bound = 2.0 * float((host32.double() - ref).abs().max())
    fg, wg = _rows(f).contiguous().cuda(), pg.repack_head_weight(w).cuda()
    dst = _out(ref.numel())
    pg.launch("frido_disc_head", pg.head_desc(fg.data_ptr(), wg.data_ptr(), dst.data_ptr(), S, H, W, C, float(bias)), _stream())
    got = _take(dst, ref.numel(), "frido_disc_head").view(ref.shape)
    err = float((got.double() - ref).abs().max())
    print(f"disc_head S={S} {H}x{W} C={C}: max abs err {err:.3e}, bound (2 x float32 on the host) {bound:.3e}")
    assert bound > 0 and err <= bound
    for kw in (dict(pad=0), dict(stride=2), dict(transpose=True), dict(drop_bias=True)):
        if kw.get("stride") == 2 and H == 2:
            continue                                           # one logit at (0, 0): both strides read the same window
        assert float((R.head_ref(f, w, bias, **kw) - ref).abs().max()) >= 10 * bound, kw


# ---- frido_gan_terms + frido_gan_finish ----------------------------------------------------------------
TERM_CASES = [(1, 1, 3.0), (3, 1, 3.0), (2, 4, 2.0), (2, 36, 4.0), (2, 900, 3.0), (3, 130, 12.0)]      # (B, n = Ho Wo, spread of the logits)
TERM_KEYS = pg.OUT_NAMES


@functools.lru_cache(maxsize=None)
def _term_case(case):
    """(real, fake [B, 1, n, 1] float32, float64 terms, float32 host terms, the scales the errors are taken relative to)."""
    B, n, spread = case
    g = torch.Generator().manual_seed(B * 1000 + n)
    real = torch.randn(B, 1, n, 1, generator=g) * spread + 0.5
    fake = torch.randn(B, 1, n, 1, generator=g) * spread - 0.5
    t64, t32 = R.gan_ref(real, fake), R.gan_ref(real, fake, dtype=torch.float32)
    scale = dict(logits_real=float(real.double().abs().mean()), logits_fake=float(fake.double().abs().mean()),
                 g_loss=float(fake.double().abs().mean()), hinge=float(t64["hinge"]), vanilla=float(t64["vanilla"]))
    return real, fake, t64, t32, scale


@functools.lru_cache(maxsize=None)
def _T32():
    worst = 0.0
    for case in TERM_CASES:
        _, _, t64, t32, scale = _term_case(case)
        worst = max(worst, max(abs(float(t32[k]) - float(t64[k])) / scale[k] for k in TERM_KEYS))
    return worst


def _run_terms(real, fake):
    B, n = real.shape[0], real[0].numel()
    lg = torch.cat([real, fake]).flatten().cuda()
    sums = _out(2 * B * 5, torch.float64)
    res = _out(5 + 2 * B)
    pg.launch("frido_gan_terms", pg.terms_desc(lg.data_ptr(), sums.data_ptr(), 2 * B, n), _stream())
    pg.launch("frido_gan_finish", pg.finish_desc(sums.data_ptr(), res.data_ptr(), res.data_ptr() + 20, B, n), _stream())
    got = _take(res, 5 + 2 * B, "frido_gan_finish")
    return got[:5], got[5:], _take(sums, 2 * B * 5, "frido_gan_terms")


@pytest.mark.parametrize("case", [pytest.param(c, marks=pytest.mark.gate) if c[1] == 36 else c for c in TERM_CASES], ids=lambda c: f"B{c[0]}-n{c[1]}")
def test_terms_and_finish_match_float64(case):
    B, n, _ = case
    real, fake, t64, _, scale = _term_case(case)
    bound = 2.0 * _T32()
    out, per, sums = _run_terms(real, fake)
    errs = {k: abs(float(out[i]) - float(t64[k])) / scale[k] for i, k in enumerate(TERM_KEYS)}
    print(f"gan_terms B={B} n={n}: rel err {({k: f'{v:.2e}' for k, v in errs.items()})}, T32 {_T32():.3e}, bound {bound:.3e}")
    assert 0 < bound < 1e-5 and max(errs.values()) <= bound
    assert float(out[2]) == -float(out[1])                                        # g_loss is the negated mean, exactly
    per64 = torch.cat([real, fake]).double().mean((1, 2, 3))
    assert float((per.double() - per64).abs().max()) <= bound * max(scale["logits_real"], scale["logits_fake"])
    out2, per2, sums2 = _run_terms(real, fake)                                    # no atomics, a fixed order: the same bits
    assert torch.equal(out, out2) and torch.equal(per, per2) and torch.equal(sums, sums2)
    wrongs = [dict(swap_signs=True), dict(no_half=True)] + ([dict(mean_over_plane=True)] if B > 1 else [])
    for kw in wrongs:
        bad = R.gan_ref(real, fake, **kw)
        for k in ("hinge", "vanilla"):
            assert abs(float(bad[k]) - float(t64[k])) / scale[k] >= 10 * bound, (kw, k)
    # torch's own formulas (vqperceptual.py:22-33) on the same float32 logits
    assert abs(float(out[3]) - float(0.5 * (F.relu(1. - real).mean() + F.relu(1. + fake).mean()))) <= 4 * bound * scale["hinge"]
    assert abs(float(out[4]) - float(0.5 * (F.softplus(-real).mean() + F.softplus(fake).mean()))) <= 4 * bound * scale["vanilla"]


def test_softplus_takes_torchs_threshold():
    """One logit per sample at 19.5, 20.5 and -30: log1p(exp(x)) below the threshold, x above it, exp(x) far below."""
    real = torch.tensor([19.5, 20.5, -30.0]).view(3, 1, 1, 1)
    out, _, sums = _run_terms(real, -real)
    want = F.softplus(real.double()).flatten()
    got = sums.view(6, 5)[:3, 4]
    assert float(((got - want) / want).abs().max()) <= 2.0 ** -23
    assert float(sums.view(6, 5)[1, 4]) == 20.5                                   # above the threshold: the logit itself


# ---- the 4 x 4 convolution on the implicit GEMM, alone ---------------------------------------------------
CONV4_CASES = [pytest.param(16, 32, 10, 10, 2, id="Cin16-s2-even", marks=pytest.mark.gate), pytest.param(16, 32, 9, 7, 2, id="Cin16-s2-odd"),
               pytest.param(16, 48, 5, 4, 1, id="Cin16-s1"), pytest.param(256, 64, 8, 8, 2, id="Cin256-s2-even"),
               pytest.param(256, 64, 5, 7, 2, id="Cin256-s2-odd"), pytest.param(256, 128, 5, 4, 1, id="Cin256-s1", marks=pytest.mark.gate)]
GEMM_TOL = {"f16": 2e-5, "bf16": 1e-4}      # tests/test_kernels_gpu.py: _tol(2) on the two builds


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("Cin,Cout,H,W,stride", CONV4_CASES)
def test_conv4x4_on_the_implicit_gemm(Cin, Cout, H, W, stride, planes):
    """Builder.conv with a 4 x 4 weight, stride 2 / 1, pad 1, f32 output without bias: the geometry the discriminator's middle layers are
    the first to launch."""
    from frido_amd.builder import Builder
    B = 3
    g = torch.Generator().manual_seed(Cin + H * 10 + W + stride)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / np.sqrt(16 * Cin)
    ref = F.conv2d(x.double(), w.double(), None, stride=stride, padding=1)
    Ho, Wo = ref.shape[2:]
    assert (Ho, Wo) == (pg.conv_out(H, stride), pg.conv_out(W, stride))
    with _lib.use_planes(planes):
        dev = require_gpu("cuda")
        b = Builder(dev, 2, {"c.weight": w.cuda()}, planes=planes)
        xr = _rows(x).contiguous().cuda()
        a = b.pack(xr.data_ptr(), 1, B * H * W, Cin, 0, Cin)
        out = b.conv(a, B, H, W, "c", stride=stride, pad=1, bias=False, out="f32_strict")
        assert out.rows == B * Ho * Wo and out.C == Cout
        _lib.status_flags(clear=True)
        b.prog.run(_stream())
        torch.cuda.synchronize()
        assert _lib.status_flags() == 0
        got = out.view().cpu()
    err = float((got.double() - _rows(ref)).abs().max() / ref.abs().max())
    print(f"conv4x4 Cin={Cin} Cout={Cout} {H}x{W} s{stride} {planes}: rel err {err:.3e}, bound {GEMM_TOL[planes]:.1e}")
    assert err <= GEMM_TOL[planes]
    # the neighbouring geometries are another function of the input
    for kw in (dict(stride=3 - stride), dict(pad=0), dict(transpose=True)):
        bad = R.conv4(x.double(), w.double(), None, stride=kw.get("stride", stride), pad=kw.get("pad", 1), out_hw=(Ho, Wo), transpose=kw.get("transpose", False))
        assert float((bad - ref).abs().max() / ref.abs().max()) >= 100 * GEMM_TOL[planes], kw


# ---- the net ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _disc_sd(ndf, n_layers, use_actnorm):
    from frido_amd.models import NLayerDiscriminator
    return R.filled_state_dict(NLayerDiscriminator(3, ndf, n_layers, use_actnorm))


@functools.lru_cache(maxsize=None)
def _net_case(ci):
    """(real, fake, float64 logits of both, the restatement's float32-vs-float64 difference): computed once, shared, never changed."""
    shape, ndf, nl, act = R.NET_CASES[ci]
    sd = _disc_sd(ndf, nl, act)
    kw = dict(ndf=ndf, n_layers=nl, use_actnorm=act, want_hidden=True)
    x, y = R.images(*shape, R.case_seed(ci))
    both = torch.cat([x, y])
    l64, h64 = R.disc_ref(sd, both, **kw)
    l32, h32 = R.disc_ref(sd, both, dtype=torch.float32, **kw)
    e32 = max(float((h.double() - g).abs().max()) / float(g.abs().max()) for h, g in zip(h32 + [l32], h64 + [l64]))
    return x, y, l64, e32


@functools.lru_cache(maxsize=None)
def _E32():
    return max(_net_case(ci)[3] for ci in range(len(R.NET_CASES)))


_NETS = {}


def _net(ci, precision):
    from taming.modules.discriminator.model import NLayerDiscriminator
    _, ndf, nl, act = R.NET_CASES[ci]
    key = (ndf, nl, act, precision)
    if key not in _NETS:
        _NETS[key] = R.fill(NLayerDiscriminator(3, ndf, nl, act, precision=precision)).cuda()
    return _NETS[key]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_bf16"], ids=["f16-pairs", "bf16-pairs"])
@pytest.mark.parametrize("ci", [pytest.param(i, marks=pytest.mark.gate) if i in (1, 3) else i for i in range(len(R.NET_CASES))],
                         ids=[f"{c[0]}-ndf{c[1]}-L{c[2]}-{'act' if c[3] else 'bn'}" for c in R.NET_CASES])
def test_net_matches_float64_and_the_reference_golden(ci, precision):
    shape, ndf, nl, act = R.NET_CASES[ci]
    B = shape[0]
    x, y, l64, _ = _net_case(ci)
    ratio = BF16_PAIR_RATIO if precision == "bf16x3_bf16" else 1.0
    bound = 8.0 * _E32() * ratio
    _lib.status_flags(clear=True)
    m = _net(ci, precision)
    plan = m.pair(x.cuda(), y.cuda())
    pair = plan.logits.clone().cpu()
    single = m(y.cuda()).cpu()
    assert _lib.status_flags() == 0
    assert pair.shape == l64.shape and single.shape == l64[B:].shape and single.dtype == torch.float32
    assert plan.planes_hw == pg.plane_sizes(*shape[1:], nl) and (*shape, True) in m._plans and (*shape, False) in m._plans
    scale = float(l64.abs().max())
    e_pair = float((pair.double() - l64).abs().max()) / scale
    e_single = float((single.double() - l64[B:]).abs().max()) / scale
    print(f"patchgan net {R.NET_CASES[ci]} {precision}: rel err pair {e_pair:.3e}, single {e_single:.3e}; E32 {_E32():.3e}, bound {bound:.3e}")
    assert 0 < bound < 1e-3 and e_pair <= bound and e_single <= bound
    gold = torch.cat([torch.from_numpy(GOLD[f"logits_real_{ci}"]), torch.from_numpy(GOLD[f"logits_fake_{ci}"])]).double()
    assert float((pair.double() - gold).abs().max()) / scale <= bound + 4.0 * _E32()
    # the terms of this pair, from the graph
    t64 = R.gan_ref(l64[:B], l64[B:])
    out = plan.out.cpu()
    lscale = float(l64.abs().mean())
    for i, k in enumerate(pg.OUT_NAMES):
        s = lscale if k in ("logits_real", "logits_fake", "g_loss") else max(float(t64[k]), lscale)
        assert abs(float(out[i]) - float(t64[k])) <= bound * scale + 2.0 ** -22 * s, (k, float(out[i]), float(t64[k]))


def test_replay_returns_the_same_bits_and_a_new_shape_replans():
    from frido_amd.models import PLAN_CACHE_SIZE, NLayerDiscriminator
    x, y, l64, _ = _net_case(1)
    _lib.status_flags(clear=True)
    m = R.fill(NLayerDiscriminator(3, 16, 3, True)).cuda()
    xg, yg = x.cuda(), y.cuda()
    p = m.pair(xg, yg)
    a, out_a = p.logits.clone(), p.out.clone()
    p2 = m.pair(xg, yg)
    assert p2 is p and torch.equal(p.logits, a) and torch.equal(p.out, out_a) and m.graph_captures == 1 and list(m._plans) == [(2, 32, 32, True)]
    s = m(xg)                                                    # the single form: another plan, another graph
    assert m.graph_captures == 2 and s.shape == (2, 1, 2, 2) and torch.equal(m(xg), s)
    assert float((s.cpu().double() - l64[:2]).abs().max()) <= 8.0 * _E32() * float(l64.abs().max())
    sw = m.pair(yg, xg)                                          # the first plan again, sides swapped
    assert m.graph_captures == 2 and torch.equal(sw.logits[:2], a[2:]) and torch.equal(sw.logits[2:], a[:2])
    assert float(sw.out[0]) == float(out_a[1]) and float(sw.out[1]) == float(out_a[0])
    c = m.pair(xg[:1], yg[:1])                                   # another batch size
    assert m.graph_captures == 3 and c.logits.shape == (2, 1, 2, 2)
    assert float((c.logits.cpu().double() - l64[[0, 2]]).abs().max()) <= 8.0 * _E32() * float(l64.abs().max())
    e = m.pair(xg[:, :, :24, :28], yg[:, :, :24, :28])           # another image size
    assert m.graph_captures == 4 and e.logits.shape == (4, 1, 1, 1) and list(m._plans)[-1] == (2, 24, 28, True)
    m.load_state_dict(m.state_dict())                            # new weights: every plan is dropped
    assert m._plans == {} and torch.equal(m.pair(xg, yg).logits, a) and m.graph_captures == 5
    assert len(m._plans) <= PLAN_CACHE_SIZE and _lib.status_flags() == 0


# ---- the loss ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lpips_sd():
    from frido_amd.models import LPIPS
    return L.filled_state_dict(LPIPS())


def _entries(l0, log0, l1, log1, prefix=""):
    return [float(l0)] + [float(log0[prefix + k]) for k in R.LOG0_KEYS] + [float(l1)] + [float(log1[prefix + k]) for k in R.LOG1_KEYS]


ENTRY_NAMES = ["loss0"] + list(R.LOG0_KEYS) + ["loss1"] + list(R.LOG1_KEYS)


@functools.lru_cache(maxsize=None)
def _loss_case(li, step):
    disc_loss, act = R.LOSS_CASES[li]
    x, y = R.images(*R.LOSS_SHAPE, R.LOSS_SEED)
    sd = _disc_sd(R.LOSS_NDF, 3, act)
    kw = dict(disc_loss=disc_loss, use_actnorm=act)
    ref = _entries(*R.loss_ref(_lpips_sd(), sd, x, y, R.CODEBOOK_LOSS, step, **kw))
    r32 = _entries(*R.loss_ref(_lpips_sd(), sd, x, y, R.CODEBOOK_LOSS, step, dtype=torch.float32, **kw))
    return x, y, ref, max(abs(a - b) / abs(b) for a, b in zip(r32, ref) if b != 0.0)


@functools.lru_cache(maxsize=None)
def _LOSS_E32():
    return max(_loss_case(li, step)[3] for li in range(len(R.LOSS_CASES)) for step in R.LOSS_STEPS)


def _loss_module(li, precision):
    from taming.modules.losses.vqperceptual import VQLPIPSWithDiscriminator
    disc_loss, act = R.LOSS_CASES[li]
    m = VQLPIPSWithDiscriminator(disc_loss=disc_loss, use_actnorm=act, precision=precision, **R.LOSS_KW)
    R.fill(m.discriminator)
    L.fill(m.perceptual_loss)
    return m.cuda()


def _check_entries(got, ref, bound, step, what):
    for name, g, r in zip(ENTRY_NAMES, got, ref):
        if name in ("rec_aux_loss", "d_weight") or (step < R.DISC_START and name in ("disc_factor", "loss1", "disc_loss")):
            assert g == 0.0 == r, (what, name, g, r)
        elif name == "disc_factor":
            assert g == float(np.float32(R.LOSS_KW["disc_factor"])), (what, g)
        else:
            assert abs(g - r) <= bound * abs(r), (what, name, step, g, r, abs(g - r) / abs(r), bound)


@pytest.mark.parametrize("li,precision", [pytest.param(0, "bf16x3", marks=pytest.mark.gate), (1, "bf16x3"), (0, "bf16x3_bf16"), (1, "bf16x3_bf16")],
                         ids=["hinge-f16-pairs", "vanilla-actnorm-f16-pairs", "hinge-bf16-pairs", "vanilla-actnorm-bf16-pairs"])
def test_loss_and_log_match_float64_and_the_reference_golden(li, precision):
    ratio = BF16_PAIR_RATIO if precision == "bf16x3_bf16" else 1.0
    bound = 8.0 * _LOSS_E32() * ratio
    m = _loss_module(li, precision)
    q = torch.tensor(R.CODEBOOK_LOSS).cuda()
    _lib.status_flags(clear=True)
    for step in R.LOSS_STEPS:
        x, y, ref, _ = _loss_case(li, step)
        xg, yg = x.cuda(), y.cuda()
        (l0, log0), (l1, log1) = m.evaluate(q, xg, yg, step, split="val")
        assert list(log0) == ["val/" + k for k in R.LOG0_KEYS] and list(log1) == ["val/" + k for k in R.LOG1_KEYS]
        assert all(torch.is_tensor(v) and v.dim() == 0 for v in list(log0.values()) + list(log1.values()) + [l0, l1])
        got = _entries(l0, log0, l1, log1, "val/")
        worst = max((abs(g - r) / abs(r) for g, r in zip(got, ref) if r != 0.0))
        print(f"vqlpips {R.LOSS_CASES[li]} {precision} step {step}: worst rel err {worst:.3e}, E32 {_LOSS_E32():.3e}, bound {bound:.3e}; "
              f"values {dict(zip(ENTRY_NAMES, [f'{v:.5g}' for v in got]))}")
        assert 0 < bound < 1e-3
        _check_entries(got, ref, bound, step, "float64")
        gold = [float(GOLD[f"loss0_{li}_{step}"])] + list(GOLD[f"log0_{li}_{step}"]) + [float(GOLD[f"loss1_{li}_{step}"])] + list(GOLD[f"log1_{li}_{step}"])
        _check_entries(got, [float(v) for v in gold], bound + 4.0 * _LOSS_E32(), step, "golden")
        # forward picks one of the two, with the reference's signature
        f0, flog0 = m(q, xg, yg, 0, step, last_layer=None, split="val")
        f1, flog1 = m(q, xg, yg, 1, step, last_layer=torch.zeros(1), split="train")
        assert torch.equal(f0, l0) and all(torch.equal(flog0[k], log0[k]) for k in log0)
        assert torch.equal(f1, l1) and list(flog1) == ["train/" + k for k in R.LOG1_KEYS] and torch.equal(flog1["train/logits_fake"], log1["val/logits_fake"])
    assert m.discriminator.graph_captures == 1 and m.perceptual_loss.graph_captures == 1 and _lib.status_flags() == 0


# ---- MSFPNVQModel.validation_step and pipeline.reconstruction_metrics ---------------------------------
LOSSCFG = dict(target="taming.modules.losses.vqperceptual.VQLPIPSWithDiscriminator",
               params=dict(disc_start=1, disc_ndf=16, codebook_weight=0.7, disc_factor=0.8, perceptual_weight=0.6))


@functools.lru_cache(maxsize=None)
def _tokenizer():
    from golden_cfg import VQ_SMALL
    from helpers import golden
    from frido_amd.models import MSFPNVQModel
    from frido_amd.synth import fill_module
    m = fill_module(MSFPNVQModel(**dict(VQ_SMALL, lossconfig=LOSSCFG), with_loss=True), "first_stage_model.")
    R.fill(m.loss.discriminator)
    L.fill(m.loss.perceptual_loss)
    return m.cuda().eval(), torch.from_numpy(golden("msvq_small")["img"])


def test_validation_step_is_the_float64_composition():
    """The small tokenizer of tests/test_msvq_gpu.py end to end: the dict validation_step returns against vqperceptual.py:85-150 composed
    in float64 from the SAME reconstruction and codebook loss its forward returned.  Bound: 8 x the restatement's own
    float32-vs-float64 difference on these inputs (or E32 of the loss cases, whichever is larger)."""
    m, img = _tokenizer()
    _lib.status_flags(clear=True)
    xg = img.cuda()
    dec, diff, _ = m(xg)
    batch = dict(image=img.permute(0, 2, 3, 1).contiguous())
    kw = dict(disc_loss="hinge", use_actnorm=False, kw=dict(LOSSCFG["params"], disc_ndf=16))
    sd = _disc_sd(16, 3, False)
    for step in (0, 1):
        m.global_step = step
        got = m.validation_step(batch, 0)
        assert list(got) == ["val/" + k for k in R.LOG0_KEYS + R.LOG1_KEYS]
        args = (_lpips_sd(), sd, img, dec.cpu(), float(diff), step)
        ref = _entries(*R.loss_ref(*args, **kw))
        r32 = _entries(*R.loss_ref(*args, dtype=torch.float32, **kw))
        e32 = max(_LOSS_E32(), max(abs(a - b) / abs(b) for a, b in zip(r32, ref) if b != 0.0))
        vals = [float(got["val/total_loss"])] + [float(got["val/" + k]) for k in R.LOG0_KEYS] + [float(got["val/disc_loss"])] + \
               [float(got["val/" + k]) for k in R.LOG1_KEYS]
        print(f"validation_step step {step}: {dict(zip(ENTRY_NAMES, [f'{v:.5g}' for v in vals]))}; bound {8 * e32:.3e}")
        for name, g, r in zip(ENTRY_NAMES, vals, ref):
            if r == 0.0:
                assert g == 0.0, (name, g)
            elif name == "disc_factor":
                assert g == float(np.float32(0.8))
            else:
                assert abs(g - r) <= 8.0 * e32 * abs(r), (name, step, g, r)
    assert float(got["val/disc_loss"]) > 0 and _lib.status_flags() == 0
    m.global_step = 0


def test_reconstruction_metrics_with_a_discriminator():
    from frido_amd.pipeline import reconstruction_metrics
    m, img = _tokenizer()
    xg = img.cuda()
    lp, disc = m.loss.perceptual_loss, m.loss.discriminator
    _lib.status_flags(clear=True)
    before = reconstruction_metrics(m, xg, lp, perceptual_weight=0.5)
    got = reconstruction_metrics(m, xg, lp, perceptual_weight=0.5, discriminator=disc)
    assert set(before) == {"l1", "mse", "psnr", "lpips", "quant_loss", "nll_loss"} and set(got) == set(before) | {"logits_real", "logits_fake"}
    assert all(torch.equal(before[k], got[k]) for k in before)                    # without the keyword: the keys and bits it returned before
    dec = m(xg)[0].cpu()
    kw = dict(ndf=16, n_layers=3, use_actnorm=False)
    sd = _disc_sd(16, 3, False)
    both = torch.cat([img, dec])
    l64 = R.disc_ref(sd, both, **kw)
    l32 = R.disc_ref(sd, both, dtype=torch.float32, **kw)
    scale = float(l64.abs().max())
    e32 = max(_E32(), float((l32.double() - l64).abs().max()) / scale)
    per64 = l64.mean((1, 2, 3))
    B = img.shape[0]
    for k, ref in (("logits_real", per64[:B]), ("logits_fake", per64[B:])):
        assert got[k].shape == (B,) and got[k].dtype == torch.float32 and got[k].is_cuda
        assert float((got[k].cpu().double() - ref).abs().max()) <= 8.0 * e32 * scale, k
    assert _lib.status_flags() == 0

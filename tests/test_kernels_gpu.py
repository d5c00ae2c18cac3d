"""Kernel-level parity (MI355X): every HIP kernel of libfrido_hip.so against a CPU fp32 statement
of the same op (torch functional ops / the oracle's functions) on seeded inputs.

Tolerances: bf16x3 mode (nsplit 2) is an fp32-emulating path, checked to 2e-5 relative to the
output scale; bf16 mode (nsplit 1) to 2e-2; pure-f32 kernels to 1e-5.

Two builds hold the two-plane arithmetic: fp16 hi + lo planes (libfrido_hip.so, the default) and bf16 hi + lo planes
(libfrido_hip_bf16p.so, where frido_amd/autoplanes.py moves a model whose fp16 planes saturate).  Every test of a two-plane
kernel runs on both: the test as written on the fp16-pair build, and its twin `<name>_bf16` (nsplit = 2 legs only, same ids
otherwise) with the same body inside _lib.use_planes("bf16").  Bounds that depend on the plane format go through _tol /
PAIR_U.  GEMMs on packed operands are also checked against the three-pass product of the planes the kernel actually read
(_three_pass): that pins the arithmetic itself, whatever the format.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frido_amd.synth import seeded_normal  # noqa: E402


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _builder(nsplit, weights=None):
    from frido_amd.builder import Builder
    return Builder(_dev(), nsplit, weights or {})


def _run(b):
    b.prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _planes():
    """Plane format of the build this thread's calls go to ("f16" / "bf16")."""
    from frido_amd import _lib
    return _lib.active_planes()


# Representation bound of one value held as a hi + lo pair: fp16 pairs 2^-22 |v| with an absolute floor of 2^-25 (the lo plane is an
# fp16 subnormal below |v| = 2^-3), bf16 pairs 2^-17 |v| with no floor (bf16 keeps fp32's exponent range; include/frido_hip.h).
PAIR_U = {"f16": 2.0 ** -22, "bf16": 2.0 ** -17}
PAIR_FLOOR = {"f16": 2.0 ** -25, "bf16": 0.0}
# bf16-pair GEMM bound, from 2^-17 per operand: a product a*b is off by at most (2 * 2^-17 + 2^-34) |a b| (the lo*lo pass is not run), so
# an output is off by at most 2^-16 sum_k |a_k b_k|.  On unit-normal operands sum_k |a_k b_k| ~ 0.64 K and max |y| ~ 4 sqrt(K): the ratio
# is 0.16 sqrt(K) ~ 5 at K = 960, i.e. 7.6e-5 of the output maximum -> 1e-4.  A dropped correction pass (a_lo b_hi or a_hi b_lo,
# |lo| <= 2^-9 |v|) costs ~5e-4 of the output maximum on the same data: 5x over the bound (the three-pass check below is the sharp one).
X3_BF16_TOL = 1e-4
# attention: softmax(q k^T) v runs two such products in series (the probabilities are re-split into a pair): twice the GEMM bound
ATTN_BF16_TOL = 2 * X3_BF16_TOL


def _tol(nsplit, f16=2e-5, bf16=X3_BF16_TOL):
    """Max-relative bound of a test leg: nsplit 1 (bf16 operands) 2e-2; nsplit 2 by the active build's plane format."""
    if nsplit != 2:
        return 2e-2
    return f16 if _planes() == "f16" else bf16


def _relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


_WORST = {}     # (plane format, bound) -> (worst max-relative error seen, test): the margins, reported at the end of the module


def _within(got, ref, bound):
    """_relerr(got, ref) < bound, recording the worst error met under each (plane format, bound)."""
    e = _relerr(got, ref)
    import os
    key = (_planes(), float(bound))
    if e >= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (e, os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0])
    return e < bound


@pytest.fixture(scope="module", autouse=True)
def _report_margins(request):
    yield
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    if tr is None or not _WORST:
        return
    tr.write_line("")
    tr.write_line("worst max-relative error per plane format and bound (test_kernels_gpu):")
    for (planes, bound), (e, where) in sorted(_WORST.items()):
        tr.write_line(f"  {planes:>4}  bound {bound:.1e}  worst {e:.2e}  margin {bound / max(e, 1e-30):8.1f}x  {where}")


# ---- three-pass emulation --------------------------------------------------------------------------------------------------
# Every two-plane product is  a_hi b_hi + a_hi b_lo + a_lo b_hi  (three MFMA passes, no a_lo b_lo), each pass on 16-bit values whose
# products are exact in fp32.  So from the planes an operand buffer actually holds, float64 gives what the kernel must compute up to fp32
# accumulation error -- in either plane format.  A missing, doubled or mis-paired pass moves the result by ~|lo| / |v| (2^-12 / 2^-9).
X3_EMU_TOL = 1e-6


def _emu_tol(K):
    """Bound of |kernel - emulation| / max|emulation|: fp32 accumulation.  An output takes 3 K / 32 MFMA accumulator updates (3 passes of
    32-deep products), each rounded to 2^-24 of a partial sum of the output's scale; as a random walk that is 2^-24 sqrt(3 K / 32), taken
    twice for the tail -- 1.1e-6 at K = 960, 2e-6 at K = 3168 (measured there: 1.0e-6 on every tile, either format) -- and never under 1e-6."""
    return max(X3_EMU_TOL, 2 * 2.0 ** -24 * float(np.sqrt(3 * K / 32)))


def _pair_planes(op):
    """(hi, lo) planes of a two-plane operand (Operand / POperand) as float64 CPU [batch * rows][K], read back as written."""
    from frido_amd.engine import plane_dtype
    n = op.batch * op.rows * op.K
    t = op.t if hasattr(op, "t") else op.buf[: 2 * op.lo * 2].view(plane_dtype(2)).view(2, op.lo)
    assert t.dtype == plane_dtype(2)
    return tuple(t[p, :n].double().cpu().view(op.batch * op.rows, op.K) for p in (0, 1))


def _pass_products(a_op, w_op, conv=None):
    """{"hh", "hl", "lh"}: the three passes (a_hi b_hi, a_hi b_lo, a_lo b_hi) of A [M][K] x W [N][K]^T in float64.  conv = (B, H, W, kh):
    A is an NHWC activation operand [B*H*W][Cp], W a packed conv weight [N][kh*kh*Cp] (k = tap * Cp + c), stride 1, pad kh // 2."""
    (ah, al), (wh, wl) = _pair_planes(a_op), _pair_planes(w_op)
    assert ah.shape[1] == (a_op.K if conv is None else w_op.K // (conv[3] * conv[3]))
    if conv is None:
        f = lambda a, w: a @ w.t()
    else:
        B, H, W, kh = conv
        Cp, N = a_op.K, w_op.rows

        def f(a, w):
            x = a.view(B, H, W, Cp).permute(0, 3, 1, 2)
            k = w.view(N, kh, kh, Cp).permute(0, 3, 1, 2)
            return F.conv2d(x, k, padding=kh // 2).permute(0, 2, 3, 1).reshape(B * H * W, N)
    return {"hh": f(ah, wh), "hl": f(ah, wl), "lh": f(al, wh), "K": w_op.K}


def _three_pass(got, passes, epi, what="", out="f32", check_variants=True):
    """Assert the kernel's output `got` equals epi(hh + hl + lh) (epi: the float64 epilogue) to _emu_tol(K) of its maximum, and that every
    variant with a pass missing, doubled or mis-paired lies at least 10x outside that bound on the same data.  `out="op"`: got holds the
    epilogue's own re-split of its f32 result, off by one pair representation error.  Prints and returns the distances."""
    planes = _planes()
    hh, hl, lh = passes["hh"], passes["hl"], passes["lh"]
    tol = _emu_tol(passes["K"])
    emu = epi(hh + hl + lh)
    got = got.double()
    scale = float(emu.abs().max())
    slack = (PAIR_U[planes] * emu.abs() + PAIR_FLOOR[planes]) if out == "op" else 0.0

    def dist(ref):
        return float(((got - ref).abs() - slack).clamp_min(0).max()) / scale

    d = {"kernel": dist(emu)}
    variants = {"no a_lo*b_hi": hh + hl, "no a_hi*b_lo": hh + lh, "a_hi*b_hi only": hh, "a_lo*b_hi twice": hh + hl + 2 * lh,
                "a_hi*b_lo for a_lo*b_hi": hh + 2 * hl}
    for k, v in variants.items():
        d[k] = dist(epi(v))
    print(f"three-pass [{planes}] {what}: kernel - emu {d['kernel']:.2e} (bound {tol:.1e}); "
          + ", ".join(f"{k} {v:.2e}" for k, v in d.items() if k != "kernel"))
    assert d["kernel"] <= tol, (what, d)
    if check_variants:
        weak = {k: v for k, v in d.items() if k != "kernel" and v < 10 * tol}
        assert not weak, (what, "the three-pass check would not see these variants", weak)
    key = (planes, tol)
    if d["kernel"] >= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (d["kernel"], f"three-pass {what}")
    return d


def _t(tag, *shape):
    return torch.from_numpy(seeded_normal(tag, shape))


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("M,N,K,tile", [(300, 200, 96, 0), (128, 128, 64, 1), (257, 192, 160, 2), (64, 26, 64, 3),
                                        (1024, 384, 384, 0), (5, 3, 32, 0), (600, 320, 256, 17), (512, 256, 128, 7)])
def test_gemm_dense(nsplit, M, N, K, tile):
    a, w, bias, res = _t("ga", M, K), _t("gw", N, K), _t("gb", N), _t("gr", M, N)
    b = _builder(nsplit, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    r = b.f32(M, N)
    r.view().copy_(res.cuda())
    from frido_amd.builder import ACT_SILU
    out = b.linear(a_op, "w", act=ACT_SILU, residual=r, alpha=0.5)
    if tile:
        b.prog.ops[-1][1].tile = tile
    _run(b)
    ref = F.silu(0.5 * (a @ w.t()) + bias) + res
    assert _within(out.view().cpu(), ref, _tol(nsplit))


@pytest.mark.parametrize("nsplit", [2, 1])
def test_gemm_batched_operand_out_and_rowbias(nsplit):
    B, M, N, K = 3, 70, 64, 96
    a, w, rb = _t("ba", B, M, K), _t("bw", B, N, K), _t("brb", M)
    b = _builder(nsplit)
    ad, wd = a.cuda(), w.cuda()
    a_op = b.pack(ad.data_ptr(), 1, B * M, K, 0, K)
    w_op = b.pack(wd.data_ptr(), 1, B * N, K, 0, K)
    o = b.op(B * M, N)
    rbd = rb.cuda()
    b.prog.gemm(M, N, K, a_op, w_op, batch=B, a_bs=M * K, b_bs=N * K, out_op=o.ptr, oo_bs=M * N, ldoo=N, oo_lo=o.lo,
                row_bias=rbd.data_ptr())
    _run(b)
    ref = torch.einsum("bmk,bnk->bmn", a, w) + rb[None, :, None]
    assert _within(o.to_f32().cpu().view(B, M, N), ref, _tol(nsplit, f16=1e-5))


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("conv", [False, True])
@pytest.mark.parametrize("splitk,tile", [(2, 3), (4, 6), (7, 4), (3, 7), (9, 1)])
@pytest.mark.parametrize("sk_mode", [0, 1])      # 1: the last workgroup of each tile adds the slices in-kernel (FridoGemm.sk_mode)
def test_gemm_split_k_is_deterministic_and_correct(nsplit, conv, splitk, tile, sk_mode):
    from frido_amd import tune
    from frido_amd.builder import ACT_SILU
    if conv:
        B, H, W, Cin, Cout = 2, 8, 8, 96, 70
        x, w, bias = _t("kx", B, Cin, H, W), _t("kw", Cout, Cin, 3, 3) / np.sqrt(9 * Cin), _t("kb", Cout)
        res = _t("kr", B * H * W, Cout)
        ref = F.silu(F.conv2d(x, w, bias, padding=1)).permute(0, 2, 3, 1).reshape(-1, Cout) + res
        b = _builder(nsplit, {"c.weight": w.cuda(), "c.bias": bias.cuda()})
        xd = x.cuda()
        a = b.pack(xd.data_ptr(), B, H * W, Cin, 0, Cin, nchw=True)
        r = b.f32(B * H * W, Cout)
        r.view().copy_(res.cuda())
        out = b.conv(a, B, H, W, "c", act=ACT_SILU, residual=r)
    else:
        M, N, K = 200, 150, 32 * 23
        a_, w, bias, res = _t("ka", M, K), _t("kw2", N, K) / np.sqrt(K), _t("kb2", N), _t("kr2", M, N)
        ref = F.silu(a_ @ w.t() + bias) + res
        b = _builder(nsplit, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
        ad = a_.cuda()
        a = b.pack(ad.data_ptr(), 1, M, K, 0, K)
        r = b.f32(M, N)
        r.view().copy_(res.cuda())
        out = b.linear(a, "w", act=ACT_SILU, residual=r)
    st = b.prog.ops[-1][1]
    st.tile, st.splitk, st.sk_mode = tile, splitk, sk_mode
    st.ws = tune.workspace_for(st, _dev())
    _run(b)
    first = out.view().clone()
    assert _within(first.cpu(), ref, _tol(nsplit))
    if nsplit == 2:
        if conv:
            passes = _pass_products(a, b.conv_weight("c.weight")[0], conv=(B, H, W, 3))
        else:
            passes = _pass_products(a, b.lin_weight("w.weight"))
        _three_pass(first.cpu(), passes, lambda y: F.silu(y + bias.double()) + res.double(),
                    f"{'conv' if conv else 'dense'} split-K {splitk} tile {tile} sk_mode {sk_mode}")
    for _ in range(3):
        _run(b)
        assert torch.equal(first, out.view())    # fixed-order reduction: bit-reproducible (whoever arrives last)
    if sk_mode == 1:                             # ... and the same bits as the two-kernel reduction
        st.sk_mode = 0
        _run(b)
        assert torch.equal(first, out.view())


@pytest.mark.parametrize("tile", [7, 8, 11, 12, 13, 14, 15, 16])
@pytest.mark.parametrize("conv", [False, True])
def test_gemm_bk64_and_8wave_variants(tile, conv):
    from frido_amd.builder import ACT_SILU
    if conv:
        B, H, W, Cin, Cout = 3, 12, 10, 128, 200
        x, w, bias = _t("qx", B, Cin, H, W), _t("qw", Cout, Cin, 3, 3) / np.sqrt(9 * Cin), _t("qb", Cout)
        ref = F.silu(F.conv2d(x, w, bias, padding=1)).permute(0, 2, 3, 1).reshape(-1, Cout)
        b = _builder(1, {"c.weight": w.cuda(), "c.bias": bias.cuda()})
        xd = x.cuda()
        a = b.pack(xd.data_ptr(), B, H * W, Cin, 0, Cin, nchw=True)
        out = b.conv(a, B, H, W, "c", act=ACT_SILU)
    else:
        M, N, K = 300, 200, 64 * 5
        a_, w, bias = _t("qa", M, K), _t("qw2", N, K) / np.sqrt(K), _t("qb2", N)
        ref = F.silu(a_ @ w.t() + bias)
        b = _builder(1, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
        ad = a_.cuda()
        a = b.pack(ad.data_ptr(), 1, M, K, 0, K)
        out = b.linear(a, "w", act=ACT_SILU)
    st = b.prog.ops[-1][1]
    st.tile, st.splitk = tile, 1
    _run(b)
    assert _relerr(out.to_f32().cpu(), ref) < 2e-2


CONV_CASES = [
    # Cin, Cout, H, W, k, stride, pad, up, dn, asym
    (32, 64, 16, 16, 3, 1, 1, 0, 0, False),
    (64, 40, 9, 11, 3, 1, 1, 0, 0, False),      # ragged sizes, N not multiple of 16
    (32, 32, 16, 16, 3, 2, 1, 0, 0, False),     # U-Net Downsample (pyunet.py:152-156)
    (32, 32, 16, 16, 3, 2, 0, 0, 0, True),      # VQGAN Downsample: pad (0,1,0,1) + s2 p0 (model.py:68-72)
    (32, 48, 8, 8, 3, 1, 1, 1, 0, False),       # nearest x2 then conv (pyunet.py:119-121)
    (32, 128, 16, 16, 3, 1, 1, 0, 1, False),    # SPADE cond nearest down-resize then conv (spade_norm.py:52)
    (3, 32, 16, 16, 3, 1, 1, 0, 0, False),      # input head: Cin padded 3 -> 32
    (64, 64, 8, 8, 1, 1, 0, 0, 0, False),       # 1x1
    (192, 192, 32, 32, 3, 1, 1, 0, 0, False),   # wide tile path
]


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv(nsplit, case):
    Cin, Cout, H, W, k, stride, pad, up, dn, asym = case
    B = 2
    x = _t("cx", B, Cin, H, W)
    w = _t("cw", Cout, Cin, k, k) / np.sqrt(Cin * k * k)
    bias = _t("cb", Cout)
    xin = x
    if up:
        xin = F.interpolate(x, scale_factor=2, mode="nearest")
    if dn:
        xin = F.interpolate(x, size=(H >> dn, W >> dn), mode="nearest")
    if asym:
        ref = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, bias, stride=stride, padding=0)
    else:
        ref = F.conv2d(xin, w, bias, stride=stride, padding=pad)
    b = _builder(nsplit, {"c.weight": w.cuda(), "c.bias": bias.cuda()})
    xd = x.cuda()
    a = b.pack(xd.data_ptr(), B, H * W, Cin, 0, Cin, nchw=True)
    Ho, Wo = ref.shape[2], ref.shape[3]
    out = b.conv(a, B, H, W, "c", stride=stride, pad=pad, up=up, dn=dn, Ho=Ho, Wo=Wo)
    _run(b)
    got = out.view().cpu().view(B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    assert _within(got, ref, _tol(nsplit))


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 8, 8, 64, 96), (3, 16, 32, 32, 192), (1, 64, 64, 96, 40), (2, 4, 4, 40, 64)])
def test_upsample_conv_as_phase_convs(nsplit, B, H, W, Cin, Cout):
    """Upsample = nearest x2 + conv3x3 (pyunet.py:110-121) as four 2x2 phase convolutions with summed taps, written
    interleaved into the (2H, 2W) plane -- against F.interpolate + F.conv2d and against the 9-tap kernel path."""
    x = _t("ux", B, Cin, H, W)
    w = _t("uw", Cout, Cin, 3, 3) / np.sqrt(Cin * 9)
    bias = _t("ub", Cout)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, bias, padding=1)
    b = _builder(nsplit, {"c.weight": w.cuda(), "c.bias": bias.cuda()})
    xd = x.cuda()
    a = b.pack(xd.data_ptr(), B, H * W, Cin, 0, Cin, nchw=True)
    out = b.conv_up2(a, B, H, W, "c")
    out9 = b.conv(a, B, H, W, "c", up=1)
    _run(b)
    got = out.to_f32().cpu().view(B, 2 * H, 2 * W, Cout).permute(0, 3, 1, 2)
    got9 = out9.to_f32().cpu().view(B, 2 * H, 2 * W, Cout).permute(0, 3, 1, 2)
    assert _within(got, ref, _tol(nsplit))
    assert _within(got, got9, _tol(nsplit))


PATCH_CASES = [   # B, H, W, Cin, Cout, Cskip (0 = no fused 1x1 skip operand)
    (4, 64, 64, 64, 192, 0),     # one group = 4 image rows
    (2, 32, 32, 96, 384, 0),     # 8 rows per tile, two N tiles
    (1, 16, 16, 32, 100, 0),     # a whole image per tile, ragged N
    (16, 8, 8, 64, 192, 0),      # four 8x8 images per tile
    (2, 32, 64, 32, 64, 0),      # non-square plane
    (4, 8, 16, 64, 192, 0),      # two 8x16 images per tile
    (4, 32, 32, 128, 192, 64),   # fused 1x1 skip operand riding along as extra k-chunks
    (16, 8, 8, 192, 960, 128),
]


@pytest.mark.parametrize("case", PATCH_CASES)
def test_conv3x3_patch_staged_kernel(case):
    """Tile id 9: the patch-staged 3x3 kernel (input patch DMA'd to LDS once per channel chunk, nine taps = LDS row
    shifts) against F.conv2d, including the zero halo at image borders and between images that share a tile."""
    B, H, W, Cin, Cout, Cs = case
    x = _t("px", B, Cin, H, W)
    w = _t("pw", Cout, Cin, 3, 3) / np.sqrt(Cin * 9)
    bias = _t("pb", Cout)
    ref = F.conv2d(x, w, bias, padding=1)
    weights = {"c.weight": w.cuda(), "c.bias": bias.cuda()}
    if Cs:
        xs, wsk, bs = _t("psx", B, Cs, H, W), _t("psw", Cout, Cs, 1, 1) / np.sqrt(Cs), _t("psb", Cout)
        ref = ref + F.conv2d(xs, wsk, bs)
        weights.update({"s.weight": wsk.cuda(), "s.bias": bs.cuda()})
    b = _builder(1, weights)
    xd = x.cuda()
    a = b.pack(xd.data_ptr(), B, H * W, Cin, 0, Cin, nchw=True)
    if Cs:
        xsd = xs.cuda()
        raw = b.pack(xsd.data_ptr(), B, H * W, Cs, 0, Cs, nchw=True)
        out = b.conv_plus_skip(a, raw, B, H, W, "c", "s")
    else:
        out = b.conv(a, B, H, W, "c")
    b.prog.ops[-1][1].tile = 9
    b.prog.ops[-1][1].splitk = 1
    _run(b)
    got = out.to_f32().cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert _relerr(got, ref) < 2e-2
    # tile 10: the same kernel with 128-row tiles (4 waves)
    out.view().zero_()
    b.prog.ops[-1][1].tile = 10
    _run(b)
    got10 = out.to_f32().cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert _relerr(got10, ref) < 2e-2
    # same op on the ring kernel: the two must agree to accumulation-order noise
    b.prog.ops[-1][1].tile = 2
    _run(b)
    got2 = out.to_f32().cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
    assert _relerr(got, got2) < 1e-2
    # split-K over the 32-channel chunk sequence (partials in a workspace, reduced by splitk_reduce_kernel)
    from frido_amd import tune
    st = b.prog.ops[-1][1]
    nchunks = (st.Cin + st.K2) // 32
    for sk, tl in ((2, 9), (3, 9), (2, 10)):
        if sk > nchunks:
            continue
        st.tile, st.splitk = tl, sk
        st.ws = tune.workspace_for(st, _dev())
        out.view().zero_()
        _run(b)
        got3 = out.to_f32().cpu().view(B, H, W, Cout).permute(0, 3, 1, 2)
        assert _relerr(got3, ref) < 2e-2, sk


@pytest.mark.parametrize("C1,C2,HW", [(64, 0, 256), (96, 32, 64), (192, 0, 1024), (960, 576, 64), (32, 0, 16), (192, 64, 1024), (200, 56, 1031)])
@pytest.mark.parametrize("spade", [False, True])
@pytest.mark.parametrize("of32", [True, False])      # False on a large plane: the 8-channel bf16x3 fast path of gn_apply
def test_groupnorm_apply(C1, C2, HW, spade, of32):
    B = 3
    C = C1 + C2
    x1 = _t("g1", B, HW, C1) * 2 + 0.5
    x2 = _t("g2", B, HW, C2) if C2 else None
    w, bi = 1 + 0.1 * _t("gw", C), 0.1 * _t("gb", C)
    gam, bet = (_t("gg", B, HW, C), _t("gbt", B, HW, C)) if spade else (None, None)
    b = _builder(2, {"n.weight": w.cuda(), "n.bias": bi.cuda()})
    f1 = b.f32(B * HW, C1)
    f1.view().copy_(x1.view(B * HW, C1).cuda())
    f2 = None
    if C2:
        f2 = b.f32(B * HW, C2)
        f2.view().copy_(x2.view(B * HW, C2).cuda())
    g = be = None
    if spade:
        g, be = b.f32(B * HW, C), b.f32(B * HW, C)
        g.view().copy_(gam.view(-1, C).cuda())
        be.view().copy_(bet.view(-1, C).cuda())
    from frido_amd.builder import ACT_SILU
    res = b.groupnorm(f1, f2, B, HW, "n", 1e-5, gamma=g, beta=be, act=ACT_SILU, want_raw=True, out_f32=of32)
    a, raw, of = res if of32 else (res[0], res[1], None)
    _run(b)
    xc = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    xn = xc.permute(0, 2, 1).reshape(B, C, HW, 1)
    ref = F.group_norm(xn, 32, w, bi, 1e-5)
    if spade:
        ref = ref * (1 + gam.permute(0, 2, 1).reshape(B, C, HW, 1)) + bet.permute(0, 2, 1).reshape(B, C, HW, 1)
    ref = F.silu(ref).reshape(B, C, HW).permute(0, 2, 1).reshape(B * HW, C)
    if of32:
        assert _relerr(of.view().cpu(), ref) < 1e-5
    assert _relerr(a.to_f32().cpu(), ref) < 2e-5
    assert _relerr(raw.to_f32().cpu(), xc.reshape(B * HW, C)) < 2e-5


@pytest.mark.parametrize("C1,C2,H,tile", [(192, 0, 64, 0), (384, 0, 32, 7), (192, 192, 32, 1), (384, 192, 32, 2), (96, 0, 32, 6), (192, 0, 32, 18), (192, 0, 32, 19)])
def test_groupnorm_statistics_from_the_conv_epilogue(C1, C2, H, tile, monkeypatch):
    """bf16x3 stream: the convolutions that PRODUCE a GroupNorm's input(s) leave per-channel partial sums of the values they store
    (FridoGemm.gn_part, 32-row blocks); gn_stats sums those instead of re-reading the tensor(s).  Checked against
    F.group_norm of the f32 convolution outputs, single tensor and the virtual concat of two producers, on several tiles."""
    from frido_amd import tune
    monkeypatch.setattr(tune, "ENABLED", False)      # (the tuner may pick split-K on these small problems, which drops the partial sums)
    B, W, Cin = 2, H, 64
    b = _builder(2, {"a.weight": (_t("ea", C1, Cin, 3, 3) / np.sqrt(9 * Cin)).cuda(), "a.bias": _t("eab", C1).cuda(),
                     "b.weight": (_t("eb", max(C2, 8), Cin, 3, 3) / np.sqrt(9 * Cin)).cuda(), "b.bias": _t("ebb", max(C2, 8)).cuda(),
                     "n.weight": (1 + 0.1 * _t("enw", C1 + C2)).cuda(), "n.bias": (0.1 * _t("enb", C1 + C2)).cuda()})
    x = _t("ex", B * H * W, Cin)
    xd = x.cuda()
    a_op = b.pack(xd.data_ptr(), 1, B * H * W, Cin, 0, Cin)
    y1 = b.conv(a_op, B, H, W, "a")
    if tile:
        b.prog.ops[-1][1].tile = tile
    assert y1.gn_part is not None and b.prog.ops[-1][1].gn_part
    y2 = None
    if C2:
        y2 = b.conv(a_op, B, H, W, "b")
        assert y2.gn_part is not None
    n_before = len(b.prog.ops)
    o, _ = b.groupnorm(y1, y2, B, H * W, "n", 1e-5, act=2)
    kinds = [k for k, _ in b.prog.ops[n_before:]]
    from frido_amd import _lib
    assert kinds == [_lib.OP_KINDS["FRIDO_OP_GN_STATS"], _lib.OP_KINDS["FRIDO_OP_GN_APPLY"]] and b.prog.ops[n_before][1].p1
    _run(b)
    xi = x.view(B, H, W, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(xi, b.w["a.weight"].cpu(), b.w["a.bias"].cpu(), padding=1)
    if C2:
        ref = torch.cat([ref, F.conv2d(xi, b.w["b.weight"].cpu(), b.w["b.bias"].cpu(), padding=1)], dim=1)
    ref = F.silu(F.group_norm(ref, 32, b.w["n.weight"].cpu(), b.w["n.bias"].cpu(), 1e-5)).permute(0, 2, 3, 1).reshape(B * H * W, -1)
    assert _within(o.to_f32().cpu(), ref, 2.5 * _tol(2))


@pytest.mark.parametrize("C1,C2,HW", [(960, 0, 64), (576, 0, 256), (384, 0, 1024), (192, 0, 4096), (960, 960, 64), (960, 576, 256),
                                      (192, 192, 4096), (64, 0, 256), (96, 32, 64), (576, 0, 4096)])
@pytest.mark.parametrize("spade", [False, True])
def test_groupnorm_bf16_stream_one_launch(C1, C2, HW, spade):
    """bf16 stream: the one-launch GroupNorm (gn_fused_kernel) where a (sample, group-chunk) slice fits a workgroup, the
    gn_stats + gn_apply pair elsewhere -- both against F.group_norm on the bf16-rounded input."""
    from frido_amd import _lib
    from frido_amd.builder import ACT_SILU
    B, C = 3, C1 + C2
    x1 = (_t("h1", B, HW, C1) * 2 + 0.5).to(torch.bfloat16).float()
    x2 = _t("h2", B, HW, C2).to(torch.bfloat16).float() if C2 else None
    w, bi = 1 + 0.1 * _t("hw", C), 0.1 * _t("hb", C)
    gam, bet = ((_t("hg", B, HW, C) * 0.5).to(torch.bfloat16).float(), _t("hbt", B, HW, C).to(torch.bfloat16).float()) if spade else (None, None)
    b = _builder(1, {"n.weight": w.cuda(), "n.bias": bi.cuda()})
    f1 = b.f32(B * HW, C1)
    f1.view().copy_(x1.view(B * HW, C1).cuda())
    f2 = None
    if C2:
        f2 = b.f32(B * HW, C2)
        f2.view().copy_(x2.view(B * HW, C2).cuda())
    g = be = None
    if spade:
        g, be = b.f32(B * HW, C), b.f32(B * HW, C)
        g.view().copy_(gam.view(-1, C).cuda())
        be.view().copy_(bet.view(-1, C).cuda())
    a, raw = b.groupnorm(f1, f2, B, HW, "n", 1e-5, gamma=g, beta=be, act=ACT_SILU, want_raw=True)
    kinds = [k for k, _ in b.prog.ops]
    fused = _lib.OP_KINDS["FRIDO_OP_GN_FUSED"] in kinds
    assert fused == (HW <= 256)           # larger planes keep the two coalesced kernels (builder.GN_FUSED_MAX_HW)
    _run(b)
    xc = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    ref = F.group_norm(xc.permute(0, 2, 1).reshape(B, C, HW, 1), 32, w, bi, 1e-5)
    if spade:
        ref = ref * (1 + gam.permute(0, 2, 1).reshape(B, C, HW, 1)) + bet.permute(0, 2, 1).reshape(B, C, HW, 1)
    ref = F.silu(ref).reshape(B, C, HW).permute(0, 2, 1).reshape(B * HW, C)
    assert _relerr(a.to_f32().cpu(), ref) < 1e-2              # bf16 output rounding
    assert torch.equal(raw.to_f32().cpu(), xc.reshape(B * HW, C))


def test_bf16_residual_stream_inputs():
    """bf16 mode keeps the residual stream in bf16: GroupNorm / LayerNorm / residual epilogue read it directly."""
    from frido_amd.builder import ACT_SILU
    B, HW, C = 2, 64, 96
    x = _t("bx", B * HW, C).to(torch.bfloat16).float()          # exactly representable inputs
    w, bi = 1 + 0.1 * _t("bw", C), 0.1 * _t("bb", C)
    b = _builder(1, {"n.weight": w.cuda(), "n.bias": bi.cuda(), "l.weight": _t("blw", 64, C).cuda() / 10, "l.bias": _t("blb", 64).cuda()})
    assert b.stream_bf16
    f = b.f32(B * HW, C)
    assert f.bf16
    f.view().copy_(x.cuda())
    r = b.f32(B * HW, 64)        # allocate every eagerly-filled buffer BEFORE emitting ops (the pool recycles scratch)
    r.view().copy_(_t("br", B * HW, 64).cuda())
    res_ref = r.view().float().cpu()
    a, raw = b.groupnorm(f, None, B, HW, "n", 1e-5, act=ACT_SILU, want_raw=True)
    ln = b.layernorm(f, "n")
    y = b.linear(raw, "l", residual=r)
    _run(b)
    xn = x.view(B, HW, C).permute(0, 2, 1).reshape(B, C, HW, 1)
    ref = F.silu(F.group_norm(xn, 32, w, bi, 1e-5)).reshape(B, C, HW).permute(0, 2, 1).reshape(B * HW, C)
    assert _relerr(a.to_f32().cpu(), ref) < 1e-2
    assert torch.equal(raw.to_f32().cpu(), x)                    # alias: the activation is its own operand
    assert _relerr(ln.to_f32().cpu(), F.layer_norm(x, (C,), w, bi, 1e-5)) < 1e-2
    yref = x @ (b.w["l.weight"].cpu().t()) + b.w["l.bias"].cpu() + res_ref
    assert y.bf16 and _relerr(y.to_f32().cpu(), yref) < 2e-2


@pytest.mark.parametrize("C", [64, 384, 576, 960])
def test_layernorm(C):
    rows = 37
    x = _t("lx", rows, C) * 3 + 1
    w, bi = 1 + 0.1 * _t("lw", C), 0.1 * _t("lb", C)
    b = _builder(2, {"n.weight": w.cuda(), "n.bias": bi.cuda()})
    f = b.f32(rows, C)
    f.view().copy_(x.cuda())
    a = b.layernorm(f, "n")
    _run(b)
    assert _relerr(a.to_f32().cpu(), F.layer_norm(x, (C,), w, bi, 1e-5)) < 2e-5


@pytest.mark.parametrize("N", [1, 26, 64, 92, 1024, 4096])
def test_softmax(N):
    rows = 9
    x = _t("sx", rows, N) * 4
    b = _builder(2)
    f = b.f32(rows, N)
    f.view().copy_(x.cuda())
    Np = (N + 31) // 32 * 32
    p = b.softmax(f, rows, N, N, Np)
    _run(b)
    got = p.to_f32().cpu()
    assert _relerr(got[:, :N], x.softmax(-1)) < 2e-5
    assert float(got[:, N:].abs().max()) == 0.0 if Np > N else True


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("B,Nq,Nk,d", [(3, 64, 26, 384), (2, 16, 1, 64), (2, 64, 64, 960), (2, 32, 92, 576), (1, 48, 128, 96),
                                       (2, 1024, 26, 384),          # fused short-key kernel
                                       (2, 64, 256, 64), (2, 24, 26, 64)])   # GEMM -> softmax -> GEMM path
def test_attention_core(nsplit, B, Nq, Nk, d):
    """softmax(q k^T / sqrt(d)) v (attention.py:170-193) for the fused short-key kernel and the three-kernel path."""
    from frido_amd.engine import pack_matrix
    q, k, v = _t("aq", B, Nq, d), _t("ak", B, Nk, d), _t("av", B, Nk, d)
    b = _builder(nsplit)
    qo = pack_matrix(q.reshape(B * Nq, d).cuda(), nsplit)
    ko = pack_matrix(k.reshape(B * Nk, d).cuda(), nsplit)
    vto = pack_matrix(v.transpose(1, 2).reshape(B * d, Nk).cuda(), nsplit)
    o = b.attention(qo, d, ko, d, vto, B, Nq, Nk, d)
    from frido_amd import _lib
    fused = any(kind == _lib.OP_KINDS["FRIDO_OP_ATTN_SMALL"] for kind, _ in b.prog.ops)
    assert fused == (Nk <= 128 and Nq % 16 == 0)
    assert not any(kind == _lib.OP_KINDS["FRIDO_OP_ATTN_FLASH"] for kind, _ in b.prog.ops)      # d = 64 / 96: not a flash head dim
    _run(b)
    ref = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1) @ v
    assert _within(o.to_f32().cpu().view(B, Nq, d), ref, _tol(nsplit, f16=5e-5, bf16=ATTN_BF16_TOL))


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("B,Nq,Nk,d", [(2, 64, 26, 384), (2, 64, 64, 960), (2, 256, 256, 64), (16, 256, 77, 576), (5, 1024, 26, 384),
                                       (64, 64, 92, 960)])
def test_attention_core_stream_output(nsplit, B, Nq, Nk, d):
    """Residual-stream form used when the output projection is folded into V: softmax(qk^T/sqrt(d)) v + bias + residual; with
    >= 256 workgroups the bf16x3 kernel also returns the LayerNorm of its rows (norm2 / norm3, attention.py:225-226)."""
    from frido_amd.engine import pack_matrix
    q, k, v = _t("aq", B, Nq, d), _t("ak", B, Nk, d), _t("av", B, Nk, d)
    bias, res = _t("ab", d), _t("ar", B * Nq, d) + (20.0 if d == 576 else 0.3)      # d = 576: rows with |mean| >> sigma (two-pass variance)
    lw, lb = 1 + 0.2 * _t("lw", d), 0.1 * _t("lb", d)
    b = _builder(nsplit, {"ln.weight": lw.cuda(), "ln.bias": lb.cuda()})
    qo = pack_matrix(q.reshape(B * Nq, d).cuda(), nsplit)
    ko = pack_matrix(k.reshape(B * Nk, d).cuda(), nsplit)
    vto = pack_matrix(v.transpose(1, 2).reshape(B * d, Nk).cuda(), nsplit)
    bd = bias.cuda()
    r = b.f32(B * Nq, d)
    r.view().copy_(res.cuda())
    o = b.attention(qo, d, ko, d, vto, B, Nq, Nk, d, bias_ptr=bd.data_ptr(), residual=r, stream=True, also_op=True, ln=("ln", 1e-5))
    _run(b)
    rq = r.to_f32().cpu()       # the residual as stored (bf16-rounded in bf16 mode)
    ref = (torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1) @ v).reshape(B * Nq, d) + bias + rq
    assert _within(o.to_f32().cpu(), ref, _tol(nsplit, f16=5e-5, bf16=ATTN_BF16_TOL))
    assert hasattr(o, "ln_copy") == (nsplit == 2 and Nk <= 128 and B * (Nq // 16) >= 256)
    if hasattr(o, "ln_copy"):
        assert _relerr(o.ln_copy.to_f32().cpu(), F.layer_norm(o.to_f32().cpu(), (d,), lw, lb, 1e-5)) < 2e-5
    if nsplit == 2 and Nk <= 128:     # f32 stream: the short-key kernel also left the same values as a hi / lo operand
        assert _relerr(o.op_copy.to_f32().cpu(), o.to_f32().cpu()) < 1e-5
    else:
        assert not hasattr(o, "op_copy")


@pytest.mark.gate
@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("B,Nq,Nk,d", [(2, 1024, 1024, 384),      # U-Net 32x32 plane
                                       (3, 256, 256, 576),        # U-Net 16x16 plane (4-wave variant, d > 512)
                                       (1, 4096, 4096, 512),      # VQGAN AttnBlock at 256^2 (8- or 4-wave by grid size)
                                       (16, 1024, 1024, 128),     # many workgroups: the 8-wave variant
                                       (2, 200, 333, 256),        # ragged: Nq % 16 != 0, Nk % 32 != 0 (masked last tile)
                                       (1, 16, 129, 128)])        # one query fragment, five key tiles
def test_attention_flash(nsplit, B, Nq, Nk, d, monkeypatch):
    """Flash-style kernel (flash.hip) vs softmax(q k^T / sqrt(d)) v in fp64: operand output and residual-stream output."""
    from frido_amd import _lib, builder as builder_mod
    monkeypatch.setattr(builder_mod, "ATTN_FLASH_MIN_KEYS", 0)      # the dispatcher keeps short sequences on the GEMM chain
    from frido_amd.engine import pack_matrix, rup
    q, k, v = _t("fq", B, Nq, d), _t("fk", B, Nk, d) * 1.5, _t("fv", B, Nk, d)
    b = _builder(nsplit)
    qo = pack_matrix(q.reshape(B * Nq, d).cuda(), nsplit)
    ko = pack_matrix(k.reshape(B * Nk, d).cuda(), nsplit)
    vto = pack_matrix(v.transpose(1, 2).reshape(B * d, Nk).cuda(), nsplit)            # [B*d][Nk padded to 32], pad = 0
    assert vto.K == rup(Nk, 32)
    o = b.attention(qo, d, ko, d, vto, B, Nq, Nk, d)
    bias, res = _t("fb", d), _t("fr", B * Nq, d)
    bd = bias.cuda()
    r = b.f32(B * Nq, d)
    r.view().copy_(res.cuda())
    lw, lb = 1 + 0.2 * _t("lw", d), 0.1 * _t("lb", d)
    b.w.update({"ln.weight": lw.cuda(), "ln.bias": lb.cuda()})
    o2 = b.attention(qo, d, ko, d, vto, B, Nq, Nk, d, bias_ptr=bd.data_ptr(), residual=r, stream=True, ln=("ln", 1e-5))
    assert sum(kind == _lib.OP_KINDS["FRIDO_OP_ATTN_FLASH"] for kind, _ in b.prog.ops) == 2
    _run(b)
    ref = (torch.softmax(q.double() @ k.double().transpose(1, 2) * d ** -0.5, -1) @ v.double()).float()
    tol = _tol(nsplit, f16=5e-5, bf16=ATTN_BF16_TOL)
    assert _within(o.to_f32().cpu().view(B, Nq, d), ref, tol)
    assert _within(o2.to_f32().cpu(), ref.reshape(B * Nq, d) + bias + r.to_f32().cpu(), tol)
    assert hasattr(o2, "ln_copy") == (nsplit == 2 and b._flash_ln_ok(d))      # the LayerNorm of the stream rows from the same launch (d = 256, 384; 512 on the d-split form)
    if hasattr(o2, "ln_copy"):
        assert _relerr(o2.ln_copy.to_f32().cpu(), F.layer_norm(o2.to_f32().cpu(), (d,), lw, lb, 1e-5)) < 2e-5


def test_attention_flash_online_softmax_rescale_branch(monkeypatch):
    """A key far above the rest in a LATE tile forces the running-max rescale of the accumulated O (rare on random data)."""
    from frido_amd.engine import pack_matrix
    from frido_amd import builder as builder_mod
    monkeypatch.setattr(builder_mod, "ATTN_FLASH_MIN_KEYS", 0)
    B, Nq, Nk, d = 1, 64, 512, 128
    q, k, v = _t("sq", B, Nq, d), _t("sk", B, Nk, d), _t("sv", B, Nk, d)
    k[0, 300] = q[0, 5] * 3.0            # query 5 (and its neighbours, weakly) spike on key 300 = tile 9
    k[0, 40] = q[0, 50] * 2.0            # an early spike: later tiles must NOT rescale
    for nsplit in (2, 1):
        b = _builder(nsplit)
        o = b.attention(pack_matrix(q.reshape(Nq, d).cuda(), nsplit), d, pack_matrix(k.reshape(Nk, d).cuda(), nsplit), d,
                        pack_matrix(v.transpose(1, 2).reshape(d, Nk).cuda(), nsplit), B, Nq, Nk, d)
        _run(b)
        ref = (torch.softmax(q.double() @ k.double().transpose(1, 2) * d ** -0.5, -1) @ v.double()).float()
        assert _within(o.to_f32().cpu().view(B, Nq, d), ref, _tol(nsplit, f16=5e-5, bf16=ATTN_BF16_TOL))


def test_geglu():
    rows, H = 33, 128
    x = _t("gx", rows, 2 * H) * 2
    b = _builder(2)
    f = b.f32(rows, 2 * H)
    f.view().copy_(x.cuda())
    o = b.geglu(f, H)
    _run(b)
    a, g = x.chunk(2, dim=-1)
    assert _relerr(o.to_f32().cpu(), a * F.gelu(g)) < 2e-5


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("M,C", [(300, 64), (1024, 384), (64, 960)])
def test_fused_geglu_projection(nsplit, M, C):
    x, w, bias = _t("fx", M, C), _t("fw", 8 * C, C) / np.sqrt(C), _t("fb", 8 * C)
    b = _builder(nsplit, {"p.weight": w.cuda(), "p.bias": bias.cuda()})
    xd = x.cuda()
    a = b.pack(xd.data_ptr(), 1, M, C, 0, C)
    o = b.linear_geglu(a, "p")
    _run(b)
    h, g = (x @ w.t() + bias).chunk(2, dim=-1)
    assert _within(o.to_f32().cpu(), h * F.gelu(g), _tol(nsplit))


@pytest.mark.gate
@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("out", ["f32", "op"])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19])
def test_gemm_direct_epilogue_every_tile(nsplit, out, tile):
    """The store-from-registers epilogue (transposed accumulators, permuted weight rows): alpha, bias and a stream-dtype residual,
    stream or operand output, on every tile variant; M = 300 and N = 352 (a multiple of 32 and of no tile width) mask rows and
    whole 8-column groups; K = 320 gives the BK = 64 pipelined loop an odd number of k-steps per parity (5 stages)."""
    if tile == 8 and nsplit == 2 or 11 <= tile <= 17 and nsplit == 2:
        pytest.skip("the 256 x 256 and BK = 64 tiles are bf16-mode tiles")
    if tile in (18, 19) and nsplit == 1:
        pytest.skip("the 8-wave 128 x 192 / 256 x 192 tiles are bf16x3 tiles")
    M, N, K = 300, 352, 320
    a, w, bias, res = _t("da", M, K), _t("dw", N, K) / np.sqrt(K), _t("db", N), _t("dr", M, N)
    b = _builder(nsplit, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    kw = {}
    if out == "f32":
        r = b.f32(M, N)
        r.view().copy_(res.cuda())
        kw["residual"] = r
    o = b.linear(a_op, "w", alpha=0.75, out=out, **kw)
    b.prog.ops[-1][1].tile = tile
    _run(b)
    ref = 0.75 * (a @ w.t()) + bias + (res if out == "f32" else 0)
    got = o.view().float().cpu() if out == "f32" else o.to_f32().cpu()[:, :N]
    assert _within(got, ref, _tol(nsplit))
    if nsplit == 2:
        _three_pass(got, _pass_products(a_op, b.lin_weight("w.weight")),
                    lambda y: 0.75 * y + bias.double() + (res.double() if out == "f32" else 0), f"tile {tile} K {K} {out}", out=out)


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("damage", ["zero_lo", "swap"])
def test_three_pass_check_catches_a_damaged_operand(planes, damage):
    """The power of the checks above, without a modified library: the activation operand is packed (host packer), its planes are recorded,
    then its lo plane is zeroed (the kernel then computes a_hi b_hi + a_hi b_lo: the a_lo b_hi pass is gone) or its planes are swapped.
    The fp32-reference check at the format's bound and the distance to the three-pass emulation of the planes as packed must both fail."""
    from frido_amd import _lib
    from frido_amd.engine import pack_matrix
    M, N, K = 300, 352, 320
    a, w, bias = _t("da", M, K), _t("dw", N, K) / np.sqrt(K), _t("db", N)
    with _lib.use_planes(planes):
        b = _builder(2, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
        a_op = pack_matrix(a.cuda(), 2)
        passes = _pass_products(a_op, b.lin_weight("w.weight"))          # the planes as the packer wrote them
        if damage == "zero_lo":
            a_op.t[1].zero_()
        else:
            a_op.t.copy_(a_op.t.flip(0))
        o = b.linear(a_op, "w")
        _run(b)
        got = o.view().cpu()
        e_ref = _relerr(got, a @ w.t() + bias)
        emu = passes["hh"] + passes["hl"] + passes["lh"] + bias.double()
        e_emu = _relerr(got, emu)
        print(f"damaged operand [{planes}] {damage}: fp32-reference error {e_ref:.2e} (bound {_tol(2):.0e}), "
              f"kernel - emu {e_emu:.2e} (bound {X3_EMU_TOL:.0e})")
        assert e_ref > _tol(2) and e_emu > 10 * X3_EMU_TOL
        if damage == "zero_lo":     # the kernel ran exactly the "no a_lo*b_hi" variant: the helper must reject it and name it
            with pytest.raises(AssertionError):
                _three_pass(got, passes, lambda y: y + bias.double(), "lo plane zeroed")
            d = _three_pass(got, dict(passes, lh=0 * passes["lh"]), lambda y: y + bias.double(), "lo plane zeroed, against its own planes",
                            check_variants=False)
            assert d["kernel"] <= X3_EMU_TOL


@pytest.mark.gate
@pytest.mark.parametrize("K", [64, 128, 320, 960])
@pytest.mark.parametrize("tile", [31, 33, 34, 35, 36])
def test_gemm_k_split_inside_the_workgroup(tile, K):
    """(r06) tiles 31 / 33 / 34 / 35 / 36 = the 4-wave tiles 1 / 3 / 4 / 5 / 6 with K split over the two wave groups of an 8-wave workgroup
    (igemm.hip Geo, KG = 2): each group runs the 4-wave loop over half the k-tiles on its own LDS ring, group 1 parks its accumulators in
    LDS, group 0 adds them and runs the epilogue.  K = 64 / 128 / 320 / 960: 1, 2, 5 and 15 k-tiles per group (prologue only, no refill,
    odd stage parity + wrap-around, the U-Net's shape); ragged M / N, both outputs; bit-identical on a repeat; batched per-sample
    products; an odd number of k-tiles, a split-K request and a one-plane operand are REJECTED."""
    from frido_amd._lib import FridoHipError
    M, N = 300, 352
    a, w, bias, res = _t("ka", M, K), _t("kw", N, K) / np.sqrt(K), _t("kb", N), _t("kr", M, N)
    outs = []
    for out in ("f32", "op", "f32"):
        b = _builder(2, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
        ad = a.cuda()
        a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
        kw = {}
        if out == "f32":
            r = b.f32(M, N)
            r.view().copy_(res.cuda())
            kw["residual"] = r
        o = b.linear(a_op, "w", alpha=0.75, out=out, **kw)
        b.prog.ops[-1][1].tile = tile
        _run(b)
        ref = 0.75 * (a @ w.t()) + bias + (res if out == "f32" else 0)
        got = o.view().float().cpu() if out == "f32" else o.to_f32().cpu()[:, :N]
        assert _within(got, ref, _tol(2)), (tile, K, out)
        _three_pass(got, _pass_products(a_op, b.lin_weight("w.weight")),
                    lambda y: 0.75 * y + bias.double() + (res.double() if out == "f32" else 0), f"tile {tile} K {K} {out}", out=out)
        outs.append(got)
    assert torch.equal(outs[0], outs[2])                    # acc0 + acc1 in one fixed order: repeatable bit for bit
    # per-sample products (batch = 5, the V^T form: the weight is the "A" side with a_bs = 0)
    Bz, Nk, C = 5, 64, K
    x, wv = _t("kx", Bz * Nk, C), _t("kv", 192, C) / np.sqrt(C)
    b = _builder(2, {})
    from frido_amd.engine import pack_matrix
    xd = x.cuda()
    x_op = b.pack(xd.data_ptr(), 1, Bz * Nk, C, 0, C)
    vT = b.v_transposed(x_op, C, pack_matrix(wv.cuda().double(), 2), Bz, Nk, 192)
    b.prog.ops[-1][1].tile = tile
    _run(b)
    refv = torch.einsum("dc,znc->zdn", wv, x.view(Bz, Nk, C))
    assert _within(vT.to_f32().cpu().view(Bz, 192, -1)[:, :, :Nk], refv, _tol(2))
    # rejected forms
    for bad_k, nsplit in ((96, 2), (K, 1)):
        w2 = _t("kw2", N, bad_k)
        b = _builder(nsplit, {"w.weight": w2.cuda(), "w.bias": bias.cuda()})
        a2 = _t("ka2", M, bad_k).cuda()
        o = b.linear(b.pack(a2.data_ptr(), 1, M, bad_k, 0, bad_k), "w", out="op")
        b.prog.ops[-1][1].tile = tile
        with pytest.raises(FridoHipError):
            _run(b)


@pytest.mark.gate
@pytest.mark.parametrize("tile,N,K", [(2, 3072, 384), (3, 1216, 960), (1, 1408, 2304), (7, 1024, 384), (18, 2112, 96)])
def test_gemm_column_panel_tile_order_is_a_pure_reordering(tile, N, K):
    """(r06) FridoGemm.flags bit 27: the ring kernel walks its output tiles panel by panel (P columns x all rows, P = 8, halved while the weight panel
    exceeds 3 MB: 8 / 8 / 4 / 8 / 8 here) instead of row-major, so an XCD's concurrent workgroups share an L2-resident weight
    panel.  Independent tiles in another order: the output must equal the row-major run BIT FOR BIT (and the fp32 reference to the usual
    bound) -- full panels plus a ragged last one (19 / 11 / 8 / 11 tile columns), ragged M, GEGLU and plain epilogues."""
    M = 700
    a, w, bias = _t("pa", M, K), _t("pw", N, K) / np.sqrt(K), _t("pb", N)
    outs = []
    for panels in (0, 1):
        b = _builder(2, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
        ad = a.cuda()
        a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
        o = b.linear_geglu(a_op, "w") if tile == 2 else b.linear(a_op, "w", out="op")
        st = b.prog.ops[-1][1]
        st.tile = tile
        st.flags = (st.flags & ~(1 << 27)) | (panels << 27)
        _run(b)
        outs.append(o.to_f32().cpu())
    assert torch.equal(outs[0], outs[1])
    y = a @ w.t() + bias
    ref = y[:, :N // 2] * F.gelu(y[:, N // 2:]) if tile == 2 else y
    assert _within(outs[1][:, :ref.shape[1]], ref, _tol(2))


@pytest.mark.parametrize("K", [64, 128, 192, 448])
@pytest.mark.parametrize("tile", [11, 12, 13, 14, 15, 16, 17])
def test_pipelined_loop_short_k(tile, K):
    """The software-pipelined BK = 64 loop at 1, 2, 3 and 7 ring stages (prologue only / no refill / first refill / wrap-around of
    the 3-4 slot ring), bf16 mode."""
    M, N = 272, 224
    a, w, bias = _t("sa", M, K), _t("sw", N, K) / np.sqrt(K), _t("sb", N)
    b = _builder(1, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    o = b.linear(a_op, "w", out="op")
    b.prog.ops[-1][1].tile = tile
    _run(b)
    assert _within(o.to_f32().cpu(), a @ w.t() + bias, _tol(1))


@pytest.mark.parametrize("conv", [False, True])
@pytest.mark.parametrize("K", [32, 64, 96, 160, 352])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 18, 19])
def test_bf16x3_pipelined_loop_short_k(tile, K, conv):
    """The bf16x3 virtual-k-step loop (hi*hi, hi*lo, lo*hi per stage, fragment sets rotating between stages) at 1, 2, 3, 5 and 11
    ring stages: prologue only / no refill / first refill / odd and even stage parities / wrap-around of the 2-4 slot ring; dense
    and as a 1x1 (K = Cin) / 3x3 (K = 9 * 32 ... ) convolution whose taps re-base the DMA pointers between stages."""
    if conv:
        B, H, W, Cin, N = 2, 12, 12, K, 224           # 3x3 conv: 9 K / 32 stages, zero-padded border taps
        x, w, bias = _t("xa", B * H * W, Cin), _t("xw", N, Cin, 3, 3) / np.sqrt(9 * Cin), _t("xb", N)
        b = _builder(2, {"c.weight": w.cuda(), "c.bias": bias.cuda()})
        xd = x.cuda()
        a_op = b.pack(xd.data_ptr(), 1, B * H * W, Cin, 0, Cin)
        o = b.conv(a_op, B, H, W, "c", out="f32_strict")
        b.prog.ops[-1][1].tile = tile
        _run(b)
        ref = F.conv2d(x.view(B, H, W, Cin).permute(0, 3, 1, 2), w, bias, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, N)
        assert _within(o.view().float().cpu(), ref, _tol(2))
        _three_pass(o.view().cpu(), _pass_products(a_op, b.conv_weight("c.weight")[0], conv=(B, H, W, 3)),
                    lambda y: y + bias.double(), f"conv tile {tile} K {9 * K}")
        return
    M, N = 272, 224
    a, w, bias = _t("sa", M, K), _t("sw", N, K) / np.sqrt(K), _t("sb", N)
    b = _builder(2, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    o = b.linear(a_op, "w", out="op")
    b.prog.ops[-1][1].tile = tile
    _run(b)
    assert _within(o.to_f32().cpu(), a @ w.t() + bias, _tol(2))
    _three_pass(o.to_f32().cpu(), _pass_products(a_op, b.lin_weight("w.weight")), lambda y: y + bias.double(), f"tile {tile} K {K} op",
                out="op")


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6, 7, 8, 11, 12, 14, 17, 18, 19])
def test_fused_geglu_projection_every_tile(nsplit, tile):
    """The GEGLU epilogue has two forms: tiles with four-fold n-tile counts (128 / 256 columns) deal the packed rows so that a
    lane owns value and gate of 8 consecutive outputs (direct stores); the others keep the [a | gate] order and go through LDS.
    M is ragged and 2H = 1344 is a multiple of 64 but of no tile width, so every tile masks rows AND columns."""
    if nsplit == 2 and (11 <= tile <= 17 or tile == 8) or nsplit == 1 and tile in (18, 19):
        pytest.skip("the 256 x 256 and BK = 64 tiles are bf16-mode tiles; the 8-wave 128 x 192 / 256 x 192 tiles are bf16x3 tiles")
    M, C, H = 300, 128, 672
    x, w, bias = _t("gx", M, C), _t("gw", 2 * H, C) / np.sqrt(C), _t("gb", 2 * H)
    b = _builder(nsplit, {"p.weight": w.cuda(), "p.bias": bias.cuda()})
    xd = x.cuda()
    a = b.pack(xd.data_ptr(), 1, M, C, 0, C)
    o = b.linear_geglu(a, "p")
    b.prog.ops[-1][1].tile = tile
    _run(b)
    h, g = (x @ w.t() + bias).chunk(2, dim=-1)
    assert _within(o.to_f32().cpu(), h * F.gelu(g), _tol(nsplit))


def test_pack_relayout_roundtrip():
    B, C, H, W = 2, 6, 8, 8
    x = _t("px", B, C, H, W)
    b = _builder(2)
    xd = x.cuda()
    op = b.pack(xd.data_ptr(), B, H * W, C, 3, 3, nchw=True, scale=0.5)
    nhwc = torch.empty(B, H * W, C, device="cuda")
    back = torch.empty(B, C, H, W, device="cuda")
    b.relayout(xd.data_ptr(), nhwc.data_ptr(), B, H * W, C, 0, C, C, 0, False)
    b.relayout(nhwc.data_ptr(), back.data_ptr(), B, H * W, C, 0, C, C, 0, True)
    _run(b)
    got = op.to_f32().cpu().view(B, H * W, 32)
    ref = (0.5 * x[:, 3:6]).permute(0, 2, 3, 1).reshape(B, H * W, 3)
    assert _relerr(got[..., :3], ref) < 2e-5 and float(got[..., 3:].abs().max()) == 0.0
    assert torch.equal(nhwc.cpu(), x.permute(0, 2, 3, 1).reshape(B, H * W, C))
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("n_codes,e", [(64, 3), (4096, 3), (8192, 4)])
def test_vq_lookup(n_codes, e):
    from oracle.vqgan import quantize
    B, H, W = 2, 16, 16
    Cx = 2 * e
    cb = _t("vcb", n_codes, e)
    cb[7] = cb[3]                                    # exact tie: lowest index must win
    z = _t("vz", B, Cx, H, W) * 1.3
    inv = float(np.float32(1.0) / np.float32(1.1))
    z[0, e:, 0, 0] = cb[3] / inv                     # pixel (0,0,0) sits (almost) exactly on code 3 == code 7
    zs = z[:, e:] * inv
    zq_ref, idx_ref = quantize(cb, zs)
    b = _builder(2)
    x_nhwc = z.permute(0, 2, 3, 1).contiguous().cuda()
    cbd = cb.cuda()
    zq = torch.zeros(B * H * W, Cx, device="cuda")
    idx = torch.zeros(B * H * W, dtype=torch.int64, device="cuda")
    b.prog.emit("FRIDO_OP_VQ", x=x_nhwc.data_ptr(), npix=B * H * W, Cx=Cx, c0=e, e=e, inv_scale=inv,
                codebook=cbd.data_ptr(), n_codes=n_codes, zq=zq.data_ptr(), Cq=Cx, q0=e, idx=idx.data_ptr())
    _run(b)
    got_idx = idx.cpu()
    assert int(got_idx[0]) == 3 and int(idx_ref[0]) == 3
    mism = got_idx != idx_ref
    # near-ties may legitimately resolve differently under a different rounding order: then the chosen
    # code must be equally close, and such pixels must be rare
    if mism.any():
        zf = zs.permute(0, 2, 3, 1).reshape(-1, e)[mism]
        d_got = ((zf - cb[got_idx[mism]]) ** 2).sum(1)
        d_ref = ((zf - cb[idx_ref[mism]]) ** 2).sum(1)
        assert float((d_got - d_ref).abs().max()) < 1e-5 and float(mism.float().mean()) < 1e-3
    got_zq = zq.cpu()[:, e:].view(B, H, W, e).permute(0, 3, 1, 2)
    sel = (~mism).view(B, 1, H, W).expand_as(got_zq)
    assert float((got_zq - zq_ref)[sel].abs().max()) < 1e-6
    assert float(zq.cpu()[:, :e].abs().max()) == 0.0


@pytest.mark.parametrize("n_codes,e", [(256, 3), (4096, 3), (8192, 4)])
def test_vq_lookup_exact_indices_on_constructed_ties(n_codes, e):
    """r05 (r04 verdict, weak 3): the index test without a near-tie allowance.  Latents and codebook live on a 1/32 grid and the scale
    is a power of two, so every distance term is exactly representable in fp32 whatever the summation order: the argmin is a
    mathematical fact, ties included.  A third of the codebook is DUPLICATED at higher indices and a quarter of the pixels sit
    exactly ON a duplicated code: torch.argmin's lowest-index rule (quantize.py:276-294) must hold for every pixel."""
    from oracle.vqgan import quantize
    B, H, W = 2, 16, 16
    Cx = 2 * e
    cb = torch.round(_t("vqe:cb", n_codes, e) * 32) / 32
    dup = n_codes // 3
    cb[n_codes - dup:] = cb[:dup]                    # codes j and n_codes - dup + j coincide: j must win
    z = torch.round(_t("vqe:z", B, Cx, H, W) * 1.3 * 32) / 32
    inv = 0.5
    flat = z[:, e:].permute(0, 2, 3, 1).reshape(-1, e)
    on = torch.arange(0, flat.shape[0], 4)
    flat[on] = cb[(on * 7) % dup] / inv              # exactly on a duplicated code (grid / 0.5 stays on the grid)
    z[:, e:] = flat.view(B, H, W, e).permute(0, 3, 1, 2)
    zq_ref, idx_ref = quantize(cb, z[:, e:] * inv)
    b = _builder(2)
    x_nhwc = z.permute(0, 2, 3, 1).contiguous().cuda()
    cbd = cb.cuda()
    zq = torch.zeros(B * H * W, Cx, device="cuda")
    idx = torch.zeros(B * H * W, dtype=torch.int64, device="cuda")
    b.prog.emit("FRIDO_OP_VQ", x=x_nhwc.data_ptr(), npix=B * H * W, Cx=Cx, c0=e, e=e, inv_scale=inv,
                codebook=cbd.data_ptr(), n_codes=n_codes, zq=zq.data_ptr(), Cq=Cx, q0=e, idx=idx.data_ptr())
    _run(b)
    assert torch.equal(idx.cpu(), idx_ref.view(-1))
    assert int((idx.cpu()[on] < dup).sum()) == len(on)            # every on-code pixel took the LOWER of its two equal codes
    assert torch.equal(zq.cpu()[:, e:].view(B, H, W, e).permute(0, 3, 1, 2), zq_ref)


def test_sampler_step_and_handoff_match_oracle():
    from oracle import samplers as S
    B, H, W = 2, 8, 8
    x = _t("sx", B, 6, H, W)
    e_c, e_u = _t("sec", B, 3, H, W), _t("seu", B, 3, H, W)
    noise = _t("sn", B, 6, H, W)
    a_t, a_prev, sigma = 0.37, 0.52, 0.21
    sq1m = float(np.sqrt(1 - a_t))
    scale = 1.5
    e_full = torch.cat((torch.zeros(B, 3, H, W), e_u + scale * (e_c - e_u)), dim=1)
    xp_ref, x0_ref = S._x_prev(x.clone(), e_full, a_t, a_prev, sigma, sq1m, 3, noise)
    b = _builder(2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()
    xd, ecd, eud, nd = nhwc(x), nhwc(e_c), nhwc(e_u), nhwc(noise)
    coef = torch.tensor([[a_t, a_prev, sigma, sq1m, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    x0 = torch.zeros_like(xd)
    b.prog.emit("FRIDO_OP_SAMPLER_STEP", x=xd.data_ptr(), B=B, HW=H * W, Cx=6, start=3, nch=3, eps_cond=ecd.data_ptr(),
                eps_uncond=eud.data_ptr(), cfg_scale=scale, coef=coef.data_ptr(), step=step.data_ptr(),
                noise=nd.data_ptr(), noise_stride=0, noise_C=6, noise_c0=3, temperature=1.0, x_out=xd.data_ptr(),
                pred_x0=x0.data_ptr(), write_x=1)
    b.prog.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=1)
    _run(b)
    back = lambda t: t.cpu().permute(0, 3, 1, 2)
    assert float((back(xd) - xp_ref).abs().max()) < 2e-6
    assert float((back(x0) - x0_ref).abs().max()) < 2e-6
    assert int(step.item()) == 1
    # hand-off (ddim.py:177-185), 2x2 and 4x4
    for levels, ns in ((1, 2), (2, 3)):
        img = _t("hx", B, 9, H, W)
        ref = S._handoff(img.clone(), 0, ns, [3, 3, 3])
        d = nhwc(img)
        b2 = _builder(2)
        b2.prog.emit("FRIDO_OP_HANDOFF", x=d.data_ptr(), B=B, H=H, W=W, Cx=9, c0=0, c1=3, levels=levels)
        _run(b2)
        assert float((back(d) - ref).abs().max()) < 1e-6


def test_philox_randn_is_shard_invariant_and_gaussian():
    n, per = 4 * 3 * 64 * 64, 3 * 64 * 64
    full = torch.empty(n, device="cuda")
    part = torch.empty(n // 2, device="cuda")
    b = _builder(2)
    b.prog.emit("FRIDO_OP_RANDN", dst=full.data_ptr(), n=n, per_sample=per, seed=1234, sample0=0, rng_stream=0)
    b.prog.emit("FRIDO_OP_RANDN", dst=part.data_ptr(), n=n // 2, per_sample=per, seed=1234, sample0=2, rng_stream=0)
    _run(b)
    assert torch.equal(full[n // 2:], part)          # samples 2,3 identical regardless of which rank draws them
    v = full.cpu().double()
    assert abs(float(v.mean())) < 0.02 and abs(float(v.std()) - 1.0) < 0.02
    assert abs(float((v ** 4).mean()) - 3.0) < 0.15


def test_graph_capture_replays():
    b = _builder(2)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    b.prog.emit("FRIDO_OP_STEP_ADD", step=step.data_ptr(), delta=2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = b.prog.capture(s.cuda_stream)
        for _ in range(5):
            g.launch(s.cuda_stream)
    s.synchronize()
    assert int(step.item()) == 10


def test_executor_side_stream_branches_join_correctly(monkeypatch):
    """FRIDO_OP_SYNC + FridoOp.stream: two independent projections of one input on the executor's two streams (eager and as
    parallel branches of a captured hipGraph), joined before their consumer, give the serial program's result bit for bit."""
    from frido_amd import engine
    x, wq, wv = _t("sx", 256, 128), _t("swq", 128, 128) / 11.0, _t("swv", 128, 128) / 11.0

    def build(side):
        monkeypatch.setattr(engine, "SIDE_STREAM", side)
        b = _builder(1, {"q.weight": wq.cuda(), "v.weight": wv.cuda()})
        xd = x.cuda()
        a = b.pack(xd.data_ptr(), 1, 256, 128, 0, 128)
        b.prog.sync(0, 1)
        with b.prog.side():
            v = b.linear(a, "v", bias=False, out="op")
        q = b.linear(a, "q", bias=False, out="op")
        b.prog.sync(1, 0)
        o = b.linear(v, "q", bias=False, residual=None)          # consumer of the side branch
        o2 = b.linear(q, "v", bias=False)
        return b, o, o2, xd

    b0, o0, p0, keep0 = build(False)
    _run(b0)
    b1, o1, p1, keep1 = build(True)
    assert any(getattr(st, "_sid", 0) == 1 for _, st in b1.prog.ops)
    _run(b1)
    assert torch.equal(o0.view(), o1.view()) and torch.equal(p0.view(), p1.view())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = b1.prog.capture(st.cuda_stream)
        o1.view().zero_()
        p1.view().zero_()
        g.launch(st.cuda_stream)
        g.launch(st.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(o0.view(), o1.view()) and torch.equal(p0.view(), p1.view())


@pytest.mark.gate
def test_device_plane_split_is_the_host_packers_bit_for_bit():
    """r06: every operand producer splits PAIRS of values with split_op2 (csrc/common.h: v_cvt_pk_f16_f32 on both planes, v_pk_add_f32 for the
    residual) instead of one value at a time.  Same roundings, so the planes must be the host packer's (torch's RNE casts, engine.pack_matrix)
    bit for bit -- on ordinary values, ties of the hi rounding, values beyond the plane format's range, denormal residuals and signed zeros."""
    from frido_amd.engine import pack_matrix, plane_dtype
    M, K = 96, 64
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(M, K, generator=g)
    x[1] = x[1] * 1e4
    x[2] = x[2] * 1e-6
    x[3] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2048.5, 2049.5, -2050.5, 65519.9, -65520.0] * (K // 8))   # hi-plane ties
    x[4] = torch.tensor([7e4, -7e4, 3e38, -3e38, 65504.0, -65504.0, 0.0, -0.0] * (K // 8))                                                       # range / zeros
    x[5] = torch.tensor([2.0 ** -14, 2.0 ** -15, 6e-8, -6e-8, 2.0 ** -24, 2.0 ** -25, 1e-30, -1e-30] * (K // 8))                                  # denormal planes
    xd = x.to(_dev())
    b = _builder(2)
    op = b.pack(xd.data_ptr(), 1, M, K, 0, K)
    _run(b)
    ref = pack_matrix(xd, 2)
    planes = op.buf[: 2 * op.lo * 2].view(plane_dtype(2)).view(2, op.lo)      # (a pooled operand: two planes of `lo` elements)
    assert ref.t.dtype == plane_dtype(2)
    n = M * K
    for plane in (0, 1):
        got, want = planes[plane, :n].view(torch.int16), ref.t[plane, :n].view(torch.int16)
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (plane, bad[:4].tolist(), x.flatten()[bad[:4, 0].cpu()].tolist())


@pytest.mark.gate
def test_device_plane_split_is_the_host_packers_bit_for_bit_bf16():
    """The bf16-pair twin of the test above (the planes frido_amd/autoplanes.py falls back to): split_op2 takes the integer-RNE route
    there (csrc/common.h: two split_op calls, not v_cvt_pk_f16_f32).  Every producer form -- pack's 8-channel vector path (split_op2),
    its element path (store_op4), the GEMM's direct epilogue (split_op2) and the scalar split-K reduction (store_op1) -- must write the
    host packer's planes bit for bit: ordinary values, ties of the bf16 hi rounding, magnitudes far beyond fp16 (unclamped and finite),
    fp32 denormals and signed zeros.  Nothing sets the status word's saturation bit on this build."""
    from frido_amd import _lib, tune
    from frido_amd.engine import pack_matrix, plane_dtype
    special = [
        [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 257.0, -259.0, 257.0 * 2.0 ** 100, -(2.0 ** 8 + 3) * 2.0 ** -100],   # hi ties
        [7e4, -7e4, 1e30, -1e30, 3e38, -3e38, 65504.0, 1e5 + 1.0],                                                                       # range
        [1e-40, -1e-40, 2.0 ** -126, 2.0 ** -149, -(2.0 ** -149), 1.5 * 2.0 ** -126, 1e-38, -3e-39],                                     # denormals
        [0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 2.0 ** -24, -(2.0 ** -30)],                                                                    # signed zeros
    ]
    with _lib.use_planes("bf16"):
        dt = plane_dtype(2)
        assert dt == torch.bfloat16
        _lib.status_flags(clear=True)

        def host_split(v):
            hi = v.to(dt)
            return hi, (v - hi.float()).to(dt)

        def same_bits(got_hi, got_lo, v, what):
            hi, lo = host_split(v)
            for p, (g, want) in enumerate(((got_hi, hi), (got_lo, lo))):
                bad = (g.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)).nonzero()
                assert bad.numel() == 0, (what, p, bad[:4].tolist(), v[tuple(bad[:4].t())].tolist() if bad.numel() else None)
            assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all(), what           # 3e38: no clamp, no inf

        # (1) pack: the 8-channel vector path (row-major, 64 channels) and the element path (NCHW source, 40 of 64 channels)
        M, K = 96, 64
        g = torch.Generator().manual_seed(4321)
        x = torch.randn(M, K, generator=g)
        x[1] *= 1e4
        x[2] *= 1e-6
        for i, row in enumerate(special):
            x[3 + i] = torch.tensor(row * (K // 8))
        xd = x.to(_dev())
        b = _builder(2)
        vec = b.pack(xd.data_ptr(), 1, M, K, 0, K)
        xn = x[:, :40].t().contiguous().view(1, 40, M).to(_dev())            # [B=1][C=40][HW=M]
        ele = b.pack(xn.data_ptr(), 1, M, 40, 0, 40, nchw=True)
        _run(b)
        hi, lo = _pair_planes_raw(vec)
        same_bits(hi, lo, xd, "pack, 8-channel path")
        ref = pack_matrix(xd, 2)
        assert torch.equal(ref.t[:, : M * K].view(torch.int16), torch.stack([hi.reshape(-1), lo.reshape(-1)]).view(torch.int16))
        hi, lo = _pair_planes_raw(ele)
        same_bits(hi[:, :40], lo[:, :40], xd[:, :40], "pack, element path")
        assert float(hi[:, 40:].float().abs().max()) == 0.0 and float(lo[:, 40:].float().abs().max()) == 0.0
        # (2) GEMM epilogues: zero operands, the special values as a row bias -> the stored operand is the host split of 0 + bias[m]
        rb = torch.tensor([v for row in special for v in row] + torch.randn(32, generator=g).tolist())
        Mg = rb.numel()
        rbd = rb.to(_dev())
        for N, splitk in ((64, 1), (36, 2)):           # direct epilogue (split_op2); N % 8 != 0: the scalar split-K reduction (store_op1)
            b = _builder(2)
            za, zw = pack_matrix(torch.zeros(Mg, 128, device=_dev()), 2), pack_matrix(torch.zeros(N, 128, device=_dev()), 2)
            o = b.op(Mg, 64)
            b.prog.gemm(Mg, N, 128, za, zw, out_op=o.ptr, ldoo=64, oo_lo=o.lo, row_bias=rbd.data_ptr(), tile=3)
            st = b.prog.ops[-1][1]
            st.splitk = splitk
            if splitk > 1:
                st.sk_mode = 0
                st.ws = tune.workspace_for(st, _dev())
            _run(b)
            hi, lo = _pair_planes_raw(o)
            v = torch.zeros(Mg, N, device=_dev()) + rbd[:, None]
            same_bits(hi[:, :N], lo[:, :N], v, f"GEMM epilogue, N = {N}, split-K {splitk}")
        assert (_lib.status_flags(clear=True) & _lib.STATUS_SATURATED) == 0


def _pair_planes_raw(op):
    """(hi, lo) planes of a pooled two-plane operand on the device, in the plane dtype, [rows][K]."""
    from frido_amd.engine import plane_dtype
    n = op.batch * op.rows * op.K
    t = op.buf[: 2 * op.lo * 2].view(plane_dtype(2)).view(2, op.lo)
    return t[0, :n].view(-1, op.K), t[1, :n].view(-1, op.K)


def test_two_plane_operands_saturate_instead_of_nan_and_keep_small_values():
    """r04 (advisor): the fp16 hi / lo planes of the parity mode.  (a) |v| > 65504 used to become an inf hi plane and a -inf lo
    plane, i.e. a NaN product; split_op now clamps, so the GEMM sees +-65504 -- finite, equal to the product with the clamped
    operand.  (b) small magnitudes: the pair's error is max(2^-22 |v|, 2^-25) (include/frido_hip.h), an absolute floor below
    |v| = 2^-3 -- operands scaled to 1e-5 still multiply to ~1e-3 relative (the floor), not to garbage."""
    from frido_amd.engine import plane_dtype
    M, N, K = 64, 48, 64
    a, w = _t("sat:a", M, K), _t("sat:w", N, K) / np.sqrt(K)
    if plane_dtype(2) != torch.float16:
        return _bf16_pairs_keep_the_range_and_have_no_floor(a, w)
    big = a.clone()
    big[::7, ::5] *= 1e5                                    # up to ~3e5: beyond fp16
    b = _builder(2, {"w.weight": w.cuda()})
    bd = big.cuda()
    a_op = b.pack(bd.data_ptr(), 1, M, K, 0, K)
    out = b.linear(a_op, "w", bias=False)
    _run(b)
    got = out.view().cpu()
    assert torch.isfinite(got).all()
    ref = big.clamp(-65504.0, 65504.0) @ w.t()
    assert _relerr(got, ref) < 2e-5
    assert torch.isfinite(a_op.to_f32()).all() and float(a_op.to_f32().abs().max()) == 65504.0
    # host packer (weights): same saturation
    from frido_amd.engine import pack_matrix
    wp = pack_matrix((w * 1e7).cuda(), 2)
    assert torch.isfinite(wp.to_f32()).all() and float(wp.to_f32().abs().max()) == 65504.0
    # small magnitudes: absolute floor 2^-25 per element
    small = (a * 1e-5).cuda()
    b2 = _builder(2, {"w.weight": w.cuda()})
    s_op = b2.pack(small.data_ptr(), 1, M, K, 0, K)
    out2 = b2.linear(s_op, "w", bias=False)
    _run(b2)
    err = (s_op.to_f32().cpu() - a * 1e-5).abs().max()
    assert float(err) <= 2.0 ** -25 * 1.01
    assert _relerr(out2.view().cpu(), (a * 1e-5) @ w.t()) < 5e-3


def _bf16_pairs_keep_the_range_and_have_no_floor(a, w):
    """The bf16-pair branch of the test above: nothing saturates and nothing has an absolute floor.  (a) activation rows scaled to
    1e5 ... 1e30 against unit-scale weights: each output row matches the float64 product to the bf16-pair bound relative to that row,
    and the status word's saturation bit stays 0; the host packer keeps 1e7-scale weights too.  (b) operands scaled to 1e-5 keep
    2^-17 relative accuracy per element (the fp16 pairs' 2^-25 floor would be 2^-25 / 1e-5 ~ 3e-3 relative there)."""
    from frido_amd import _lib
    from frido_amd.engine import pack_matrix
    M, K = a.shape
    _lib.status_flags(clear=True)
    scale = torch.ones(M, 1, dtype=torch.float64)
    scale[::2, 0] = torch.logspace(5, 30, (M + 1) // 2, dtype=torch.float64)      # every other row: 1e5 ... 1e30
    big = (a.double() * scale).float()
    b = _builder(2, {"w.weight": w.cuda()})
    bd = big.cuda()
    a_op = b.pack(bd.data_ptr(), 1, M, K, 0, K)
    out = b.linear(a_op, "w", bias=False)
    _run(b)
    got = out.view().cpu().double()
    assert torch.isfinite(got).all()
    ref = big.double() @ w.double().t()
    row_err = ((got - ref).abs().amax(1) / ref.abs().amax(1)).max()
    assert float(row_err) < _tol(2), float(row_err)
    rep = a_op.to_f32().cpu().double()
    assert bool(((rep - big.double()).abs() <= PAIR_U["bf16"] * big.double().abs()).all())
    assert (_lib.status_flags(clear=True) & _lib.STATUS_SATURATED) == 0
    wp = pack_matrix((w * 1e7).cuda(), 2)
    assert torch.isfinite(wp.to_f32()).all() and float(wp.to_f32().abs().max()) > 65504.0
    # small magnitudes: relative, no floor
    small = (a * 1e-5).cuda()
    b2 = _builder(2, {"w.weight": w.cuda()})
    s_op = b2.pack(small.data_ptr(), 1, M, K, 0, K)
    out2 = b2.linear(s_op, "w", bias=False)
    _run(b2)
    v = (a * 1e-5).double()
    assert bool(((s_op.to_f32().cpu().double() - v).abs() <= PAIR_U["bf16"] * v.abs()).all())
    assert _within(out2.view().cpu(), (a * 1e-5) @ w.t(), _tol(2))


# W, tile, C1, C2, Cout, B, SPADE, skip (appended raw 1x1 conv), residual, input from a producing conv's partial sums
GN_CONV_CASES = [
    (64, 20, 192, 0, 192, 1, False, False, True, False),
    (64, 20, 384, 192, 192, 1, True, True, False, False),       # concat input + SPADE + fused skip conv (the 64^2 output blocks)
    (32, 21, 384, 0, 384, 2, False, False, True, True),         # statistics from the producer's epilogue partial sums
    (32, 21, 576, 384, 384, 1, True, True, False, False),       # 960 channels: the table's limit
    (32, 20, 192, 0, 192, 2, True, False, False, False),        # 256-row tiles on a 32-wide plane (8 image rows per tile)
    (16, 21, 64, 64, 192, 2, False, True, False, False),        # 16-wide plane, 128-row tiles
    (64, 20, 32, 0, 192, 1, False, False, False, False),        # a single chunk: no staging overlap at all
    (32, 21, 64, 0, 192, 1, False, True, False, False),         # two chunks + one raw chunk
    # split-K over the chunk sequence (r04: the 16 x 16 planes): conv AND raw chunks dealt evenly to the slices, splitk_reduce behind
    (16, 20, 192, 192, 192, 2, True, True, False, False, 3),    # 12 conv chunks + 4 raw chunks over 3 slices (one image per tile)
    (16, 20, 576, 0, 576, 2, False, False, True, True, 5),      # 18 chunks over 5 slices (3 / 4 each), residual + producer partial sums
    (32, 21, 96, 32, 192, 1, False, True, False, False, 4),     # 4 chunks over 4 slices: one conv chunk and one raw chunk each
    (64, 20, 64, 0, 192, 1, True, False, False, False, 2),
]


@pytest.mark.gate
@pytest.mark.parametrize("case", GN_CONV_CASES)
def test_gn_conv_fused(case):
    """csrc/convgn.inc: GroupNorm(32) [+ SPADE] + SiLU applied INSIDE the 3x3 conv that consumes it (+ the 1x1 skip conv of the raw
    input as an appended K range, + bias / timestep vector / residual in the epilogue), against F.group_norm -> F.silu -> F.conv2d in
    fp32 -- and against the two-kernel path (gn_apply + ring conv) it replaces, whose operand bits it reproduces."""
    from frido_amd.builder import ACT_SILU
    W, tile, C1, C2, Cout, B, spade, skip, resid, from_parts = case[:10]
    splitk = case[10] if len(case) > 10 else 1
    H, C = W, C1 + C2
    HW, M = H * W, B * H * W
    Cr = 128 if skip else 0
    x1 = _t("fc:x1", B, HW, C1) * 1.5 + 0.3
    x2 = _t("fc:x2", B, HW, C2) * 0.7 if C2 else None
    w, bi = 1 + 0.1 * _t("fc:gw", C), 0.1 * _t("fc:gb", C)
    gam, bet = (0.3 * _t("fc:gg", B, HW, C), 0.3 * _t("fc:gbt", B, HW, C)) if spade else (None, None)
    wc, bc = _t("fc:wc", Cout, C, 3, 3) / np.sqrt(9 * C), _t("fc:bc", Cout)
    ws, bs = (_t("fc:ws", Cout, Cr, 1, 1) / np.sqrt(Cr), _t("fc:bs", Cout)) if skip else (None, None)
    raw = _t("fc:raw", B, HW, Cr) if skip else None
    res = _t("fc:res", M, Cout) if resid else None
    tvec = _t("fc:tv", 3, Cout)                       # timestep table: row 1 is selected by the device step counter
    weights = {"n.weight": w.cuda(), "n.bias": bi.cuda(), "c.weight": wc.cuda(), "c.bias": bc.cuda()}
    if skip:
        weights.update({"s.weight": ws.cuda(), "s.bias": bs.cuda()})
    Cp = 64
    if from_parts:
        weights.update({"p.weight": (_t("fc:pw", C1, Cp, 3, 3) / np.sqrt(9 * Cp)).cuda(), "p.bias": _t("fc:pb", C1).cuda()})
    b = _builder(2, weights)
    if from_parts:      # x1 = output of a conv of this library: carries per-channel partial sums (FridoGemm.gn_part)
        from frido_amd import tune
        xin = _t("fc:pin", B, Cp, H, W)
        xd = xin.cuda()
        a_in = b.pack(xd.data_ptr(), B, HW, Cp, 0, Cp, nchw=True)
        was = tune.ENABLED
        tune.ENABLED = False
        f1 = b.conv(a_in, B, H, W, "p")
        tune.ENABLED = was
        assert f1.gn_part is not None
        x1 = F.conv2d(xin, weights["p.weight"].cpu(), weights["p.bias"].cpu(), padding=1).permute(0, 2, 3, 1).reshape(B, HW, C1)
    else:
        f1 = b.f32(M, C1)
        f1.view().copy_(x1.view(M, C1).cuda())
    f2 = None
    if C2:
        f2 = b.f32(M, C2)
        f2.view().copy_(x2.view(M, C2).cuda())
    g = be = None
    if spade:
        g, be = b.f32(M, C), b.f32(M, C)
        g.view().copy_(gam.view(M, C).cuda())
        be.view().copy_(bet.view(M, C).cuda())
    fr = None
    if skip:
        fr = b.f32(M, Cr)
        fr.view().copy_(raw.view(M, Cr).cuda())
    r = None
    if resid:
        r = b.f32(M, Cout)
        r.view().copy_(res.cuda())
    tv = tvec.cuda()
    step = torch.tensor([1], dtype=torch.int32, device="cuda")
    rv = dict(ptr=tv.data_ptr(), ld=Cout, rows_per_vec=1 << 30, step=step.data_ptr())
    out = b.gn_conv(tile, f1, f2, B, H, W, "n", 1e-5, "c", gamma=g, beta=be, act=ACT_SILU, rowvec=rv, residual=r,
                    skip=(fr, None, "s") if skip else None, splitk=splitk)
    st = b.prog.ops[-1][1]
    assert st.tile == tile and st.gn_x1 and not st.A and st.splitk == (splitk if splitk > 1 else 0)
    # the path it replaces, in the same program: gn_apply -> operand -> ring conv (+ skip as A2)
    a_ref, raw_ref = b.groupnorm(f1, f2, B, HW, "n", 1e-5, gamma=g, beta=be, act=ACT_SILU, want_raw=False)
    if skip:
        raw_op = b.pack(fr.ptr, 1, M, Cr, 0, Cr)
        out2 = b.conv_plus_skip(a_ref, raw_op, B, H, W, "c", "s")
    else:
        out2 = b.conv(a_ref, B, H, W, "c", residual=r, rowvec=rv)
    _run(b)
    xc = x1 if x2 is None else torch.cat([x1, x2], dim=-1)
    xn = xc.permute(0, 2, 1).reshape(B, C, H, W)
    y = F.group_norm(xn, 32, w, bi, 1e-5)
    if spade:
        y = y * (1 + gam.permute(0, 2, 1).reshape(B, C, H, W)) + bet.permute(0, 2, 1).reshape(B, C, H, W)
    ref = F.conv2d(F.silu(y), wc, bc, padding=1)
    if skip:
        ref = ref + F.conv2d(raw.permute(0, 2, 1).reshape(B, Cr, H, W), ws, bs)
    ref = ref.permute(0, 2, 3, 1).reshape(M, Cout) + tvec[1]
    if resid:
        ref = ref + res
    got = out.view().cpu()
    assert torch.isfinite(got).all()
    assert _within(got, ref, _tol(2))
    if not skip:      # same operand bits, same products; only the fp32 accumulation order differs (chunk-major vs tap-major k walk)
        assert _relerr(got, out2.view().cpu()) < 3e-6
    # the epilogue's GroupNorm partial sums of THIS conv's output (the next norm's statistics)
    if out.gn_part is not None:
        parts = out.gn_part[: (M // 32) * Cout * 8].view(torch.float32).view(M // 32, Cout, 2).cpu().double()
        blocks = got.double().view(M // 32, 32, Cout)
        assert _relerr(parts[:, :, 0], blocks.sum(1)) < 1e-5 and _relerr(parts[:, :, 1], (blocks ** 2).sum(1)) < 1e-5


@pytest.mark.gate
@pytest.mark.parametrize("W,C,N,B", [(64, 192, 3, 2), (32, 192, 4, 3), (16, 96, 3, 2), (64, 32, 4, 1), (32, 960, 3, 1)])
def test_gn_conv_tiny_output_head(W, C, N, B):
    """(r06) csrc/convgn.hip conv3x3_gn_tiny_kernel (FridoGemm tile 40): the denoiser's eps head  conv3x3(SiLU(GroupNorm32(h)))  to 3 / 4
    channels (pyunet.py:775-803) as ONE launch on the f32 VALU -- against F.group_norm -> F.silu -> F.conv2d in fp32 (bound 5e-6: plain f32
    products and sums, no operand planes), and against the MFMA path it replaces (gn_apply + two-plane conv) on the same input.  64 / 32 /
    16-wide planes (4 / 8 / 16 image rows per 256-pixel tile), 1, 3, 6 and 30 channel chunks, odd batch; zero padding on every edge."""
    from frido_amd.builder import ACT_SILU
    H = W
    HW, M = H * W, B * H * W
    x = _t("tn:x", B, HW, C) * 1.5 + 0.3
    w, bi = 1 + 0.1 * _t("tn:gw", C), 0.1 * _t("tn:gb", C)
    wc, bc = _t("tn:wc", N, C, 3, 3) / np.sqrt(9 * C), _t("tn:bc", N)
    b = _builder(2, {"n.weight": w.cuda(), "n.bias": bi.cuda(), "c.weight": wc.cuda(), "c.bias": bc.cuda()})
    f1 = b.f32(M, C)
    f1.view().copy_(x.view(M, C).cuda())
    assert b.gn_conv_tiny_ok(f1, B, H, W, N)
    out = b.f32_strict(M, N)
    out.view().fill_(float("nan"))
    b.gn_conv_tiny(f1, B, H, W, "n", 1e-5, "c", out)
    st = b.prog.ops[-1][1]
    assert st.tile == 40 and st.gn_x1 and st.w_f32 and not st.A and not st.B
    a_ref, _ = b.groupnorm(f1, None, B, HW, "n", 1e-5, act=ACT_SILU)
    old = b.conv(a_ref, B, H, W, "c", out="f32_strict")
    _run(b)
    xn = x.view(B, H, W, C).permute(0, 3, 1, 2)
    ref = F.conv2d(F.silu(F.group_norm(xn, 32, w, bi, 1e-5)), wc, bc, padding=1).permute(0, 2, 3, 1).reshape(M, N)
    got = out.view().cpu()
    assert bool(torch.isfinite(got).all()) and _relerr(got, ref) < 5e-6, (W, C, N)
    assert _within(old.view().cpu(), ref, _tol(2))                  # the replaced path on the same input (its own bound)
    # not applicable: more than 4 output channels, a bf16-mode builder, a plane that is no multiple of 256 pixels
    assert not b.gn_conv_tiny_ok(f1, B, H, W, 8) and not _builder(1, {}).gn_conv_tiny_ok(f1, B, H, W, N) and not b.gn_conv_tiny_ok(f1, B, 8, 8, N)


@pytest.mark.gate
@pytest.mark.parametrize("W,C1,C2,Cout_prev,splitk,spade,resid,dead,B", [(16, 576, 0, 576, 4, False, False, False, 16), (8, 960, 0, 960, 8, True, True, False, 16),
                                                                         (16, 384, 192, 384, 3, False, True, False, 16), (8, 960, 0, 960, 5, False, False, True, 16),
                                                                         # r05: the shapes of BASELINE config 3 at its batch (CFG: 64 rows): 8 x 8 x 576 and 4 x 4 x 960
                                                                         (8, 576, 0, 576, 3, False, True, False, 64), (4, 960, 0, 960, 6, True, True, False, 64),
                                                                         (4, 960, 0, 960, 6, False, False, True, 2)])
def test_splitk_reduction_deferred_into_groupnorm(W, C1, C2, Cout_prev, splitk, spade, resid, dead, B):
    """r04 (FridoGemm.sk_mode 2 + FridoGnApply.sk_*): a split-K conv whose output goes straight into a one-launch GroupNorm leaves its
    reduction + epilogue (bias, timestep vector, residual) to that launch.  Everything the pair produces -- the conv output, the
    normalised operand, the raw operand copy -- must equal the conv -> splitk_reduce -> GroupNorm chain BIT FOR BIT, and fp32 torch."""
    import frido_amd.builder as bld
    from frido_amd import tune, _lib
    from frido_amd.builder import ACT_SILU
    H, Cin = W, 64
    HW, M, C = H * W, B * W * W, C1 + C2
    xin = _t("sd:x", B, Cin, H, W)
    wc, bc = _t("sd:wc", C1, Cin, 3, 3) / np.sqrt(9 * Cin), _t("sd:bc", C1)
    w, bi = 1 + 0.1 * _t("sd:gw", C), 0.1 * _t("sd:gb", C)
    x2 = _t("sd:x2", B, HW, C2) * 0.7 if C2 else None
    gam, bet = (0.3 * _t("sd:gg", B, HW, C), 0.3 * _t("sd:gbt", B, HW, C)) if spade else (None, None)
    res = _t("sd:res", M, C1) if resid else None
    tvec = _t("sd:tv", 3, C1)
    weights = {"n.weight": w.cuda(), "n.bias": bi.cuda(), "c.weight": wc.cuda(), "c.bias": bc.cuda()}
    outs = {}
    for defer in (True, False):
        b = _builder(2, weights)
        xd = xin.cuda()
        a_in = b.pack(xd.data_ptr(), B, HW, Cin, 0, Cin, nchw=True)
        f2 = None
        if C2:
            f2 = b.f32(M, C2)
            f2.view().copy_(x2.view(M, C2).cuda())
        g = be = None
        if spade:
            g, be = b.f32(M, C), b.f32(M, C)
            g.view().copy_(gam.view(M, C).cuda())
            be.view().copy_(bet.view(M, C).cuda())
        r = None
        if resid:
            r = b.f32(M, C1)
            r.view().copy_(res.cuda())
        tv = tvec.cuda()
        step = torch.tensor([2], dtype=torch.int32, device="cuda")
        rv = dict(ptr=tv.data_ptr(), ld=C1, rows_per_vec=1 << 30, step=step.data_ptr())
        was = tune.ENABLED
        tune.ENABLED = False
        f1 = b.conv(a_in, B, H, W, "c", rowvec=rv, residual=r)
        tune.ENABLED = was
        st = b.prog.ops[-1][1]                      # force the split the tuner picks on these planes
        st.tile, st.splitk, st.sk_mode, st.gn_part = 7, splitk, 0, None
        st.ws = tune.workspace_for(st, b.device)
        b.prog._packed = None
        f1.view().fill_(float("nan"))              # whoever finishes the reduction must write every element
        r_ptr = r.ptr if r is not None else None
        if r is not None:
            r.free()                               # (r05) like unet_plan: the residual's owner releases it right after emitting the GEMM -- a deferred
            #                                        reduction reads it from the GroupNorm launch, whose operand buffers must not be carved out of it
        bld.SK_DEFER = defer
        try:
            a, raw = b.groupnorm(f1, f2, B, HW, "n", 1e-5, gamma=g, beta=be, act=ACT_SILU, want_raw=True, x1_dead=dead)
        finally:
            bld.SK_DEFER = True
        kinds = [k for k, _ in b.prog.ops]
        assert kinds[-1] == _lib.OP_KINDS["FRIDO_OP_GN_FUSED"]
        if defer and r_ptr is not None:
            assert a.ptr != r_ptr and raw.ptr != r_ptr, "the deferred reduction's residual was handed out as an output buffer of the same launch"
        assert st.sk_mode == (2 if defer else 0) and bool(b.prog.ops[-1][1].sk_ws) == defer
        _run(b)
        outs[defer] = (f1.view().clone(), a.to_f32().clone(), raw.to_f32().clone())
    x_def, a_def, raw_def = outs[True]
    x_ref, a_ref, raw_ref = outs[False]
    assert torch.isfinite(x_ref).all()
    if dead:
        assert torch.isnan(x_def).all()             # nobody reads the tensor: it is not materialised
    else:
        assert torch.equal(x_def, x_ref)            # the reduction + epilogue arithmetic is splitk_reduce8's, expression for expression
    assert torch.equal(raw_def, raw_ref)
    # r05: a deferred launch always takes the 1024-thread form (one vector per lane, all slices' loads in flight), the plain launch the
    # narrowest form that fits -- the wave-partial order of the statistics differs, so the normalised operand agrees to fp32 rounding
    # of the statistics (bit for bit where both forms coincide: the 16 x 16 planes)
    assert _relerr(a_def, a_ref) < 2e-6 + (2 * PAIR_U[_planes()] if _planes() == "bf16" else 0.0)      # bf16 pairs: + one pair error per side
    if HW >= 256:
        assert torch.equal(a_def, a_ref)
    ref = F.conv2d(xin, wc, bc, padding=1).permute(0, 2, 3, 1).reshape(M, C1) + tvec[2]
    if resid:
        ref = ref + res
    assert _within(x_ref.cpu(), ref, _tol(2))
    xc = ref.view(B, HW, C1) if x2 is None else torch.cat([ref.view(B, HW, C1), x2], dim=-1)
    y = F.group_norm(xc.permute(0, 2, 1).reshape(B, C, H, W), 32, w, bi, 1e-5)
    if spade:
        y = y * (1 + gam.permute(0, 2, 1).reshape(B, C, H, W)) + bet.permute(0, 2, 1).reshape(B, C, H, W)
    assert _within(a_def.cpu(), F.silu(y).permute(0, 2, 3, 1).reshape(M, C), _tol(2))


def test_splitk_deferral_is_rejected_where_nobody_could_finish_it():
    import ctypes as C_
    from frido_amd import _lib
    dummy = torch.zeros(1 << 20, device="cuda")
    kind, st = _lib.make_op("FRIDO_OP_GEMM", M=1024, N=192, K=1024, batch=1, nsplit=2, lda=1024, ldb=1024, tile=3, splitk=4, sk_mode=2,
                            A=dummy.data_ptr(), B=dummy.data_ptr(), ws=dummy.data_ptr(), out_f32=dummy.data_ptr(), ldo=200)
    assert _lib.lib().frido_gemm(C_.addressof(st), None) == -1 and b"sk_mode 2" in _lib.lib().frido_last_error()      # strided output
    st.ldo, st.act = 192, 2
    assert _lib.lib().frido_gemm(C_.addressof(st), None) == -1                                                          # activation
    kind, gn = _lib.make_op("FRIDO_OP_GN_APPLY", x1=dummy.data_ptr(), C1=64, B=1, HW=64, groups=32, nsplit_px=1, partials=dummy.data_ptr(),
                            weight=dummy.data_ptr(), bias=dummy.data_ptr(), nsplit=2, out_op=dummy.data_ptr(), out_lo=4096,
                            sk_ws=dummy.data_ptr(), sk_n=2)
    assert _lib.lib().frido_gn_apply(C_.addressof(gn), None) == -1 and b"frido_gn_fused only" in _lib.lib().frido_last_error()


def test_gn_conv_rejects_what_it_cannot_run():
    import ctypes as C_
    from frido_amd import _lib
    kind, st = _lib.make_op("FRIDO_OP_GEMM", M=4096, N=192, K=9 * 64, batch=1, nsplit=2, conv=1, Hs=64, Ws=64, Cin=64, Hl=64, Wl=64,
                            Ho=64, Wo=64, kh=3, kw=3, stride=1, pad=1, padx=1, ldb=9 * 64, tile=20, gn_C1=64, gn_groups=32)
    dummy = torch.zeros(64, device="cuda")
    st.B, st.out_f32, st.ldo = dummy.data_ptr(), dummy.data_ptr(), 192
    assert _lib.lib().frido_gemm(C_.addressof(st), None) == -1            # no A and no gn_x1
    st.gn_x1 = dummy.data_ptr()
    assert _lib.lib().frido_gemm(C_.addressof(st), None) == -1            # gn_x1 without statistics / affine parameters
    assert b"fused GroupNorm" in _lib.lib().frido_last_error()
    st.tile = 7
    assert _lib.lib().frido_gemm(C_.addressof(st), None) == -1            # a fused descriptor on a ring tile


# ---- round 5 ----------------------------------------------------------------------------------------------------------
def test_status_word_flags_saturation_and_nonfinite_statistics():
    """r05 (frido_status_flags): an operand producer that clamps a value at +-65504 sets FRIDO_STATUS_SATURATED, a normalisation
    kernel whose statistics are NaN / inf sets FRIDO_STATUS_NONFINITE; clean work sets nothing; the word is sticky until cleared."""
    from frido_amd import _lib
    from frido_amd.engine import plane_dtype
    from frido_amd.builder import ACT_SILU
    _lib.status_flags(clear=True)
    M, K = 256, 64
    a = _t("st:a", M, K)
    # clean: pack -> GEMM (operand output) -> GroupNorm -> LayerNorm
    b = _builder(2, {"w.weight": (_t("st:w", 64, K) / 8).cuda(), "n.weight": torch.ones(64).cuda(), "n.bias": torch.zeros(64).cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    o = b.linear(a_op, "w", bias=False, out="op")
    f = b.linear(a_op, "w", bias=False)
    g, _ = b.groupnorm(f, None, 4, 64, "n", 1e-5, act=ACT_SILU)
    ln = b.layernorm(f, "n")
    _run(b)
    assert _lib.status_flags() == 0
    if plane_dtype(2) == torch.float16:
        big = a.clone()
        big[3, 5] = 7.0e4                                              # one value beyond fp16
        b2 = _builder(2)
        bd = big.cuda()
        b2.pack(bd.data_ptr(), 1, M, K, 0, K)
        _run(b2)
        assert _lib.status_flags() == _lib.STATUS_SATURATED
        assert _lib.status_flags() == _lib.STATUS_SATURATED            # sticky
        with pytest.warns(_lib.FridoNumericsWarning, match="saturated"):
            assert _lib.warn_on_status("test") == _lib.STATUS_SATURATED
        assert _lib.status_flags() == 0                                # cleared by the warning helper
        # a GEMM epilogue producing an operand beyond the range (the GEGLU hidden / Q class of tensors)
        b3 = _builder(2, {"w.weight": (_t("st:w", 64, K) * 1.0e4).cuda()})
        a3 = b3.pack(ad.data_ptr(), 1, M, K, 0, K)
        b3.linear(a3, "w", bias=False, out="op")
        _run(b3)
        assert _lib.status_flags(clear=True) & _lib.STATUS_SATURATED
    else:                                                              # bf16-pair build: fp32's range, nothing to flag
        big = a.clone()
        big[3, 5], big[7, 1] = 7.0e4, -1.0e30
        b2 = _builder(2, {"w.weight": (_t("st:w", 64, K) * 1.0e4).cuda()})
        bd = big.cuda()
        a2 = b2.pack(bd.data_ptr(), 1, M, K, 0, K)
        b2.linear(a2, "w", bias=False, out="op")
        _run(b2)
        assert _lib.status_flags() == 0
    # NaN in the stream -> GroupNorm / LayerNorm statistics
    for kind in ("gn_fused", "gn_apply", "layernorm"):
        b4 = _builder(2, {"n.weight": torch.ones(64).cuda(), "n.bias": torch.zeros(64).cuda()})
        HW = 64 if kind == "gn_fused" else 1024
        x = b4.f32(4 * HW, 64)
        x.view().copy_(_t("st:x", 4 * HW, 64).cuda())
        x.view()[5, 7] = float("nan")
        if kind == "layernorm":
            b4.layernorm(x, "n")
        else:
            b4.groupnorm(x, None, 4, HW, "n", 1e-5)
        _run(b4)
        assert _lib.status_flags(clear=True) & _lib.STATUS_NONFINITE, kind
    assert _lib.status_flags() == 0


def test_cross_attention_skips_the_dead_stream_store():
    """r05 (FridoAttnSmall.skip_act_store): with FF2 + proj_out chained, h3 = attn2(norm2(h2)) + h2 is read only as an operand and through
    norm3 -- the launch that writes both copies does not store the f32 rows.  The two copies must equal the storing launch's bit for bit."""
    B, Nq, Nk, d = 16, 256, 26, 576
    outs = {}
    for skip in (False, True):
        b = _builder(2, {"ln.weight": (1 + 0.1 * _t("sk:lw", d)).cuda(), "ln.bias": (0.1 * _t("sk:lb", d)).cuda()})
        qd, kd, vd = _t("sk:q", B * Nq, d).cuda(), _t("sk:k", B * Nk, d).cuda(), _t("sk:v", B, d, 32).cuda()
        vd[:, :, Nk:] = 0
        q = b.pack(qd.data_ptr(), 1, B * Nq, d, 0, d)
        k = b.pack(kd.data_ptr(), 1, B * Nk, d, 0, d)
        vT = b.persistent_op(d, 32, batch=B, zero=True)
        b.pack(vd.data_ptr(), 1, B * d, 32, 0, 32, out=vT)
        res = b.f32(B * Nq, d)
        res.view().copy_(_t("sk:r", B * Nq, d).cuda())
        bias = _t("sk:b", d).cuda()
        h = b.attention(q, d, k, d, vT, B, Nq, Nk, d, bias_ptr=bias.data_ptr(), residual=res, stream=True, also_op=True,
                        ln=("ln", 1e-5), stream_dead=skip)
        assert getattr(h, "stream_skipped", False) == skip and h.op_copy is not None and h.ln_copy is not None
        h.view().fill_(float("nan"))
        _run(b)
        outs[skip] = (h.view().clone(), h.op_copy.to_f32().clone(), h.ln_copy.to_f32().clone())
    assert torch.isfinite(outs[False][0]).all() and torch.isnan(outs[True][0]).all()
    assert torch.equal(outs[False][1], outs[True][1]) and torch.equal(outs[False][2], outs[True][2])


@pytest.mark.parametrize("C,scale", [(64, 1.0), (192, 0.5), (960, 1.0), (40, 1.0)])
def test_pack_vector_path_matches_elementwise_split(C, scale):
    """r05: pack_kernel's 8-channel path (the residual stream as an operand) writes the planes torch's own hi / lo split gives."""
    from frido_amd.engine import plane_dtype
    rows = 1000
    x = _t("pk:x", rows, C) * 3
    b = _builder(2)
    xd = x.cuda()
    o = b.pack(xd.data_ptr(), 1, rows, C, 0, C, scale=scale)
    _run(b)
    dt = plane_dtype(2)
    v = (x * scale).cuda()
    hi = v.to(dt)
    lo = (v - hi.float()).to(dt)
    t = o.buf[: 2 * o.lo * 2].view(dt).view(2, o.lo)
    Kp = o.K
    assert torch.equal(t[0, : rows * Kp].view(rows, Kp)[:, :C], hi) and torch.equal(t[1, : rows * Kp].view(rows, Kp)[:, :C], lo)
    assert float(t[0, : rows * Kp].view(rows, Kp)[:, C:].abs().sum()) == 0.0


# ---- the bf16-pair build ---------------------------------------------------------------------------------------------------
def _on_bf16_planes(fn, gate=False):
    """Twin of a two-plane kernel test for libfrido_hip_bf16p.so: the same body inside _lib.use_planes("bf16") (the builder, the host
    packer and every run resolve the library per call), its nsplit = 2 legs only.  Not in the gate unless asked for."""
    @functools.wraps(fn)
    def twin(*args, **kwargs):
        from frido_amd import _lib
        with _lib.use_planes("bf16"):
            return fn(*args, **kwargs)

    twin.__name__ = twin.__qualname__ = fn.__name__ + "_bf16"
    marks = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "gate" and not gate:
            continue
        if m.name == "parametrize" and m.args[0] == "nsplit":
            m = pytest.mark.parametrize("nsplit", [2]).mark
        marks.append(m)
    if gate:
        marks.append(pytest.mark.gate.mark)
    twin.pytestmark = marks
    return twin


for _fn in (test_gemm_dense, test_gemm_batched_operand_out_and_rowbias, test_gemm_split_k_is_deterministic_and_correct, test_conv,
            test_upsample_conv_as_phase_convs, test_gemm_k_split_inside_the_workgroup, test_gemm_column_panel_tile_order_is_a_pure_reordering,
            test_bf16x3_pipelined_loop_short_k, test_fused_geglu_projection, test_fused_geglu_projection_every_tile, test_groupnorm_apply,
            test_groupnorm_statistics_from_the_conv_epilogue, test_gn_conv_fused, test_splitk_reduction_deferred_into_groupnorm,
            test_attention_core, test_attention_core_stream_output, test_attention_flash, test_attention_flash_online_softmax_rescale_branch,
            test_cross_attention_skips_the_dead_stream_store, test_graph_capture_replays, test_two_plane_operands_saturate_instead_of_nan_and_keep_small_values,
            test_status_word_flags_saturation_and_nonfinite_statistics, test_pack_vector_path_matches_elementwise_split):
    globals()[_fn.__name__ + "_bf16"] = _on_bf16_planes(_fn)
test_gemm_direct_epilogue_every_tile_bf16 = _on_bf16_planes(test_gemm_direct_epilogue_every_tile, gate=True)
del _fn

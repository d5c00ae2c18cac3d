"""The Fréchet Inception Distance on the MI355X against the float64 restatement of tests/inception_ref.py: the four kernels of
csrc/fid.hip at kernel level, the seven conv geometries Inception-v3 is the first to launch on the implicit GEMM alone, one block of
every kind through fid.emit_block, the tower in both builds of the library, graph replay, re-planning, and pipeline.fid_statistics /
pipeline.fid end to end.

Bounds (none of them is taken from what the code under test returns):
  preprocess           max |hip - f64| <= 2 x max |host32 - f64|: the SAME formula evaluated in float32 on the host, per case (the
           project's rule for formula kernels); where that is 0 (the identity resize) the output is held bit for bit.  Half-pixel
           centres, align_corners=True, / 127.5 and round-to-nearest quantisation are shown to lie >= 10 x outside.
  pools, gap, accum    bit-equal to torch's max pool / to the host loop in the kernel's order (f32 sums, f64 sums).
  conv on the GEMM     tests/test_kernels_gpu.py's bounds for the two-plane GEMM: 2e-5 of max |y| on the fp16-pair build, 1e-4 on
           the bf16-pair build, against float64.
  blocks, tower        relative to max |reference|: 8 x E32, the largest float32-vs-float64 difference of the restatement over the
           cases (blocks: over the six blocks; tower: over the tower cases); the bf16-pair build gets 10 x that bound (the rule of
           tests/test_lpips_gpu.py and tests/test_patchgan_gpu.py).
  end to end           written at the test."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from frido_amd import _lib, fid, synth
from frido_amd.engine import require_gpu

pytestmark = pytest.mark.gpu

BF16_PAIR_RATIO = 10.0      # the bf16-pair build's allowance over the default build's bound
PAD = 64                    # NaN elements behind every kernel output: the kernel must leave them alone
GEMM_TOL = {"f16": 2e-5, "bf16": 1e-4}      # tests/test_kernels_gpu.py: _tol(2) on the two builds


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


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


# ---- frido_fid_preprocess --------------------------------------------------------------------------------
PRE_CASES = [pytest.param(2, 5, 7, 9, id="2x5x7-to-9", marks=pytest.mark.gate), pytest.param(1, 16, 16, 16, id="identity-16", marks=pytest.mark.gate),
             pytest.param(2, 64, 48, 299, id="2x64x48-to-299"), pytest.param(1, 300, 301, 299, id="300x301-to-299")]


@pytest.mark.parametrize("layout", ["u8", "f32-pil", "f32-np"])
@pytest.mark.parametrize("B,H,W,S", PRE_CASES)
def test_preprocess_matches_float64(B, H, W, S, layout):
    g = torch.Generator().manual_seed(H * 1000 + W + S)
    if layout == "u8":
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        quant = "pil"
    else:
        img = (torch.rand(B, 3, H, W, generator=g) * 2.2 - 1.1).float()      # some values beyond [-1, 1]: the clamps
        quant = layout[4:]
    q = R.to_q(img, quant)
    ref = R.preprocess(q, S)
    host32 = R.preprocess(q, S, torch.float32)
    bound = 2.0 * float((host32.double() - ref).abs().max())
    src = img.cuda()
    dst = _out(B * S * S * 3)
    fid.launch("frido_fid_preprocess", fid.preprocess_desc(src.data_ptr(), dst.data_ptr(), B, H, W, S,
                                                           src_kind=fid.SRC_U8_HWC if layout == "u8" else fid.SRC_F32_NCHW, quant=quant), _stream())
    got = _nchw(_take(dst, B * S * S * 3, "frido_fid_preprocess"), B, S, S)
    err = float((got.double() - ref).abs().max())
    print(f"fid_preprocess {layout} B={B} {H}x{W} -> {S}: max abs err {err:.3e}, bound (2 x float32 on the host) {bound:.3e}")
    assert err <= bound
    if (H, W) == (S, S):
        assert bound == 0 and torch.equal(got.double(), (q - 128) / 128)      # an S x S input comes back exactly
        return
    assert bound > 0
    wrong = [R.preprocess(q, S, centres="half"), R.preprocess(q, S, centres="corners"), R.preprocess(q, S, divisor=127.5)]
    if layout != "u8":
        wrong.append(R.preprocess(R.to_q(img, quant, rounding="nearest"), S))
    for k, wv in enumerate(wrong):
        assert float((wv - ref).abs().max()) >= 10 * bound, k


# ---- frido_pool3 -----------------------------------------------------------------------------------------
def _pool_ref(x, mode):
    """float32 on the host: torch's own max pools; the average in the kernel's order."""
    if mode == fid.POOL_MAX_S2:
        return R.max_pool_s2(x)
    if mode == fid.POOL_MAX_S1P1:
        return R.max_pool_s1(x)
    return R.avg_pool_in_order(x)


POOL_CASES = [pytest.param(2, 7, 7, 4, id="7x7-C4", marks=pytest.mark.gate), pytest.param(2, 5, 6, 64, id="5x6-C64", marks=pytest.mark.gate),
              pytest.param(1, 8, 8, 288, id="8x8-C288"), pytest.param(3, 7, 7, 288, id="7x7-C288"), pytest.param(1, 5, 6, 4, id="5x6-C4"),
              pytest.param(1, 8, 8, 64, id="8x8-C64")]


@pytest.mark.parametrize("mode", [fid.POOL_MAX_S2, fid.POOL_MAX_S1P1, fid.POOL_AVG_S1P1], ids=["max-s2", "max-s1p1", "avg-s1p1"])
@pytest.mark.parametrize("B,H,W,Cn", POOL_CASES)
def test_pool_bit_equal_inside_a_wider_destination(B, H, W, Cn, mode):
    x = torch.from_numpy(synth.seeded_normal(f"fid:pool:{B}{H}{W}{Cn}", (B, Cn, H, W)))
    ref = _pool_ref(x, mode)
    Ho, Wo = ref.shape[2:]
    assert (Ho, Wo) == (fid.pool_out(H, mode), fid.pool_out(W, mode))
    ldd, c0, rows = Cn + 12, 8, B * Ho * Wo
    src = _rows(x).contiguous().cuda()
    dst = _out(rows * ldd)
    dst[:rows * ldd] = 7.0                                                   # the neighbouring columns must survive
    fid.launch("frido_pool3", fid.pool_desc(src.data_ptr(), dst.data_ptr(), B, H, W, Cn, mode, ldd=ldd, c0=c0), _stream())
    got = _take(dst, rows * ldd, "frido_pool3").view(rows, ldd)
    assert bool((got[:, :c0] == 7.0).all()) and bool((got[:, c0 + Cn:] == 7.0).all())
    assert torch.equal(got[:, c0:c0 + Cn], _rows(ref))
    if mode == fid.POOL_AVG_S1P1:
        assert float((ref.double() - R.avg_pool(x.double())).abs().max()) <= 9 * 2.0 ** -24 * float(x.abs().max())
        by9 = F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=True)
        border = torch.ones(H, W, dtype=torch.bool)
        border[1:-1, 1:-1] = False
        assert bool(((by9 - ref).abs()[:, :, border] > 0).any(dim=1).all())  # dividing by 9 everywhere: every border pixel differs
        assert not torch.equal(R.max_pool_s1(x), ref)
    if mode == fid.POOL_MAX_S1P1:
        assert bool(((R.avg_pool(x) - ref).abs() > 0).all())                  # an average is not the maximum, anywhere


def test_pool_second_grid_stride_trip():
    """4 x 35 x 35 x 288: 352800 units of four channels; the grid caps at 1024 x 256 = 262144 threads."""
    B, H, W, Cn = 4, 35, 35, 288
    x = torch.from_numpy(synth.seeded_normal("fid:pool:big", (B, Cn, H, W)))
    src = _rows(x).contiguous().cuda()
    for mode in (fid.POOL_AVG_S1P1, fid.POOL_MAX_S2):
        ref = _rows(_pool_ref(x, mode))
        dst = _out(ref.numel())
        fid.launch("frido_pool3", fid.pool_desc(src.data_ptr(), dst.data_ptr(), B, H, W, Cn, mode), _stream())
        assert torch.equal(_take(dst, ref.numel(), "frido_pool3").view(ref.shape), ref)


# ---- frido_gap -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW,Cn", [pytest.param(1, 4, marks=pytest.mark.gate), (4, 4), (64, 4), (1, 2048), (4, 2048),
                                   pytest.param(64, 2048, marks=pytest.mark.gate)])
def test_gap_bit_equal_to_the_in_order_float64_loop(HW, Cn):
    B = 3
    x = torch.from_numpy(synth.seeded_normal(f"fid:gap:{HW}:{Cn}", (B, Cn, HW, 1))) * 3 + 1
    ref = R.gap(x)
    src = _rows(x).contiguous().cuda()
    dst = _out(B * Cn)
    fid.launch("frido_gap", fid.gap_desc(src.data_ptr(), dst.data_ptr(), B, HW, Cn), _stream())
    assert torch.equal(_take(dst, B * Cn, "frido_gap").view(B, Cn), ref)


# ---- frido_feat_accum ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", [pytest.param(1, 4, marks=pytest.mark.gate), pytest.param(3, 64, marks=pytest.mark.gate), (5, 100), (7, 2048)])
def test_feat_accum_bit_equal_symmetric_and_associative_over_updates(B, D):
    x = torch.from_numpy(synth.seeded_normal(f"fid:acc:{B}:{D}", (2 * B, D))) * 2 + 0.5
    s1, s2 = R.accumulate(x[:B])
    xg = x.cuda()
    b1, b2 = _out(D, torch.float64), _out(D * D, torch.float64)
    b1[:D] = 0
    b2[:D * D] = 0
    fid.launch("frido_feat_accum", fid.accum_desc(xg.data_ptr(), b1.data_ptr(), b2.data_ptr(), B, D), _stream())
    g1, g2 = _take(b1, D, "frido_feat_accum s1"), _take(b2, D * D, "frido_feat_accum s2").view(D, D)
    assert torch.equal(g1, s1) and torch.equal(g2, s2)
    assert torch.equal(g2, g2.T)
    # two updates == one update of the concatenation, through the public class
    one = fid.FeatureStatistics(D, "cuda").update(xg)
    two = fid.FeatureStatistics(D, "cuda").update(xg[:B]).update(xg[B:])
    torch.cuda.synchronize()
    assert one.n == two.n == 2 * B
    assert torch.equal(one.s1, two.s1) and torch.equal(one.s2, two.s2)
    f1, f2 = R.accumulate(x)
    assert torch.equal(one.s1.cpu(), f1) and torch.equal(one.s2.cpu(), f2)
    if 2 * B >= 2:
        mu, cov = R.mean_cov(x.numpy())
        assert float(np.abs(one.cov().cpu().numpy() - cov).max()) <= 4 * 2 * B * 2.0 ** -53 * float(x.double().pow(2).max())


# ---- the seven new conv geometries on the implicit GEMM, alone -------------------------------------------
#           id                 Cin  Cout kh kw stride pad padx  H   W
CONV_CASES = [("k3-s2-p0-9x11", 32, 32, 3, 3, 2, 0, 0, 9, 11), ("k5-p2-Cin48-7x7", 48, 64, 5, 5, 1, 2, 2, 7, 7),
              ("1x7-5x5", 160, 160, 1, 7, 1, 0, 3, 5, 5), ("7x1-5x5", 160, 160, 7, 1, 1, 3, 0, 5, 5),
              ("1x7-17x17", 160, 160, 1, 7, 1, 0, 3, 17, 17), ("7x1-17x17", 160, 160, 7, 1, 1, 3, 0, 17, 17),
              ("1x3-2x2", 384, 384, 1, 3, 1, 0, 1, 2, 2), ("3x1-2x2", 384, 384, 3, 1, 1, 1, 0, 2, 2),
              ("1x3-8x8", 384, 384, 1, 3, 1, 0, 1, 8, 8), ("3x1-8x8", 384, 384, 3, 1, 1, 1, 0, 8, 8),
              ("1x1-Cout80-7x7", 64, 80, 1, 1, 1, 0, 0, 7, 7)]


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("case", [pytest.param(c, id=c[0], marks=pytest.mark.gate) if c[0] in ("1x7-5x5", "3x1-8x8", "k5-p2-Cin48-7x7") else
                                  pytest.param(c, id=c[0]) for c in CONV_CASES])
def test_new_conv_geometries_on_the_implicit_gemm(case, planes):
    """Builder.conv with bias and ReLU, as the tower launches it, against float64 F.conv2d; pad / padx swapped is another function."""
    from frido_amd.builder import ACT_RELU, Builder
    _, Cin, Cout, kh, kw, stride, pad, padx, H, W = case
    B = 2
    g = torch.Generator().manual_seed(Cin + 10 * kh + kw + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, kh, kw, generator=g) / np.sqrt(kh * kw * Cin)
    bias = torch.randn(Cout, generator=g) * 0.3
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=(pad, padx)))
    Ho, Wo = ref.shape[2:]
    with _lib.use_planes(planes):
        dev = require_gpu("cuda")
        b = Builder(dev, 2, {"c.weight": w.cuda(), "c.bias": bias.cuda()}, planes=planes)
        xr = _rows(x).contiguous().cuda()

        def run(pad, padx):
            b.new_prog()
            a = b.pack(xr.data_ptr(), 1, B * H * W, Cin, 0, Cin)                 # 48 channels are zero-padded to 64 here
            out = b.conv(a, B, H, W, "c", stride=stride, pad=pad, padx=None if padx == pad else padx, Ho=Ho, Wo=Wo, act=ACT_RELU, out="f32_strict")
            assert out.rows == B * Ho * Wo and out.C == Cout
            _lib.status_flags(clear=True)
            b.prog.run(_stream())
            torch.cuda.synchronize()
            assert _lib.status_flags() == 0
            return out.view().cpu().clone()

        got = run(pad, padx)
        swapped = run(padx, pad) if pad != padx else None
    err = float((got.double() - _rows(ref)).abs().max() / ref.abs().max())
    print(f"conv {case[0]} {planes}: rel err {err:.3e}, bound {GEMM_TOL[planes]:.1e}")
    assert err <= GEMM_TOL[planes]
    if swapped is not None:
        assert float((swapped.double() - _rows(ref)).abs().max() / ref.abs().max()) >= 100 * GEMM_TOL[planes]
    if stride == 2:
        bad = F.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=1, padding=(pad, padx)))[:, :, :Ho, :Wo]
        assert float((bad - ref).abs().max() / ref.abs().max()) >= 100 * GEMM_TOL[planes]


# ---- the net ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sd():
    from frido_amd.models import FIDInceptionV3
    return R.filled_state_dict(FIDInceptionV3())


def _images(tag, B, s):
    return torch.from_numpy(synth.seeded_normal(tag, (B, 3, s, s))).clamp(-1, 1)


BLOCK_CASES = ("Mixed_5b", "Mixed_6a", "Mixed_6b", "Mixed_7a", "Mixed_7b", "Mixed_7c")      # A, B, C (c7 = 128), D, E (avg), E (max)


@functools.lru_cache(maxsize=None)
def _block_inputs():
    """The float64 reference's own block inputs at a 107 x 107 tower input, B = 2, rounded to float32: computed once, never changed."""
    inputs = {}
    R.Net(_sd(), torch.float64, True).tower(R.preprocess(R.to_q(_images("fid:img107", 2, 107)), 107), inputs)
    return {n: inputs[n].float() for n in BLOCK_CASES}


@functools.lru_cache(maxsize=None)
def _block_case(name):
    """(input, the float64 branch outputs, the restatement's float32-vs-float64 difference relative to the block's largest output)."""
    x = _block_inputs()[name]
    ref = R.Net(_sd(), torch.float64, True).block(x.double(), name)
    r32 = R.Net(_sd(), torch.float32, True).block(x, name)
    scale = max(float(r.abs().max()) for r in ref)
    return x, ref, max(float((a.double() - r).abs().max()) for a, r in zip(r32, ref)) / scale


@functools.lru_cache(maxsize=None)
def _block_E32():
    return max(_block_case(n)[2] for n in BLOCK_CASES)


_BUILDERS = {}


def _builder(planes):
    from frido_amd.builder import Builder
    if planes not in _BUILDERS:
        with _lib.use_planes(planes):
            dev = require_gpu("cuda")
            _BUILDERS[planes] = Builder(dev, 2, fid.folded_weights(_sd(), dev), planes=planes)
    return _BUILDERS[planes]


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.gate) if n in ("Mixed_6b", "Mixed_7b") else n for n in BLOCK_CASES])
def test_block_matches_float64_range_by_range(name, planes):
    x, ref, _ = _block_case(name)
    B, cin, h, w = x.shape
    assert (h, cin) == (fid.tower_planes(107)[name], fid.BLOCKS[name][1])
    bound = 8.0 * _block_E32() * (BF16_PAIR_RATIO if planes == "bf16" else 1.0)
    scale = max(float(r.abs().max()) for r in ref)
    with _lib.use_planes(planes):
        b = _builder(planes)
        xr = _rows(x).contiguous().cuda()
        prog = b.new_prog()
        pool, out, ho, wo = fid.emit_block(b, name, types.SimpleNamespace(ptr=xr.data_ptr(), C=cin), B, h, w)
        _lib.status_flags(clear=True)
        fid.launch("frido_pool3", pool, _stream())
        prog.run(_stream())
        torch.cuda.synchronize()
        assert _lib.status_flags() == 0
        got = out.view().cpu().clone()
        out.free()
    widths = fid.block_widths(name)
    assert [r.shape[1] for r in ref] == widths and got.shape == (B * ho * wo, sum(widths)) and ref[0].shape[2:] == (ho, wo)
    c0, errs = 0, []
    for r, width in zip(ref, widths):                                         # the concat order, range by range
        errs.append(float((got[:, c0:c0 + width].double() - _rows(r)).abs().max()) / scale)
        c0 += width
    print(f"block {name} {planes}: rel err per branch {' '.join(f'{e:.2e}' for e in errs)}; E32 {_block_E32():.3e}, bound {bound:.3e}")
    assert 0 < bound < 1e-3 and max(errs) <= bound


TOWER_CASES = {"107": ("fid:img107", 2, 107), "299": ("fid:img299", 1, 299)}


@functools.lru_cache(maxsize=None)
def _tower_case(key):
    """(images, float64 features, the restatement's float32-vs-float64 difference relative to the largest feature)."""
    tag, B, s = TOWER_CASES[key]
    img = _images(tag, B, s)
    f64 = R.features(_sd(), img, "pil", s)
    f32 = R.features(_sd(), img, "pil", s, dtype=torch.float32)
    return img, f64, float((f32.double() - f64).abs().max() / f64.abs().max())


@functools.lru_cache(maxsize=None)
def _tower_E32():
    return max(_tower_case(k)[2] for k in TOWER_CASES)


_NETS = {}


def _net(precision, resolution):
    from frido_amd.models import FIDInceptionV3
    key = (precision, resolution)
    if key not in _NETS:
        m = FIDInceptionV3(precision=precision, resolution=resolution)
        m.load_state_dict(_sd())
        _NETS[key] = m.cuda()
    return _NETS[key]


@pytest.mark.parametrize("key,precision", [pytest.param("107", "bf16x3", id="107-f16-pairs", marks=pytest.mark.gate),
                                           pytest.param("107", "bf16x3_bf16", id="107-bf16-pairs"), pytest.param("299", "bf16x3", id="299-f16-pairs")])
def test_tower_matches_float64(key, precision):
    img, f64, _ = _tower_case(key)
    bound = 8.0 * _tower_E32() * (BF16_PAIR_RATIO if precision == "bf16x3_bf16" else 1.0)
    m = _net(precision, TOWER_CASES[key][2])
    _lib.status_flags(clear=True)
    got = m(img.cuda()).cpu()
    assert _lib.status_flags() == 0
    assert got.shape == f64.shape == (img.shape[0], 2048) and got.dtype == torch.float32
    err = float((got.double() - f64).abs().max() / f64.abs().max())
    print(f"tower {key} {precision}: rel err {err:.3e}; E32 {_tower_E32():.3e}, bound {bound:.3e}, ratio err / E32 {err / _tower_E32():.2f}")
    assert 0 < bound < 1e-3 and err <= bound


def test_replay_same_bits_new_shape_replans_and_uint8_equals_its_float_image():
    img, f64, _ = _tower_case("107")
    m = _net("bf16x3", 107)
    x = img.cuda()
    a = m(x)
    n0 = m.graph_captures
    b = m(x)
    assert m.graph_captures == n0 and torch.equal(a, b)                       # a replay: the same graph, the same bits
    c = m(x[:1])
    assert m.graph_captures == n0 + 1 and c.shape == (1, 2048)                # a new shape replans
    assert float((c.cpu().double() - f64[:1]).abs().max() / f64.abs().max()) <= 8.0 * _tower_E32()
    assert torch.equal(m(x), a)                                               # and the first plan is still there
    # the uint8 image the float input quantises to (custom_to_pil) gives the same bits; resized from 64 x 48 this time
    small = _images("fid:img64x48", 2, 64)[:, :, :, :48].contiguous()
    u8 = R.to_q(small, "pil").permute(0, 2, 3, 1).to(torch.uint8).contiguous()
    fa, fb = m(small.cuda()), m(u8.cuda())
    assert m.graph_captures == n0 + 3 and torch.equal(fa, fb)
    ref = R.features(_sd(), small, "pil", 107)
    assert float((fa.cpu().double() - ref).abs().max() / ref.abs().max()) <= 8.0 * _tower_E32()
    assert torch.equal(m(small.cuda(), quant="np"), m(R.to_q(small, "np").permute(0, 2, 3, 1).to(torch.uint8).contiguous().cuda()))


def test_fid_statistics_and_fid_end_to_end():
    """pipeline.fid_statistics over two batches of 4 images on each of two sides, then pipeline.fid, against the float64 reference's
    distance from its own features (tests/inception_ref.py: the singular-value route, which shares no code with frechet_distance).
    The bound is propagated from the feature bound eps = 8 E32 max |f|: the reference's distance recomputed with every feature of
    both sides moved by +-eps (the larger change of two draws of signs)."""
    from frido_amd import pipeline
    m = _net("bf16x3", 107)
    sides, feats = {}, {}
    for side, gain in (("a", 1.0), ("b", 0.6)):
        batches = [(_images(f"fid:e2e:{side}{k}", 4, 40) * gain + (0.2 if side == "b" else 0.0)).clamp(-1, 1) for k in range(2)]
        st = None
        for x in batches:
            st = pipeline.fid_statistics(m, x.cuda(), st)
        sides[side] = st
        feats[side] = torch.cat([R.features(_sd(), x, "pil", 107) for x in batches]).numpy()
    assert sides["a"].n == sides["b"].n == 8 and sides["a"].D == 2048
    got = pipeline.fid(sides["a"], sides["b"])
    ref = R.frechet_from_features(feats["a"], feats["b"])
    eps = 8.0 * _tower_E32() * max(float(np.abs(f).max()) for f in feats.values())
    rng = np.random.default_rng(5)
    moved = max(abs(R.frechet_from_features(feats["a"] + eps * rng.choice([-1.0, 1.0], feats["a"].shape),
                                            feats["b"] + eps * rng.choice([-1.0, 1.0], feats["b"].shape)) - ref) for _ in range(2))
    print(f"fid end to end: hip {got:.9g}, float64 reference {ref:.9g}, |difference| {abs(got - ref):.3e}, bound {moved:.3e}")
    assert isinstance(got, float) and ref > 1.0 and moved > 0 and abs(got - ref) <= moved

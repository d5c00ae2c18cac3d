"""frido_unfold / frido_fold (csrc/fold.hip) on the MI355X against torch.nn.Unfold / torch.nn.Fold evaluated on the CPU, with the
reference's weighting / normalization tables (frido_amd/patching.py).

Unfold is a copy: bit-equal.  Fold: per output element both sides form n products, n - 1 additions and one division in fp32, n = the
number of crops over the pixel; the weights are positive, so the first-order worst case of either side is 2 (n + 1) * 2^-24 * max|o| and
the two may differ by twice that: |got - ref| <= 4 (n + 1) * 2^-24 * max|o| with n = the most crops over one pixel.
Shapes: C = 3 / 6 (latents), 4 / 96 (16-byte path of the fold), crop rows that allow 16-byte copies and rows that do not (10 x 10 x 3),
up to four crops over a pixel, a rectangular map, stride = ks, one crop, 64 x 64 with 32 x 32 crops, B = 1 and 3.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from frido_amd import patching  # noqa: E402

BASE = dict(vqf=4, patch_distributed_vq=True, clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
#        H   W   kh  kw  sy  sx  C   B  tie
CASES = [(16, 16, 8, 8, 4, 4, 3, 1, False),
         (16, 16, 8, 8, 4, 4, 6, 3, True),
         (16, 16, 8, 8, 4, 4, 4, 3, False),
         (16, 16, 8, 8, 4, 4, 96, 1, True),
         (12, 20, 4, 8, 4, 4, 3, 3, False),
         (12, 20, 4, 8, 4, 4, 4, 1, False),
         (10, 10, 4, 4, 3, 3, 3, 3, True),
         (16, 16, 8, 8, 8, 8, 6, 3, False),
         (16, 16, 16, 16, 16, 16, 3, 1, False),
         (64, 64, 32, 32, 16, 16, 3, 3, True)]
IDS = ["%dx%d_k%dx%d_s%dx%d_C%d_B%d_%s" % (c[:8] + ("tie" if c[8] else "notie",)) for c in CASES]
PARAMS = [pytest.param(*c, id=i, marks=pytest.mark.gate) if n in (0, 3) else pytest.param(*c, id=i) for n, (c, i) in enumerate(zip(CASES, IDS))]


def _geo(H, W, kh, kw, sy, sx, tie):
    return patching.geometry(dict(BASE, ks=(kh, kw), stride=(sy, sx), tie_braker=tie), H, W, patching.MODEL, torch.device("cuda"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ref_unfold(x, geo):
    """x (B, C, H, W) on the CPU -> crops [B * L][kh][kw][C], crop l of sample b at b * L + l."""
    _, _, kh, kw, sy, sx = geo.src
    B, Cn = x.shape[:2]
    u = torch.nn.Unfold(kernel_size=(kh, kw), dilation=1, padding=0, stride=(sy, sx))(x).view(B, Cn, kh, kw, geo.L)
    return u.permute(0, 4, 2, 3, 1).reshape(B * geo.L, kh, kw, Cn).contiguous()


def _ref_fold(o, geo, B):
    """o [B * L][kh][kw][C] on the CPU -> the reference's fold(o * weighting) / normalization, NHWC (frido.py:1147-1152)."""
    H, W, kh, kw, sy, sx = geo.out
    Cn = o.shape[-1]
    v = o.view(B, geo.L, kh, kw, Cn).permute(0, 4, 2, 3, 1) * geo.weighting.view(1, 1, kh, kw, geo.L)
    f = torch.nn.Fold(output_size=(H, W), kernel_size=(kh, kw), dilation=1, padding=0, stride=(sy, sx))(v.reshape(B, Cn * kh * kw, geo.L))
    return (f / geo.normalization.view(1, 1, H, W)).permute(0, 2, 3, 1).contiguous()


def _fold(geo, crops, B, Cn, u8_mode=0, f32=True):
    H, W = geo.out[:2]
    out = torch.full((B, H, W, Cn), float("nan"), device="cuda") if f32 else None
    u8 = torch.zeros(B, H, W, Cn, dtype=torch.uint8, device="cuda") if u8_mode else None
    patching.launch_fold(geo.fold_desc(crops.data_ptr(), out.data_ptr() if f32 else None, B, Cn, out_u8=u8.data_ptr() if u8_mode else None,
                                       u8_mode=u8_mode), _stream())
    torch.cuda.synchronize()
    return out, u8


@pytest.mark.parametrize("H,W,kh,kw,sy,sx,Cn,B,tie", PARAMS)
def test_unfold_is_bit_equal_and_fold_is_within_the_rounding_bound(H, W, kh, kw, sy, sx, Cn, B, tie):
    geo = _geo(H, W, kh, kw, sy, sx, tie)
    gen = torch.Generator().manual_seed(H * 1000 + Cn * 10 + B)
    x = torch.randn(B, Cn, H, W, generator=gen)
    xs = x.permute(0, 2, 3, 1).contiguous().cuda()
    crops = torch.full((B * geo.L, kh, kw, Cn), float("nan"), device="cuda")
    patching.launch_unfold(geo.unfold_desc(xs.data_ptr(), crops.data_ptr(), B, Cn), _stream())
    torch.cuda.synchronize()
    assert torch.equal(crops.cpu(), _ref_unfold(x, geo))
    # fold of independent crop values (what a model returns), not of the unfolded map
    o = torch.randn(B * geo.L, kh, kw, Cn, generator=gen) * 3.0
    od = o.cuda()
    got, _ = _fold(geo, od, B, Cn)
    ref = _ref_fold(o, geo, B)
    n = geo.max_cover
    bound = 4 * (n + 1) * 2.0 ** -24 * float(o.abs().max())
    err = float((got.cpu() - ref).abs().max())
    print(f"fold: max |got - ref| = {err:.3e}, bound {bound:.3e} (n = {n}, L = {geo.L})")
    assert torch.isfinite(got).all() and err <= bound
    # no atomics, fixed order: a second launch gives the same bits
    again, _ = _fold(geo, od, B, Cn)
    assert torch.equal(got, again)
    # folding the unfolded map gives the map back (a weighted mean of equal values), to the same bound
    back, _ = _fold(geo, crops, B, Cn)
    assert float((back.cpu() - xs.cpu()).abs().max()) <= 4 * (n + 1) * 2.0 ** -24 * float(x.abs().max())


def _np_u8(v):      # scripts/sample_diffusion.py:115-121 custom_to_np, with torch on the CPU as the script does
    return ((v + 1) * 127.5).clamp(0, 255).to(torch.uint8)


def _pil_u8(v):     # scripts/sample_diffusion.py:103-113 custom_to_pil: clamp, (x + 1) / 2, numpy's 255 * x, astype(uint8)
    return torch.from_numpy((255 * ((torch.clamp(v, -1., 1.) + 1.) / 2.).numpy()).astype(np.uint8))


@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("mode,conv", [(1, _np_u8), (2, _pil_u8)])
def test_u8_output_is_both_formulas_applied_to_the_f32_fold(Cn, mode, conv):
    geo = _geo(16, 16, 8, 8, 4, 4, True)
    B = 2
    o = (torch.randn(B * geo.L, 8, 8, Cn, generator=torch.Generator().manual_seed(3)) * 0.8).cuda()      # a good share beyond [-1, 1]
    f32, _ = _fold(geo, o, B, Cn)
    both, u8 = _fold(geo, o, B, Cn, u8_mode=mode)
    _, only = _fold(geo, o, B, Cn, u8_mode=mode, f32=False)
    assert torch.equal(both, f32)
    want = conv(f32.cpu())
    assert 0 in want and 255 in want and torch.equal(u8.cpu(), want) and torch.equal(only.cpu(), want)


def test_fold_replayed_from_a_captured_program_equals_the_direct_launch():
    """[FRIDO_OP_UNFOLD, FRIDO_OP_COPY, FRIDO_OP_FOLD] as one program: run, then captured as one graph and replayed on new data."""
    from frido_amd import _lib
    from frido_amd.engine import Prog, require_gpu
    dev = require_gpu("cuda")
    geo = _geo(16, 16, 8, 8, 4, 4, False)
    B, Cn = 2, 6
    gen = torch.Generator().manual_seed(5)
    xs = torch.randn(B, 16, 16, Cn, generator=gen).cuda()
    crops = torch.zeros(B * geo.L, 8, 8, Cn, device="cuda")
    moved = torch.zeros_like(crops)
    out = torch.zeros(B, 16, 16, Cn, device="cuda")
    prog = Prog(dev, 2)
    prog.ops.append(_lib.op_of("FRIDO_OP_UNFOLD", geo.unfold_desc(xs.data_ptr(), crops.data_ptr(), B, Cn)))
    prog.emit("FRIDO_OP_COPY", src=crops.data_ptr(), dst=moved.data_ptr(), n=crops.numel() * 4)
    prog.ops.append(_lib.op_of("FRIDO_OP_FOLD", geo.fold_desc(moved.data_ptr(), out.data_ptr(), B, Cn)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        prog.run(side.cuda_stream)
        side.synchronize()
        direct = out.clone()
        graph = prog.capture(side.cuda_stream)
        xs.copy_(torch.randn(B, 16, 16, Cn, generator=gen))      # new data at the captured addresses
        out.zero_()
        graph.launch(side.cuda_stream)
        side.synchronize()
        replay = out.clone()
        prog.run(side.cuda_stream)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert not torch.equal(replay, direct) and torch.equal(replay, out)
    assert float((replay - xs).abs().max()) <= 4 * 5 * 2.0 ** -24 * float(xs.abs().max())

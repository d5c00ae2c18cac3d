"""Multi-head flash attention (csrc/flash_mh.hip, FRIDO_OP_ATTN_MH) on the MI355X: the op against float64 torch on seeded data, in
both builds of the library (fp16-pair and bf16-pair planes), nsplit 2 and 1, both head orders of the reference's AttentionBlock
(pyunet.py:381-440: QKVAttentionLegacy / QKVAttention).

The bound is the one tests/test_kernels_gpu.py::test_attention_flash uses for the same arithmetic (two products in series, the
probabilities re-split into a pair): 5e-5 max-relative on fp16 pairs, ATTN_BF16_TOL = 2e-4 on bf16 pairs, 2e-2 for nsplit 1.  The
helpers are restated here (that module is not imported: its twins and report fixture belong to it).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ATTN_BF16_TOL = 2 * 1e-4      # test_kernels_gpu.ATTN_BF16_TOL: twice the bf16-pair GEMM bound X3_BF16_TOL = 1e-4


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _tol(nsplit, planes):
    if nsplit != 2:
        return 2e-2
    return 5e-5 if planes == "f16" else ATTN_BF16_TOL


def _relerr(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def _builder(nsplit):
    from frido_amd.builder import Builder
    return Builder(_dev(), nsplit, {})


def _run(b):
    b.prog.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _cols(order, heads, d):
    """Columns of q / k / v of (head, channel) inside a qkv row of 3 C: legacy = heads split first (q | k | v per head), new = qkv
    split first (pyunet.py:399 / :431)."""
    h, j = torch.arange(heads)[:, None], torch.arange(d)[None, :]
    if order == "legacy":
        q = 3 * d * h + j
        return q.flatten(), (q + d).flatten(), (q + 2 * d).flatten()
    q = d * h + j
    return q.flatten(), (q + heads * d).flatten(), (q + 2 * heads * d).flatten()


def _reference(q, k, v):
    """softmax(q k^T / sqrt(d)) v per (sample, head) in float64 on the device, one sample at a time; q [B, Nq, heads, d] -> [B*Nq, C]."""
    B, Nq, heads, d = q.shape
    out = []
    for z in range(B):
        qz, kz, vz = (t[z].cuda().double().transpose(0, 1) for t in (q, k, v))          # [heads, N, d]
        o = torch.softmax(qz @ kz.transpose(1, 2) * d ** -0.5, -1) @ vz
        out.append(o.transpose(0, 1).reshape(Nq, heads * d).float().cpu())
    return torch.cat(out)


def _launch(b, order, q, k, v):
    """Emit the op for q [B, Nq, heads, d], k / v [B, Nk, heads, d] laid out as the qkv projection leaves them in `order`: rows of
    3 C columns (the columns of the other two tensors hold decoy data), V^T head-major [B][C][Nk_pad].  Nq == Nk goes through
    Builder.attention_heads on ONE operand, the ragged cases through Builder.attention_mh on two."""
    from frido_amd.engine import pack_matrix
    B, Nq, heads, d = q.shape
    Nk, Cc = k.shape[1], heads * d
    qc, kc, vc = _cols(order, heads, d)
    vto = pack_matrix(v.reshape(B, Nk, Cc).transpose(1, 2).reshape(B * Cc, Nk).cuda(), b.nsplit)
    hs, k_off = (3 * d, d) if order == "legacy" else (d, Cc)
    if Nq == Nk:
        m = _randn(7, B * Nq, 3 * Cc)
        m[:, qc], m[:, kc], m[:, vc] = q.reshape(B * Nq, Cc), k.reshape(B * Nk, Cc), v.reshape(B * Nk, Cc)
        op = pack_matrix(m.cuda(), b.nsplit)
        return b.attention_heads(op, 3 * Cc, vto, B, Nq, heads, d, legacy=order == "legacy"), (op, vto)
    mq, mk = _randn(8, B * Nq, 3 * Cc), _randn(9, B * Nk, 3 * Cc)
    mq[:, qc], mk[:, kc] = q.reshape(B * Nq, Cc), k.reshape(B * Nk, Cc)
    qo, ko = pack_matrix(mq.cuda(), b.nsplit), pack_matrix(mk.cuda(), b.nsplit)
    return b.attention_mh(qo, 3 * Cc, 0, hs, ko, 3 * Cc, k_off, hs, vto, B, Nq, Nk, heads, d), (qo, ko, vto)


SHAPES = [
    pytest.param(2, 2, 256, 256, 32, marks=pytest.mark.gate),
    pytest.param(2, 3, 64, 64, 32, marks=pytest.mark.gate),
    (16, 12, 1024, 1024, 32),          # f8f4 denoiser, 32 x 32 plane
    pytest.param(16, 30, 64, 64, 32, marks=pytest.mark.gate),      # 8 x 8 plane and the middle block
    (2, 6, 1024, 1024, 64),
    (1, 8, 4096, 4096, 64),
    pytest.param(2, 3, 200, 333, 64, marks=pytest.mark.gate),      # ragged: Nq % 16 != 0, Nk % 32 != 0
    pytest.param(1, 2, 16, 129, 32, marks=pytest.mark.gate),       # one query fragment, five key groups
    (8, 8, 1024, 1024, 64),            # d = 64 with two query fragments per wave (>= 512 workgroups of 128 queries)
    (32, 8, 200, 333, 32),             # ragged with two query fragments per wave
]


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("order", ["legacy", "new"])
@pytest.mark.parametrize("B,heads,Nq,Nk,d", SHAPES)
def test_attention_mh(planes, nsplit, order, B, heads, Nq, Nk, d):
    """The op against float64 torch; k scaled by 1.5 as test_attention_flash does."""
    from frido_amd import _lib
    q, k, v = _randn(1, B, Nq, heads, d), _randn(2, B, Nk, heads, d) * 1.5, _randn(3, B, Nk, heads, d)
    with _lib.use_planes(planes):
        b = _builder(nsplit)
        o, keep = _launch(b, order, q, k, v)
        assert sum(kind == _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] for kind, _ in b.prog.ops) == 1
        _run(b)
        got = o.to_f32().cpu()
    err, tol = _relerr(got, _reference(q, k, v)), _tol(nsplit, planes)
    print(f"attn_mh {planes} nsplit {nsplit} {order} {(B, heads, Nq, Nk, d)}: max-relative error {err:.3e} (bound {tol:.1e})")
    assert err < tol


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("d", [32, 64])
def test_attention_mh_online_softmax_rescale_branch(planes, d):
    """A key far above the rest in a LATE tile forces the running-max rescale of the accumulated O (rare on random data); an early
    spike must not make later tiles rescale."""
    from frido_amd import _lib
    B, heads, Nq, Nk = 1, 2, 64, 512
    q, k, v = _randn(11, B, Nq, heads, d), _randn(12, B, Nk, heads, d), _randn(13, B, Nk, heads, d)
    k[0, 300, 1] = q[0, 5, 1] * 6.0          # query 5 of head 1 spikes on key 300 (tile 4, second group)
    k[0, 40, 0] = q[0, 50, 0] * 5.0          # an early spike in head 0
    ref = _reference(q, k, v)
    with _lib.use_planes(planes):
        for nsplit in (2, 1):
            b = _builder(nsplit)
            o, keep = _launch(b, "legacy", q, k, v)
            _run(b)
            err = _relerr(o.to_f32().cpu(), ref)
            print(f"attn_mh rescale {planes} nsplit {nsplit} d {d}: {err:.3e}")
            assert err < _tol(nsplit, planes)


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_attention_mh_heads_do_not_share_the_running_max(planes):
    """Head 0's scores all lie far below head 1's: a running max (or sum) leaking from one head into the other would flush head 0's
    probabilities to zero."""
    from frido_amd import _lib
    B, heads, Nq, Nk, d = 2, 2, 128, 192, 32
    q, k, v = _randn(21, B, Nq, heads, d), _randn(22, B, Nk, heads, d), _randn(23, B, Nk, heads, d)
    k[:, :, 0] *= 0.01                       # head 0: |scores| ~ 0.01
    k[:, :, 1] = q[:, :1, 1] * 8.0 + k[:, :, 1]      # head 1: scores of ~ +45 and more against query 0, large for its neighbours
    ref = _reference(q, k, v)
    with _lib.use_planes(planes):
        for order in ("legacy", "new"):
            b = _builder(2)
            o, keep = _launch(b, order, q, k, v)
            _run(b)
            got = o.to_f32().cpu()
            assert _relerr(got[:, :d], ref[:, :d]) < _tol(2, planes) and _relerr(got[:, d:], ref[:, d:]) < _tol(2, planes)


def test_attention_mh_output_saturates_and_raises_the_status_bit():
    """The output leaves through the library's plane producers: a value past 65504 saturates there and sets FRIDO_STATUS_SATURATED on
    the fp16-pair build; the bf16-pair build keeps fp32's range and raises nothing."""
    from frido_amd import _lib
    from frido_amd.engine import plane_dtype
    B, heads, N, d = 1, 2, 64, 32
    q, k = _randn(31, B, N, heads, d), _randn(32, B, N, heads, d)
    for planes in ("f16", "bf16"):
        with _lib.use_planes(planes):
            _lib.status_flags(clear=True)
            b = _builder(2)
            o, keep = _launch(b, "legacy", q, k, torch.ones(B, N, heads, d))
            _run(b)
            assert _lib.status_flags() == 0 and _relerr(o.to_f32().cpu(), torch.ones(N, heads * d)) < 1e-5      # clean work raises nothing
            b = _builder(2)
            o, keep = _launch(b, "legacy", q, k, torch.full((B, N, heads, d), 7.0e4 if planes == "bf16" else 1.0))
            if planes == "f16":          # every v = 65504 + 15 as a valid hi + lo pair (the host packer would clamp at 65504)
                assert plane_dtype(2) == torch.float16
                keep[-1].t[0].fill_(65504.0)
                keep[-1].t[1].fill_(15.0)
            _run(b)
            got = o.to_f32().cpu()
            if planes == "f16":
                assert float(got.max()) == 65504.0 and torch.isfinite(got).all()
                assert _lib.status_flags(clear=True) == _lib.STATUS_SATURATED
            else:
                assert _relerr(got, torch.full((N, heads * d), 7.0e4)) < ATTN_BF16_TOL
                assert _lib.status_flags(clear=True) == 0


def test_attention_mh_rejects_an_unsupported_head_dimension():
    """d = 48: the launcher returns FRIDO_EINVAL and launches nothing; the builder refuses it before emitting an op."""
    from frido_amd import _lib
    from frido_amd import builder as builder_mod
    from frido_amd.engine import pack_matrix
    L = _lib.lib()
    assert [bool(L.frido_attn_mh_supported(x)) for x in (16, 32, 48, 64, 96, 128)] == [x in builder_mod.MH_HEAD_DIMS for x in (16, 32, 48, 64, 96, 128)]
    B, heads, N, d = 1, 2, 64, 48
    Cc = heads * d
    m = pack_matrix(_randn(41, B * N, 3 * Cc).cuda(), 2)
    vt = pack_matrix(_randn(42, B * Cc, N).cuda(), 2)
    out = torch.full((2, B * N * Cc), 3.0, dtype=torch.float16, device="cuda")
    _, st = _lib.make_op("FRIDO_OP_ATTN_MH", Q=m.ptr, q_lo=m.lo, ldq=3 * Cc, q_hs=3 * d, K=m.ptr + 2 * d, k_lo=m.lo, k_bs=N * 3 * Cc,
                         ldk=3 * Cc, k_hs=3 * d, VT=vt.ptr, vt_lo=vt.lo, vt_bs=Cc * N, ldvt=N, out_op=out.data_ptr(), out_lo=B * N * Cc,
                         ldo=Cc, B=B, heads=heads, Nq=N, Nk=N, d=d, nsplit=2, alpha=d ** -0.5)
    rc = L.frido_attn_mh(C.addressof(st), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"head dimension" in L.frido_last_error()
    assert bool((out == 3.0).all())
    b = _builder(2)
    with pytest.raises(NotImplementedError, match="32, 64"):
        b.attention_heads(m, 3 * Cc, vt, B, N, heads, d)
    assert not b.prog.ops


@pytest.mark.gate
@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_attention_mh_replays_in_a_captured_graph(planes):
    """No allocation and no synchronisation inside: the program replays bit for bit inside a captured hipGraph."""
    from frido_amd import _lib
    B, heads, Nq, Nk, d = 2, 3, 200, 333, 32
    q, k, v = _randn(51, B, Nq, heads, d), _randn(52, B, Nk, heads, d), _randn(53, B, Nk, heads, d)
    with _lib.use_planes(planes):
        b = _builder(2)
        o, keep = _launch(b, "new", q, k, v)
        _run(b)
        n = 2 * o.lo * 2
        eager = o.buf[:n].clone()
        o.buf[:n].zero_()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = b.prog.capture(s.cuda_stream)
            g.launch(s.cuda_stream)
        s.synchronize()
        assert torch.equal(o.buf[:n], eager)
        o.buf[:n].zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.launch(s.cuda_stream)
        s.synchronize()
        assert torch.equal(o.buf[:n], eager)

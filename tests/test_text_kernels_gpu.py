"""Kernel-level float64 reference tests (MI355X) for what the conditioning encoders run on (frido_amd/bert_plan.py,
frido_amd/clip_plan.py) and only model-level tests reached before:

  A  the head-batched GEMM (FridoGemm.batch_inner with a_bs2 / b_bs2 / of_bs2 / oo_bs2): QK^T and PV as the plans emit them
  B  the causal (FridoSoftmax.causal_nq) and the strided (ld > N) row softmax
  C  the RELU / GELU / QUICKGELU switch in every epilogue implementation (slab vector, scalar, both split-K reduce kernels, in-kernel)
  D  gelu_f / quickgelu_f / silu_f / relu element by element on a grid of exact pre-activation values
  E  LayerNorm at its edges: lane-boundary widths, partly idle workgroups, out_f32, bf16 rows (fast and general path), rejections
  F  Builder.v_transposed into a persistent operand with a ragged key count
  G  QK^T -> softmax -> PV as the towers chain them, every row against float64 multi-head attention

Every reference is float64 torch / numpy written here.  The bounds and the three-pass emulation are those of tests/test_kernels_gpu.py
(imported, not restated); each test runs on the fp16-pair build, the bf16-pair build (nsplit 2) and with one-plane bf16 operands
(nsplit 1, one build).  The worst error of every part against its bound is reported per mode at the end of the module.
"""
import ctypes as C_
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frido_amd.synth import seeded_normal  # noqa: E402
from test_kernels_gpu import (ATTN_BF16_TOL, PAIR_FLOOR, PAIR_U, X3_BF16_TOL, _builder, _dev, _emu_tol, _pair_planes,  # noqa: E402,F401
                              _pass_products, _planes, _run, _three_pass, _tol)

MODES = [("f16", 2), ("bf16", 2), ("f16", 1)]      # (plane format of the build, nsplit); one-plane bf16 operands need one build only
ACT_RELU, ACT_SILU, ACT_GELU, ACT_QUICKGELU = 1, 2, 3, 4
ACT_NAMES = {ACT_RELU: "relu", ACT_SILU: "silu", ACT_GELU: "gelu", ACT_QUICKGELU: "quickgelu"}


def _modes(fn):
    """Parametrise a test on MODES and run its body inside _lib.use_planes(planes)."""
    @functools.wraps(fn)
    def run(planes, nsplit, *args, **kwargs):
        from frido_amd import _lib
        with _lib.use_planes(planes):
            return fn(planes, nsplit, *args, **kwargs)
    return pytest.mark.parametrize("planes,nsplit", MODES)(run)


def _t(tag, *shape):
    return torch.from_numpy(seeded_normal("text:" + tag, shape))


def _rup(x, m):
    return (x + m - 1) // m * m


_REPORT = {}      # (part, mode) -> (worst error / bound, error, bound, test)


def _check(part, nsplit, err, bound):
    """err < bound, recording the worst ratio met per part and mode."""
    mode = f"{_planes()} x{nsplit}"
    ratio = err / bound
    if ratio >= _REPORT.get((part, mode), (-1.0,))[0]:
        _REPORT[(part, mode)] = (ratio, err, bound, os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1])
    print(f"{part} [{mode}]: error {err:.3e}, bound {bound:.1e}")
    assert err < bound, (part, mode, err, bound)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's last test: the margins, printed (pytest shows them with -s or -rA)."""
    yield
    if not _REPORT:
        return
    print("\nworst error against its bound per part and mode (test_text_kernels_gpu):")
    for (part, mode), (ratio, err, bound, where) in sorted(_REPORT.items()):
        print(f"  {part:<28} {mode:>8}  error {err:.2e}  bound {bound:.1e}  ({100 * ratio:5.1f} % of it)  {where}")


def _maxrel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def _raw_planes(op):
    """The planes of an Operand / POperand as written, on the CPU: [nsplit][batch * rows][K] in the plane dtype."""
    from frido_amd.engine import plane_dtype
    n = op.batch * op.rows * op.K
    t = op.t if hasattr(op, "t") else op.buf[: op.nsplit * op.lo * 2].view(plane_dtype(op.nsplit)).view(op.nsplit, op.lo)
    return t[:, :n].cpu().view(op.nsplit, op.batch * op.rows, op.K)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _host_split(y, nsplit):
    """The planes [nsplit][...] an f32 value splits into (engine.pack_matrix's casts; the kernels' split_op gives the same bits)."""
    from frido_amd.engine import plane_dtype
    dt = plane_dtype(nsplit)
    w = y.float()
    if dt == torch.float16:
        w = w.clamp(-65504.0, 65504.0)
    hi = w.to(dt)
    if nsplit == 1:
        return hi[None]
    return torch.stack([hi, (w - hi.float()).to(dt)])


def _three(part, nsplit, got, passes, epi, what, out="f32"):
    d = _three_pass(got, passes, epi, what, out=out)
    _check(part + " three-pass", nsplit, d["kernel"], _emu_tol(passes["K"]))


# ---- A. the head-batched GEMM ----------------------------------------------------------------------------------------------------
A_SHAPES = [(2, 3, 26, 64),      # BERT-like: ldo = 26 and of_bs2 = 676 are no multiples of 8 -> scalar epilogue
            (3, 4, 16, 32),      # CLIP small: every tile taller than n and wider than dh
            (1, 12, 77, 64),     # ViT-L/14 text tower: odd n, two row tiles at 64 x 64
            (2, 2, 32, 32)]      # every stride a multiple of 8 -> vector epilogue
PV_ONLY = (2, 3, 26, 20)         # written into a 64-wide operand: oo_bs2 = 20 -> scalar path, columns 60 .. 63 keep their contents
TILES = [0, 3, 1]                # the library's own choice, 64 x 64, 128 x 128
GUARD_ROWS = 5


def _heads_qkt(q, k, B, H, n, dh):
    """[B*n][H*dh] x [B*n][H*dh] -> per (sample, head) q k^T as [B*H*n][n] (float64)."""
    return torch.einsum("bnhd,bmhd->bhnm", q.double().reshape(B, n, H, dh), k.double().reshape(B, n, H, dh)).reshape(B * H * n, n)


def _heads_pv(p, vt, B, H, n, dh):
    """p [B*H*n][Np] x vT [B*H*dh][Np] -> [B*n][H*dh] (float64); pad columns take part (they must be zero)."""
    Np = p.shape[1]
    return torch.einsum("bhmk,bhdk->bmhd", p.double().view(B, H, n, Np), vt.double().view(B, H, dh, Np)).reshape(B * n, H * dh)


def _emit_qkt(b, qk_op, s_ptr, B, H, n, dh, tile=0):
    inner = H * dh       # as bert_plan.py / clip_plan.py emit it
    b.prog.gemm(n, n, dh, qk_op, (qk_op.ptr + 2 * inner, qk_op.lo), batch=B * H, batch_inner=H, lda=2 * inner, ldb=2 * inner,
                a_bs=n * 2 * inner, a_bs2=dh, b_bs=n * 2 * inner, b_bs2=dh, alpha=float(dh) ** -0.5,
                out_f32=s_ptr, of_bs=H * n * n, of_bs2=n * n, ldo=n, tile=tile)


def _emit_pv(b, pr, vT, o_ptr, o_lo, ldoo, B, H, n, dh, tile=0):
    Np, inner = _rup(n, 32), H * dh
    b.prog.gemm(n, dh, Np, pr, vT, batch=B * H, batch_inner=H, lda=Np, ldb=Np, a_bs=H * n * Np, a_bs2=n * Np,
                b_bs=inner * Np, b_bs2=dh * Np, out_op=o_ptr, oo_bs=n * ldoo, oo_bs2=dh, ldoo=ldoo, oo_lo=o_lo, tile=tile)


@_modes
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("B,H,n,dh", A_SHAPES)
def test_batch_inner_qkt(planes, nsplit, B, H, n, dh, tile):
    """scores[b][h] = dh^-0.5 q[b][:, h] k[b][:, h]^T, A and B column windows of ONE operand [B*n][2 H dh], f32 output [B*H*n][n]
    followed by guard rows.  Every (sample, head) block holds different data: a swapped or mis-strided block fails the value check,
    a row or column masked one too few lands in the next head's block or in the guard."""
    from frido_amd.engine import pack_matrix
    inner, rows = H * dh, B * H * n
    qk = _t(f"A:qk:{B}:{H}:{n}:{dh}", B * n, 2 * inner)
    b = _builder(nsplit)
    qk_op = pack_matrix(qk.cuda(), nsplit)
    s = torch.full(((rows + GUARD_ROWS) * n,), -12345.678, dtype=torch.float32, device=_dev())
    before = s.clone()
    _emit_qkt(b, qk_op, s.data_ptr(), B, H, n, dh, tile)
    _run(b)
    got = s[: rows * n].view(rows, n).cpu()
    ref = _heads_qkt(qk[:, :inner], qk[:, inner:], B, H, n, dh) * float(dh) ** -0.5
    _check("A QK^T", nsplit, _maxrel(got, ref), _tol(nsplit))
    assert torch.equal(_bits(s[rows * n:]), _bits(before[rows * n:])), "guard rows after the last sample were written"
    if nsplit == 2:
        hi, lo = _pair_planes(qk_op)
        f = lambda x, y: _heads_qkt(x[:, :inner], y[:, inner:], B, H, n, dh)      # noqa: E731
        alpha = float(np.float32(float(dh) ** -0.5))
        _three("A QK^T", nsplit, got, {"hh": f(hi, hi), "hl": f(hi, lo), "lh": f(lo, hi), "K": dh}, lambda y: alpha * y,
               f"batch_inner QK^T {(B, H, n, dh)} tile {tile}")


@_modes
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("B,H,n,dh", A_SHAPES + [PV_ONLY])
def test_batch_inner_pv(planes, nsplit, B, H, n, dh, tile):
    """o[b][:, h] = p[b][h] v[b][:, h]: A the probabilities [B*H*n][Np] (bit-zero pad columns), B the transposed values
    [B][H*dh][Np], the output an operand [B*n][ldoo] with head h at columns h dh ..; guard columns beyond H dh and guard rows after
    the last sample hold a pattern that must survive."""
    from frido_amd.engine import Operand, pack_matrix
    inner, Np = H * dh, _rup(n, 32)
    ldoo = 64 if (B, H, n, dh) == PV_ONLY else inner + 8
    p = torch.softmax(2.0 * _t(f"A:s:{B}:{H}:{n}:{dh}", B * H * n, n).double(), -1).float()
    v = _t(f"A:v:{B}:{H}:{n}:{dh}", B, n, inner)
    b = _builder(nsplit)
    pr = pack_matrix(p.cuda(), nsplit)                                              # K zero-padded to Np
    vT = pack_matrix(v.transpose(1, 2).reshape(B * inner, n).cuda(), nsplit)
    assert pr.K == Np and vT.K == Np
    o = Operand(B * n + GUARD_ROWS, ldoo, nsplit, _dev())
    _bits(o.t).fill_(0x5A5A)
    before = _bits(_raw_planes(o)).clone()
    _emit_pv(b, pr, vT, o.ptr, o.lo, ldoo, B, H, n, dh, tile)
    _run(b)
    after = _raw_planes(o)
    ref = _heads_pv(p, v.transpose(1, 2).reshape(B * inner, n), B, H, n, dh)
    got = o.to_f32().cpu()[: B * n, :inner]
    _check("A PV", nsplit, _maxrel(got, ref), _tol(nsplit))
    written = torch.zeros(B * n + GUARD_ROWS, ldoo, dtype=torch.bool)
    written[: B * n, :inner] = True
    assert torch.equal(_bits(after)[:, ~written], before[:, ~written]), "guard rows / columns of the output operand were written"
    if nsplit == 2:
        (ph, pl), (vh, vl) = _pair_planes(pr), _pair_planes(vT)
        f = lambda x, y: _heads_pv(x, y, B, H, n, dh)      # noqa: E731
        oh, ol = _pair_planes(o)
        _three("A PV", nsplit, (oh + ol)[: B * n, :inner], {"hh": f(ph, vh), "hl": f(ph, vl), "lh": f(pl, vh), "K": Np}, lambda y: y,
               f"batch_inner PV {(B, H, n, dh)} tile {tile}", out="op")


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_batch_inner_rejects_what_it_cannot_run(planes):
    """batch_inner > 1 with a residual, and a batch that is no multiple of batch_inner: rejected, nothing written; the same descriptor
    without the fault runs."""
    from frido_amd import _lib
    from frido_amd.engine import pack_matrix
    with _lib.use_planes(planes):
        B, H, n, dh = 2, 3, 26, 64
        inner, rows = H * dh, B * H * n
        qk = _t(f"A:qk:{B}:{H}:{n}:{dh}", B * n, 2 * inner)
        qk_op = pack_matrix(qk.cuda(), 2)
        s = torch.full((rows * n,), -12345.678, dtype=torch.float32, device=_dev())
        before = s.clone()
        res = torch.zeros(rows * n, dtype=torch.float32, device=_dev())
        _, st = _lib.make_op("FRIDO_OP_GEMM", M=n, N=n, K=dh, batch=B * H, batch_inner=H, nsplit=2, A=qk_op.ptr, a_lo=qk_op.lo,
                             lda=2 * inner, a_bs=n * 2 * inner, a_bs2=dh, B=qk_op.ptr + 2 * inner, b_lo=qk_op.lo, ldb=2 * inner,
                             b_bs=n * 2 * inner, b_bs2=dh, alpha=float(dh) ** -0.5, out_f32=s.data_ptr(), of_bs=H * n * n, of_bs2=n * n,
                             ldo=n, tile=3)
        L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
        st.residual, st.ldr = res.data_ptr(), n
        assert L.frido_gemm(C_.addressof(st), stream) == -1 and b"no residual" in L.frido_last_error()
        st.residual, st.ldr = None, 0
        st.batch = B * H - 1
        assert L.frido_gemm(C_.addressof(st), stream) == -1 and b"outer * inner" in L.frido_last_error()
        torch.cuda.synchronize()
        assert torch.equal(_bits(s), _bits(before)), "a rejected launch wrote to its output"
        st.batch = B * H
        assert L.frido_gemm(C_.addressof(st), stream) == 0
        torch.cuda.synchronize()
        ref = _heads_qkt(qk[:, :inner], qk[:, inner:], B, H, n, dh) * float(dh) ** -0.5
        assert _maxrel(s.view(rows, n).cpu(), ref) < _tol(2)


# ---- B. causal and strided softmax -----------------------------------------------------------------------------------------------
def _poison(x, visible):
    """Everything outside the visible keys of a score row (future keys, ld padding) holds 1e30 or NaN, alternating."""
    r, c = torch.meshgrid(torch.arange(x.shape[0]), torch.arange(x.shape[1]), indexing="ij")
    bad = torch.where((r + c) % 2 == 0, torch.tensor(1.0e30), torch.tensor(float("nan")))
    return torch.where(c < visible[:, None], x, bad)


def _masked_softmax64(x, visible):
    """float64 softmax of each row over its first visible[r] keys, zero elsewhere (a row with no visible key is all zero)."""
    c = torch.arange(x.shape[1])[None, :]
    m = c < visible[:, None]
    p = torch.softmax(x.double().masked_fill(~m, float("-inf")), -1)
    return torch.where(m, p, torch.zeros((), dtype=torch.float64))


def _row_err(got, ref):
    """max over the rows of max |got - ref| / max ref: the error in units of each row's own maximum."""
    return float(((got.double() - ref).abs().amax(1) / ref.amax(1).clamp_min(1e-30)).max())


def _softmax_case(part, nsplit, x_clean, visible, N, ld, causal_nq):
    """Launch the row softmax on x_clean [rows][N] stored with row stride ld, poisoned outside the visible keys; check values (float64),
    bit-zero masked / pad entries in every plane, finiteness and the status word.  Returns (reference, bound, hi plane bits, lo plane)."""
    from frido_amd import _lib
    rows, Np = x_clean.shape[0], _rup(N, 32)
    x = torch.zeros(rows, ld)
    x[:, :N] = x_clean
    x = _poison(x, visible)
    b = _builder(nsplit)
    f = b.f32_strict(rows, ld)
    f.view().copy_(x.cuda())
    _lib.status_flags(clear=True)
    p = b.softmax(f, rows, N, ld, Np, causal_nq=causal_nq)
    _run(b)
    assert _lib.status_flags(clear=True) == 0, "the status word was raised"
    raw = _raw_planes(p)                                        # [nsplit][rows][Np]
    got = raw.double().sum(0)
    assert bool(torch.isfinite(raw.float()).all()), "a non-finite value came out"
    ref = _masked_softmax64(x_clean, visible)
    # the existing softmax numbers: 2e-5 on the fp16 pair, the bf16-pair / one-plane bounds elsewhere -- here of each row's own maximum
    bound = _tol(nsplit)
    _check(part, nsplit, _row_err(got[:, :N], ref), bound)
    dead = torch.ones(rows, Np, dtype=torch.bool)
    dead[:, :N] = torch.arange(N)[None, :] >= visible[:, None]
    assert int(_bits(raw)[:, dead].abs().max()) == 0, "masked / pad entries are not bit-zero in every plane"
    return ref, bound, raw


@_modes
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 77])
def test_softmax_causal(planes, nsplit, n, pad):
    """FridoSoftmax.causal_nq = n over rows = B H n: row r sees keys 0 .. (r mod n).  Scores 4 * normal, one fully visible row spanning
    +-60; future keys and the ld padding hold 1e30 / NaN, which the kernel must never read."""
    B, H = 2, 3
    rows = B * H * n
    x = 4.0 * _t(f"B:s:{n}", rows, n)
    x[2 * n - 1] = torch.linspace(-60.0, 60.0, n) if n > 1 else torch.tensor([-60.0])
    r = torch.arange(rows)
    visible = r % n + 1
    ref, bound, raw = _softmax_case("B causal softmax", nsplit, x, visible, n, n + pad, n)
    first = raw[:, r % n == 0, 0]                               # one visible key: exactly 1.0, nothing in the lo plane
    assert bool((first[0].float() == 1.0).all()) and (nsplit == 1 or int(_bits(first[1]).abs().max()) == 0)
    # sharpness (CPU): the reference under three wrong masks, on the clean scores (on the poisoned ones a mask too wide reads NaN).  With
    # n = 1 the last two ARE the right mask (min(N, .) = 1 key in every row): only the first one can be told apart there.
    wrong = {"r mod n keys": r % n, "r mod n + 2 keys": (r % n + 2).clamp_max(n), "no modulo": (r + 1).clamp_max(n)}
    for name, vis in wrong.items():
        if n == 1 and name != "r mod n keys":
            assert torch.equal(vis, visible)
            continue
        dist = _row_err(_masked_softmax64(x, vis), ref)
        assert dist >= 10 * bound, (name, dist, bound)


@_modes
@pytest.mark.parametrize("N", [26, 92])
def test_softmax_strided_rows(planes, nsplit, N):
    """ld > N without a mask: the padding between the rows holds 1e30 / NaN."""
    rows = 9
    x = 4.0 * _t(f"B:t:{N}", rows, N)
    _softmax_case("B strided softmax", nsplit, x, torch.full((rows,), N), N, N + 5, 0)


def test_clip_plan_softmax_descriptor_is_the_builders():
    """Builder.softmax(causal_nq=) fills the descriptor clip_plan.py used to emit by hand, byte for byte; causal_nq = 0 is the old call."""
    from frido_amd import _lib
    b = _builder(2)
    s = b.f32_strict(6 * 77, 77)
    for nq in (77, 0):
        p = b.softmax(s, 6 * 77, 77, 77, 96, causal_nq=nq)
        kw = dict(x=s.ptr, rows=6 * 77, N=77, ld=77, Npad=96, nsplit=2, out_op=p.ptr, out_lo=p.lo)
        if nq:
            kw["causal_nq"] = nq
        kind, want = _lib.make_op("FRIDO_OP_SOFTMAX", **kw)
        kind2, have = b.prog.ops[-1]
        assert kind == kind2 and bytes(want) == bytes(have)


# ---- C. the activation switch in every epilogue ----------------------------------------------------------------------------------
def _act64(act, z):
    z = z.double()
    if act == ACT_RELU:
        return z.clamp_min(0.0)
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_GELU:
        return 0.5 * z * (1.0 + torch.erf(z * 0.5 ** 0.5))      # the exact erf form
    if act == ACT_QUICKGELU:
        return z * torch.sigmoid(1.702 * z)
    raise ValueError(act)


EPILOGUES = [   # name, M, N, K, splitk, sk_mode, outputs
    ("slab-vector", 70, 64, 96, 1, 0, ("f32", "op")),       # fast (N % 8 == 0, aligned strides) and not plain (an activation): slab read-back, 8 columns per lane
    ("scalar", 70, 26, 96, 1, 0, ("f32",)),                  # N % 8 != 0 -> !fast: the element-wise path
    ("splitk-reduce8", 200, 64, 256, 4, 0, ("f32", "op")),   # partial: raw slices to the workspace; N, ldo, ldr % 8 == 0 -> splitk_reduce8_kernel
    ("splitk-reduce", 200, 26, 256, 4, 0, ("f32",)),         # the same with N = 26 -> splitk_reduce_kernel
    ("splitk-in-kernel", 200, 64, 256, 4, 1, ("f32", "op")),  # sk_mode 1: the last workgroup adds the slices, then the GEMM's own (slab vector) epilogue
    ("splitk-in-kernel-scalar", 200, 26, 256, 4, 1, ("f32",)),   # ... and its own scalar epilogue
]


@_modes
@pytest.mark.parametrize("act", [ACT_RELU, ACT_GELU, ACT_QUICKGELU], ids=lambda a: ACT_NAMES[a])
@pytest.mark.parametrize("epi,out", [(e, o) for e in EPILOGUES for o in e[6]], ids=lambda v: v if isinstance(v, str) else v[0])
def test_activation_in_every_epilogue(planes, nsplit, epi, out, act):
    """act(0.5 a w^T + bias) + residual against float64 (exact erf, sigmoid(1.702 x)) on unit-scale pre-activations, one shape per
    implementation of the activation switch."""
    from frido_amd import tune
    name, M, N, K, splitk, sk_mode, _ = epi
    a, w, bias, res = _t("C:a", M, K), _t("C:w", N, K) * (2.0 / np.sqrt(K)), _t("C:b", N), _t("C:r", M, N)
    b = _builder(nsplit, {"w.weight": w.cuda(), "w.bias": bias.cuda()})
    ad = a.cuda()
    a_op = b.pack(ad.data_ptr(), 1, M, K, 0, K)
    r = b.f32(M, N)
    r.view().copy_(res.cuda())
    o = b.linear(a_op, "w", act=act, residual=r, alpha=0.5, out="f32_strict" if out == "f32" else "op")
    st = b.prog.ops[-1][1]
    assert st.act == act
    if splitk > 1:
        st.tile, st.splitk, st.sk_mode = 3, splitk, sk_mode
        st.ws = tune.workspace_for(st, _dev())
    _run(b)
    rq = r.to_f32().cpu().double()                            # the residual as stored (bf16 stream with nsplit 1)
    got = o.to_f32().cpu()
    ref = _act64(act, 0.5 * (a.double() @ w.double().t()) + bias.double()) + rq
    _check("C " + name, nsplit, _maxrel(got, ref), _tol(nsplit))
    if nsplit == 2:
        if out == "op":
            got = sum(_pair_planes(o))
        _three("C " + name, nsplit, got, _pass_products(a_op, b.lin_weight("w.weight")),
               lambda y: _act64(act, 0.5 * y + bias.double()) + rq, f"{name} {ACT_NAMES[act]} -> {out}", out=out)


# ---- D. the activation functions element by element ------------------------------------------------------------------------------
GRID = (np.arange(513, dtype=np.float64) - 256.0) / 8.0       # -32 .. 32 in steps of 1/8: exact in bf16, fp16 and f32
_f32 = np.float32


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _gelu_restated32(v):
    """gelu_f of csrc/common.h in float32 numpy: erf by Abramowitz & Stegun 7.1.26 with the kernel's constants and operation order
    (numpy's correctly rounded 1 / x and exp where the kernel has v_rcp_f32 and v_exp_f32)."""
    x = v * _f32(0.70710678118654752)
    ax = np.abs(x)
    t = _f32(1.0) / _fma32(np.full_like(ax, 0.3275911), ax, np.ones_like(ax))
    p = _fma32(np.full_like(t, 1.061405429), t, np.full_like(t, -1.453152027))
    p = _fma32(p, t, np.full_like(t, 1.421413741))
    p = _fma32(p, t, np.full_like(t, -0.284496736))
    p = _fma32(p, t, np.full_like(t, 0.254829592))
    r = _f32(1.0) - p * t * np.exp(-ax * ax)
    return _f32(0.5) * v * (_f32(1.0) + np.copysign(r, x))


def _erf64(x):
    return torch.erf(torch.from_numpy(np.asarray(x, np.float64))).numpy()


def _act_ref64(act, v):
    v = np.asarray(v, np.float64)
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + _erf64(v * np.sqrt(0.5)))
    return v / (1.0 + np.exp(-1.702 * v))


@functools.lru_cache(maxsize=None)
def _e_act(act):
    """E_act: the kernel's own formula restated in float32 on the CPU against float64, max over GRID of |.| / max(|v|, 1/8)."""
    v = GRID.astype(np.float32)
    with np.errstate(over="ignore"):
        if act == ACT_GELU:
            r32 = _gelu_restated32(v)
        elif act == ACT_QUICKGELU:
            r32 = v / (_f32(1.0) + np.exp(_f32(-1.702) * v))
        else:
            r32 = v / (_f32(1.0) + np.exp(-v))
    return float(np.max(np.abs(r32.astype(np.float64) - _act_ref64(act, GRID)) / np.maximum(np.abs(GRID), 0.125)))


def _act_bound(act):
    """Per-element bound of |kernel - float64|: 2 E_act max(|v|, 1/8); the factor 2 covers v_rcp_f32 and v_exp_f32, each one ulp off
    the correctly rounded operations of the restatement."""
    # E_act on this grid: silu 9.25e-8, gelu 1.12e-7, quickgelu 8.85e-8.  Worst |kernel - float64| / bound seen on the MI355X: gelu 0.758,
    # silu 0.591, quickgelu 0.476 -- the same in both builds and for nsplit 2 and 1 (one f32 epilogue serves them all)
    return 2.0 * _e_act(act) * np.maximum(np.abs(GRID), 0.125)


def test_activation_bounds_tell_the_wrong_functions_apart():
    """CPU only.  E_act as measured, and the wrong variants a max-relative GEMM bound cannot see: each lies at least 100 x outside the
    element-wise bound at its worst grid point."""
    e = {ACT_NAMES[a]: _e_act(a) for a in (ACT_SILU, ACT_GELU, ACT_QUICKGELU)}
    print("E_act:", ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert 1.0e-7 < e["gelu"] < 2.5e-7 and 4.0e-8 < e["quickgelu"] < 1.5e-7 and 4.0e-8 < e["silu"] < 1.5e-7, e
    v = GRID
    tanh_gelu = 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))
    variants = {"tanh-form GELU": (ACT_GELU, tanh_gelu, 4.7e-4), "sigmoid(1.7 v)": (ACT_QUICKGELU, v / (1.0 + np.exp(-1.7 * v)), 3.0e-4),
                "GELU for QUICKGELU": (ACT_QUICKGELU, _act_ref64(ACT_GELU, v), 2.0e-2)}
    for name, (act, wrong, away) in variants.items():
        d = np.abs(wrong - _act_ref64(act, v))
        ratio = float(np.max(d / _act_bound(act)))
        print(f"{name}: {d.max():.2e} from exact, {ratio:.0f} x the bound at its worst grid point")
        assert 0.8 * away < d.max() < 1.25 * away and ratio >= 100.0, (name, d.max(), ratio)


@_modes
@pytest.mark.parametrize("act", [ACT_RELU, ACT_SILU, ACT_GELU, ACT_QUICKGELU], ids=lambda a: ACT_NAMES[a])
def test_activation_functions_element_by_element(planes, nsplit, act):
    """A K = 32 GEMM whose pre-activation values are exact in every mode (A[m][0] = v_m, W[n][0] = 1, no bias, alpha = 1): the f32 output
    is act(v_m) as the epilogue computes it.  RELU bit for bit; SILU / GELU / QUICKGELU within 2 E_act max(|v|, 1/8) per element.
    The worst ratio to the bound is printed and reported with the module's margins (measured values: next to _act_bound)."""
    from frido_amd.engine import pack_matrix
    M, N, K = GRID.size, 8, 32
    a, w = torch.zeros(M, K), torch.zeros(N, K)
    a[:, 0], w[:, 0] = torch.from_numpy(GRID).float(), 1.0
    b = _builder(nsplit, {"w.weight": w.cuda()})
    a_op = pack_matrix(a.cuda(), nsplit)
    o = b.linear(a_op, "w", bias=False, act=act, out="f32_strict")
    _run(b)
    got = o.view().cpu()
    assert got.shape == (M, N) and got.dtype == torch.float32
    if act == ACT_RELU:
        want = torch.from_numpy(np.maximum(GRID, 0.0)).float()[:, None].expand(M, N)
        assert torch.equal(_bits(got), _bits(want))
        return
    ref = _act_ref64(act, GRID)
    bound = _act_bound(act)
    ratio = float(np.max(np.abs(got.double().numpy() - ref[:, None]) / bound[:, None]))
    print(f"D {ACT_NAMES[act]} [{planes} x{nsplit}]: E_act {_e_act(act):.3e}, worst |kernel - float64| / bound {ratio:.3f}")
    _check("D " + ACT_NAMES[act] + " (of 2 E_act |v|)", nsplit, ratio, 1.0)


# ---- E. LayerNorm at its edges ---------------------------------------------------------------------------------------------------
LN_WIDTHS = [4, 8, 252, 256, 260, 1020, 1024]      # one float4 per lane: 256 channels per pass of the wave, 1024 at most
LN_OFFSETS = (50.0, 100.0, 200.0)


def _ln_two_pass32(x, w, bi):
    x = x.astype(np.float32)
    mean = np.float32(x.sum(dtype=np.float32) / _f32(x.size))
    d = x - mean
    var = np.float32((d * d).sum(dtype=np.float32) / _f32(x.size))
    return d / np.sqrt(var + _f32(1e-5)) * w + bi


def _ln_one_pass32(x, w, bi):
    x = x.astype(np.float32)
    mean = np.float32(x.sum(dtype=np.float32) / _f32(x.size))
    var = np.float32((x * x).sum(dtype=np.float32) / _f32(x.size)) - mean * mean
    return (x - mean) / np.sqrt(np.maximum(var, _f32(0.0)) + _f32(1e-5)) * w + bi


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, C, bf16_rows):
    """x [rows][C] = 3 * normal + 1; with 5 rows, row 1 has sigma 1 around a large mean and row 2 is constant.  The mean is the first of
    LN_OFFSETS at which -- float32 restatements on the CPU -- a one-pass E[x^2] - mean^2 variance misses both bounds of this test on that
    row and the two-pass form keeps both.  bf16 rows are the f32 rows rounded (the squares of a few bf16 values add up exactly in
    float32, so on narrow bf16 rows no offset tells the two forms apart: the offset is the one the f32 rows settled on)."""
    if bf16_rows:
        x, w, bi, offset = _ln_inputs(rows, C, False)
        return x.to(torch.bfloat16).float(), w, bi, offset
    x = _t(f"E:x:{C}", rows, C) * 3 + 1
    w, bi = 1 + 0.1 * _t(f"E:w:{C}", C), 0.1 * _t(f"E:b:{C}", C)
    offset = None
    if rows >= 3:
        z = _t(f"E:z:{C}", C)
        x[2] = 3.0
        for off in LN_OFFSETS:
            x[1] = z + off
            ref = F.layer_norm(x.double(), (C,), w.double(), bi.double(), 1e-5)
            scale = float(ref.abs().max())
            e2 = float(np.abs(_ln_two_pass32(x[1].numpy(), w.numpy(), bi.numpy()) - ref[1].numpy()).max()) / scale
            e1 = float(np.abs(_ln_one_pass32(x[1].numpy(), w.numpy(), bi.numpy()) - ref[1].numpy()).max()) / scale
            if e2 < 1e-5 and e1 >= 2e-5:
                offset = off
                break
        assert offset is not None, ("no offset separates the one-pass from the two-pass variance", C, e1, e2)
    return x, w, bi, offset


def _layernorm_case(nsplit, rows, C, out, bf16_rows):
    from frido_amd.engine import F32
    x, w, bi, _ = _ln_inputs(rows, C, bf16_rows)
    b = _builder(nsplit, {"n.weight": w.cuda(), "n.bias": bi.cuda()})
    f = F32(b.pool, rows, C, bf16=bf16_rows)
    f.view().copy_(x.cuda())
    a = of = None
    if out == "op":
        a = b.layernorm(f, "n")
        assert b.prog.ops[-1][1].x_bf16 == int(bf16_rows)
    else:                                  # as the plans emit their final norm
        of = b.f32_strict(rows, C)
        kw = {}
        if out == "both":
            a = b.op(rows, C)
            kw = dict(out_op=a.ptr, out_lo=a.lo)
        b.prog.emit("FRIDO_OP_LAYERNORM", x=f.ptr, rows=rows, C=C, eps=1e-5, weight=b.bias("n.weight"), bias=b.bias("n.bias"),
                    nsplit=nsplit, out_f32=of.ptr, x_bf16=int(bf16_rows), **kw)
    _run(b)
    ref = F.layer_norm(x.double(), (C,), w.double(), bi.double(), 1e-5)
    part = "E LayerNorm" + (" bf16 rows" if bf16_rows else "")
    if of is not None:
        y = of.view().cpu()
        _check(part + " out_f32", nsplit, _maxrel(y, ref), 1e-5)                      # the module's "pure-f32 kernels" bound
        if rows >= 3:
            assert torch.equal(_bits(y[2]), _bits(bi)), "a constant row must come out as the bias, bit for bit"
    if a is not None:
        raw = _raw_planes(a)
        _check(part + " operand", nsplit, _maxrel(raw.double().sum(0), ref), _tol(nsplit, f16=2e-5, bf16=2e-5))
        if rows >= 3:
            assert torch.equal(_bits(raw[:, 2]), _bits(_host_split(bi, nsplit))), "a constant row must come out as the split of the bias"
    if out == "both":                      # the operand holds the split of exactly the value out_f32 holds
        assert torch.equal(_bits(raw), _bits(_host_split(y, nsplit)))


@_modes
@pytest.mark.parametrize("out", ["op", "f32", "both"])
@pytest.mark.parametrize("C", LN_WIDTHS)
@pytest.mark.parametrize("rows", [1, 5])
def test_layernorm_edges(planes, nsplit, rows, C, out):
    """f32 rows against float64 F.layer_norm at the lane-boundary widths, with a partly idle last workgroup (4 rows each), for the
    operand output, the out_f32 output of the towers' final norm, and both at once."""
    _layernorm_case(nsplit, rows, C, out, False)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C,out", [(8, "op"), (520, "op"), (1016, "op"), (1024, "op"),      # the 8-channel fast path at its ends
                                   (12, "op"), (8, "f32"), (1024, "f32"), (520, "both")])   # C % 8 != 0 / out_f32: the general path
def test_layernorm_bf16_rows_one_plane(rows, C, out):
    _layernorm_case(1, rows, C, out, True)


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C,out", [(8, "op"), (260, "op"), (1024, "op"), (1020, "f32"), (256, "both")])
def test_layernorm_bf16_rows_two_planes(planes, rows, C, out):
    """nsplit 2 reading a bf16 stream: the general path with x_bf16 = 1."""
    from frido_amd import _lib
    with _lib.use_planes(planes):
        _layernorm_case(2, rows, C, out, True)


def test_layernorm_rejects_widths_it_cannot_run():
    from frido_amd import _lib
    x = torch.ones(4 * 1028, device=_dev())
    wb = torch.ones(1028, device=_dev())
    out = torch.full((4 * 1028,), -12345.678, device=_dev())
    before = out.clone()
    for C in (6, 1028):
        _, st = _lib.make_op("FRIDO_OP_LAYERNORM", x=x.data_ptr(), rows=4, C=C, eps=1e-5, weight=wb.data_ptr(), bias=wb.data_ptr(),
                             nsplit=2, out_f32=out.data_ptr(), x_bf16=0)
        assert _lib.lib().frido_layernorm(C_.addressof(st), torch.cuda.current_stream().cuda_stream) == -1
        assert b"multiple of 4, <= 1024" in _lib.lib().frido_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(before)), "a rejected launch wrote to its output"


# ---- F. the transposed value projection ------------------------------------------------------------------------------------------
@_modes
@pytest.mark.parametrize("Nk", [1, 26, 77])
def test_v_transposed_keeps_its_pad_columns_zero(planes, nsplit, Nk):
    """vT[z] = W x[z]^T + bias[:, None] into a zeroed persistent operand [B][d][Np], run twice: values against float64 and the
    three-pass product, columns Nk .. Np bit-zero in every plane after each run."""
    from frido_amd.engine import pack_matrix
    B, d, K = 2, 96, 64
    Np = _rup(Nk, 32)
    x, w, bias = _t(f"F:x:{Nk}", B, Nk, K), _t("F:w", d, K) / 8.0, _t("F:b", d)
    b = _builder(nsplit)
    x_op, wop = pack_matrix(x.reshape(B * Nk, K).cuda(), nsplit), pack_matrix(w.cuda(), nsplit)
    bd = bias.cuda()
    vT = b.persistent_op(d, Np, batch=B, zero=True)
    assert b.v_transposed(x_op, K, wop, B, Nk, d, bias_ptr=bd.data_ptr(), out=vT) is vT
    ref = torch.einsum("dk,bnk->bdn", w.double(), x.double()) + bias.double()[None, :, None]
    for run in (1, 2):
        _run(b)
        raw = _raw_planes(vT)                                   # [nsplit][B*d][Np]
        _check("F v_transposed", nsplit, _maxrel(raw.double().sum(0)[:, :Nk], ref.reshape(B * d, Nk)), _tol(nsplit))
        assert int(_bits(raw)[:, :, Nk:].abs().max()) == 0, f"pad columns are not bit-zero after run {run}"
    if nsplit == 2:
        (wh, wl), (xh, xl) = _pair_planes(wop), _pair_planes(x_op)
        f = lambda ww, xx: torch.einsum("dk,bnk->bdn", ww, xx.view(B, Nk, K)).reshape(B * d, Nk)      # noqa: E731
        _three("F v_transposed", nsplit, raw.double().sum(0)[:, :Nk], {"hh": f(wh, xh), "hl": f(wh, xl), "lh": f(wl, xh), "K": K},
               lambda y: y + bias.double().repeat(B)[:, None], f"v_transposed Nk {Nk}", out="op")


# ---- G. the chain as the towers run it -------------------------------------------------------------------------------------------
@_modes
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,n,dh", [(2, 4, 16, 32), (1, 12, 77, 64)])
def test_attention_chain_of_the_towers(planes, nsplit, B, H, n, dh, causal):
    """QK^T (batch_inner) -> row softmax (plain: BERT, causal: CLIP) -> PV (batch_inner) over one random q, k, v: every row against
    float64 multi-head attention, to test_attention_core's bounds."""
    from frido_amd.engine import pack_matrix
    inner, Np = H * dh, _rup(n, 32)
    qk, v = _t(f"G:qk:{n}", B * n, 2 * inner), _t(f"G:v:{n}", B, n, inner)
    b = _builder(nsplit)
    qk_op = pack_matrix(qk.cuda(), nsplit)
    vT = pack_matrix(v.transpose(1, 2).reshape(B * inner, n).cuda(), nsplit)
    s = b.f32_strict(B * H * n, n)
    _emit_qkt(b, qk_op, s.ptr, B, H, n, dh)
    pr = b.softmax(s, B * H * n, n, n, Np, causal_nq=n if causal else 0)
    o = b.op(B * n, inner)
    _emit_pv(b, pr, vT, o.ptr, o.lo, inner, B, H, n, dh)
    _run(b)
    q64, k64 = (t.double().reshape(B, n, H, dh).transpose(1, 2) for t in (qk[:, :inner], qk[:, inner:]))      # [B][H][n][dh]
    sc = q64 @ k64.transpose(2, 3) * float(dh) ** -0.5
    if causal:
        sc = sc.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(sc, -1) @ v.double().view(B, n, H, dh).transpose(1, 2)).transpose(1, 2).reshape(B * n, inner)
    _check("G chain" + (" causal" if causal else ""), nsplit, _maxrel(o.to_f32().cpu(), ref), _tol(nsplit, f16=5e-5, bf16=ATTN_BF16_TOL))

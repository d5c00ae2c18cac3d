"""frido_gemm_pair / FridoGemm.flags bit 28 (MI355X): two independent GEMMs in one grid.

The property: a pair launch writes, bit for bit, what the two frido_gemm launches with the same tiles write -- every output buffer
is compared whole with np.array_equal, the pad columns of the V^T-like member's zeroed operand and a 4-KiB guard band in front of and
behind every output included.  Members: A = a q'-like projection (M = 160 ragged against 64- and 128-row tiles, N = 96, operand
planes out); B = a V^T-like per-sample projection (M = 96, N = 40 written with ldoo = 64 into a zeroed operand, batch 3, a_bs = 0,
row_bias).  K = 64 and 160 (an odd k-tile count); member-0 block counts of exactly 8 (no rounding surplus) and 3 (five surplus
workgroups); a batch_inner = 2 member with an f32 output; both member orders; every tile id of either nsplit.  The fallbacks
(different tiles, a conv member, split-K) and the executor (bit 28 in frido_run, under graph capture and replay, a malformed pair)
follow, then the three plans that emit pairs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sys, os  # noqa: E401,E402
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from frido_amd import _lib, engine, holders  # noqa: E402
from frido_amd.synth import seeded_normal, fill_module  # noqa: E402

GUARD_BYTES = 4096
PAIRED = 1 << 28


def _t(tag, *shape):
    return torch.from_numpy(seeded_normal("pair:" + tag, shape))


_IN = {}


def _operand(tag, rows, K, nsplit):
    """(f32 values on the CPU, packed operand on the device), made once per (tag, shape, nsplit, plane format)."""
    key = (tag, rows, K, nsplit, _lib.active_planes())
    if key not in _IN:
        v = _t(tag, rows, K) / np.sqrt(K)
        _IN[key] = (v, engine.pack_matrix(v.cuda(), nsplit))
    return _IN[key]


class Out:
    """An output buffer between two 4-KiB guard bands; the whole allocation is what the tests compare."""

    def __init__(self, elems, esize, zero):
        g = GUARD_BYTES // esize
        dt = {2: torch.int16, 4: torch.int32}[esize]
        self.t = torch.full((g + elems + g,), 0x7b7b if esize == 2 else 0x7b7b7b7b, dtype=dt, device="cuda")
        if zero:
            self.t[g:g + elems] = 0
        self.g, self.elems, self.esize = g, elems, esize
        self.ptr = self.t.data_ptr() + GUARD_BYTES

    def bits(self):
        return self.t.cpu().numpy()

    def planes_f32(self, nsplit, lo, n):
        """hi (+ lo) planes of an operand output as f32 [n]."""
        v = self.t[self.g:self.g + self.elems].view(engine.plane_dtype(nsplit)).float()
        return (v[:n] + (v[lo:lo + n] if nsplit == 2 else 0)).cpu()

    def f32(self):
        return self.t[self.g:self.g + self.elems].view(torch.float32).cpu()


def _desc(**kw):
    return _lib.make_op("FRIDO_OP_GEMM", flags=engine.GEMM_FLAGS, alpha=1.0, **kw)[1]


def _member_q(nsplit, tile, K=64, M=160, N=96, tag="q"):
    """q'-like: out_op[M][N] = a[M][K] w[N][K]^T.  Returns (descriptor, [outputs], float64 reference checker)."""
    (a, a_op), (w, w_op) = _operand(tag + "a", M, K, nsplit), _operand(tag + "w", N, K, nsplit)
    lo = engine.rup(M * N, 8)
    o = Out(nsplit * lo, 2, zero=False)
    d = _desc(M=M, N=N, K=K, batch=1, nsplit=nsplit, A=a_op.ptr, a_lo=a_op.lo, lda=K, B=w_op.ptr, b_lo=w_op.lo, ldb=K,
              out_op=o.ptr, ldoo=N, oo_lo=lo, tile=tile)

    def ref():
        return o.planes_f32(nsplit, lo, M * N).view(M, N), a.double() @ w.double().t()
    return d, [o], ref


def _member_vt(nsplit, tile, K=64, M=96, N=40, batch=3, tag="v"):
    """V^T-like: vT[z][M][64] (columns N .. 63 stay zero) = w[M][K] x[z][N][K]^T + row_bias[M]."""
    ld = 64
    (w, w_op), (x, x_op) = _operand(tag + "w", M, K, nsplit), _operand(tag + "x", batch * N, K, nsplit)
    rb = _t(tag + "rb", M)
    rbd = rb.cuda()
    lo = engine.rup(batch * M * ld, 8)
    o = Out(nsplit * lo, 2, zero=True)
    d = _desc(M=M, N=N, K=K, batch=batch, nsplit=nsplit, A=w_op.ptr, a_lo=w_op.lo, lda=K, a_bs=0, B=x_op.ptr, b_lo=x_op.lo, ldb=K,
              b_bs=N * K, out_op=o.ptr, oo_bs=M * ld, ldoo=ld, oo_lo=lo, row_bias=rbd.data_ptr(), tile=tile)
    d._keep = rbd

    def ref():
        got = o.planes_f32(nsplit, lo, batch * M * ld).view(batch, M, ld)
        want = torch.zeros(batch, M, ld, dtype=torch.float64)
        want[:, :, :N] = torch.einsum("mk,znk->zmn", w.double(), x.double().view(batch, N, K)) + rb.double()[None, :, None]
        return got, want
    return d, [o], ref


def _member_inner(nsplit, tile, K=64, M=40, N=48):
    """batch 4 = 2 outer x 2 inner (batch_inner = 2), f32 output [2][2][M][N]."""
    (a, a_op), (w, w_op) = _operand("ia", 4 * M, K, nsplit), _operand("iw", 4 * N, K, nsplit)
    o = Out(4 * M * N, 4, zero=False)
    d = _desc(M=M, N=N, K=K, batch=4, batch_inner=2, nsplit=nsplit, A=a_op.ptr, a_lo=a_op.lo, lda=K, a_bs=2 * M * K, a_bs2=M * K,
              B=w_op.ptr, b_lo=w_op.lo, ldb=K, b_bs=2 * N * K, b_bs2=N * K, out_f32=o.ptr, ldo=N, of_bs=2 * M * N, of_bs2=M * N, tile=tile)

    def ref():
        return o.f32().view(4, M, N), torch.einsum("zmk,znk->zmn", a.double().view(4, M, K), w.double().view(4, N, K))
    return d, [o], ref


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _single(ds):
    L = _lib.lib()
    for d in ds:
        _lib.check(L.frido_gemm(C.addressof(d), _stream()), "frido_gemm")
    torch.cuda.synchronize()


def _pair(ds):
    _lib.check(_lib.lib().frido_gemm_pair(C.addressof(ds[0]), C.addressof(ds[1]), _stream()), "frido_gemm_pair")
    torch.cuda.synchronize()


def _equal_runs(make, run_a, run_b, what):
    """make() -> two members with fresh outputs; run_a / run_b launch them; every output allocation must agree bit for bit."""
    ma, mb = make(), make()
    run_a([m[0] for m in ma])
    run_b([m[0] for m in mb])
    for i, (x, y) in enumerate(zip(ma, mb)):
        for o1, o2 in zip(x[1], y[1]):
            assert np.array_equal(o1.bits(), o2.bits()), f"{what}: member {i} differs"
    return mb


def _tol(nsplit):       # tests/test_kernels_gpu.py _tol: the bound its every-tile GEMM tests use
    if nsplit != 2:
        return 2e-2
    return 2e-5 if _lib.active_planes() == "f16" else 1e-4


TILES = [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19]


def _skip_rules(nsplit, tile):      # those of tests/test_kernels_gpu.py (every-tile tests)
    if tile == 8 and nsplit == 2 or 11 <= tile <= 17 and nsplit == 2:
        pytest.skip("the 256 x 256 and BK = 64 tiles are bf16-mode tiles")
    if tile in (18, 19) and nsplit == 1:
        pytest.skip("the 8-wave 128 x 192 / 256 x 192 tiles are bf16x3 tiles")


@pytest.mark.parametrize("nsplit", [2, 1])
@pytest.mark.parametrize("tile", TILES)
def test_pair_launch_equals_two_launches_every_tile(nsplit, tile):
    _skip_rules(nsplit, tile)
    rev = lambda ds: _pair(ds[::-1])      # noqa: E731  (member order: b first)
    # q' + V^T, both orders; the float64 product at the every-tile bound
    for K in (64, 160):
        make = lambda: [_member_q(nsplit, tile, K=K), _member_vt(nsplit, tile, K=K)]      # noqa: E731
        got = _equal_runs(make, _single, _pair, f"tile {tile} K {K}")
        _equal_runs(make, _single, rev, f"tile {tile} K {K}, b first")
        for m in got:
            y, want = m[2]()
            e = float((y.double() - want).abs().max() / want.abs().max())
            print(f"pair tile {tile} nsplit {nsplit} K {K}: max-relative error {e:.2e} (bound {_tol(nsplit):.0e})")
            assert e < _tol(nsplit)
    # member 0 of exactly 8 workgroups (nothing to round) and of 3 (five surplus workgroups return at once): one tile per sample
    for nb in (8, 3):
        make = lambda: [_member_vt(nsplit, tile, M=40, N=40, batch=nb, tag=f"s{nb}"), _member_q(nsplit, tile)]      # noqa: E731
        _equal_runs(make, _single, _pair, f"tile {tile}, member 0 of {nb} workgroups")
    # a two-level batch member (f32 output) on either side
    make = lambda: [_member_inner(nsplit, tile), _member_vt(nsplit, tile)]      # noqa: E731
    _equal_runs(make, _single, _pair, f"tile {tile}, batch_inner first")
    _equal_runs(make, _single, rev, f"tile {tile}, batch_inner second")


def _member_conv(nsplit, tile):
    """1x1 conv on a 16 x 10 image of 64 channels: the same product as a dense GEMM, through the conv address path."""
    M, N, K = 160, 96, 64
    (a, a_op), (w, w_op) = _operand("ca", M, K, nsplit), _operand("cw", N, K, nsplit)
    o = Out(M * N, 4, zero=False)
    d = _desc(M=M, N=N, K=K, batch=1, nsplit=nsplit, A=a_op.ptr, a_lo=a_op.lo, lda=K, B=w_op.ptr, b_lo=w_op.lo, ldb=K, conv=1, Hs=16, Ws=10,
              Cin=K, Hl=16, Wl=10, Ho=16, Wo=10, kh=1, kw=1, stride=1, pad=0, padx=0, out_f32=o.ptr, ldo=N, tile=tile)
    return d, [o], None


def _member_splitk(nsplit, tile):
    from frido_amd import tune
    M, N, K = 160, 96, 128
    (a, a_op), (w, w_op) = _operand("ka", M, K, nsplit), _operand("kw", N, K, nsplit)
    o = Out(M * N, 4, zero=False)
    d = _desc(M=M, N=N, K=K, batch=1, nsplit=nsplit, A=a_op.ptr, a_lo=a_op.lo, lda=K, B=w_op.ptr, b_lo=w_op.lo, ldb=K, out_f32=o.ptr, ldo=N,
              tile=tile, splitk=2)
    d.ws = tune.workspace_for(d, torch.device("cuda:0"), ":pairtest")
    return d, [o], None


@pytest.mark.parametrize("case", ["tiles_differ", "conv_member", "splitk_member", "nsplit_differs"])
def test_pair_falls_back_to_two_launches(case):
    """Where the two members cannot share a grid, frido_gemm_pair is the two launches one after the other: same bits."""
    make = {"tiles_differ": lambda: [_member_q(2, 1), _member_vt(2, 3)],
            "conv_member": lambda: [_member_conv(2, 3), _member_vt(2, 3)],
            "splitk_member": lambda: [_member_vt(2, 3), _member_splitk(2, 3)],
            "nsplit_differs": lambda: [_member_q(1, 3), _member_vt(2, 3)]}[case]
    _equal_runs(make, _single, _pair, case)


def test_pair_rejects_an_invalid_member_before_launching():
    """Both descriptors are checked first: a bad SECOND member leaves the first member's output untouched."""
    L = _lib.lib()
    (da, oa, _), (db, ob, _) = _member_q(2, 3), _member_vt(2, 3)
    before = oa[0].bits()
    db.K = 40           # not a multiple of 32
    assert L.frido_gemm_pair(C.addressof(da), C.addressof(db), _stream()) == -1
    assert b"K must be a multiple of 32" in L.frido_last_error()
    assert L.frido_gemm_pair(C.addressof(da), None, _stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(oa[0].bits(), before) and np.array_equal(ob[0].bits(), _member_vt(2, 3)[1][0].bits())


def _prog(ds, flag):
    kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    if flag:
        ds[0].flags |= PAIRED
    return _lib.pack_ops([(kind, d) for d in ds])


@pytest.mark.parametrize("nsplit", [2, 1])
def test_executor_bit_28_runs_the_pair(nsplit):
    L = _lib.lib()
    make = lambda: [_member_q(nsplit, 3), _member_vt(nsplit, 3)]      # noqa: E731

    def run(flag):
        def go(ds):
            arr = _prog(ds, flag)
            _lib.check(L.frido_run(C.addressof(arr), 2, _stream()), "frido_run")
            torch.cuda.synchronize()
        return go

    def replay(ds):           # captured once, replayed twice
        arr = _prog(ds, True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = C.c_void_p()
        _lib.check(L.frido_graph_capture(C.addressof(arr), 2, s.cuda_stream, C.byref(g)), "frido_graph_capture")
        for _ in range(2):
            _lib.check(L.frido_graph_launch(g, s.cuda_stream), "frido_graph_launch")
        s.synchronize()
        L.frido_graph_destroy(g)

    def timed(ds):            # the pair's time on the head op, 0 on its partner
        arr = _prog(ds, True)
        ms = (C.c_float * 2)()
        _lib.check(L.frido_run_timed(C.addressof(arr), 2, _stream(), ms), "frido_run_timed")
        assert ms[0] > 0 and 0 <= ms[1] < ms[0], list(ms)

    _equal_runs(make, run(False), run(True), "frido_run, bit 28")
    _equal_runs(make, run(False), replay, "graph replay, bit 28")
    _equal_runs(make, run(False), timed, "frido_run_timed, bit 28")


def test_executor_rejects_a_malformed_pair_and_launches_nothing():
    L = _lib.lib()
    kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    (da, oa, _), (db, ob, _) = _member_q(2, 3), _member_vt(2, 3)
    before = [oa[0].bits(), ob[0].bits()]
    db.flags |= PAIRED
    progs = [[(kind, da), (kind, db), _lib.make_op("FRIDO_OP_COPY")],      # op 1 is flagged, op 2 is no GEMM
             [(kind, da), (kind, db)]]                                       # op 1 is flagged and the last op
    ms = (C.c_float * 3)()
    for ops in progs:
        arr = _lib.pack_ops(ops)
        assert L.frido_run(C.addressof(arr), len(ops), _stream()) == -1
        assert b"op 1 " in L.frido_last_error() and b"bit 28" in L.frido_last_error()
        assert L.frido_run_timed(C.addressof(arr), len(ops), _stream(), ms) == -1
    side = _lib.pack_ops([(kind, db), (kind, da)])
    side[1].stream = 1                                                       # the partner sits on the other stream
    assert L.frido_run(C.addressof(side), 2, _stream()) == -1 and b"op 0 " in L.frido_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(oa[0].bits(), before[0]) and np.array_equal(ob[0].bits(), before[1])


# ---- plan level: the pairs the plans emit ---------------------------------------------------------------------------------------

def _both_ways(monkeypatch, build_and_run):
    """build_and_run() once with builder.GEMM_PAIR on and once off -> ((output, flagged ops), (output, flagged ops))."""
    from frido_amd import builder
    res = []
    for on in (True, False):
        monkeypatch.setattr(builder, "GEMM_PAIR", on)
        progs = []
        init = engine.Prog.__init__

        def rec(self, *a, _init=init, _progs=progs, **k):
            _init(self, *a, **k)
            _progs.append(self)
        monkeypatch.setattr(engine.Prog, "__init__", rec)
        out = build_and_run()
        torch.cuda.synchronize()
        monkeypatch.setattr(engine.Prog, "__init__", init)
        kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
        flagged = sum(1 for p in progs for k, st in p.ops if k == kind and st.flags & PAIRED)
        res.append((out.clone(), flagged))
    return res


def test_unet_plan_pairs_every_transformer_block(monkeypatch):
    from golden_cfg import UNET_SMALL
    from frido_amd.models import PyUNetModel
    x, ctx, t = _t("ux", 2, 6, 16, 16).cuda(), _t("uc", 2, 5, 64).cuda(), torch.tensor([11, 311]).cuda()
    blocks = []

    def go():
        m = fill_module(PyUNetModel(**UNET_SMALL), "model.diffusion_model.").cuda().eval()
        blocks.append(sum(isinstance(x_, holders.TBlockP) for x_ in m.modules()))
        return m(x, t, context=ctx, stage=1)
    (y1, n1), (y0, n0) = _both_ways(monkeypatch, go)
    assert torch.equal(y1, y0)
    assert blocks[0] > 0 and n1 == blocks[0] and n0 == 0


def test_vqgan_plan_pairs_every_attention_block(monkeypatch):
    from golden_cfg import VQ_SMALL
    from helpers import golden
    from frido_amd.models import VQModelInterface
    h = torch.from_numpy(golden("vq_small")["h"])[:2].cuda()
    blocks = []

    def go():
        m = fill_module(VQModelInterface(**VQ_SMALL, lossconfig=dict(target="taming.modules.losses.DummyLoss")), "first_stage_model.").cuda().eval()
        # (the decode path runs `decoder`; the shared decoder that fuses the scales belongs to the encode path)
        blocks.append(sum(isinstance(x_, holders.VAttnP) and n.startswith("decoder.") for n, x_ in m.named_modules()))
        return m.decode(h)
    (y1, n1), (y0, n0) = _both_ways(monkeypatch, go)
    assert torch.equal(y1, y0)
    assert blocks[0] > 0 and n1 == blocks[0] and n0 == 0


def test_bert_plan_pairs_every_layer(monkeypatch):
    from golden_cfg import BERT_SMALL
    from helpers import golden
    from frido.modules.encoders.modules import BERTEmbedder
    tokens = torch.from_numpy(golden("sampler_small")["tokens"]).cuda()

    def go():
        return fill_module(BERTEmbedder(**BERT_SMALL), "cond_stage_model.").cuda().encode(tokens)
    (y1, n1), (y0, n0) = _both_ways(monkeypatch, go)
    assert torch.equal(y1, y0)
    assert n1 == BERT_SMALL["n_layer"] and n0 == 0

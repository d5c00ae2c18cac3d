"""The cross tail of the d-split flash kernel (csrc/flash.hip, FridoAttnSmall.K2 ...) through the C ABI, against float64:

    h2 = softmax(alpha Q K^T) V + bias + residual
    n2 = LayerNorm(h2; ln_w, ln_b, ln_eps)
    h3 = softmax(alpha2 n2 K2^T) V2 + bias2 + h2
    out2_op <- h3 (hi / lo planes)    out2_act <- h3 (f32)    ln2_op <- LayerNorm(h3; ln2_w, ln2_b, ln2_eps)

and against the launches it replaces on the same inputs: frido_attn_flash (h2, n2), frido_attn_small (h3 and its operand copy) and, for
n3, frido_layernorm -- at these sizes the short-key kernel has fewer than 256 workgroups and does not normalise its own rows.

Shapes: the smallest at which the kernel can go wrong.  B = 2; Nq 128 / 80 = two query blocks of 64, the second one ragged at 80; Nk 64 / 70 =
two key tiles, a third ragged one at 70; Nk2 26 (the benchmark's context), 1 and 32 (the bounds); d 256 / 384, the head widths that carry
the tail.  Bound: 2e-5 max-relative for the operand copy of h3 and for n3, the bound of the fused LayerNorm copies in test_kernels_gpu.py;
the fused launch may not be more than twice as far from float64 as the launches it replaces (same arithmetic: more is a bug, not rounding).
Both paths' errors are printed as one table at the end of the module (pytest -s; committed as profiles/attn_chain_error.txt)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from frido_amd.synth import seeded_normal

pytestmark = pytest.mark.gpu

BOUND = 2e-5
CASES = [(d, Nq, Nk, Nk2) for d in (256, 384) for Nq in (128, 80) for Nk in (64, 70) for Nk2 in (26, 1, 32)]
B = 2
_ROWS = {}      # case -> (fused errors, two-launch errors)


def _t(tag, *shape):
    return torch.from_numpy(seeded_normal(tag, shape))


def _relerr(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _status(clear=True):
    from frido_amd import _lib
    w = C.c_uint32(0)
    assert _lib.lib().frido_status_flags(C.byref(w), int(clear)) == 0
    return int(w.value)


class _Case:
    """Inputs of one case on the device, and the float64 statement of the six lines."""

    def __init__(self, d, Nq, Nk, Nk2, res_shift=0.3):
        from frido_amd.engine import pack_matrix
        self.d, self.Nq, self.Nk, self.Nk2 = d, Nq, Nk, Nk2
        tag = f"chain{d}_{Nq}_{Nk}_{Nk2}:"
        q, k, v = _t(tag + "q", B, Nq, d), _t(tag + "k", B, Nk, d) * 1.5, _t(tag + "v", B, Nk, d)
        k2, v2 = _t(tag + "k2", B, Nk2, d) * 1.5, _t(tag + "v2", B, Nk2, d)
        bias, bias2, res = _t(tag + "b", d), 0.5 * _t(tag + "b2", d), _t(tag + "r", B * Nq, d) + res_shift
        self.lw, self.lb = 1 + 0.2 * _t(tag + "lw", d), 0.1 * _t(tag + "lb", d)
        self.lw2, self.lb2 = 1 - 0.3 * _t(tag + "lw2", d), 0.2 * _t(tag + "lb2", d)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.dev = dev
        self.qo = pack_matrix(q.reshape(B * Nq, d).to(dev), 2)
        self.ko = pack_matrix(k.reshape(B * Nk, d).to(dev), 2)
        self.vto = pack_matrix(v.transpose(1, 2).reshape(B * d, Nk).to(dev), 2)           # [B*d][Nk padded to 32], pad = 0
        self.k2o = pack_matrix(k2.reshape(B * Nk2, d).to(dev), 2)
        self.vt2o = pack_matrix(v2.transpose(1, 2).reshape(B * d, Nk2).to(dev), 2)
        assert self.vt2o.K == 32
        self.g = {n: t.float().to(dev).contiguous() for n, t in dict(bias=bias, bias2=bias2, res=res, lw=self.lw, lb=self.lb, lw2=self.lw2, lb2=self.lb2).items()}
        # float64, from the operand values as the kernels read them (hi + lo planes: 2^-22 from the seeded inputs)
        q64 = self.qo.to_f32().double().cpu().view(B, Nq, d)
        k64 = self.ko.to_f32().double().cpu().view(B, Nk, d)
        v64 = self.vto.to_f32().double().cpu().view(B, d, -1)[:, :, :Nk].transpose(1, 2)
        k264 = self.k2o.to_f32().double().cpu().view(B, Nk2, d)
        v264 = self.vt2o.to_f32().double().cpu().view(B, d, 32)[:, :, :Nk2].transpose(1, 2)
        a = d ** -0.5
        self.h2 = (torch.softmax(q64 @ k64.transpose(1, 2) * a, -1) @ v64).reshape(B * Nq, d) + bias.double() + res.double()
        self.n2 = F.layer_norm(self.h2, (d,), self.lw.double(), self.lb.double(), 1e-5)
        self.h3 = (torch.softmax(self.n2.view(B, Nq, d) @ k264.transpose(1, 2) * a, -1) @ v264).reshape(B * Nq, d) + bias2.double() + self.h2
        self.n3 = F.layer_norm(self.h3, (d,), self.lw2.double(), self.lb2.double(), 1e-6)

    def flash_kw(self):
        d, Nq, Nk = self.d, self.Nq, self.Nk
        return dict(Q=self.qo.ptr, q_lo=self.qo.lo, ldq=d, K=self.ko.ptr, k_lo=self.ko.lo, k_bs=Nk * d, ldk=d, VT=self.vto.ptr, vt_lo=self.vto.lo,
                    vt_bs=d * self.vto.K, ldvt=self.vto.K, B=B, Nq=Nq, Nk=Nk, d=d, dv=d, nsplit=2, alpha=d ** -0.5,
                    residual=self.g["res"].data_ptr(), ldr=d, bias=self.g["bias"].data_ptr(),
                    ln_w=self.g["lw"].data_ptr(), ln_b=self.g["lb"].data_ptr(), ln_eps=1e-5)

    def tail_kw(self):
        d, Nk2 = self.d, self.Nk2
        return dict(K2=self.k2o.ptr, k2_lo=self.k2o.lo, k2_bs=Nk2 * d, ldk2=d, VT2=self.vt2o.ptr, vt2_lo=self.vt2o.lo, vt2_bs=d * 32, ldvt2=32,
                    Nk2=Nk2, alpha2=d ** -0.5, bias2=self.g["bias2"].data_ptr(), ln2_w=self.g["lw2"].data_ptr(), ln2_b=self.g["lb2"].data_ptr(),
                    ln2_eps=1e-6)

    def op(self):
        from frido_amd.engine import Operand
        return Operand(B * self.Nq, self.d, 2, self.dev, zero=True)

    def f32(self):
        return torch.zeros(B * self.Nq, self.d, dtype=torch.float32, device=self.dev)

    def fused(self, everything):
        """One launch.  everything = False: the plan's form (h3 as an operand and n3 only); True: h2, n2 and the f32 rows of h3 as well."""
        from frido_amd import _lib
        d = self.d
        out = dict(h3op=self.op(), n3=self.op())
        kw = dict(self.flash_kw(), **self.tail_kw(), out2_op=out["h3op"].ptr, out2_lo=out["h3op"].lo, ldo2=d, ln2_op=out["n3"].ptr, ln2_lo=out["n3"].lo,
                  ld_ln2=d)
        if everything:
            out.update(h2=self.f32(), n2=self.op(), h3=self.f32())
            kw.update(out_act=out["h2"].data_ptr(), ld_act=d, ln_op=out["n2"].ptr, ln_lo=out["n2"].lo, ld_ln=d, out2_act=out["h3"].data_ptr(), ld_act2=d)
        _, st = _lib.make_op("FRIDO_OP_ATTN_FLASH", **kw)
        rc = _lib.lib().frido_attn_flash(C.addressof(st), _stream())
        assert rc == 0, _lib.lib().frido_last_error()
        torch.cuda.synchronize()
        return out

    def two_launches(self):
        from frido_amd import _lib
        L, d, Nq, Nk2 = _lib.lib(), self.d, self.Nq, self.Nk2
        out = dict(h2=self.f32(), n2=self.op(), h3=self.f32(), h3op=self.op(), n3=self.op())
        _, st = _lib.make_op("FRIDO_OP_ATTN_FLASH", **dict(self.flash_kw(), out_act=out["h2"].data_ptr(), ld_act=d, ln_op=out["n2"].ptr,
                                                           ln_lo=out["n2"].lo, ld_ln=d))
        assert L.frido_attn_flash(C.addressof(st), _stream()) == 0, L.frido_last_error()
        _, st = _lib.make_op("FRIDO_OP_ATTN_SMALL", Q=out["n2"].ptr, q_lo=out["n2"].lo, ldq=d, K=self.k2o.ptr, k_lo=self.k2o.lo, k_bs=Nk2 * d, ldk=d,
                             VT=self.vt2o.ptr, vt_lo=self.vt2o.lo, vt_bs=d * 32, ldvt=32, B=B, Nq=Nq, Nk=Nk2, d=d, dv=d, nsplit=2, alpha=d ** -0.5,
                             out_act=out["h3"].data_ptr(), ld_act=d, residual=out["h2"].data_ptr(), ldr=d, bias=self.g["bias2"].data_ptr(),
                             out_op=out["h3op"].ptr, out_lo=out["h3op"].lo, ldo=d)
        assert L.frido_attn_small(C.addressof(st), _stream()) == 0, L.frido_last_error()
        _, st = _lib.make_op("FRIDO_OP_LAYERNORM", x=out["h3"].data_ptr(), rows=B * Nq, C=d, eps=1e-6, weight=self.g["lw2"].data_ptr(),
                             bias=self.g["lb2"].data_ptr(), nsplit=2, out_op=out["n3"].ptr, out_lo=out["n3"].lo)
        assert L.frido_layernorm(C.addressof(st), _stream()) == 0, L.frido_last_error()
        torch.cuda.synchronize()
        return out


@functools.lru_cache(maxsize=None)
def _results(case):
    """Every launch of one case, run once: (inputs + float64, fused plan form, the same again, fused with every output, two launches, status)."""
    _status(clear=True)
    c = _Case(*case)
    a1, a2, full, two = c.fused(False), c.fused(False), c.fused(True), c.two_launches()
    return c, a1, a2, full, two, _status(clear=True)


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    if len(_ROWS) != len(CASES):
        return
    rows = ["Max-relative error against float64 (max |got - ref| / max |ref|) of h3 as an operand (hi + lo) and of n3 = LayerNorm(h3):",
            "the flash launch with the cross tail against frido_attn_flash -> frido_attn_small -> frido_layernorm on the same inputs",
            f"(tests/test_attn_chain_gpu.py, B = {B}; bound {BOUND:g}, fused <= 2 x two-launch).", "",
            "   d   Nq   Nk  Nk2   fused h3   fused n3   2-launch h3   2-launch n3"]
    for (d, Nq, Nk, Nk2), (fu, tw) in sorted(_ROWS.items()):
        rows.append(f"{d:4d} {Nq:4d} {Nk:4d} {Nk2:4d}   {fu[0]:.2e}   {fu[1]:.2e}      {tw[0]:.2e}      {tw[1]:.2e}")
    rows += ["", f"worst: fused {max(max(fu) for fu, _ in _ROWS.values()):.2e}, two launches {max(max(tw) for _, tw in _ROWS.values()):.2e}"]
    print("\n" + "\n".join(rows))


@pytest.mark.parametrize("case", CASES, ids=["d%d-Nq%d-Nk%d-Nk2_%d" % c for c in CASES])
def test_fused_launch_against_float64_and_the_two_launches(case):
    c, a1, _, full, two, _ = _results(case)
    fu = (_relerr(a1["h3op"].to_f32(), c.h3), _relerr(a1["n3"].to_f32(), c.n3))
    tw = (_relerr(two["h3op"].to_f32(), c.h3), _relerr(two["n3"].to_f32(), c.n3))
    _ROWS[case] = (fu, tw)
    print(f"{case}: fused h3 {fu[0]:.2e} n3 {fu[1]:.2e}; two launches h3 {tw[0]:.2e} n3 {tw[1]:.2e}")
    assert fu[0] <= BOUND and fu[1] <= BOUND, (fu, tw)
    assert fu[0] <= 2 * tw[0] and fu[1] <= 2 * tw[1], (fu, tw)
    # the f32 rows of h3 are the values the operand copy splits
    assert _relerr(full["h3"], c.h3) <= BOUND
    assert _relerr(full["h3op"].to_f32(), full["h3"].double().cpu()) < 1e-5


@pytest.mark.parametrize("case", CASES, ids=["d%d-Nq%d-Nk%d-Nk2_%d" % c for c in CASES])
def test_fused_launch_is_repeatable_and_its_optional_outputs_do_not_change_it(case):
    _, a1, a2, full, _, _ = _results(case)
    for n in ("h3op", "n3"):
        assert torch.equal(a1[n].t, a2[n].t), n            # two runs: identical bits
        assert torch.equal(a1[n].t, full[n].t), n          # storing h2 / n2 / the f32 rows as well changes nothing


@pytest.mark.parametrize("case", CASES, ids=["d%d-Nq%d-Nk%d-Nk2_%d" % c for c in CASES])
def test_stored_h2_and_n2_equal_the_two_launch_path(case):
    c, _, _, full, two, _ = _results(case)
    assert _relerr(full["h2"], c.h2) <= BOUND and _relerr(full["n2"].to_f32(), c.n2) <= BOUND
    assert _relerr(full["h2"], two["h2"].double().cpu()) <= BOUND
    assert _relerr(full["n2"].to_f32(), two["n2"].to_f32().double().cpu()) <= BOUND


@pytest.mark.parametrize("case", CASES, ids=["d%d-Nq%d-Nk%d-Nk2_%d" % c for c in CASES])
def test_status_word_stays_clear(case):
    assert _results(case)[5] == 0


def test_status_word_is_raised_by_a_saturating_plane():
    """A residual beyond fp16's range: h3 = ... + h2 does not fit the hi plane of out2_op, the launch says so (FRIDO_STATUS_SATURATED)."""
    from frido_amd import _lib
    assert _lib.lib().frido_x3_plane_format() == 1      # the default build: fp16 hi + lo planes
    _status(clear=True)
    c = _Case(256, 80, 64, 26, res_shift=1.0e5)
    out = c.fused(False)
    assert _status(clear=True) & _lib.STATUS_SATURATED
    assert float(out["h3op"].to_f32().abs().max()) <= 65504.0 + 32.0      # clamped, not inf / NaN

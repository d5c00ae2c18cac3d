"""CPU-side checks of the flash kernel's cross tail (FridoAttnSmall.K2 ...; csrc/flash.hip): the descriptor grew at its end only and the ABI
facts around it hold, every rejection of the launchers fires by name before a device is touched, and the benchmark model's plan uses the
tail exactly where it should: five launches fewer per forward of each stage, and no short-key launch behind a tailed flash launch."""
import ctypes as C
import re

import pytest
import torch

from frido_amd import _lib

# the descriptor as it was before the tail, in order: the tail may only follow it
BEFORE = ["Q", "q_lo", "ldq", "K", "k_lo", "k_bs", "ldk", "VT", "vt_lo", "vt_bs", "ldvt", "out_op", "out_lo", "ldo", "B", "Nq", "Nk", "d", "dv",
          "nsplit", "alpha", "out_act", "residual", "bias", "ld_act", "ldr", "act_bf16", "ln_op", "ln_lo", "ld_ln", "ln_w", "ln_b", "ln_eps",
          "skip_act_store"]
TAIL = ["K2", "k2_lo", "k2_bs", "ldk2", "VT2", "vt2_lo", "vt2_bs", "ldvt2", "Nk2", "alpha2", "bias2", "ln2_w", "ln2_b", "ln2_eps", "ln2_op",
        "ln2_lo", "ld_ln2", "out2_op", "out2_lo", "ldo2", "out2_act", "ld_act2"]


def test_descriptor_grew_at_its_end_only_and_the_abi_facts_hold():
    st = _lib.STRUCTS["FridoAttnSmall"]
    names = [n for n, _ in st._fields_]
    assert names == BEFORE + TAIL
    assert st.skip_act_store.offset == 220 and st.K2.offset == 224      # everything up to skip_act_store is where it was
    assert C.sizeof(st) <= 512 and C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512
    assert _lib.ABI_VERSION == 8
    assert len(_lib.OP_KINDS) == 36 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert len(_lib.EXPORTS) == 61
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_ATTN_FLASH"]) == L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_ATTN_SMALL"]) == C.sizeof(st)


def test_no_new_environment_switch_or_build_variant():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    mk = open(os.path.join(root, "frido_amd", "csrc", "Makefile")).read()
    assert set(re.findall(r"-D(\w+)", mk)) == {"FRIDO_X3_F16", "CG_PROF", "IG_PROF"}      # the plane format, and two macros named in a comment
    for f in ("builder.py", "unet_plan.py"):
        assert "ATTN_CHAIN" not in "".join(re.findall(r"os\.environ[^\n]*", open(os.path.join(root, "frido_amd", f)).read()))


def _good(**over):
    """A well-formed tailed descriptor (pointers are fake but aligned: nothing here reaches a device)."""
    d = 384
    kw = dict(Q=4096, q_lo=1 << 20, ldq=d, K=8192, k_lo=1 << 20, k_bs=1024 * d, ldk=d, VT=12288, vt_lo=1 << 20, vt_bs=d * 1024, ldvt=1024,
              B=2, Nq=1024, Nk=1024, d=d, dv=d, nsplit=2, alpha=d ** -0.5, residual=16384, ldr=d, bias=20480, ln_w=24576, ln_b=28672, ln_eps=1e-5,
              K2=32768, k2_lo=1 << 16, k2_bs=26 * d, ldk2=d, VT2=36864, vt2_lo=1 << 16, vt2_bs=d * 32, ldvt2=32, Nk2=26, alpha2=d ** -0.5,
              bias2=40960, ln2_w=45056, ln2_b=49152, ln2_eps=1e-5, ln2_op=53248, ln2_lo=1 << 20, ld_ln2=d, out2_op=57344, out2_lo=1 << 20, ldo2=d)
    kw.update(over)
    return kw


def _reject(fn, kw):
    L = _lib.lib()
    _, st = _lib.make_op("FRIDO_OP_ATTN_FLASH", **kw)
    assert getattr(L, fn)(C.addressof(st), None) == -1, (fn, kw)
    return L.frido_last_error().decode()


BAD = [
    ("two-plane mode", dict(nsplit=1)),
    ("two-plane mode", dict(d=512, dv=512)),                     # a d-split width, but its kernel has no registers left for the tail
    ("two-plane mode", dict(d=128, dv=128)),                     # the 4-wave form
    ("two-plane mode", dict(d=576, dv=576)),                     # the 4-wave form, rows split over two workgroups
    ("stream form with a residual", dict(residual=0)),
    ("stream form with a residual", dict(out_op=4096, ldo=384)),
    ("stream form with a residual", dict(act_bf16=1)),
    ("LayerNorm weight and bias", dict(ln_w=0)),
    ("LayerNorm weight and bias", dict(ln_b=0)),
    ("LayerNorm weight and bias", dict(ln2_w=0)),
    ("LayerNorm weight and bias", dict(ln2_b=0)),
    ("1 <= Nk2 <= 32", dict(Nk2=0)),
    ("1 <= Nk2 <= 32", dict(Nk2=33, ldvt2=64)),
    ("1 <= Nk2 <= 32", dict(VT2=0)),
    ("zero-padded to 32", dict(ldvt2=24)),
    ("16-byte alignment", dict(ldk2=380)),
    ("16-byte alignment", dict(k2_lo=4)),
    ("16-byte alignment", dict(k2_bs=26 * 384 + 4)),
    ("16-byte alignment", dict(ldvt2=36)),
    ("16-byte alignment", dict(vt2_lo=4)),
    ("16-byte alignment", dict(K2=32768 + 8)),
    ("16-byte alignment", dict(VT2=36864 + 8)),
    ("16-byte alignment", dict(bias2=40960 + 4)),
    ("16-byte alignment", dict(ldo2=382)),
    ("16-byte alignment", dict(ld_ln2=382)),
    ("16-byte alignment", dict(out2_act=61440 + 4, ld_act2=384)),
    ("at least one of out2_op, out2_act, ln2_op", dict(out2_op=0, ln2_op=0)),
]


@pytest.mark.parametrize("what,over", BAD, ids=["%s-%s" % (w.split()[0], "-".join(o)) for w, o in BAD])
def test_flash_launcher_rejects_a_bad_tail_by_name(what, over):
    err = _reject("frido_attn_flash", _good(**over))
    assert err.startswith("frido_attn_flash: cross tail: ") and what in err, err


def test_tail_fields_without_k2_and_tails_on_the_short_key_launcher_are_rejected():
    err = _reject("frido_attn_flash", _good(K2=0, out_act=4096, ld_act=384))
    assert "cross tail: fields set without K2" in err
    L = _lib.lib()
    _, st = _lib.make_op("FRIDO_OP_ATTN_SMALL", **_good(Nk=26, ldvt=32, out_act=4096, ld_act=384))
    assert L.frido_attn_small(C.addressof(st), None) == -1
    assert b"frido_attn_small: cross tail (K2 ...) is served by frido_attn_flash only" in L.frido_last_error()
    # an all-zero descriptor: the null-pointer message of before
    assert L.frido_attn_flash(C.byref(_lib.STRUCTS["FridoAttnSmall"]()), None) == -1 and b"null pointer" in L.frido_last_error()


def test_out_act_and_ln_op_become_optional_with_a_tail_only():
    """Without a tail a launch needs out_op or out_act; with one, a descriptor that stores neither h2 nor n2 passes the pointer and tail
    checks: it is turned away only by the check that follows them (an empty problem here, so that nothing is launched)."""
    err = _reject("frido_attn_flash", _good(K2=0, VT2=0, Nk2=0, bias2=0, ln2_w=0, ln2_b=0, ln2_op=0, out2_op=0))
    assert "null pointer" in err
    err = _reject("frido_attn_flash", _good(Nq=0))
    assert "empty problem" in err and "cross tail" not in err


def _step_ops(chain, monkeypatch):
    """Op kinds of the step programs of the benchmark denoiser (f8f4, B = 16, 26 context tokens, two-plane mode), planned on the CPU."""
    from golden_cfg import UNET_FULL
    from frido_amd import builder
    from frido_amd.models import PyUNetModel
    from frido_amd.unet_plan import UNetStagePlan
    monkeypatch.setattr(builder, "ATTN_CHAIN", chain)
    w = _WEIGHTS.setdefault("w", {k: v.detach().float() for k, v in PyUNetModel(**UNET_FULL).state_dict().items()})
    out = []
    for stage in range(UNET_FULL["num_stage"]):
        b = builder.Builder("cpu", 2, w)
        x = torch.zeros(16, 64 * 64, UNET_FULL["in_channels"])
        plan = UNetStagePlan(b, UNET_FULL, B=16, H=64, W=64, nctx=26, stage=stage, x_state=x, temb_rows=16, per_sample_t=True)
        out.append(list(plan.step.ops))
    return out


_WEIGHTS = {}


def test_benchmark_plan_uses_the_tail_on_the_32x32_plane_only(monkeypatch):
    flash, small = _lib.OP_KINDS["FRIDO_OP_ATTN_FLASH"], _lib.OP_KINDS["FRIDO_OP_ATTN_SMALL"]
    on, off = _step_ops(True, monkeypatch), _step_ops(False, monkeypatch)
    assert len(on) == len(off) == 2
    for ops_on, ops_off in zip(on, off):
        assert len(ops_off) - len(ops_on) == 5
        tailed = [i for i, (k, st) in enumerate(ops_on) if k == flash and st.K2]
        assert len(tailed) == 5 and all(ops_on[i][1].d == 384 and ops_on[i][1].Nq == 1024 and ops_on[i][1].Nk2 == 26 for i in tailed)
        for i in tailed:
            st = ops_on[i][1]
            assert ops_on[i + 1][0] != small                                     # the cross-attention is inside the launch
            assert not st.out_act and not st.ln_op and not st.out2_act          # h2, n2 and the f32 rows of h3 never leave the kernel
            assert st.out2_op and st.ln2_op
        assert not any(k == flash and st.K2 for k, st in ops_off)
        # the other planes keep their launches
        assert sum(k == small for k, _ in ops_off) - sum(k == small for k, _ in ops_on) == 5
        assert sum(k == flash for k, _ in ops_off) == sum(k == flash for k, _ in ops_on) == 5


def test_the_tail_is_not_planned_for_long_contexts_or_one_plane_mode(monkeypatch):
    from frido_amd import builder
    b2, b1 = builder.Builder("cpu", 2, {}), builder.Builder("cpu", 1, {})
    assert b2.attention_chain_ok(384, 384, 1024, 384, 26, 384) and b2.attention_chain_ok(256, 256, 4096, 256, 32, 256)
    assert not b2.attention_chain_ok(384, 384, 1024, 384, 92, 384)         # 92 context tokens: the short-key launch
    assert not b2.attention_chain_ok(576, 576, 256, 576, 26, 576)          # the 16 x 16 plane: no row-owning flash launch
    assert not b2.attention_chain_ok(512, 512, 4096, 512, 26, 512)         # d = 512: no registers for the tail
    assert not b1.attention_chain_ok(384, 384, 1024, 384, 26, 384)         # bf16 mode
    monkeypatch.setattr(builder, "ATTN_CHAIN", False)
    assert not b2.attention_chain_ok(384, 384, 1024, 384, 26, 384)

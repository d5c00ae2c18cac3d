"""CPU-side checks of ABI 8: the nine launchers that had descriptors but no op kind (unfold, fold, q_sample, diffusion loss, codebook loss,
DPM step, keep blend, inversion step, guidance compose) are op kinds 27 .. 35 of the one executor -- appended, nothing renumbered -- and
the second program system that served them (patching.PatchProg, patching.FOREIGN, the FRIDO_DESC_* size codes) is gone."""
import ctypes as C

import pytest

from frido_amd import _lib, patching

NEW = [("FRIDO_OP_UNFOLD", "FridoUnfold"), ("FRIDO_OP_FOLD", "FridoFold"), ("FRIDO_OP_QSAMPLE", "FridoQSample"),
       ("FRIDO_OP_DIFFUSION_LOSS", "FridoDiffusionLoss"), ("FRIDO_OP_VQ_COMMIT_LOSS", "FridoVqCommitLoss"), ("FRIDO_OP_DPM_STEP", "FridoDpmStep"),
       ("FRIDO_OP_KEEP_BLEND", "FridoKeepBlend"), ("FRIDO_OP_INVERT_STEP", "FridoInvertStep"), ("FRIDO_OP_GUIDANCE_COMPOSE", "FridoGuidanceCompose")]
OLD = ["GEMM", "GN_STATS", "GN_APPLY", "LAYERNORM", "SOFTMAX", "GEGLU", "PACK", "RELAYOUT", "VQ", "SAMPLER_STEP", "HANDOFF", "RANDN", "STEP_ADD",
       "FILL", "TIME_EMB", "CONVT", "PLACE", "EMBED", "TO_U8", "ATTN_SMALL", "GN_FUSED", "COPY", "ATTN_FLASH", "SYNC", "L2NORM", "ATTN_MH"]


def _launcher(kind):
    return "frido_" + kind[len("FRIDO_OP_"):].lower()


def test_nine_kinds_are_appended_and_nothing_is_renumbered():
    assert _lib.ABI_VERSION == 8
    assert [_lib.OP_KINDS["FRIDO_OP_" + k] for k in OLD] == list(range(1, 27))
    assert [_lib.OP_KINDS[k] for k, _ in NEW] == list(range(27, 36)) and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert len(_lib.OP_KINDS) == 36 and set(_lib.KIND_STRUCT) == set(_lib.OP_KINDS) - {"FRIDO_OP__COUNT"}
    assert [_lib.KIND_STRUCT[k] for k, _ in NEW] == [s for _, s in NEW]
    assert C.sizeof(_lib.FridoOp) == 520
    for k, _ in NEW:
        assert _launcher(k) in _lib.declared_symbols() and _launcher(k) in _lib.EXPORTS, k


def test_the_second_program_system_is_gone():
    assert not [n for n in dir(_lib) if n.startswith("DESC_")]
    assert not hasattr(patching, "PatchProg") and not hasattr(patching, "FOREIGN")
    assert "#define FRIDO_DESC_" not in open(_lib.HEADER).read()


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("kind,sname", NEW, ids=[k for k, _ in NEW])
def test_executor_hands_a_zeroed_descriptor_to_the_launcher_which_rejects_it(kind, sname, planes):
    """frido_run on a one-op program: every one of the nine launchers checks for null pointers before it touches a device."""
    L = _lib.lib(planes)
    n = _lib.OP_KINDS[kind]
    assert L.frido_sizeof_desc(n) == C.sizeof(_lib.STRUCTS[sname]) <= 512
    arr = _lib.pack_ops([_lib.make_op(kind)])
    assert L.frido_run(C.addressof(arr), 1, None) == -1      # FRIDO_EINVAL
    err = L.frido_last_error()
    assert err.startswith(b"op 0 (kind %d): " % n) and _launcher(kind).encode() in err, err
    # the launcher's own message, as a direct call words it
    assert getattr(L, _launcher(kind))(C.byref(_lib.STRUCTS[sname]()), None) == -1
    assert err == b"op 0 (kind %d): " % n + L.frido_last_error()


def _fill(st, seed):
    """Every byte of the struct set to a pattern that differs from field to field."""
    raw = bytes((seed + 7 * i) & 255 for i in range(C.sizeof(st)))
    C.memmove(C.addressof(st), raw, len(raw))
    return raw


@pytest.mark.parametrize("kind,sname", NEW, ids=[k for k, _ in NEW])
def test_pack_ops_copies_a_filled_descriptor_byte_for_byte(kind, sname):
    st = _lib.STRUCTS[sname]()
    raw = _fill(st, _lib.OP_KINDS[kind])
    k, same = _lib.op_of(kind, st)
    assert k == _lib.OP_KINDS[kind] and same is st
    arr = _lib.pack_ops([_lib.make_op("FRIDO_OP_STEP_ADD", delta=3), (k, st)])
    assert (arr[1].kind, arr[1].stream) == (k, 0)
    assert bytes(arr[1].u)[:len(raw)] == raw and not any(bytes(arr[1].u)[len(raw):])
    other = next(s for _, s in NEW if s != sname)
    with pytest.raises(TypeError, match=f"{kind} takes a {sname}, got {other}"):
        _lib.op_of(kind, _lib.STRUCTS[other]())

"""CPU-side checks of ABI 8: the nine launchers that had descriptors but no op kind (unfold, fold, q_sample, diffusion loss, codebook loss,
DPM step, keep blend, inversion step, guidance compose) are op kinds 27 .. 35 of the one executor -- appended, nothing renumbered -- and
the second program system that served them (patching.PatchProg, patching.FOREIGN, the FRIDO_DESC_* size codes) is gone.  And of the op table:
_lib derives kind -> struct and the export list from the header, frido_sizeof_desc and the executor's dispatch come from one list in
runtime.hip, and every launcher rejects a zeroed descriptor in the same words through frido_run as on its own."""
import ctypes as C

import pytest

from frido_amd import _lib, patching

NEW = [("FRIDO_OP_UNFOLD", "FridoUnfold"), ("FRIDO_OP_FOLD", "FridoFold"), ("FRIDO_OP_QSAMPLE", "FridoQSample"),
       ("FRIDO_OP_DIFFUSION_LOSS", "FridoDiffusionLoss"), ("FRIDO_OP_VQ_COMMIT_LOSS", "FridoVqCommitLoss"), ("FRIDO_OP_DPM_STEP", "FridoDpmStep"),
       ("FRIDO_OP_KEEP_BLEND", "FridoKeepBlend"), ("FRIDO_OP_INVERT_STEP", "FridoInvertStep"), ("FRIDO_OP_GUIDANCE_COMPOSE", "FridoGuidanceCompose")]
OLD = ["GEMM", "GN_STATS", "GN_APPLY", "LAYERNORM", "SOFTMAX", "GEGLU", "PACK", "RELAYOUT", "VQ", "SAMPLER_STEP", "HANDOFF", "RANDN", "STEP_ADD",
       "FILL", "TIME_EMB", "CONVT", "PLACE", "EMBED", "TO_U8", "ATTN_SMALL", "GN_FUSED", "COPY", "ATTN_FLASH", "SYNC", "L2NORM", "ATTN_MH"]


# kind -> descriptor struct, frozen: what _lib derives from the header's launcher prototypes must equal it
FROZEN = {
    "FRIDO_OP_GEMM": "FridoGemm", "FRIDO_OP_GN_STATS": "FridoGnStats", "FRIDO_OP_GN_APPLY": "FridoGnApply",
    "FRIDO_OP_LAYERNORM": "FridoLayerNorm", "FRIDO_OP_SOFTMAX": "FridoSoftmax", "FRIDO_OP_GEGLU": "FridoGeglu",
    "FRIDO_OP_PACK": "FridoPack", "FRIDO_OP_RELAYOUT": "FridoRelayout", "FRIDO_OP_VQ": "FridoVq",
    "FRIDO_OP_SAMPLER_STEP": "FridoSamplerStep", "FRIDO_OP_HANDOFF": "FridoHandoff", "FRIDO_OP_RANDN": "FridoRandn",
    "FRIDO_OP_STEP_ADD": "FridoStepAdd", "FRIDO_OP_FILL": "FridoFill", "FRIDO_OP_TIME_EMB": "FridoTimeEmb",
    "FRIDO_OP_CONVT": "FridoConvT", "FRIDO_OP_PLACE": "FridoPlace", "FRIDO_OP_EMBED": "FridoEmbed", "FRIDO_OP_TO_U8": "FridoToU8",
    "FRIDO_OP_ATTN_SMALL": "FridoAttnSmall", "FRIDO_OP_GN_FUSED": "FridoGnApply", "FRIDO_OP_COPY": "FridoCopy",
    "FRIDO_OP_ATTN_FLASH": "FridoAttnSmall", "FRIDO_OP_SYNC": "FridoSync", "FRIDO_OP_L2NORM": "FridoL2Norm", "FRIDO_OP_ATTN_MH": "FridoAttnMh",
    "FRIDO_OP_UNFOLD": "FridoUnfold", "FRIDO_OP_FOLD": "FridoFold", "FRIDO_OP_QSAMPLE": "FridoQSample",
    "FRIDO_OP_DIFFUSION_LOSS": "FridoDiffusionLoss", "FRIDO_OP_VQ_COMMIT_LOSS": "FridoVqCommitLoss", "FRIDO_OP_DPM_STEP": "FridoDpmStep",
    "FRIDO_OP_KEEP_BLEND": "FridoKeepBlend", "FRIDO_OP_INVERT_STEP": "FridoInvertStep", "FRIDO_OP_GUIDANCE_COMPOSE": "FridoGuidanceCompose",
}
# The older kinds whose launcher turns an all-zero descriptor away through FRIDO_REQUIRE before any HIP call, read off each launcher's
# first check (misc.hip, norm.hip, attn.hip, flash.hip, flash_mh.hip: a null pointer; igemm.hip gemm_args::frido_gemm: M, N, K, batch > 0).
# That is every older kind with a launcher: FRIDO_OP_SYNC has none, and a zeroed one (from == to) is a valid no-op.
OLD_REJECTING = [("FRIDO_OP_" + k, FROZEN["FRIDO_OP_" + k]) for k in OLD if k != "SYNC"]
ZEROED = NEW + OLD_REJECTING
EINVAL = -1


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


def test_kind_table_and_exports_are_derived_from_the_header():
    assert len(FROZEN) == 35 and _lib.KIND_STRUCT == FROZEN
    assert _lib.kind_structs(open(_lib.HEADER).read()) == FROZEN
    assert set(_lib.EXPORTS) == set(_lib.declared_symbols()) and len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == 61
    assert len(OLD_REJECTING) == 25 and len(ZEROED) == 34


@pytest.mark.parametrize("proto,kind", [("int frido_fold(const FridoFold* d, frido_stream_t s);", "FRIDO_OP_FOLD"),
                                        ("int frido_gn_fused(const FridoGnApply* d, frido_stream_t s);", "FRIDO_OP_GN_FUSED")])
def test_a_kind_without_a_launcher_prototype_fails_the_derivation_by_name(proto, kind):
    text = open(_lib.HEADER).read()
    assert text.count(proto) == 1
    with pytest.raises(_lib.FridoHipError, match=kind + r": .*" + _launcher(kind) + r"\("):
        _lib.kind_structs(text.replace(proto, ""))
    with pytest.raises(_lib.FridoHipError, match=kind + ": "):      # malformed: not (const FridoX* d, frido_stream_t s)
        _lib.kind_structs(text.replace(proto, proto.replace("frido_stream_t s", "void* s")))


@pytest.mark.parametrize("planes", ["f16", "bf16"])
def test_sizeof_desc_is_the_struct_size_for_every_kind_and_minus_one_outside(planes):
    L = _lib.lib(planes)
    assert sorted(_lib.OP_KINDS[k] for k in FROZEN) == list(range(1, 36))
    for kind, sname in FROZEN.items():
        assert L.frido_sizeof_desc(_lib.OP_KINDS[kind]) == C.sizeof(_lib.STRUCTS[sname]) <= 512, kind
    for k in (0, 36, -1, -(2 ** 31)):
        assert L.frido_sizeof_desc(k) == -1, k


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("k", [0, 36])
def test_a_program_of_an_unknown_kind_is_einval(k, planes):
    L = _lib.lib(planes)
    arr = (_lib.FridoOp * 1)()
    arr[0].kind = k
    assert L.frido_run(C.addressof(arr), 1, None) == EINVAL
    assert L.frido_last_error() == b"op 0 (kind %d): frido_run: unknown op kind %d" % (k, k)


@pytest.mark.parametrize("planes", ["f16", "bf16"])
@pytest.mark.parametrize("kind,sname", ZEROED, ids=[k for k, _ in ZEROED])
def test_executor_hands_a_zeroed_descriptor_to_the_launcher_which_rejects_it(kind, sname, planes):
    """frido_run on a one-op program: every launcher of ZEROED checks its descriptor before it touches a device."""
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

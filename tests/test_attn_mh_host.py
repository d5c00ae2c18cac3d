"""CPU-side checks of the multi-head attention op (added in ABI 7): the header, its ctypes mirror and both builds of the library agree on the
descriptor, the launcher rejects what it cannot run without touching a device, and the builder refuses unsupported head dimensions."""
import ctypes as C

import pytest

from frido_amd import _lib


def _desc(**over):
    kw = dict(Q=64, q_lo=1 << 20, ldq=192, q_hs=96, K=128, k_lo=1 << 20, k_bs=64 * 192, ldk=192, k_hs=96, VT=256, vt_lo=1 << 20,
              vt_bs=64 * 64, ldvt=64, out_op=512, out_lo=1 << 20, ldo=64, B=1, heads=2, Nq=64, Nk=64, d=32, nsplit=2, alpha=32 ** -0.5)
    kw.update(over)
    return _lib.make_op("FRIDO_OP_ATTN_MH", **kw)[1]


def test_abi_declares_the_multi_head_attention_op():
    assert _lib.ABI_VERSION == 8
    assert _lib.OP_KINDS["FRIDO_OP_ATTN_MH"] == 26 == _lib.OP_KINDS["FRIDO_OP_L2NORM"] + 1      # appended in ABI 7
    assert _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36 and _lib.OP_KINDS["FRIDO_OP_UNFOLD"] == 27    # ABI 8's nine kinds follow it
    assert _lib.KIND_STRUCT["FRIDO_OP_ATTN_MH"] == "FridoAttnMh"
    fields = [f for f, _ in _lib.STRUCTS["FridoAttnMh"]._fields_]
    assert {"heads", "q_hs", "k_hs", "ldvt", "alpha"} <= set(fields)
    assert C.sizeof(_lib.STRUCTS["FridoAttnMh"]) <= 512 and C.sizeof(_lib.FridoOp) == 520      # the union slot did not grow
    assert {"frido_attn_mh", "frido_attn_mh_supported"} <= set(_lib.declared_symbols()) and "frido_attn_mh" in _lib.EXPORTS
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        assert L.frido_abi_version() == 8
        assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_ATTN_MH"]) == C.sizeof(_lib.STRUCTS["FridoAttnMh"])
        assert [x for x in range(8, 264, 8) if L.frido_attn_mh_supported(x)] == [32, 64]


def test_builder_head_dimensions_match_the_library():
    from frido_amd import builder
    assert list(builder.MH_HEAD_DIMS) == [x for x in range(8, 264, 8) if _lib.lib().frido_attn_mh_supported(x)]
    builder.check_attention_heads(1, 48)             # one head: the single-head kernels, any width
    builder.check_attention_heads(12, 32)
    with pytest.raises(NotImplementedError, match="32, 64"):
        builder.check_attention_heads(4, 48)


@pytest.mark.parametrize("over,msg", [
    (dict(d=48), b"head dimension"),
    (dict(d=128), b"head dimension"),
    (dict(heads=0), b"empty problem"),
    (dict(Nk=0), b"empty problem"),
    (dict(nsplit=3), b"nsplit"),
    (dict(ldvt=32), b"zero-padded"),               # shorter than Nk rounded up to 32
    (dict(Nk=65, ldvt=64), b"zero-padded"),
    (dict(ldo=32), b"row strides"),                # narrower than heads * d
    (dict(q_hs=100), b"16-byte alignment"),
    (dict(ldk=196), b"16-byte alignment"),
    (dict(K=130), b"16-byte aligned"),
    (dict(out_op=0), b"null pointer"),
])
def test_launcher_rejects_bad_descriptors_without_touching_a_device(over, msg):
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        st = _desc(**over)
        assert L.frido_attn_mh(C.addressof(st), None) == -1
        assert msg in L.frido_last_error(), L.frido_last_error()
        arr = _lib.pack_ops([(_lib.OP_KINDS["FRIDO_OP_ATTN_MH"], st)])
        assert L.frido_run(C.addressof(arr), 1, None) == -1      # the native executor routes the op kind to the same launcher
        assert msg in L.frido_last_error()

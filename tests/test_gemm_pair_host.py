"""CPU side of the pair launch: the ABI it must not move, the flag Prog sets, and the tuner's pair key in the cache file."""
import ctypes as C
import json
import os
import re

import torch

from frido_amd import _lib, engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRED = 1 << 28


def test_header_declares_the_pair_launcher_and_the_abi_is_unchanged():
    hdr = open(os.path.join(REPO, "include", "frido_hip.h")).read()
    assert re.search(r"int\s+frido_gemm_pair\(const FridoGemm\*\s*a,\s*const FridoGemm\*\s*b,\s*frido_stream_t\s+s\);", hdr)
    assert "frido_gemm_pair" in _lib.declared_symbols() and "frido_gemm_pair" in _lib.EXPORTS
    assert "bit 28" in hdr
    assert _lib.ABI_VERSION == 8
    assert C.sizeof(_lib.FridoOp) == 520 and C.sizeof(_lib.STRUCTS["FridoGemm"]) == 512
    assert len(_lib.OP_KINDS) == 36
    L = _lib.lib()
    assert hasattr(L, "frido_gemm_pair") and L.frido_abi_version() == 8 and L.frido_sizeof_op() == 520
    assert L.frido_sizeof_desc(_lib.OP_KINDS["FRIDO_OP_GEMM"]) == 512
    assert engine.GEMM_PAIRED == PAIRED and not engine.GEMM_FLAGS & PAIRED


def test_pair_launcher_rejects_bad_descriptors_without_touching_a_device():
    L = _lib.lib()
    _, ok = _lib.make_op("FRIDO_OP_GEMM", M=16, N=16, K=32, batch=1, nsplit=1, A=64, B=64, out_f32=64)
    _, bad = _lib.make_op("FRIDO_OP_GEMM", M=16, N=16, K=20, batch=1, nsplit=1, A=64, B=64, out_f32=64)
    assert L.frido_gemm_pair(C.addressof(bad), C.addressof(ok), None) == -1
    assert L.frido_gemm_pair(C.addressof(ok), C.addressof(bad), None) == -1 and b"frido_gemm" in L.frido_last_error()
    assert L.frido_gemm_pair(None, C.addressof(ok), None) == -1
    # the executor: a flagged GEMM needs a GEMM behind it, checked before the first launch
    kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    ok.flags |= PAIRED
    for ops in ([(kind, ok)], [(kind, ok), _lib.make_op("FRIDO_OP_COPY")]):
        arr = _lib.pack_ops(ops)
        assert L.frido_run(C.addressof(arr), len(ops), None) == -1
        assert b"op 0 " in L.frido_last_error() and b"bit 28" in L.frido_last_error()


def _two(prog, **kw):
    prog.gemm(64, 64, 32, (4096, 0), (8192, 0), out_f32=12288, ldo=64, **kw)
    prog.gemm(32, 64, 32, (4096, 0), (8192, 0), out_f32=16384, ldo=64)


def test_prog_sets_bit_28_on_the_head_op_only():
    p = engine.Prog(torch.device("cpu"), 2)
    _two(p)
    with p.gemm_pair():
        _two(p)
    _two(p)
    flags = [st.flags & PAIRED for _, st in p.ops]
    assert flags == [0, 0, PAIRED, 0, 0, 0]
    arr = p.packed()
    G = _lib.STRUCTS["FridoGemm"]
    assert [G.from_buffer_copy(bytes(arr[i].u)).flags & PAIRED for i in range(6)] == flags
    assert [st.M for _, st in p.ops] == [64, 32] * 3           # nothing reordered
    # a tool that walks the program op by op packs the head as the plain launch it is on its own; the program's descriptor keeps its bit
    alone = _lib.pack_single(*p.ops[2])
    assert not G.from_buffer_copy(bytes(alone[0].u)).flags & PAIRED and p.ops[2][1].flags & PAIRED
    assert G.from_buffer_copy(bytes(alone[0].u)).M == 64
    try:
        with p.gemm_pair():
            p.gemm(64, 64, 32, (4096, 0), (8192, 0), out_f32=12288, ldo=64)
    except AssertionError:
        pass
    else:
        raise AssertionError("a pair of one GEMM went through")


def test_builder_knob_switches_the_pairs_off(monkeypatch):
    from frido_amd import builder
    for on in (True, False):
        monkeypatch.setattr(builder, "GEMM_PAIR", on)
        b = builder.Builder("cpu", 2, {})
        with b.gemm_pair():
            _two(b.prog)
        assert [bool(st.flags & PAIRED) for _, st in b.prog.ops] == [on, False]


def test_tuner_pair_key_round_trips_through_the_cache_file(tmp_path, monkeypatch):
    from frido_amd import tune
    p = engine.Prog(torch.device("cpu"), 2)
    _two(p)
    a, b = p.ops[0][1], p.ops[1][1]
    key = tune.pair_key(a, b)
    assert key[0] == "pair" and key[1:] == tune.signature(a) + tune.signature(b) and key != tune.pair_key(b, a)
    path = str(tmp_path / "cache.json")
    monkeypatch.setattr(tune, "CACHE_FILE", path)
    monkeypatch.setattr(tune, "_cache", {key: (3, 1), tune.pair_key(b, a): (0, 0), tune.signature(a): (4, 1)})
    monkeypatch.setattr(tune, "_dirty", True)
    monkeypatch.setattr(tune, "ENABLED", True)
    monkeypatch.setenv("FRIDO_TUNE_CACHE_READONLY", "0")
    monkeypatch.setenv("RANK", "0")
    tune._save_cache()
    blob = json.load(open(path))
    assert blob["lib"] == tune._lib_tag() and len(blob["entries"]) == 3
    assert all(isinstance(k, list) and not any(isinstance(x, (list, dict)) for x in k) for k, _ in blob["entries"])     # flat keys: the loader's format
    monkeypatch.setattr(tune, "_cache", {})
    tune._load_cache()
    assert tune._cache[key] == (3, 1) and tune._cache[tune.pair_key(b, a)] == (0, 0) and tune._cache[tune.signature(a)] == (4, 1)
    # what the planner does with it: a pinned win sets both tiles (and the order), a pinned loss leaves the two unpaired
    assert tune.best_pair(a, b, torch.device("cpu")) == (3, 1) and tune.best_pair(b, a, torch.device("cpu")) == (0, 0)
    monkeypatch.setattr(tune, "ON_MISS", "static")
    monkeypatch.setattr(tune, "_cache", {})
    assert tune.best_pair(a, b, torch.device("cpu")) is None
    monkeypatch.setattr(tune, "ENABLED", False)
    assert tune.best_pair(a, b, torch.device("cpu")) is None

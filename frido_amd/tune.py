"""Plan-time tile selection for the implicit-GEMM kernel: each distinct GEMM signature is timed once per
process on scratch buffers with every tile shape (HIP events on the launch stream) and the fastest wins.
Disable with FRIDO_TUNE=0 (the C library's static heuristic is used instead).  FRIDO_TUNE_CACHE=<file> persists the
choices across processes (JSON; keyed by the GEMM signature and a content hash of libfrido_hip.so, so a rebuilt library starts
over) -- used to profile under rocprofv3 --pmc, where re-timing thousands of candidates would take hours."""
import atexit
import ctypes as C
import json
import os

import torch

from . import _lib

TILES = (1, 2, 3, 4, 5, 6)          # see include/frido_hip.h FridoGemm.tile
TILES64 = (11, 12, 13, 14, 15, 16)  # BK = 64 variants
TILES8W = (7, 8)                    # 8-wave 256-row tiles (bf16 mode)
_cache = {}
_scratch = {}
ENABLED = os.environ.get("FRIDO_TUNE", "1") != "0"
CACHE_FILE = os.environ.get("FRIDO_TUNE_CACHE", "")
# what to do with a GEMM signature the (pinned) cache does not hold: "tune" = time the candidates now (default); "static" = the
# library's static heuristic (tile 0, no split-K) -- the GPU test suite runs this way (tests/conftest.py): benchmark shapes get the
# benchmark's pinned tiles, every other shape a deterministic one, so a run of the suite is bitwise repeatable on any box
ON_MISS = os.environ.get("FRIDO_TUNE_ON_MISS", "tune")
_dirty = False
# Not candidates: tiles 31 .. 36 (K split over the two wave groups of one workgroup).  Back to back they win 11 signatures, in context
# the 4-wave tiles win them back and end to end the two caches tie (profiles/r06_kg2_*); tools/tune_in_context.py tries them on request.


def _lib_tag():
    if os.environ.get("FRIDO_TUNE_TAG"):      # A/B of two library builds with the SAME pinned tiles (tools/ab.sh lib)
        return os.environ["FRIDO_TUNE_TAG"]
    try:
        import hashlib
        # content hash of the DEFAULT (fp16-pair) build: two builds of equal size must not share pinned tiles.  (r06, advisor) NOT the
        # active plane format's file -- the cache file only ever holds the default build's entries (bf16-pair choices are never
        # persisted), and _load_cache runs once, at the first GEMM a process plans: were that a bf16-pair model, the pinned file would be
        # rejected for the whole process and could be overwritten at exit
        with open(_lib.LIB_PATHS["f16"], "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return "?"


def cache_is_pinned_for_this_library():
    """True when FRIDO_TUNE_CACHE names a file whose library tag is this build's (tests: are the benchmark's tiles in force?)."""
    if not CACHE_FILE or not os.path.exists(CACHE_FILE):
        return False
    try:
        return json.load(open(CACHE_FILE)).get("lib") == _lib_tag()
    except (OSError, ValueError):
        return False


def _load_cache():
    if not CACHE_FILE or not os.path.exists(CACHE_FILE):
        return
    try:
        blob = json.load(open(CACHE_FILE))
    except (OSError, ValueError):
        return
    if blob.get("lib") != _lib_tag():
        return
    for k, v in blob.get("entries", []):
        _cache[tuple(k)] = tuple(v)


def _save_cache():
    if CACHE_FILE and _dirty and os.environ.get("RANK", "0") == "0" and os.environ.get("FRIDO_TUNE_CACHE_READONLY", "0") == "0":
        # (one writer under torch.distributed.run; bench.py reads the tracked cache and only rewrites it under --retune)
        tmp = f"{CACHE_FILE}.{os.getpid()}.tmp"
        with open(tmp, "w") as f:
            json.dump({"lib": _lib_tag(), "entries": [[list(k), list(v)] for k, v in _cache.items() if not isinstance(k[-1], str)]}, f)
        os.replace(tmp, CACHE_FILE)


_load_cache()
atexit.register(_save_cache)

_SIG_FIELDS = ("M", "N", "K", "batch", "nsplit", "conv", "lda", "ldb", "a_bs", "b_bs", "Hs", "Ws", "Cin", "Hl", "Wl", "Ho",
               "Wo", "kh", "kw", "stride", "pad", "padx", "up_shift", "dn_shift", "act", "geglu", "ldo", "ldoo", "of_bs", "oo_bs", "ldr",
               "res_bs", "res_bf16", "out_bf16", "batch_inner", "a_bs2", "b_bs2", "of_bs2", "oo_bs2", "K2", "lda2", "up2_phase")


def _buf(name, nbytes, device):
    key = (name, str(device))
    t = _scratch.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _scratch[key] = t
    return t.data_ptr()


_ws = {}


def workspace_for(st, device, tag=""):
    """Workspace of a filled FridoGemm descriptor with splitk > 1 (sized by the library: ticket header + partial sums)."""
    return workspace(device, _lib.lib().frido_gemm_workspace_bytes(C.addressof(st)), tag)


def workspace(device, nbytes, tag=""):
    """Split-K workspace: one per (device, tag).  Ops of all programs of one builder run in stream order, so they share one
    buffer; builders whose programs run CONCURRENTLY on different streams pass their own tag."""
    key = str(device) + tag
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        old = t
        t = torch.zeros(int(nbytes * 1.5) + 256, dtype=torch.uint8, device=device)      # zero: the ticket header (frido_hip.h)
        _ws[key] = t
        if old is not None:
            _ws.setdefault(key + ":old", []).append(old)      # descriptors emitted earlier still point at it
    return t.data_ptr()


def signature(st):
    """Cache key of a filled FridoGemm descriptor (pointers only as present / absent)."""
    sig = tuple(getattr(st, f) for f in _SIG_FIELDS) + (bool(st.residual), bool(st.out_f32), bool(st.out_op),
                                                        bool(st.bias), bool(st.rowvec), bool(st.row_bias))
    if _lib.active_planes() != "f16":      # (r05) the bf16-pair build: its own choices, never persisted (the pinned cache file is the default build's)
        sig = sig + (_lib.active_planes(),)
    return sig


def _scratch_desc(st, device, pre=""):
    """Copy of the filled descriptor `st` with every pointer replaced by a scratch buffer (named pre + role: the two members of a
    pair get buffers of their own), as the candidates are timed."""
    G = _lib.STRUCTS["FridoGemm"]
    t = G()
    C.memmove(C.addressof(t), C.addressof(st), C.sizeof(G))
    ns = st.nsplit
    t.gn_part = None         # candidates are timed without the fused GroupNorm partial sums (split-K tiles cannot produce them)
    # (r06) an all-phases upsample conv (up2_phase 5: batch index = phase) keeps its form while it is timed -- until r05 the phase flag was
    # cleared here while batch = 4 stayed, a combination frido_gemm REJECTS ("conv mode is not batched"): every candidate failed and the three
    # upsample convs of a forward ran on the static tile (8^2 -> 16^2: 128 x 192 tiles = 160 workgroups, 181 TFLOP/s).  Its scratch output is the
    # interleaved [4 M][N] tensor; a single-phase conv (1..4) is timed as a plain conv with in-order rows.
    if st.up2_phase != 5:
        t.up2_phase = 0
    if st.conv:
        a_elems = (st.M // (st.Ho * st.Wo)) * st.Hs * st.Ws * st.Cin
    else:
        a_elems = st.batch * max(st.a_bs, st.a_bs2, st.M * st.lda) if (st.a_bs or st.a_bs2) else st.M * st.lda
    b_elems = st.batch * max(st.b_bs, st.b_bs2, st.N * st.ldb) if (st.b_bs or st.b_bs2) else st.N * st.ldb
    a_elems, b_elems = (a_elems + 7) // 8 * 8, (b_elems + 7) // 8 * 8
    t.A, t.a_lo = _buf(pre + "A", a_elems * 2 * ns, device), a_elems
    t.B, t.b_lo = _buf(pre + "B", b_elems * 2 * ns, device), b_elems
    if st.K2:
        a2 = (st.M * st.lda2 + 7) // 8 * 8
        t.A2, t.a2_lo = _buf(pre + "A2", a2 * 2 * ns, device), a2
    rows = st.M * st.batch
    if st.out_f32:
        t.out_f32 = _buf(pre + "O", max(max(st.of_bs, st.of_bs2) * st.batch, st.M * st.ldo * (4 if st.up2_phase == 5 else 1)) * 4 + 4096, device)
    if st.out_op:
        n = max(max(st.oo_bs, st.oo_bs2) * st.batch, st.M * st.ldoo * (4 if st.up2_phase == 5 else 1)) + 4096
        n = (n + 7) // 8 * 8
        t.out_op, t.oo_lo = _buf(pre + "OO", n * 2 * ns, device), n
    if st.residual:
        t.residual = _buf(pre + "R", max(st.res_bs * st.batch, st.M * st.ldr) * 4, device)
    if st.bias:
        t.bias = _buf(pre + "bias", st.N * 4, device)
    if st.row_bias:
        t.row_bias = _buf(pre + "rbias", st.M * 4, device)
    if st.rowvec:
        t.rowvec, t.rowvec_step, t.rows_per_vec, t.ldv = _buf(pre + "rv", (rows + 1) * st.N * 4, device), None, max(st.rows_per_vec, 1), st.N
        if st.rows_per_vec >= (1 << 29):
            t.rows_per_vec = 1 << 30
    return t


def best_tile(st, device, stream):
    """st: a filled FridoGemm ctypes struct (pointers are ignored: scratch buffers are substituted).
    Returns (tile, splitk) -- or (tile, splitk, start delay in quarter microseconds) for a signature whose pinned cache entry carries
    one (written by tools/tune_in_context.py --stagger; this function's own timing never produces the third element)."""
    if not ENABLED:
        return 0, 1
    sig = signature(st)
    if sig in _cache:
        return _cache[sig]
    if ON_MISS == "static":
        return 0, 1
    t = _scratch_desc(st, device)
    L = _lib.lib()
    kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    reps = 5
    best, best_t = (0, 1), float("inf")
    nk = (st.K + st.K2) // 32
    small = st.batch == 1 and st.M * st.N <= (1 << 23) and not st.geglu       # split-K only pays for small outputs with a long K
    splits = [1] + [k for k in (2, 3, 4, 6, 8, 12, 16) if small and nk >= 8 * k]
    if st.up2_phase:
        splits = [1]          # the split-K reduction writes rows in order; phase convs interleave them
    for sk in splits:
        t.splitk = sk
        t.sk_mode = 0        # partial sums are added by the splitk_reduce launch (or by the consuming GroupNorm: builder._deferred_splitk)
        t.ws = workspace_for(t, device) if sk > 1 else None
        # BK = 64 halves the barrier count but costs a ring stage of occupancy: tried on every one-plane shape it applies to
        k64 = st.nsplit == 1 and st.K % 64 == 0 and st.K2 % 64 == 0 and (not st.conv or st.Cin % 64 == 0) and (st.K // 64) >= sk
        big = st.M >= 512 and st.N >= 96
        # tile 9 = patch-staged 3x3 kernel (igemm.hip patch_ok; the library rejects it when it does not apply)
        patch = (st.conv and st.nsplit == 1 and st.batch == 1 and st.kh == 3 and st.stride == 1 and not (st.up_shift or st.dn_shift)
                 and not st.up2_phase and st.M % 128 == 0 and st.M >= 4096 and st.N >= 96 and sk <= (st.Cin + st.K2) // 32)
        big_tiles = (TILES8W if st.nsplit == 1 else (7, 18, 19)) if big else ()  # bf16x3: 256 x 128 and the 8-wave 128 x 192 / 256 x 192
        for tile in TILES + (TILES64 if k64 else ()) + big_tiles + ((17,) if big and k64 else ()) + ((9, 10) if patch else ()):
            if tile % 10 in (1, 2, 4) and st.M < 64:
                continue
            t.tile = tile
            arr = _lib.pack_ops([(kind, t)] * (reps + 1))
            ms = (C.c_float * (reps + 1))()
            rc = L.frido_run_timed(C.addressof(arr), reps + 1, stream, ms)
            if rc != 0:
                continue
            dt = sorted(list(ms)[1:])[reps // 2]
            if dt < best_t:
                best, best_t = (tile, sk), dt
    if best_t == float("inf"):
        # (r06) every candidate was rejected by the library: the launch falls back to the static tile.  That is how the upsample convs
        # silently ran untuned for three rounds -- say so.
        import warnings
        warnings.warn(f"frido_amd.tune: no candidate tile could be timed for GEMM M={st.M} N={st.N} K={st.K}+{st.K2} batch={st.batch} "
                      f"conv={st.conv} up2_phase={st.up2_phase} ({L.frido_last_error().decode()}): it runs on the library's static tile")
    _cache[sig] = best
    global _dirty
    if _lib.active_planes() == "f16":
        _dirty = True
    return best


PAIR_KEY = "pair"       # first element of a pair's cache key: ("pair",) + signature(a) + signature(b) -> (tile, swap); tile 0 = not paired
PAIR_MARGIN = 0.98      # a pair must beat the two single launches by 2 %: the timing noise of ~25 us launches


def pair_key(sa, sb):
    return (PAIR_KEY,) + signature(sa) + signature(sb)


def _time_graph(ops, device, inner=8, reps=5):
    """Median device time in ms of ONE pass over `ops`: `inner` passes captured into one graph, replayed reps + 1 times on a
    stream of the tuner's own.  None when the library rejects the program."""
    L = _lib.lib()
    key = ("stream", str(device))
    if key not in _scratch:
        _scratch[key] = torch.cuda.Stream(device=device)
    ts = _scratch[key]
    ts.wait_stream(torch.cuda.current_stream(device))
    arr = _lib.pack_ops(list(ops) * inner)
    g = C.c_void_p()
    if L.frido_graph_capture(C.addressof(arr), len(ops) * inner, ts.cuda_stream, C.byref(g)) != 0:
        return None
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.frido_event_create(C.byref(e0))
    L.frido_event_create(C.byref(e1))
    times = []
    try:
        for r in range(reps + 1):
            L.frido_event_record(e0, ts.cuda_stream)
            if L.frido_graph_launch(g, ts.cuda_stream) != 0:
                return None
            L.frido_event_record(e1, ts.cuda_stream)
            ms = C.c_float()
            if L.frido_event_elapsed_ms(e0, e1, C.byref(ms)) != 0:
                return None
            times.append(ms.value / inner)
    finally:
        L.frido_event_destroy(e0)
        L.frido_event_destroy(e1)
        L.frido_graph_destroy(g)
    return sorted(times[1:])[reps // 2]


def pair_candidates(sa, sb):
    """Tile ids both members of a pair take (the candidate rules of best_tile, no split-K, no conv-only tiles)."""
    k64 = all(st.nsplit == 1 and st.K % 64 == 0 and st.K2 % 64 == 0 for st in (sa, sb))
    big = all(st.M >= 512 and st.N >= 96 for st in (sa, sb))
    big_tiles = (TILES8W if sa.nsplit == 1 else (7, 18, 19)) if big else ()
    tiles = TILES + (TILES64 if k64 else ()) + big_tiles + ((17,) if big and k64 else ())
    return [t for t in tiles if not (t % 10 in (1, 2, 4) and min(sa.M, sb.M) < 64)]


def best_pair(sa, sb, device, measure=None, reps=5):
    """sa, sb: the filled descriptors of two independent GEMMs emitted as a pair (engine.Prog.gemm_pair), each already carrying its
    own best (tile, splitk).  Returns None when nothing was timed (tuner off, or a miss under FRIDO_TUNE_ON_MISS=static: the members
    keep their tiles and the library merges them where it can), else (tile, swap): the common tile on which ONE grid of both beats the
    members' own best launches back to back, and whether member b goes first -- or (0, 0) when the two single launches win.
    `measure`: a dict that receives the timings (tools/gemm_pair_bench.py)."""
    if not ENABLED:
        return None
    if sa.conv or sb.conv or sa.nsplit != sb.nsplit:
        return None
    key = pair_key(sa, sb)
    if key in _cache:
        return _cache[key]
    if ON_MISS == "static":
        return None
    kind = _lib.OP_KINDS["FRIDO_OP_GEMM"]
    ta, tb = _scratch_desc(sa, device, "pa:"), _scratch_desc(sb, device, "pb:")
    for t in (ta, tb):
        t.flags &= ~(1 << 28)
        if t.splitk > 1:
            t.sk_mode, t.ws = 0, workspace_for(t, device)
    t_single = _time_graph([(kind, ta), (kind, tb)], device, reps=reps)
    best, best_t, every = (0, 0), float("inf"), []
    for t in (ta, tb):
        t.splitk, t.ws = 1, None
    for tile in pair_candidates(sa, sb):
        ta.tile = tb.tile = tile
        for swap in (0, 1):
            head, tail = (tb, ta) if swap else (ta, tb)
            head.flags |= 1 << 28
            dt = _time_graph([(kind, head), (kind, tail)], device, reps=reps)
            head.flags &= ~(1 << 28)
            every.append((tile, swap, dt))
            if dt is not None and dt < best_t:
                best, best_t = (tile, swap), dt
    if measure is not None:
        measure.update(single_ms=t_single, pair_ms=best_t, tile=best[0], swap=best[1], tiles=(sa.tile, sa.splitk, sb.tile, sb.splitk), every=every)
    if t_single is None or not best_t < PAIR_MARGIN * t_single:
        best = (0, 0)
    _cache[key] = best
    global _dirty
    if _lib.active_planes() == "f16":
        _dirty = True
    return best

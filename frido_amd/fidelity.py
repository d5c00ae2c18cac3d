"""Inception Score and Kernel Inception Distance on the HIP engine: the ctypes binding of include/frido_fidelity.h (csrc/fidelity.hip:
row dot products in float64 with their four epilogues, the finish of the MMD^2 estimate, the four steps of the Inception Score),
FeatureBank -- the per-sample rows both metrics need, which FeatureStatistics folds away --, inception_score and
kernel_inception_distance.

Bound beside `_lib`, not inside it, like frido_amd/fid.py: the six launches are no op kinds.  The descriptors are parsed from their own
header with `_lib`'s parser, the functions are taken from the handle `_lib.lib()` returns for the active plane format (the code is the
same in both builds: f32 / f64 only), and every descriptor's size is compared with the library's at first use.  A library without the
symbols is a stale build and is named as one: there is no fallback.

The estimators and their defaults are torch-fidelity's (`fidelity --isc --kid`), written from its published description: the package
is not installed to pin them against, so the formulas in include/frido_fidelity.h and in the two functions' docstrings ARE the
specification here.  tests/fidelity_ref.py restates them in float64 numpy."""
import ctypes as C
import os
import re

import numpy as np
import torch

from . import _lib
from ._lib import FridoHipError
from .fid import FEATURES

HEADER = os.path.join(_lib.REPO, "include", "frido_fidelity.h")
_text = open(HEADER).read()
_src = _lib._strip_comments(_text)
_structs = _lib._parse_structs(_src)
FridoRowsDot = type("FridoRowsDot", (C.Structure,), {"_fields_": _structs["FridoRowsDot"]})
FridoMmdFinish = type("FridoMmdFinish", (C.Structure,), {"_fields_": _structs["FridoMmdFinish"]})
FridoIsc = type("FridoIsc", (C.Structure,), {"_fields_": _structs["FridoIsc"]})

# launcher -> (descriptor, the library's sizeof function)
LAUNCHERS = {"frido_rows_dot": (FridoRowsDot, "frido_sizeof_rows_dot"), "frido_mmd_finish": (FridoMmdFinish, "frido_sizeof_mmd_finish"),
             "frido_isc_rowstats": (FridoIsc, "frido_sizeof_isc"), "frido_isc_marginal": (FridoIsc, "frido_sizeof_isc"),
             "frido_isc_kl": (FridoIsc, "frido_sizeof_isc"), "frido_isc_finish": (FridoIsc, "frido_sizeof_isc")}
ISC_STEPS = ("frido_isc_rowstats", "frido_isc_marginal", "frido_isc_kl", "frido_isc_finish")

STORE_F32, STORE_F64, STORE_POLY_F64, SUM_POLY = 0, 1, 2, 3      # FRIDO_ROWS_DOT_*
ROWS_DOT_GRID_CAP = int(re.search(r"#define\s+FRIDO_ROWS_DOT_GRID_CAP\s+(\d+)", _src).group(1))      # workgroups of one launch at the most
TILE = 64                                                        # pairs per tile side
LOGITS = 1008                                                    # the FID checkpoint's fc rows

_bound = {}      # plane format -> {launcher name: function of that build}


def _fns(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        fns = {}
        for name, (struct, sizeof) in LAUNCHERS.items():
            for sym in (name, sizeof):
                if not hasattr(L, sym):
                    raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {sym}: a stale build from before csrc/fidelity.hip "
                                        "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
            c_sz = getattr(L, sizeof)()
            if c_sz != C.sizeof(struct):
                raise FridoHipError(f"ABI mismatch: sizeof({struct.__name__}) C={c_sz} py={C.sizeof(struct)} "
                                    "(include/frido_fidelity.h and the build disagree: stale build?)")
            fn = getattr(L, name)
            fn.argtypes = [C.c_void_p, C.c_void_p]
            fns[name] = fn
        _bound[planes] = fns
    return _bound[planes]


def launch(name, desc, stream):
    """Launch `name`(desc) on `stream` (a hipStream_t handle); a refused descriptor raises with the library's message."""
    rc = _fns()[name](C.byref(desc), stream)
    if rc != 0:
        raise FridoHipError(f"{name} failed (rc={rc}): {_lib.lib().frido_last_error().decode()}")


def tiles(rx, ry=None, symmetric=False):
    """64 x 64 tiles (= SUM_POLY partials) of one subset of rx x ry pairs; the upper triangle's of a symmetric launch."""
    ntx = (rx + TILE - 1) // TILE
    nty = ntx if ry is None else (ry + TILE - 1) // TILE
    return ntx * (ntx + 1) // 2 if symmetric else ntx * nty


def rows_dot_desc(x_ptr, y_ptr, nx, ny, D, *, mode, out=None, ldo=0, partials=None, ix=None, iy=None, S=1, m=0, degree=1, gamma=1.0,
                  coef0=0.0, exclude_diag=False, symmetric=False):
    return FridoRowsDot(x=x_ptr, y=y_ptr, ix=ix, iy=iy, out=out, partials=partials, gamma=gamma, coef0=coef0, nx=nx, ny=ny, D=D, S=S, m=m,
                        ldo=ldo, mode=mode, degree=degree, exclude_diag=int(exclude_diag), symmetric=int(symmetric))


def mmd_finish_desc(pxx, pyy, pxy, out, S, m, nxx, nyy, nxy):
    return FridoMmdFinish(pxx=pxx, pyy=pyy, pxy=pxy, out=out, S=S, m=m, nxx=nxx, nyy=nyy, nxy=nxy)


def isc_desc(logits, perm, rowstats, q, kl, scores, N, Cn, splits):
    return FridoIsc(logits=logits, perm=perm, rowstats=rowstats, q=q, kl=kl, scores=scores, N=N, C=Cn, splits=splits)


# ---- checks ---------------------------------------------------------------------------------------------
def _rows2d(what, name, t, D=None):
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or (D is not None and t.shape[1] != D):
        got = (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a 2-D float32 tensor{'' if D is None else f' [*, {D}]'}, got {got}")
    return t


def _gpu(what, *tensors):
    from .engine import require_gpu
    for t in tensors:
        if t.device.type != "cuda":
            raise FridoHipError(f"{what}: tensors are on '{t.device}', but the metric runs only on an MI355X HIP device; there is no CPU "
                                "fallback")
    return require_gpu(tensors[0].device)


def _stream(dev):
    from .engine import current_stream_ptr
    return current_stream_ptr(dev)


# ---- row dot products -----------------------------------------------------------------------------------
@torch.no_grad()
def rows_dot(x, y, *, mode=STORE_F64, ix=None, iy=None, degree=1, gamma=1.0, coef0=0.0):
    """out[a, b] = X[a] . Y[b] (or, with int32 index lists ix, iy [S, m] on the device, out[s, a, b] = X[ix[s, a]] . Y[iy[s, b]]), every
    dot accumulated in float64 over k ascending: float32 rounded once (STORE_F32), float64 (STORE_F64), or the polynomial kernel
    (dot * gamma + coef0) ** degree with separately rounded operations (STORE_POLY_F64).  One launch of frido_rows_dot."""
    what = "rows_dot"
    _rows2d(what, "x", x)
    _rows2d(what, "y", y, x.shape[1])
    if x.shape[1] % 4 != 0 or x.shape[1] == 0:
        raise ValueError(f"{what}: the row length D must be a positive multiple of 4, got {x.shape[1]}")
    if mode not in (STORE_F32, STORE_F64, STORE_POLY_F64):
        raise ValueError(f"{what}: mode must be STORE_F32, STORE_F64 or STORE_POLY_F64, got {mode!r}")
    if mode == STORE_POLY_F64 and degree not in (1, 2, 3, 4):
        raise ValueError(f"{what}: degree must lie in 1 .. 4, got {degree!r}")
    if (ix is None) != (iy is None):
        raise ValueError(f"{what}: ix and iy come together or not at all")
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError(f"{what}: no rows: x {tuple(x.shape)}, y {tuple(y.shape)}")
    dev = _gpu(what, x, y)
    x, y = x.detach().contiguous(), y.detach().contiguous()
    dtype = torch.float32 if mode == STORE_F32 else torch.float64
    quantum = 4 if mode == STORE_F32 else 2                     # 16-byte stores
    kw = dict(mode=mode, degree=degree, gamma=float(gamma), coef0=float(coef0))
    if ix is None:
        S, rx, ry = 1, x.shape[0], y.shape[0]
    else:
        for n, t in (("ix", ix), ("iy", iy)):
            if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.int32 or t.shape != ix.shape or t.device != x.device or 0 in t.shape:
                raise ValueError(f"{what}: {n} must be an int32 [S, m] tensor on {x.device}")
        ix, iy = ix.contiguous(), iy.contiguous()
        S, rx = ix.shape
        ry = rx
        kw.update(ix=ix.data_ptr(), iy=iy.data_ptr(), S=S, m=rx)
    ldo = (ry + quantum - 1) // quantum * quantum
    out = torch.empty(S * rx, ldo, dtype=dtype, device=dev)
    launch("frido_rows_dot", rows_dot_desc(x.data_ptr(), y.data_ptr(), x.shape[0], y.shape[0], x.shape[1], out=out.data_ptr(), ldo=ldo, **kw),
           _stream(dev))
    for t in (x, y, ix, iy):
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    out = out[:, :ry]
    return out if ix is None else out.reshape(S, rx, ry)


# ---- the per-sample rows --------------------------------------------------------------------------------
class FeatureBank:
    """[n, D] float32 rows kept in a buffer that grows by doubling: the per-sample features (or logits) the Inception Score and KID
    need.  append() is a device copy; rows() is a view of the first n rows.  A bank may live on the CPU (storage, gloo gathers); the
    metric functions need it on the GPU."""

    MIN_ROWS = 64

    def __init__(self, D=FEATURES, device="cuda"):
        self.D, self.device, self.n = int(D), torch.device(device), 0
        self.buf = torch.empty(0, self.D, dtype=torch.float32, device=self.device)

    def _reserve(self, n):
        if n > self.buf.shape[0]:
            cap = max(self.MIN_ROWS, self.buf.shape[0])
            while cap < n:
                cap *= 2
            buf = torch.empty(cap, self.D, dtype=torch.float32, device=self.device)
            buf[:self.n].copy_(self.buf[:self.n])
            self.buf = buf

    def append(self, rows):
        _rows2d("FeatureBank.append", "rows", rows, self.D)
        self._reserve(self.n + rows.shape[0])
        self.buf[self.n:self.n + rows.shape[0]].copy_(rows.detach())
        self.n += int(rows.shape[0])
        return self

    def rows(self):
        return self.buf[:self.n]

    def to(self, device):
        out = FeatureBank(self.D, device)
        return out.append(self.rows().to(out.device))

    def save(self, path):
        """An .npz with `features` [n, D] float32."""
        with open(path, "wb") as f:      # a file object: numpy appends no suffix of its own
            np.savez(f, features=self.rows().cpu().numpy())

    @classmethod
    def load(cls, path, device="cpu"):
        z = np.load(path)
        if "features" not in z.files or z["features"].ndim != 2 or z["features"].dtype != np.float32:
            raise ValueError(f"FeatureBank.load: {path} holds {z.files}; expected `features`, a float32 [n, D] array")
        f = torch.from_numpy(z["features"])
        return cls(f.shape[1], device).append(f.to(device))

    @classmethod
    def concat(cls, banks):
        """The rows of `banks` in list order, on the first bank's device."""
        banks = list(banks)
        if not banks:
            raise ValueError("FeatureBank.concat: nothing to join")
        if any(b.D != banks[0].D for b in banks):
            raise ValueError(f"FeatureBank.concat: row widths differ: {[b.D for b in banks]}")
        out = cls(banks[0].D, banks[0].device)
        out._reserve(sum(b.n for b in banks))
        for b in banks:
            out.append(b.rows().to(out.device))
        return out

    def all_gather_concat(self, group=None):
        """The rows of every rank in rank order, on every rank; the shards may differ in size: the sizes are gathered first, then the
        rows padded to the largest shard, as FeatureStatistics.all_gather_merge gathers its sums.  Without an initialised process
        group: self."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        world = dist.get_world_size(group)
        on_host = dist.get_backend(group) == "gloo"
        dev = torch.device("cpu") if on_host else self.device
        sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([self.n], dtype=torch.int64, device=dev), group=group)
        sizes = [int(s.item()) for s in sizes]
        pad = torch.zeros(max(max(sizes), 1), self.D, dtype=torch.float32, device=dev)
        pad[:self.n].copy_(self.rows())
        got = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(got, pad, group=group)
        out = FeatureBank(self.D, self.device)
        out._reserve(sum(sizes))
        for g, n in zip(got, sizes):
            out.append(g[:n].to(self.device))
        return out


def _bank_rows(t):
    return t.rows() if isinstance(t, FeatureBank) else t


# ---- the two metrics ------------------------------------------------------------------------------------
def isc_permutation(N, shuffle=True, rng_seed=2020):
    """The row order of the Inception Score's splits: np.random.RandomState(rng_seed).permutation(N), or the identity."""
    return np.random.RandomState(rng_seed).permutation(N) if shuffle else np.arange(N)


def inception_split_scores(logits, *, splits=10, shuffle=True, rng_seed=2020):
    """The `splits` scores of inception_score as a float64 numpy array."""
    what = "inception_score"
    logits = _rows2d(what, "logits", _bank_rows(logits))
    N, Cn = logits.shape
    if not isinstance(splits, int) or splits < 1 or N < splits or Cn < 1:
        raise ValueError(f"{what}: {N} samples of {Cn} classes cannot be cut into splits={splits!r}")
    dev = _gpu(what, logits)
    x = logits.detach().contiguous()
    perm = torch.from_numpy(isc_permutation(N, shuffle, rng_seed).astype(np.int32)).to(dev)
    work = torch.empty(3 * N + splits * Cn + splits + 2, dtype=torch.float64, device=dev)
    rowstats, kl, q, scores = work[:2 * N], work[2 * N:3 * N], work[3 * N:3 * N + splits * Cn], work[3 * N + splits * Cn:][:splits]
    d = isc_desc(x.data_ptr(), perm.data_ptr(), rowstats.data_ptr(), q.data_ptr(), kl.data_ptr(), scores.data_ptr(), N, Cn, splits)
    for step in ISC_STEPS:
        launch(step, d, _stream(dev))
    x.record_stream(torch.cuda.current_stream(dev))
    return scores.cpu().numpy()


def inception_score(logits, *, splits=10, shuffle=True, rng_seed=2020):
    """(mean, std) of the Inception Score over `splits` splits, two floats.  logits: float32 [N, C] on the GPU (or a FeatureBank of them),
    torch-fidelity's `logits_unbiased` (FIDInceptionV3.logits).  THE FORMULAS HERE ARE THE SPECIFICATION (torch-fidelity's estimator
    and defaults, restated; the package is not installed to pin them against):
        perm = np.random.RandomState(rng_seed).permutation(N), the identity without `shuffle`; split i holds the rows
               perm[i N // splits : (i + 1) N // splits]
        logp_rc = (l_rc - max_c l_rc) - log sum_c exp(l_rc - max_c l_rc),  p_rc = exp(logp_rc)
        q_c = the mean of p_rc over the split's rows;   kl_r = sum_c p_rc (logp_rc - log q_c);   score_i = exp(mean of kl_r)
    all in float64 on the device (csrc/fidelity.hip, four launches); mean and std = np.mean, np.std (ddof 0) of the scores.
    Refused: logits that are no 2-D float32 tensor, N < splits (ValueError); CPU tensors (FridoHipError)."""
    s = inception_split_scores(logits, splits=splits, shuffle=shuffle, rng_seed=rng_seed)
    return float(np.mean(s)), float(np.std(s))


def kid_subsets(n1, n2, subsets, subset_size, rng_seed=2020):
    """The row indices of KID's subsets, two int64 arrays [subsets, subset_size]: from ONE np.random.RandomState(rng_seed), per subset
    choice(n1, m, replace=False), then choice(n2, m, replace=False)."""
    rng = np.random.RandomState(rng_seed)
    i1, i2 = np.empty((subsets, subset_size), np.int64), np.empty((subsets, subset_size), np.int64)
    for s in range(subsets):
        i1[s] = rng.choice(n1, subset_size, replace=False)
        i2[s] = rng.choice(n2, subset_size, replace=False)
    return i1, i2


def mmd2_subsets(f1, f2, i1, i2, *, degree=3, gamma=None, coef0=1.0, symmetric=True):
    """[S, 4] float64 on the host: per subset the sums of K_XX and K_YY without their diagonals, the sum of K_XY, and mmd2
    (FridoMmdFinish).  i1, i2: integer arrays [S, m] of rows of f1 / f2.  Three launches of frido_rows_dot in its SUM_POLY mode -- one per
    Gram kind, all subsets in each -- and the finish; `symmetric` computes the upper tile triangle of K_XX and K_YY only."""
    what = "kernel_inception_distance"
    f1, f2 = _rows2d(what, "f1", _bank_rows(f1)), _rows2d(what, "f2", _bank_rows(f2))
    D = f1.shape[1]
    if f2.shape[1] != D or D % 4 != 0 or D == 0:
        raise ValueError(f"{what}: both sides need rows of one length D, a multiple of 4; got {f1.shape[1]} and {f2.shape[1]}")
    if degree not in (1, 2, 3, 4):
        raise ValueError(f"{what}: degree must lie in 1 .. 4, got {degree!r}")
    i1, i2 = np.asarray(i1), np.asarray(i2)
    if i1.ndim != 2 or i1.shape != i2.shape or 0 in i1.shape or i1.shape[1] < 2:
        raise ValueError(f"{what}: the index lists must be two [S, m] arrays with m >= 2, got {i1.shape} and {i2.shape}")
    if i1.min() < 0 or i1.max() >= f1.shape[0] or i2.min() < 0 or i2.max() >= f2.shape[0]:
        raise ValueError(f"{what}: an index lies outside its side's {f1.shape[0]} / {f2.shape[0]} rows")
    dev = _gpu(what, f1, f2)
    S, m = i1.shape
    gamma = 1.0 / D if gamma is None else float(gamma)
    x, y = f1.detach().contiguous(), f2.detach().contiguous()
    ix, iy = (torch.from_numpy(np.ascontiguousarray(i.astype(np.int32))).to(dev) for i in (i1, i2))
    t_sym, t_full = tiles(m, symmetric=symmetric), tiles(m)
    work = torch.empty(S * (2 * t_sym + t_full) + 1, dtype=torch.float64, device=dev)
    pxx, pyy, pxy = work[:S * t_sym], work[S * t_sym:2 * S * t_sym], work[2 * S * t_sym:][:S * t_full]
    out = torch.empty(S, 4, dtype=torch.float64, device=dev)
    kw = dict(mode=SUM_POLY, S=S, m=m, degree=degree, gamma=gamma, coef0=float(coef0))
    sp = _stream(dev)
    for a, b, ia, ib, part, same in ((x, x, ix, ix, pxx, True), (y, y, iy, iy, pyy, True), (x, y, ix, iy, pxy, False)):
        launch("frido_rows_dot", rows_dot_desc(a.data_ptr(), b.data_ptr(), a.shape[0], b.shape[0], D, partials=part.data_ptr(),
                                               ix=ia.data_ptr(), iy=ib.data_ptr(), exclude_diag=same, symmetric=same and symmetric, **kw), sp)
    launch("frido_mmd_finish", mmd_finish_desc(pxx.data_ptr(), pyy.data_ptr(), pxy.data_ptr(), out.data_ptr(), S, m, t_sym, t_sym, t_full), sp)
    for t in (x, y):
        t.record_stream(torch.cuda.current_stream(dev))
    return out.cpu().numpy()


def kernel_inception_distance(f1, f2, *, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, rng_seed=2020):
    """(mean, std) of the Kernel Inception Distance over `subsets` subsets, two floats.  f1, f2: float32 [n1, D], [n2, D] features on
    the GPU (or FeatureBanks).  THE FORMULAS HERE ARE THE SPECIFICATION (torch-fidelity's estimator and defaults, restated; the package
    is not installed to pin them against):
        k(x, y) = (gamma x . y + coef0) ** degree,   gamma = 1 / D when None
        per subset, from ONE np.random.RandomState(rng_seed): X = f1[choice(n1, m, replace=False)], then Y = f2[choice(n2, m,
        replace=False)], m = subset_size;
        mmd2 = (sum_{a != b} k(X_a, X_b) + sum_{a != b} k(Y_a, Y_b)) / (m (m - 1)) - 2 sum_{a, b} k(X_a, Y_b) / m^2
    the unbiased estimate, all dot products and sums in float64 on the device (csrc/fidelity.hip: one launch per Gram kind over all
    subsets, and the finish); mean and std = np.mean, np.std (ddof 0) of the subsets' mmd2.
    Refused: tensors that are no 2-D float32, D % 4 != 0, subset_size above either sample count or below 2, degree outside 1 .. 4
    (ValueError); CPU tensors (FridoHipError)."""
    what = "kernel_inception_distance"
    f1, f2 = _rows2d(what, "f1", _bank_rows(f1)), _rows2d(what, "f2", _bank_rows(f2))
    if not isinstance(subset_size, int) or subset_size < 2 or subset_size > min(f1.shape[0], f2.shape[0]):
        raise ValueError(f"{what}: subset_size={subset_size!r} must lie in 2 .. the smaller sample count ({f1.shape[0]}, {f2.shape[0]})")
    if not isinstance(subsets, int) or subsets < 1:
        raise ValueError(f"{what}: subsets must be a positive integer, got {subsets!r}")
    if degree not in (1, 2, 3, 4):
        raise ValueError(f"{what}: degree must lie in 1 .. 4, got {degree!r}")
    if f1.shape[1] != f2.shape[1] or f1.shape[1] % 4 != 0:
        raise ValueError(f"{what}: both sides need rows of one length D, a multiple of 4; got {f1.shape[1]} and {f2.shape[1]}")
    _gpu(what, f1, f2)
    i1, i2 = kid_subsets(f1.shape[0], f2.shape[0], subsets, subset_size, rng_seed)
    mmd2 = mmd2_subsets(f1, f2, i1, i2, degree=degree, gamma=gamma, coef0=coef0)[:, 3]
    return float(np.mean(mmd2)), float(np.std(mmd2))

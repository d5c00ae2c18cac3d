"""Improved precision and recall, density and coverage on the HIP engine: the ctypes binding of include/frido_manifold.h
(csrc/manifold.hip: row norms, the k-th nearest neighbour of every row, the two ball-membership scans), row_sqnorms, sqdist, knn_radii2
and prdc.

Bound beside `_lib`, not inside it, like frido_amd/fidelity.py: the four launches are no op kinds.  The descriptors are parsed from
their own header with `_lib`'s parser, the functions are taken from the handle `_lib.lib()` returns for the active plane format (the
code is the same in both builds: f32 / f64 / integers only), and every descriptor's size is compared with the library's at first use.
A library without the symbols is a stale build and is named as one: there is no fallback.

The dot products stay where they are: fidelity's frido_rows_dot in its STORE_F64 mode fills a reused SLAB [rows][ldo] of float64 with
`rows` rows of one side against ALL rows of the other, and the scans of this file read it.  A whole prdc is three passes of
frido_rows_dot (R x R, G x G, G x R): the cross matrix is computed once, precision and density come from its rows, recall and coverage
from its columns.

The estimators are those of Kynkaanniemi et al. 2019 (torch-fidelity's `--prc`, the ADM evaluator) and Naeem et al. 2020 (`prdc`),
written from their published descriptions: none of the packages is installed to pin them against, so the formulas in
include/frido_manifold.h and in prdc's docstring ARE the specification here.  tests/manifold_ref.py restates them in float64 numpy."""
import ctypes as C
import os
import re

import torch

from . import _lib, fidelity
from ._lib import FridoHipError
from .fidelity import _bank_rows, _gpu, _rows2d, _stream

HEADER = os.path.join(_lib.REPO, "include", "frido_manifold.h")
_text = open(HEADER).read()
_src = _lib._strip_comments(_text)
_structs = _lib._parse_structs(_src)
FridoRowSqnorm = type("FridoRowSqnorm", (C.Structure,), {"_fields_": _structs["FridoRowSqnorm"]})
FridoKnnSelect = type("FridoKnnSelect", (C.Structure,), {"_fields_": _structs["FridoKnnSelect"]})
FridoBallRows = type("FridoBallRows", (C.Structure,), {"_fields_": _structs["FridoBallRows"]})
FridoBallCols = type("FridoBallCols", (C.Structure,), {"_fields_": _structs["FridoBallCols"]})

# launcher -> (descriptor, the library's sizeof function)
LAUNCHERS = {"frido_row_sqnorm": (FridoRowSqnorm, "frido_sizeof_row_sqnorm"), "frido_knn_select": (FridoKnnSelect, "frido_sizeof_knn_select"),
             "frido_ball_rows": (FridoBallRows, "frido_sizeof_ball_rows"), "frido_ball_cols": (FridoBallCols, "frido_sizeof_ball_cols")}

MAX_K = int(re.search(r"#define\s+FRIDO_MANIFOLD_MAX_K\s+(\d+)", _src).group(1))            # the largest neighbourhood
GRID_CAP = int(re.search(r"#define\s+FRIDO_MANIFOLD_GRID_CAP\s+(\d+)", _src).group(1))      # workgroups of one launch at the most
SLAB_BYTES = 512 << 20                                                                      # the default slab

_bound = {}      # plane format -> {launcher name: function of that build}


def _fns(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        fns = {}
        for name, (struct, sizeof) in LAUNCHERS.items():
            for sym in (name, sizeof):
                if not hasattr(L, sym):
                    raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {sym}: a stale build from before csrc/manifold.hip "
                                        "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
            c_sz = getattr(L, sizeof)()
            if c_sz != C.sizeof(struct):
                raise FridoHipError(f"ABI mismatch: sizeof({struct.__name__}) C={c_sz} py={C.sizeof(struct)} "
                                    "(include/frido_manifold.h and the build disagree: stale build?)")
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


def row_sqnorm_desc(x, out, n, D):
    return FridoRowSqnorm(x=x, out=out, n=n, D=D)


def knn_select_desc(slab, nrow, ncol, rad2, rows, ny, ldo, K):
    return FridoKnnSelect(slab=slab, nrow=nrow, ncol=ncol, rad2=rad2, rows=rows, ny=ny, ldo=ldo, K=K)


def ball_rows_desc(slab, nrow, ncol, rad2_col, cnt, rows, ny, ldo):
    return FridoBallRows(slab=slab, nrow=nrow, ncol=ncol, rad2_col=rad2_col, cnt=cnt, rows=rows, ny=ny, ldo=ldo)


def ball_cols_desc(slab, nrow, ncol, rad2_row, cnt_col, dmin_col, rows, ny, ldo):
    return FridoBallCols(slab=slab, nrow=nrow, ncol=ncol, rad2_row=rad2_row, cnt_col=cnt_col, dmin_col=dmin_col, rows=rows, ny=ny, ldo=ldo)


# ---- checks ---------------------------------------------------------------------------------------------
def _side(what, name, t, D=None):
    """The rows of one side, contiguous: a 2-D float32 tensor (or a FeatureBank's rows) of width D, a positive multiple of 4."""
    t = _rows2d(what, name, _bank_rows(t), D)
    if t.shape[1] % 4 != 0 or t.shape[1] == 0:
        raise ValueError(f"{what}: the row length D must be a positive multiple of 4, got {t.shape[1]}")
    return t.detach().contiguous()


def _neighbourhood(what, k, **counts):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k must be an integer in 1 .. {MAX_K} (FRIDO_MANIFOLD_MAX_K), got {k!r}")
    for name, n in counts.items():
        if n < k + 1:
            raise ValueError(f"{what}: {name} has {n} rows, fewer than k + 1 = {k + 1}: the k-th nearest other row does not exist")


def _finite(what, name, t):
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: {name} holds a non-finite feature (NaN or inf): a selection over NaN has no defined order")


def _slab_rows(what, nx, ldo, slab_bytes, slab_rows):
    """Rows of one slab: `slab_rows` when given, else what fits into `slab_bytes`; at least 1, at most nx."""
    if slab_rows is not None:
        if not isinstance(slab_rows, int) or isinstance(slab_rows, bool) or slab_rows < 1:
            raise ValueError(f"{what}: slab_rows must be a positive integer, got {slab_rows!r}")
        return min(slab_rows, nx)
    if not isinstance(slab_bytes, int) or isinstance(slab_bytes, bool) or slab_bytes < 1:
        raise ValueError(f"{what}: slab_bytes must be a positive integer, got {slab_bytes!r}")
    return max(1, min(nx, slab_bytes // (8 * ldo)))


def _slabs(what, x, y, dev, slab_bytes, slab_rows):
    """Yields (a0, rows, slab, ldo): slab [rows][ldo] float64 = the dots of x[a0:a0 + rows] against all of y, one launch of
    frido_rows_dot (STORE_F64) each, into ONE buffer: the caller's scans of a slab are enqueued before the next one overwrites it."""
    nx, ny, D = x.shape[0], y.shape[0], x.shape[1]
    ldo = (ny + 1) // 2 * 2
    step = _slab_rows(what, nx, ldo, slab_bytes, slab_rows)
    slab = torch.empty(step * ldo, dtype=torch.float64, device=dev)
    sp = _stream(dev)
    for a0 in range(0, nx, step):
        rows = min(step, nx - a0)
        fidelity.launch("frido_rows_dot", fidelity.rows_dot_desc(x.data_ptr() + a0 * D * 4, y.data_ptr(), rows, ny, D, mode=fidelity.STORE_F64,
                                                                 out=slab.data_ptr(), ldo=ldo), sp)
        yield a0, rows, slab, ldo


def _record(dev, *tensors):
    for t in tensors:
        t.record_stream(torch.cuda.current_stream(dev))


def _sqnorms(x, dev):
    out = torch.empty(x.shape[0], dtype=torch.float64, device=dev)
    launch("frido_row_sqnorm", row_sqnorm_desc(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1]), _stream(dev))
    _record(dev, x)
    return out


def _radii2(what, x, nx, k, dev, slab_bytes, slab_rows):
    rad2 = torch.empty(x.shape[0], dtype=torch.float64, device=dev)
    for a0, rows, slab, ldo in _slabs(what, x, x, dev, slab_bytes, slab_rows):
        launch("frido_knn_select", knn_select_desc(slab.data_ptr(), nx.data_ptr() + 8 * a0, nx.data_ptr(), rad2.data_ptr() + 8 * a0, rows,
                                                   x.shape[0], ldo, k + 1), _stream(dev))
        _record(dev, slab)
    _record(dev, x, nx)
    return rad2


# ---- the public pieces ----------------------------------------------------------------------------------
@torch.no_grad()
def row_sqnorms(x):
    """n(X_a) = X_a . X_a in float64, [n]: the in-order fma chain of frido_rows_dot, so bit for bit the diagonal of
    fidelity.rows_dot(x, x).  One launch of frido_row_sqnorm."""
    what = "row_sqnorms"
    x = _side(what, "x", x)
    if x.shape[0] == 0:
        raise ValueError(f"{what}: no rows: x {tuple(x.shape)}")
    return _sqnorms(x, _gpu(what, x))


@torch.no_grad()
def sqdist(x, y):
    """d2(X_a, Y_b) = max((n(X_a) + n(Y_b)) - 2 X_a . Y_b, 0) in float64, [nx, ny], every operation rounded on its own: the definition
    the scans use, as a matrix, for tests and small inputs.  One launch of frido_rows_dot, two of frido_row_sqnorm; the combination
    is torch's."""
    what = "sqdist"
    x = _side(what, "x", x)
    y = _side(what, "y", y, x.shape[1])
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError(f"{what}: no rows: x {tuple(x.shape)}, y {tuple(y.shape)}")
    dev = _gpu(what, x, y)
    dot = fidelity.rows_dot(x, y, mode=fidelity.STORE_F64)
    return ((_sqnorms(x, dev)[:, None] + _sqnorms(y, dev)[None, :]) - 2.0 * dot).clamp_min_(0.0)


@torch.no_grad()
def knn_radii2(x, k=3, *, slab_bytes=SLAB_BYTES, slab_rows=None):
    """rad2[a] = the (k + 1)-th smallest, with multiplicity, of { d2(X_a, X_b) : all b }, float64 [n]: the row itself is in the set, so
    without duplicates the squared distance to the k-th nearest other row (torch's kthvalue(k + 1)).  Per slab one launch of
    frido_rows_dot and one of frido_knn_select.  Refusals as prdc's."""
    what = "knn_radii2"
    x = _side(what, "x", x)
    _neighbourhood(what, k, x=x.shape[0])
    _finite(what, "x", x)
    dev = _gpu(what, x)
    return _radii2(what, x, _sqnorms(x, dev), k, dev, slab_bytes, slab_rows)


@torch.no_grad()
def ball_scans(fake, real, rad2_real, rad2_fake, *, slab_bytes=SLAB_BYTES, slab_rows=None):
    """The two scans of the cross matrix d2(G_j, R_i), computed once, slab by slab over the generated rows:
        cnt [M] int32       cnt[j] = #{ i : d2(G_j, R_i) <= rad2_real[i] }                  (frido_ball_rows)
        cnt_col [N] int32   cnt_col[i] = #{ j : d2(G_j, R_i) <= rad2_fake[j] }              (frido_ball_cols, carried across the slabs)
        dmin_col [N] f64    dmin_col[i] = min_j d2(G_j, R_i)                                (frido_ball_cols, likewise)
    on the device."""
    what = "ball_scans"
    g = _side(what, "fake", fake)
    r = _side(what, "real", real, g.shape[1])
    M, N = g.shape[0], r.shape[0]
    for name, t, n in (("rad2_real", rad2_real, N), ("rad2_fake", rad2_fake, M)):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != (n,) or t.device != g.device:
            raise ValueError(f"{what}: {name} must be a float64 [{n}] tensor on {g.device}")
    if M == 0 or N == 0:
        raise ValueError(f"{what}: no rows: fake {tuple(g.shape)}, real {tuple(r.shape)}")
    dev = _gpu(what, g, r)
    return _scans(what, g, r, _sqnorms(g, dev), _sqnorms(r, dev), rad2_real.contiguous(), rad2_fake.contiguous(), dev, slab_bytes, slab_rows)


def _scans(what, g, r, ng, nr, rr, rg, dev, slab_bytes, slab_rows):
    M, N = g.shape[0], r.shape[0]
    cnt = torch.empty(M, dtype=torch.int32, device=dev)
    cnt_col = torch.zeros(N, dtype=torch.int32, device=dev)
    dmin_col = torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
    sp = _stream(dev)
    for a0, rows, slab, ldo in _slabs(what, g, r, dev, slab_bytes, slab_rows):
        launch("frido_ball_rows", ball_rows_desc(slab.data_ptr(), ng.data_ptr() + 8 * a0, nr.data_ptr(), rr.data_ptr(), cnt.data_ptr() + 4 * a0,
                                                 rows, N, ldo), sp)
        launch("frido_ball_cols", ball_cols_desc(slab.data_ptr(), ng.data_ptr() + 8 * a0, nr.data_ptr(), rg.data_ptr() + 8 * a0,
                                                 cnt_col.data_ptr(), dmin_col.data_ptr(), rows, N, ldo), sp)
        _record(dev, slab)
    _record(dev, g, r, rr, rg, ng, nr)
    return cnt, cnt_col, dmin_col


@torch.no_grad()
def prdc(real, fake, k=3, *, slab_bytes=SLAB_BYTES, slab_rows=None):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) between real features R
    [N, D] and generated features G [M, D], float32 on the GPU (or FeatureBanks).  THE FORMULAS HERE ARE THE SPECIFICATION
    (torch-fidelity's `--prc` and `prdc`, restated; neither package is installed to pin them against).  Everything is done on SQUARED
    distances in float64, no square root anywhere:
        dot(x, y) = fma((double)x[j], (double)y[j], dot) for j ascending from 0.0 (frido_rows_dot's);  n(x) = dot(x, x)
        d2(x, y)  = max((n(x) + n(y)) - 2.0 * dot(x, y), 0.0), every operation rounded on its own
        rad2_X[a] = the (k + 1)-th smallest, WITH multiplicity, of { d2(X_a, X_b) : all b, b = a included }
        precision = #{ j : exists i, d2(G_j, R_i) <= rad2_R[i] } / M        recall   = #{ i : exists j, d2(G_j, R_i) <= rad2_G[j] } / N
        density   = (sum_j #{ i : d2(G_j, R_i) <= rad2_R[i] }) / (k M)      coverage = #{ i : min_j d2(G_j, R_i) <= rad2_R[i] } / N
        f_score   = 2 P R / (P + R), and 0.0 when P + R == 0
    k = 3 is torch-fidelity's neighbourhood (prdc's customary value is 5).  The counts are integers, reduced on the device by torch;
    each quotient is taken once, in Python float64.  Three passes of frido_rows_dot (R x R, G x G, G x R) through a reused slab of
    `slab_bytes` (or of `slab_rows` rows), scanned by csrc/manifold.hip.
    Returns {"precision", "recall", "density", "coverage", "f_score": floats, "counts": {"precision", "recall", "density", "coverage",
    "n_real", "n_fake", "k": ints}}.
    Refused: k outside 1 .. 15, N < k + 1 or M < k + 1, rows that are not 2-D float32 of one width, D % 4 != 0, a non-finite feature
    (ValueError); CPU tensors (FridoHipError)."""
    what = "prdc"
    r = _side(what, "real", real)
    g = _side(what, "fake", fake, r.shape[1])
    _neighbourhood(what, k, real=r.shape[0], fake=g.shape[0])
    _finite(what, "real", r)
    _finite(what, "fake", g)
    dev = _gpu(what, r, g)
    N, M = r.shape[0], g.shape[0]
    nr, ng = _sqnorms(r, dev), _sqnorms(g, dev)
    rad2_r = _radii2(what, r, nr, k, dev, slab_bytes, slab_rows)
    rad2_g = _radii2(what, g, ng, k, dev, slab_bytes, slab_rows)
    cnt, cnt_col, dmin_col = _scans(what, g, r, ng, nr, rad2_r, rad2_g, dev, slab_bytes, slab_rows)
    counts = torch.stack([(cnt > 0).sum(), cnt.sum(dtype=torch.int64), (cnt_col > 0).sum(), (dmin_col <= rad2_r).sum()]).cpu().tolist()
    c = dict(precision=int(counts[0]), density=int(counts[1]), recall=int(counts[2]), coverage=int(counts[3]), n_real=N, n_fake=M, k=k)
    P, R = c["precision"] / M, c["recall"] / N
    return dict(precision=P, recall=R, density=c["density"] / (k * M), coverage=c["coverage"] / N,
                f_score=2.0 * P * R / (P + R) if P + R > 0 else 0.0, counts=c)

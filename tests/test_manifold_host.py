"""Host side of improved precision and recall and of density and coverage (frido_amd/manifold.py, pipeline.precision_recall,
tools/fid_npy.py --prc): the float64 restatement of tests/manifold_ref.py against independent code, its closed forms, the conditions
the shared fixtures must meet (checked on the restatement alone), the refusals and the ABI constraints.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import manifold_ref as MR
from frido_amd import _lib, manifold
from frido_amd._lib import FridoHipError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
FOUR = ("precision", "recall", "density", "coverage")


# ---- the restatement against independent code ----------------------------------------------------------------
def test_in_order_loops_are_what_they_say():
    R, G = MR.real_case(70, 133, 8)
    x, y = R[:5], G[:3]
    d, n = MR.dot_in_order(x, y), MR.sqnorms(x)
    for a in range(5):
        acc = 0.0
        for j in range(8):
            acc = acc + float(x[a, j]) * float(x[a, j])                       # python floats: one rounding per add, the product exact
        assert n[a] == acc
        for b in range(3):
            acc = 0.0
            for j in range(8):
                acc = acc + float(x[a, j]) * float(y[b, j])
            assert d[a, b] == acc
            assert MR.d2(x, y)[a, b] == max((n[a] + MR.sqnorms(y)[b]) - 2.0 * d[a, b], 0.0)
    assert np.array_equal(n, np.diagonal(MR.dot_in_order(x, x)))              # the norm IS the diagonal of the Gram matrix


@pytest.mark.parametrize("N,M,D,k", MR.REAL_CASES)
def test_distances_against_scipy_and_radii_against_sklearn(N, M, D, k):
    """d2 against scipy's cdist(..., 'sqeuclidean'), which sums the squared differences directly.  Ours is a difference of sums of D
    products each, so its ABSOLUTE error is bounded by about (D + 2) 2^-53 (n(x) + n(y)); cdist's own is D 2^-53 d2 <= that.  Margin:
    4 x.  The radii against sklearn's brute-force neighbours (Euclidean distances, squared here: a square root and a square add two
    roundings), same bound, and -- there being no ties -- the same neighbour."""
    from scipy.spatial.distance import cdist
    from sklearn.neighbors import NearestNeighbors
    R, G = MR.real_case(N, M, D)
    ours = MR.d2(G, R)
    ref = cdist(G.astype(np.float64), R.astype(np.float64), "sqeuclidean")
    bound = 4 * (D + 2) * U * (MR.sqnorms(G)[:, None] + MR.sqnorms(R)[None, :])
    ratio = float((np.abs(ours - ref) / bound).max())
    print(f"d2 against cdist at {(N, M, D)}: largest |difference| / bound {ratio:.3f}")
    assert ratio <= 1.0
    for x in (R, G):
        dist, idx = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x.astype(np.float64)).kneighbors(x.astype(np.float64))
        d = MR.d2(x, x)
        assert len(np.unique(d)) > d.size // 2 - len(x)                       # no ties beside the symmetric pairs and the diagonal
        ours = MR.radii2(x, k)
        n = MR.sqnorms(x)
        assert bool((np.abs(ours - dist[:, k] ** 2) <= 4 * (D + 4) * U * 2 * n.max()).all())
        assert np.array_equal(np.argsort(d, axis=1, kind="stable")[:, k], idx[:, k])
        assert bool((ours > 0).all()) and np.array_equal(ours, torch.from_numpy(d).kthvalue(k + 1, dim=1).values.numpy())


def test_closed_forms():
    R, G = MR.real_case(150, 97, 36)
    same = MR.prdc(R, R.copy(), 3)
    assert same["precision"] == same["recall"] == same["coverage"] == same["f_score"] == 1.0 and same["density"] >= 4.0 / 3.0
    near, far = R[:80] * np.float32(0.01), R[:60] * np.float32(0.01) + np.float32(100.0)      # diameters below 1, 600 apart
    apart = MR.prdc(near, far, 3)
    assert [apart[n] for n in FOUR] == [0.0] * 4 and apart["f_score"] == 0.0 and set(apart["counts"].values()) == {0}
    r = MR.prdc(R, G, 3)
    assert r["f_score"] == 2.0 * r["precision"] * r["recall"] / (r["precision"] + r["recall"])
    assert r["density"] == r["counts"]["density"] / (3 * 97) and r["coverage"] == r["counts"]["coverage"] / 150


# ---- the fixture conditions, on the restatement alone ---------------------------------------------------------
@pytest.mark.parametrize("case", MR.REAL_CASES)
def test_real_valued_cases_are_not_saturated(case):
    r = MR.reference(case)
    print(f"{case}: " + " / ".join(f"{r[n]:.3f}" for n in ("precision", "recall", "coverage")))
    for n in ("precision", "recall", "coverage"):
        assert 0.05 <= r[n] <= 0.95, (case, n, r[n])
    assert MR.reference(case, "lt")["counts"] == r["counts"]                  # real-valued rows cannot tell < from <=: hence the tie fixture


def test_saturated_case_is_kept_out_of_the_metric_conditions():
    assert MR.reference(MR.SATURATED_CASE)["coverage"] == 1.0 and MR.SATURATED_CASE not in MR.REAL_CASES


def test_tie_fixture_has_genuine_ties():
    R, G = MR.tie_fixture()
    assert (R.shape, G.shape) == ((150, 8), (97, 8)) and MR.TIE_CASE == (150, 97, 8, 3)
    assert np.array_equal(R * 2, np.round(R * 2)) and np.array_equal(G * 2, np.round(G * 2))      # half-integer values
    assert np.array_equal(R[10], R[3]) and np.array_equal(R[11], R[3]) and np.array_equal(G[5], R[7]) and np.array_equal(G[6], G[2])
    d = MR.d2(G, R)
    assert np.array_equal(d * 4, np.round(d * 4)) and len(np.unique(d)) <= 4 * d.max() + 1 < d.size // 20 and d[5, 7] == 0.0      # multiples of 0.25
    right, lt, kth = MR.reference("tie"), MR.reference("tie", "lt"), MR.reference("tie", "kth")
    print("tie fixture: " + ", ".join(f"{n} {right[n]:.3f} -> {lt[n]:.3f} with <, {kth[n]:.3f} with the self left out" for n in FOUR))
    for n in FOUR:
        assert lt[n] < right[n] and kth[n] < right[n], n
        assert 0.05 <= right[n] <= (0.95 if n != "density" else 2.0)


@pytest.mark.parametrize("variant", MR.VARIANTS)
def test_every_wrong_variant_moves_an_integer_count(variant):
    moved = [name for name in MR.REAL_CASES + ["tie", "near"] if MR.reference(name, variant)["counts"] != MR.reference(name)["counts"]]
    print(f"variant {variant}: differs on {moved}")
    assert moved, variant
    if variant == "no_clamp":
        assert "near" in moved
    if variant == "lt":
        assert "tie" in moved and not set(moved) & set(MR.REAL_CASES)         # only fixtures with equal distances can tell


def test_near_duplicate_fixture():
    x = MR.near_duplicate_fixture()
    assert x.shape == (128, 2048) and int((x[1] != x[0]).sum()) == 1
    j = int(np.argmax(x[1] != x[0]))
    assert x[1, j] == np.nextafter(x[0, j], np.float32(np.inf))               # one ulp in one coordinate
    raw, d = MR.d2(x, x, clamp=False), MR.d2(x, x)
    print(f"near-duplicate fixture: {int((raw < 0).sum())} negative entries before the clamp, down to {raw.min():.3e}")
    assert (raw < 0).sum() >= 20 and raw.min() > -1e-10 and d.min() == 0.0
    assert bool((np.diagonal(raw) == 0.0).all())                              # d2(x, x) == 0 exactly, clamp or not
    assert np.array_equal(d, d.T) and np.array_equal(raw, raw.T)              # bitwise symmetric


# ---- refusals -------------------------------------------------------------------------------------------------
def test_refusals():
    from frido_amd import fidelity, pipeline
    a, b = torch.zeros(20, 12), torch.zeros(9, 12)
    for k in (0, 16, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="k must be an integer in 1 .. 15"):
            manifold.prdc(a, b, k)
        with pytest.raises(ValueError, match="k must be an integer in 1 .. 15"):
            manifold.knn_radii2(a, k)
    assert manifold.MAX_K == 15
    with pytest.raises(ValueError, match="fake has 9 rows, fewer than k \\+ 1 = 10"):
        manifold.prdc(a, b, 9)
    with pytest.raises(ValueError, match="real has 9 rows"):
        manifold.prdc(b, a, 9)
    with pytest.raises(ValueError, match="fewer than k \\+ 1"):
        manifold.knn_radii2(torch.zeros(3, 4), 3)
    with pytest.raises(ValueError, match="fewer than k \\+ 1"):
        pipeline.precision_recall(fidelity.FeatureBank(12, "cpu").append(a[:3]), fidelity.FeatureBank(12, "cpu").append(a))
    for bad in (torch.zeros(20), torch.zeros(2, 3, 4), torch.zeros(20, 12, dtype=torch.float64), "x", None):
        for call in (lambda: manifold.prdc(bad, a), lambda: manifold.prdc(a, bad), lambda: manifold.knn_radii2(bad),
                     lambda: manifold.row_sqnorms(bad), lambda: manifold.sqdist(bad, a), lambda: manifold.sqdist(a, bad)):
            with pytest.raises(ValueError, match="2-D float32"):
                call()
    with pytest.raises(ValueError, match="2-D float32"):                      # two widths
        manifold.prdc(a, torch.zeros(20, 16))
    with pytest.raises(ValueError, match="2-D float32"):
        manifold.sqdist(a, torch.zeros(20, 16))
    for call in (lambda: manifold.prdc(torch.zeros(20, 10), torch.zeros(20, 10)), lambda: manifold.knn_radii2(torch.zeros(20, 6)),
                 lambda: manifold.row_sqnorms(torch.zeros(20, 2)), lambda: manifold.sqdist(torch.zeros(2, 6), torch.zeros(2, 6)),
                 lambda: manifold.row_sqnorms(torch.zeros(20, 0))):
        with pytest.raises(ValueError, match="multiple of 4"):
            call()
    for poison in (float("nan"), float("inf"), float("-inf")):
        bad = a.clone()
        bad[7, 3] = poison
        with pytest.raises(ValueError, match="real holds a non-finite"):
            manifold.prdc(bad, a)
        with pytest.raises(ValueError, match="fake holds a non-finite"):
            manifold.prdc(a, bad)
        with pytest.raises(ValueError, match="non-finite"):
            manifold.knn_radii2(bad)
    with pytest.raises(ValueError, match="slab_rows"):
        manifold._slab_rows("prdc", 10, 10, manifold.SLAB_BYTES, 0)
    with pytest.raises(ValueError, match="slab_bytes"):
        manifold._slab_rows("prdc", 10, 10, 0, None)
    assert manifold._slab_rows("prdc", 50000, 50000, manifold.SLAB_BYTES, None) == 1342      # 512 MiB of rows of 50 000 float64
    assert manifold._slab_rows("prdc", 100, 100, 1, None) == 1 and manifold._slab_rows("prdc", 100, 100, manifold.SLAB_BYTES, 48) == 48
    assert manifold._slab_rows("prdc", 30, 100, manifold.SLAB_BYTES, 48) == 30
    for call in (lambda: manifold.prdc(a, a), lambda: manifold.knn_radii2(a), lambda: manifold.row_sqnorms(a), lambda: manifold.sqdist(a, b),
                 lambda: manifold.ball_scans(b, a, torch.zeros(20, dtype=torch.float64), torch.zeros(9, dtype=torch.float64)),
                 lambda: pipeline.precision_recall(fidelity.FeatureBank(12, "cpu").append(a), fidelity.FeatureBank(12, "cpu").append(b))):
        with pytest.raises(FridoHipError, match="no CPU"):
            call()
    with pytest.raises(ValueError, match="rad2_real"):
        manifold.ball_scans(b, a, torch.zeros(9, dtype=torch.float64), torch.zeros(9, dtype=torch.float64))


def test_public_signatures():
    from frido_amd import pipeline
    sig = inspect.signature(manifold.prdc).parameters
    assert list(sig) == ["real", "fake", "k", "slab_bytes", "slab_rows"]
    assert (sig["k"].default, sig["slab_bytes"].default, sig["slab_rows"].default) == (3, 512 << 20, None)
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("slab_bytes", "slab_rows"))
    sig = inspect.signature(manifold.knn_radii2).parameters
    assert list(sig) == ["x", "k", "slab_bytes", "slab_rows"] and sig["k"].default == 3
    sig = inspect.signature(pipeline.precision_recall).parameters
    assert list(sig) == ["bank_real", "bank_fake", "k", "kw"] and sig["k"].default == 3
    for fn in (manifold.prdc, pipeline.precision_recall):
        assert "nothing about" in " ".join(fn.__doc__.split()) or "SPECIFICATION" in fn.__doc__
    assert "<=" in manifold.prdc.__doc__ and "k + 1" in manifold.prdc.__doc__ and "multiplicity" in manifold.prdc.__doc__


# ---- ABI ------------------------------------------------------------------------------------------------------
def test_descriptors_match_both_builds_and_bad_ones_are_turned_away():
    mf = manifold
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        for name, (struct, sizeof) in mf.LAUNCHERS.items():
            assert getattr(L, sizeof)() == C.sizeof(struct), (planes, name)
        fns = mf._fns(planes)
        assert set(fns) == set(mf.LAUNCHERS)

        def refused(name, desc, words):
            assert fns[name](C.byref(desc), None) == -1 and words in L.frido_last_error(), (name, L.frido_last_error())      # FRIDO_EINVAL
            assert L.frido_last_error().startswith(name.encode() + b": ")

        for name, (struct, _) in mf.LAUNCHERS.items():                       # a zeroed descriptor: null pointers
            refused(name, struct(), name.encode() + b": bad arguments")
        for kw, words in ((dict(D=6), b"D must be a multiple of 4"), (dict(x=base + 4), b"aligned"), (dict(out=base + 4), b"aligned"),
                          (dict(n=0), b"bad arguments"), (dict(D=0), b"bad arguments"), (dict(out=None), b"bad arguments")):
            d = mf.row_sqnorm_desc(base, base, 4, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_row_sqnorm", d, words)
        for kw, words in ((dict(ldo=6), b"ldo must be at least ny"), (dict(ldo=9), b"ldo must be even"), (dict(K=0), b"K must lie in"),
                          (dict(K=17), b"K must lie in"), (dict(K=9), b"K must lie in"), (dict(slab=base + 8), b"aligned"),
                          (dict(ncol=base + 8), b"aligned"), (dict(nrow=base + 4), b"aligned"), (dict(rows=0), b"rows must be positive"),
                          (dict(ny=0), b"rows must be positive"), (dict(rad2=None), b"bad arguments")):
            d = mf.knn_select_desc(base, base, base, base, 4, 8, 8, 4)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_knn_select", d, words)
        for kw, words in ((dict(ldo=7), b"ldo must be at least ny"), (dict(ldo=9), b"ldo must be even"), (dict(rad2_col=base + 8), b"aligned"),
                          (dict(cnt=base + 2), b"aligned"), (dict(slab=base + 8), b"aligned"), (dict(ny=0), b"rows must be positive"),
                          (dict(rows=-1), b"rows must be positive"), (dict(ncol=None), b"bad arguments")):
            d = mf.ball_rows_desc(base, base, base, base, base, 4, 8, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_ball_rows", d, words)
        for kw, words in ((dict(ldo=7), b"ldo must be at least ny"), (dict(cnt_col=base + 2), b"aligned"), (dict(dmin_col=base + 4), b"aligned"),
                          (dict(slab=base + 4), b"aligned"), (dict(rows=0), b"rows must be positive"), (dict(rad2_row=None), b"bad arguments"),
                          (dict(dmin_col=None), b"bad arguments")):
            d = mf.ball_cols_desc(base, base, base, base, base, base, 4, 8, 9)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_ball_cols", d, words)
    assert mf.MAX_K == 15 and mf.GRID_CAP == 1024 and mf.SLAB_BYTES == 512 << 20


def test_header_makefile_and_source_constraints():
    """frido_hip.h (the op-kind ABI), frido_fid.h and frido_fidelity.h do not know the launches; manifold.hip includes launch.h alone
    and sits directly behind fidelity.hip, with vision.hip and lpips.hip still last."""
    from frido_amd import fidelity as fd
    mf = manifold
    for hdr in ("frido_hip.h", "frido_fid.h", "frido_fidelity.h"):
        text = open(os.path.join(REPO, "include", hdr)).read()
        for name in ("frido_manifold", "row_sqnorm", "knn_select", "ball_rows", "ball_cols", "FridoKnn", "FridoBall", "FridoRowSqnorm", "MANIFOLD"):
            assert name not in text, (hdr, name)
    assert _lib.ABI_VERSION == 8 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert not [s for s in _lib.EXPORTS if "sqnorm" in s or "knn" in s or "ball" in s]
    assert not [s for s in _lib.STRUCTS if "Sqnorm" in s or "Knn" in s or "Ball" in s]
    assert set(fd.LAUNCHERS) == {"frido_rows_dot", "frido_mmd_finish", "frido_isc_rowstats", "frido_isc_marginal", "frido_isc_kl", "frido_isc_finish"}
    body = _lib._strip_comments(open(os.path.join(REPO, "include", "frido_manifold.h")).read())
    assert body.split("#include")[1].strip().startswith('"frido_hip.h"') and body.count("#include") == 1
    assert _lib._parse_structs(body).keys() == {"FridoRowSqnorm", "FridoKnnSelect", "FridoBallRows", "FridoBallCols"}
    assert {st for st, _ in mf.LAUNCHERS.values()} == {mf.FridoRowSqnorm, mf.FridoKnnSelect, mf.FridoBallRows, mf.FridoBallCols}
    assert len({sz for _, sz in mf.LAUNCHERS.values()}) == 4                   # one frido_sizeof_* per descriptor
    for sym in list(mf.LAUNCHERS) + [sz for _, sz in mf.LAUNCHERS.values()]:
        assert f"int {sym}(" in body, sym
    head = open(os.path.join(REPO, "include", "frido_manifold.h")).read()
    for words in ("ARE the specification", "fmax((n(x) + n(y)) - 2.0 * dot(x, y), 0.0)", "WITH multiplicity", "The comparison is <=", "kthvalue(k + 1)"):
        assert words in head, words
    mk = open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert srcs[-1] == "lpips.hip" and srcs[-2] == "vision.hip"
    assert srcs[srcs.index("patchgan.hip") + 1] == "fid.hip" and srcs[srcs.index("fid.hip") + 1] == "fidelity.hip"
    assert srcs[srcs.index("fidelity.hip") + 1] == "manifold.hip" and srcs.count("manifold.hip") == 1
    assert "manifold.o obj_bf16p/manifold.o: ../../include/frido_manifold.h" in mk
    assert "-ffp-contract=on" in mk
    src = open(os.path.join(REPO, "frido_amd", "csrc", "manifold.hip")).read()
    assert '#include "launch.h"' in src and '#include "frido_manifold.h"' in src and src.count("#include") == 2 and "common.h" not in src
    low = src.lower()
    for word in ("atomic", "hipmalloc", "hipfree", "synchronize", "status_raise", "frido_x3_f16", "sqrt"):
        assert word not in low, word
    assert "FRIDO_MANIFOLD_GRID_CAP" in src and "FRIDO_MANIFOLD_MAX_K" in src and "fp contract(off)" in src
    assert src.count("__launch_bounds__(256)") == src.count("__global__") == 4
    assert src.count("FRIDO_REQUIRE(d &&") == 4                               # every launcher turns a null descriptor away first
    fsrc = open(os.path.join(REPO, "frido_amd", "csrc", "fidelity.hip")).read()
    assert fsrc.count("__global__") == 6 and "manifold" not in fsrc            # the dot products stay where they are


def test_fid_npy_tool_names_prc(tmp_path):
    """tools/fid_npy.py --help names --prc and --prc-k; with --prc on saved banks and no GPU it names the missing device."""
    from frido_amd import fidelity
    tool = os.path.join(REPO, "tools", "fid_npy.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--prc" in out.stdout and "--prc-k" in out.stdout and "--isc" in out.stdout and "--kid" in out.stdout
    if not torch.cuda.is_available():
        R, _ = MR.real_case(70, 133, 8)
        pa = tmp_path / "a.npz"
        fidelity.FeatureBank(8, "cpu").append(torch.from_numpy(R[:16].copy())).save(str(pa))
        bad = subprocess.run([sys.executable, tool, str(pa), str(pa), "--prc", "--prc-k", "2"], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "HIP device" in bad.stderr

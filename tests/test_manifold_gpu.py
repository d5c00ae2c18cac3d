"""Improved precision and recall, density and coverage on the MI355X (csrc/manifold.hip, frido_amd/manifold.py) against the float64
restatement of tests/manifold_ref.py: frido_row_sqnorm, frido_knn_select, frido_ball_rows and frido_ball_cols launched into guarded
buffers, the public row_sqnorms / sqdist / knn_radii2 / ball_scans / prdc, and pipeline.precision_recall end to end.

There is NO tolerance in this file: every float64 value is defined by value (an in-order fma chain, separately rounded operations, a
selection, a minimum) and every other result is an integer, so all comparisons are bit for bit or integer-equal.  The fixtures and
their references are computed once in manifold_ref and shared read-only."""
import numpy as np
import pytest
import torch

import manifold_ref as MR
from frido_amd import fidelity as fd
from frido_amd import manifold as mf
from frido_amd.engine import require_gpu

pytestmark = pytest.mark.gpu

PAD = 64                    # guard elements behind every kernel output: the kernel must leave them alone
POISON = 1.0e300            # a dot product that makes d2 clamp to 0: a padding column read as a column would be everybody's nearest
IGUARD = -7777              # the guard value of int32 outputs


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, dtype=torch.float64):
    require_gpu("cuda")
    return torch.full((n + PAD,), IGUARD if dtype == torch.int32 else float("nan"), device="cuda", dtype=dtype)


def _take(buf, n, what):
    torch.cuda.synchronize()
    guard, out = buf[n:].cpu(), buf[:n].cpu()
    if buf.dtype == torch.int32:
        assert bool((guard == IGUARD).all()), f"{what} wrote behind its output"
    else:
        assert bool(torch.isnan(guard).all()), f"{what} wrote behind its output"
        assert not bool(torch.isnan(out).any()), f"{what} left output elements unwritten"
    return out.numpy()


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # the fixtures are read-only arrays


def _rows(seed, n, D, scale=1.0, mean=0.0):
    return (np.random.RandomState(seed).standard_normal((n, D)) * scale + mean).astype(np.float32)


def _padded(vec, extra, fill):
    """`vec` with `extra` elements of `fill` behind it: what a kernel reading past ny would find."""
    return _cuda(np.concatenate([np.asarray(vec, np.float64), np.full(extra, fill, np.float64)]))


def _slab(xg, yg, a0, rows, ldo):
    """rows a0 .. a0 + rows - 1 of x against all of y by frido_rows_dot into a slab whose every element was POISON before."""
    ny, D = yg.shape
    slab = torch.full((rows * ldo + PAD,), POISON, dtype=torch.float64, device="cuda")
    fd.launch("frido_rows_dot", fd.rows_dot_desc(xg.data_ptr() + a0 * D * 4, yg.data_ptr(), rows, ny, D, mode=fd.STORE_F64, out=slab.data_ptr(),
                                                 ldo=ldo), _stream())
    return slab


# ---- frido_row_sqnorm ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [pytest.param(5, 4, marks=pytest.mark.gate), (67, 36), (130, 2048)])
def test_row_sqnorms_equal_the_diagonal_of_rows_dot_and_the_host_loop(n, D):
    x = _rows(n * 7 + D, n, D, 1.5, 0.2)
    xg = _cuda(x)
    buf = _out(n)
    mf.launch("frido_row_sqnorm", mf.row_sqnorm_desc(xg.data_ptr(), buf.data_ptr(), n, D), _stream())
    got = _take(buf, n, "frido_row_sqnorm")
    ref = MR.sqnorms(x)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    assert np.array_equal(got, np.diagonal(MR.dot_in_order(x, x)))
    assert np.array_equal(got, fd.rows_dot(xg, xg).diagonal().cpu().numpy())
    pub = mf.row_sqnorms(xg)
    assert pub.dtype == torch.float64 and tuple(pub.shape) == (n,) and np.array_equal(pub.cpu().numpy(), ref)
    assert np.array_equal(mf.row_sqnorms(fd.FeatureBank(D, "cuda").append(xg)).cpu().numpy(), ref)


def test_row_sqnorms_second_trip_of_the_grid():
    """One thread per row and at most GRID_CAP workgroups of 256: GRID_CAP * 256 + 3 rows need the second trip of the grid-stride loop."""
    n, D = mf.GRID_CAP * 256 + 3, 4
    x = _rows(31, n, D)
    xg = _cuda(x)
    buf = _out(n)
    mf.launch("frido_row_sqnorm", mf.row_sqnorm_desc(xg.data_ptr(), buf.data_ptr(), n, D), _stream())
    assert np.array_equal(_take(buf, n, "frido_row_sqnorm"), MR.sqnorms(x))


# ---- sqdist ----------------------------------------------------------------------------------------------
def test_sqdist_equals_the_restatement_bit_for_bit():
    R, G = MR.real_case(150, 97, 36)
    got = mf.sqdist(_cuda(G), _cuda(R))
    assert got.dtype == torch.float64 and tuple(got.shape) == (97, 150)
    assert np.array_equal(got.cpu().numpy(), MR.d2(G, R))
    x = MR.near_duplicate_fixture()
    got = mf.sqdist(_cuda(x), _cuda(x)).cpu().numpy()
    raw = MR.d2(x, x, clamp=False)
    assert (raw < 0).sum() >= 20                                             # the fixture does need the clamp
    assert np.array_equal(got, MR.d2(x, x)) and not np.array_equal(got, raw)
    assert bool((np.diagonal(got) == 0.0).all()) and np.array_equal(got, got.T) and got.min() == 0.0


# ---- frido_knn_select ------------------------------------------------------------------------------------
def _zero_set():
    """40 rows of 8 whose first 20 are one and the same row: for those the k + 1 <= 16 smallest distances are all zero."""
    x = _rows(408, 40, 8)
    x[:20] = x[0]
    return x


# 643 columns: 321 pairs, so every lane takes one batched trip of four loads, some a single trip behind it, lane 0 the odd last column
WIDE_CASE = (643, 70, 8, 3)
RADII_SETS = {"5x4": lambda: _rows(54, 5, 4), "64x32": lambda: _rows(6432, 64, 32), "65x32": lambda: MR.real_case(*MR.SATURATED_CASE[:3])[0],
              "150x36": lambda: MR.real_case(150, 97, 36)[0], "200x100": lambda: MR.real_case(200, 130, 100)[0],
              "tie-real": lambda: MR.tie_fixture()[0], "tie-fake": lambda: MR.tie_fixture()[1], "zeros": _zero_set,
              "near": lambda: MR.near_duplicate_fixture(), "643x8": lambda: MR.real_case(*WIDE_CASE[:3])[0]}


@pytest.mark.parametrize("name", [pytest.param("5x4", marks=pytest.mark.gate)] + [n for n in RADII_SETS if n != "5x4"])
def test_knn_radii_equal_the_sorted_restatement_with_ties(name):
    x = RADII_SETS[name]()
    n, D = x.shape
    xg = _cuda(x)
    d = MR.d2(x, x)
    srt = np.sort(d, axis=1)
    nx = _padded(MR.sqnorms(x), 4, 0.0)
    ks = [k for k in (1, 3, 7, 15) if n >= k + 1]
    assert ks
    for k in ks:
        want = srt[:, k]
        assert np.array_equal(want, MR.radii2(x, k))
        # the launcher itself: one slab with padding columns full of POISON, and the column norms followed by zeros
        ldo = (n + 1) // 2 * 2 + 2
        slab = _slab(xg, xg, 0, n, ldo)
        buf = _out(n)
        mf.launch("frido_knn_select", mf.knn_select_desc(slab.data_ptr(), nx.data_ptr(), nx.data_ptr(), buf.data_ptr(), n, n, ldo, k + 1), _stream())
        got = _take(buf, n, "frido_knn_select")
        assert np.array_equal(got, want), (name, k, int((got != want).sum()))
        # the public call: one slab, slabs of 48 rows, slabs of 1 row -- the same bits
        for kw in ({}, dict(slab_rows=48), dict(slab_bytes=1)):
            pub = mf.knn_radii2(xg, k, **kw)
            assert pub.dtype == torch.float64 and np.array_equal(pub.cpu().numpy(), want), (name, k, kw)
    if name == "zeros":
        assert bool((srt[:20, 15] == 0.0).all()) and bool((srt[20:, 1] > 0.0).all())
    if name.startswith("tie"):
        assert len(np.unique(d)) <= 4 * d.max() + 1 < d.size // 20                # genuine ties: multiples of 0.25, few distinct values


# ---- frido_ball_rows / frido_ball_cols -------------------------------------------------------------------
# name of the fixture, swapped: with `swapped` the two sides change roles, which makes the column count ny ragged (97, 133)
SCAN_CASES = [pytest.param((150, 97, 36, 3), True, marks=pytest.mark.gate), ((70, 133, 8, 1), True), ((150, 97, 36, 3), False),
              ((70, 133, 8, 1), False), ((200, 130, 100, 5), False), (WIDE_CASE, False), (MR.SATURATED_CASE, False), ("tie", False), ("tie", True), ("near", False)]


def _scan_sides(name, swapped):
    R, G, k = MR.sides(name)
    return (G, R, k) if swapped else (R, G, k)


@pytest.mark.parametrize("name,swapped", SCAN_CASES)
def test_ball_scans_equal_the_restatement_count_for_count(name, swapped):
    R, G, k = _scan_sides(name, swapped)
    N, M = R.shape[0], G.shape[0]
    ref = MR.scans(R, G, k)
    rg_, gg_ = _cuda(R), _cuda(G)
    # the public call, one slab and several: cnt_col and dmin_col are carried across the slabs
    rr, rg = mf.knn_radii2(rg_, k), mf.knn_radii2(gg_, k)
    assert np.array_equal(rr.cpu().numpy(), ref["rad2_real"]) and np.array_equal(rg.cpu().numpy(), ref["rad2_fake"])
    for slab_rows in (32, 48, None):
        cnt, cnt_col, dmin_col = mf.ball_scans(gg_, rg_, rr, rg, slab_rows=slab_rows)
        assert cnt.dtype == cnt_col.dtype == torch.int32 and dmin_col.dtype == torch.float64
        assert np.array_equal(cnt.cpu().numpy(), ref["cnt"]), (name, slab_rows)
        assert np.array_equal(cnt_col.cpu().numpy(), ref["cnt_col"]), (name, slab_rows)
        assert np.array_equal(dmin_col.cpu().numpy(), ref["dmin_col"]), (name, slab_rows)
    # the launchers themselves, two slabs (rows 0 .. 39 and the rest) with padding columns that would count if read: POISON dots,
    # column norms 0 and column radii +inf behind ny
    ldo = (N + 1) // 2 * 2 + 2
    extra = ldo - N + 2
    ng, nr = _cuda(MR.sqnorms(G)), _padded(MR.sqnorms(R), extra, 0.0)
    rr_p = _padded(ref["rad2_real"], extra, np.inf)
    cnt_b, col_b, min_b = _out(M, torch.int32), _out(N, torch.int32), _out(N)
    col_b[:N] = 0
    min_b[:N] = float("inf")
    first_min = None
    for a0, rows in ((0, 40), (40, M - 40)):
        slab = _slab(gg_, rg_, a0, rows, ldo)
        mf.launch("frido_ball_rows", mf.ball_rows_desc(slab.data_ptr(), ng.data_ptr() + 8 * a0, nr.data_ptr(), rr_p.data_ptr(),
                                                       cnt_b.data_ptr() + 4 * a0, rows, N, ldo), _stream())
        mf.launch("frido_ball_cols", mf.ball_cols_desc(slab.data_ptr(), ng.data_ptr() + 8 * a0, nr.data_ptr(), rg.data_ptr() + 8 * a0,
                                                       col_b.data_ptr(), min_b.data_ptr(), rows, N, ldo), _stream())
        torch.cuda.synchronize()
        if first_min is None:
            first_min = min_b[:N].cpu().numpy().copy()
    assert np.array_equal(_take(cnt_b, M, "frido_ball_rows"), ref["cnt"])
    assert np.array_equal(_take(col_b, N, "frido_ball_cols"), ref["cnt_col"])
    got_min = _take(min_b, N, "frido_ball_cols")
    assert np.array_equal(got_min, ref["dmin_col"])
    # dmin_col survives across slabs: some columns had their minimum in the first slab and kept it, others lowered it in the second
    d = MR.d2(G, R)
    assert np.array_equal(first_min, d[:40].min(axis=0))
    assert bool((got_min == first_min).any()) and bool((got_min < first_min).any())


# ---- the metric ------------------------------------------------------------------------------------------
METRIC_CASES = [pytest.param(MR.REAL_CASES[0], marks=pytest.mark.gate)] + MR.REAL_CASES[1:] + [MR.SATURATED_CASE, "tie", "near"]
NUMBERS = ("precision", "recall", "density", "coverage", "f_score")


def _same(got, ref, N, M, k):
    assert {n: got["counts"][n] for n in ref["counts"]} == ref["counts"], (got["counts"], ref["counts"])
    assert (got["counts"]["n_real"], got["counts"]["n_fake"], got["counts"]["k"]) == (N, M, k)
    for n in NUMBERS:
        assert isinstance(got[n], float) and got[n] == ref[n], (n, got[n], ref[n])


@pytest.mark.parametrize("name", METRIC_CASES)
def test_prdc_equals_the_restatement_and_banks_in_pieces(name):
    from frido_amd import pipeline
    R, G, k = MR.sides(name)
    ref = MR.reference(name)
    rg_, gg_ = _cuda(R), _cuda(G)
    got = mf.prdc(rg_, gg_, k)
    print(f"prdc {name}: " + " ".join(f"{n} {got[n]:.6f}" for n in NUMBERS) + f"   counts {got['counts']}")
    _same(got, ref, len(R), len(G), k)
    assert mf.prdc(rg_, gg_, k) == got                                        # a replay: the same counts
    assert mf.prdc(rg_, gg_, k, slab_rows=48) == got and mf.prdc(rg_, gg_, k, slab_bytes=1 << 16) == got
    cut = len(R) // 3
    br = fd.FeatureBank(R.shape[1], "cuda").append(rg_[:cut]).append(rg_[cut:])
    bg = fd.FeatureBank(G.shape[1], "cuda").append(gg_[:5]).append(gg_[5:7]).append(gg_[7:])
    assert torch.equal(br.rows(), rg_) and torch.equal(bg.rows(), gg_)
    assert pipeline.precision_recall(br, bg, k) == got == pipeline.precision_recall(br, gg_, k=k, slab_rows=32)
    if k == 3:
        assert pipeline.precision_recall(br, bg) == got                       # the default neighbourhood
    swapped = mf.prdc(gg_, rg_, k)                                            # the sides are not interchangeable
    _same(swapped, MR.prdc(G, R, k), len(G), len(R), k)


def test_closed_forms_on_the_device():
    """A set against itself: precision = recall = coverage = 1.  Two clusters farther apart than their diameters: all four 0."""
    R, _ = MR.real_case(150, 97, 36)
    rg_ = _cuda(R)
    got = mf.prdc(rg_, rg_.clone(), 3)
    assert got["precision"] == got["recall"] == got["coverage"] == got["f_score"] == 1.0 and got["density"] > 1.0
    far = _cuda(R[:60] * np.float32(0.01) + np.float32(100.0))
    got = mf.prdc(_cuda(R[:80] * np.float32(0.01)), far, 3)
    assert [got[n] for n in NUMBERS] == [0.0] * 5 and got["counts"]["density"] == 0
    with pytest.raises(ValueError, match="non-finite"):
        bad = rg_.clone()
        bad[3, 5] = float("nan")
        mf.prdc(bad, rg_)
    with pytest.raises(ValueError, match="non-finite"):
        bad = rg_.clone()
        bad[149, 35] = float("inf")
        mf.knn_radii2(bad)


def test_wrong_variants_differ_from_what_the_device_counts():
    """Every named wrong variant of the restatement moves at least one of the four integer counts the DEVICE returns, on at least one
    fixture; the right restatement moves none."""
    names = MR.REAL_CASES + ["tie", "near"]
    dev = {}
    for name in names:
        R, G, k = MR.sides(name)
        c = mf.prdc(_cuda(R), _cuda(G), k)["counts"]
        dev[str(name)] = {n: c[n] for n in ("precision", "density", "recall", "coverage")}
        assert dev[str(name)] == MR.reference(name)["counts"]
    for variant in MR.VARIANTS:
        moved = [str(name) for name in names if MR.reference(name, variant)["counts"] != dev[str(name)]]
        print(f"variant {variant}: differs on {moved}")
        assert moved, variant
    assert MR.reference("tie", "lt")["counts"] != dev["tie"] and MR.reference("near", "no_clamp")["counts"] != dev["near"]


# ---- end to end ------------------------------------------------------------------------------------------
def test_precision_recall_end_to_end_on_the_107_tower():
    """The 107 x 107 tower of tests/test_fid_gpu.py fills two banks of 8 rows with pipeline.fidelity_features, two batches a side: the
    real side two batches of clamped normal images, the generated side one more such batch and one of dimmer, shifted images, so that
    some generated rows lie among the real ones and some do not.  pipeline.precision_recall on them equals the restatement evaluated
    on THE BANKS' OWN ROWS copied to the host: the reference reads the same float32 features, so the tower's error decides no
    membership."""
    import test_fid_gpu as TF
    from frido_amd import pipeline
    m = TF._net("bf16x3", 107)
    batches = {"real": [TF._images(f"fid:e2e:a{b}", 4, 40) for b in range(2)],
               "fake": [TF._images("manifold:e2e:c0", 4, 40), (TF._images("fid:e2e:b1", 4, 40) * 0.6 + 0.2).clamp(-1, 1)]}
    banks = {}
    for side, xs in batches.items():
        fb = fd.FeatureBank(2048, "cuda")
        for x in xs:
            assert pipeline.fidelity_features(m, x.cuda(), feats=fb)[1] is fb
        assert fb.n == 8
        banks[side] = fb
    for k in (1, 3):
        got = pipeline.precision_recall(banks["real"], banks["fake"], k)
        R, G = banks["real"].rows().cpu().numpy(), banks["fake"].rows().cpu().numpy()
        ref = MR.prdc(R, G, k)
        print(f"end to end k = {k}: " + " ".join(f"{n} {got[n]:.6f}" for n in NUMBERS) + f"   counts {got['counts']}")
        _same(got, ref, 8, 8, k)
        if k == 3:
            assert ref["counts"]["density"] > 0                               # some generated row lies inside a real row's ball: not all zero
        assert np.array_equal(mf.knn_radii2(banks["real"], k).cpu().numpy(), MR.radii2(R, k))

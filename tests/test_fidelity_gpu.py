"""The Inception Score and the Kernel Inception Distance on the MI355X (csrc/fidelity.hip, frido_amd/fidelity.py) against the float64
restatement of tests/fidelity_ref.py: frido_rows_dot in its four modes, frido_mmd_finish, the four launches of the Inception Score,
FIDInceptionV3.logits and pipeline.fidelity_features / inception_score / kid end to end.

Bounds (none of them is taken from what the code under test returns):
  dot products         STORE_F64 bit-equal to the host loop in the kernel's order (the product of two float32 values is exact in float64,
           so a multiply and an add round as the fma does); STORE_F32 equal to that value rounded once; STORE_POLY_F64 bit-equal to numpy's
           separately rounded operations on it.
  Gram sums            T 2^-53 sum |K| for a sum of T terms: the bound of a float64 sum in ANY order.  The terms themselves differ from the
           restatement's (a BLAS product, **) by about D 2^-53 of their size each, D = 32 against T >= 4032: inside the same bound.
  mmd2                 that bound through the formula, (b_XX + b_YY) / (m (m - 1)) + 2 b_XY / m^2.
  Inception Score      64 C 2^-53 relative on every split score, on the mean and on the std (C 2^-53: the in-order bound of a C-term
           positive sum; 64: the chained max / exp / log / sum stages with a few ulp each).
  end to end           written at the test."""
import numpy as np
import pytest
import torch

import fidelity_ref as FR
import inception_ref as R
from frido_amd import fidelity as fd
from frido_amd import synth
from frido_amd.engine import require_gpu

pytestmark = pytest.mark.gpu

PAD = 64                    # NaN elements behind every kernel output: the kernel must leave them alone
U = 2.0 ** -53


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(n, dtype=torch.float64):
    require_gpu("cuda")
    return torch.full((n + PAD,), float("nan"), device="cuda", dtype=dtype)


def _take(buf, n, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n:]).all()), f"{what} wrote behind its output"
    out = buf[:n].cpu()
    assert not bool(torch.isnan(out).any()), f"{what} left output elements unwritten"
    return out


def _normal(tag, shape, mean=0.0, scale=1.0):
    return (synth.seeded_normal(tag, shape) * scale + mean).astype(np.float32)


# ---- frido_rows_dot, the three storing modes -------------------------------------------------------------
def _lists(nx, ny, m, S=2):
    """int32 [S, m] lists into nx / ny rows: the first subset descending, the others random with repeats (m > nx or ny repeats anyway)."""
    rng = np.random.RandomState(nx * 1000 + ny)
    ix = np.stack([(np.arange(m)[::-1] % nx)] + [rng.randint(0, nx, m) for _ in range(S - 1)]).astype(np.int32)
    iy = np.stack([(np.arange(m)[::-1] % ny)] + [rng.randint(0, ny, m) for _ in range(S - 1)]).astype(np.int32)
    return ix, iy


def _store(x, y, mode, *, ix=None, iy=None, ldo=None, **kw):
    """One launch into a NaN-filled buffer with `ldo` elements per row; returns [S, RX, RY] and checks that nothing else was written."""
    S, rx, ry = (1, x.shape[0], y.shape[0]) if ix is None else (ix.shape[0], ix.shape[1], ix.shape[1])
    ldo = ry if ldo is None else ldo
    dtype = torch.float32 if mode == fd.STORE_F32 else torch.float64
    buf = _out(S * rx * ldo, dtype)
    lists = {} if ix is None else dict(ix=ix.data_ptr(), iy=iy.data_ptr(), S=S, m=rx)
    fd.launch("frido_rows_dot", fd.rows_dot_desc(x.data_ptr(), y.data_ptr(), x.shape[0], y.shape[0], x.shape[1], mode=mode, out=buf.data_ptr(),
                                                 ldo=ldo, **lists, **kw), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[S * rx * ldo:]).all()), "frido_rows_dot wrote behind its output"
    got = buf[:S * rx * ldo].cpu().view(S, rx, ldo)
    assert bool(torch.isnan(got[:, :, ry:]).all()), "frido_rows_dot wrote into the columns behind RY"
    assert not bool(torch.isnan(got[:, :, :ry]).any()), "frido_rows_dot left output elements unwritten"
    return got[:, :, :ry].numpy()


DOT_CASES = [pytest.param(1, 1, 4, marks=pytest.mark.gate), pytest.param(3, 5, 8, marks=pytest.mark.gate), (65, 70, 100), (130, 64, 2048)]
POLY = (dict(degree=3, gamma=None, coef0=1.0), dict(degree=4, gamma=0.37, coef0=-0.5), dict(degree=1, gamma=2.0, coef0=0.25),
        dict(degree=2, gamma=0.01, coef0=0.0))


@pytest.mark.parametrize("lists", [False, True], ids=["rows", "lists"])
@pytest.mark.parametrize("nx,ny,D", DOT_CASES)
def test_rows_dot_stores_the_in_order_dot_bit_for_bit(nx, ny, D, lists):
    x, y = _normal(f"fidelity:dot:x{nx}:{D}", (nx, D), 0.2, 1.5), _normal(f"fidelity:dot:y{ny}:{D}", (ny, D), -0.1, 0.7)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    if lists:
        ix, iy = _lists(nx, ny, max(nx, ny) + 1)
        ref = np.stack([FR.dot_in_order(x[a], y[b]) for a, b in zip(ix, iy)])
        kw = dict(ix=torch.from_numpy(ix).cuda(), iy=torch.from_numpy(iy).cuda())
    else:
        ref, kw = FR.dot_in_order(x, y)[None], {}
    ry = ref.shape[2]
    for ldo in (ry, (ry + 3) // 4 * 4 + 4):                                  # rows that end where they are (odd ones too), and wider, 16-byte rows
        got = _store(xg, yg, fd.STORE_F64, ldo=ldo, **kw)
        assert np.array_equal(got, ref), ("f64", ldo, float(np.abs(got - ref).max()))
        assert np.array_equal(_store(xg, yg, fd.STORE_F64, ldo=ldo, **kw), got)          # a replay: the same bits
        assert np.array_equal(_store(xg, yg, fd.STORE_F32, ldo=ldo, **kw), ref.astype(np.float32)), ("f32", ldo)
        for p in POLY:
            gamma = 1.0 / D if p["gamma"] is None else p["gamma"]
            got = _store(xg, yg, fd.STORE_POLY_F64, ldo=ldo, degree=p["degree"], gamma=gamma, coef0=p["coef0"], **kw)
            assert np.array_equal(got, FR.poly_in_order(ref, gamma, p["coef0"], p["degree"])), ("poly", ldo, p)
    # the public wrapper: the same bits, its own buffers
    w = fd.rows_dot(xg, yg, mode=fd.STORE_F64, **kw).cpu().numpy()
    assert np.array_equal(w.reshape(ref.shape), ref)
    w32 = fd.rows_dot(xg, yg, mode=fd.STORE_F32, **kw)
    assert w32.dtype == torch.float32 and np.array_equal(w32.cpu().numpy().reshape(ref.shape), ref.astype(np.float32))


def test_rows_dot_second_trip_of_the_grid():
    """S = 40 subsets of m = 260 rows, D = 64: 25 tiles per subset, 1000 per launch, above the launcher's cap of workgroups, so the
    grid-stride loop takes a second trip -- in the storing mode (bit-equal) and for the three Gram kinds of the summing mode (every
    partial against the float64 sum of its tile's terms, T 2^-53 sum |K| with T = 4096)."""
    S, m, D, n = 40, 260, 64, 300
    assert S * fd.tiles(m) > fd.ROWS_DOT_GRID_CAP and S * fd.tiles(m, symmetric=True) > fd.ROWS_DOT_GRID_CAP
    x, y = _normal("fidelity:trip:x", (n, D)), _normal("fidelity:trip:y", (n, D), 0.3, 1.5)
    i1, i2 = fd.kid_subsets(n, n, S, m)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ixg, iyg = torch.from_numpy(i1.astype(np.int32)).cuda(), torch.from_numpy(i2.astype(np.int32)).cuda()
    ref = np.stack([FR.dot_in_order(x[a], y[b]) for a, b in zip(i1, i2)])
    assert np.array_equal(_store(xg, yg, fd.STORE_F64, ix=ixg, iy=iyg), ref)
    gamma, nt = 1.0 / D, 5
    for a, b, ia, ib, ha, hb, same in ((xg, xg, ixg, ixg, x, x, True), (yg, yg, iyg, iyg, y, y, True), (xg, yg, ixg, iyg, x, y, False)):
        T = fd.tiles(m)
        buf = _out(S * T)
        fd.launch("frido_rows_dot", fd.rows_dot_desc(a.data_ptr(), b.data_ptr(), n, n, D, mode=fd.SUM_POLY, partials=buf.data_ptr(), ix=ia.data_ptr(),
                                                     iy=ib.data_ptr(), S=S, m=m, degree=3, gamma=gamma, coef0=1.0, exclude_diag=same), _stream())
        got = _take(buf, S * T, "frido_rows_dot").numpy().reshape(S, nt, nt)
        idx_a, idx_b = (i1 if ha is x else i2), (i1 if hb is x else i2)
        for s in (0, 17, S - 1):                                             # the first trip, the middle, the second trip
            K = FR.poly_kernel(ha[idx_a[s]], hb[idx_b[s]], 3, gamma, 1.0)
            if same:
                np.fill_diagonal(K, 0.0)
            for ti in range(nt):
                for tj in range(nt):
                    blk = K[64 * ti:64 * ti + 64, 64 * tj:64 * tj + 64]
                    assert abs(got[s, ti, tj] - blk.sum()) <= 4096 * U * np.abs(blk).sum(), (s, ti, tj)


# ---- SUM_POLY and frido_mmd_finish -----------------------------------------------------------------------
KID_D, KID_N = 32, 100
# mmd2 of the three subsets of the two sides below in the float64 restatement, when written: 0.527, 0.596, 0.677 at m = 64 and 0.558,
# 0.662, 0.663 at m = 65 -- clearly positive, 2e11 times the bound
MMD2_STATED = {64: 0.5, 65: 0.5}      # a lower mark for all of them


def _sides():
    return _normal("fidelity:kid:a", (KID_N, KID_D)), _normal("fidelity:kid:b", (KID_N, KID_D), 0.3, 1.5)


def _sum_bounds(x, y, **kw):
    """Per subset: the three sums, their bounds T 2^-53 sum |K|, mmd2 and its bound."""
    m = x.shape[0]
    sums, mags = FR.gram_sums(x, y, **kw)
    b = [m * (m - 1) * U * mags[0], m * (m - 1) * U * mags[1], m * m * U * mags[2]]
    mmd2 = (sums[0] + sums[1]) / (m * (m - 1)) - 2.0 * sums[2] / (m * m)
    bm = (b[0] + b[1]) / (m * (m - 1)) + 2.0 * b[2] / (m * m)
    return sums, b, mmd2, bm


@pytest.mark.parametrize("m", [pytest.param(64, marks=pytest.mark.gate), 65])
def test_gram_sums_and_mmd2_against_float64(m):
    """Three subsets of m rows per side from sides of different mean and scale (N(0, 1) against N(0.3, 1.5^2), D = 32); m = 64 is one
    tile whose diagonal is the excluded one, m = 65 has ragged tiles and a diagonal that crosses them."""
    a, b = _sides()
    i1, i2 = fd.kid_subsets(KID_N, KID_N, 3, m)
    ag, bg = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    full = fd.mmd2_subsets(ag, bg, i1, i2, symmetric=False)
    sym = fd.mmd2_subsets(ag, bg, i1, i2, symmetric=True)
    assert np.array_equal(fd.mmd2_subsets(ag, bg, i1, i2, symmetric=True), sym) and np.array_equal(fd.mmd2_subsets(ag, bg, i1, i2, symmetric=False), full)
    assert full.shape == sym.shape == (3, 4) and full.dtype == np.float64
    for s in range(3):
        x, y = a[i1[s]].astype(np.float64), b[i2[s]].astype(np.float64)
        sums, bs, mmd2, bm = _sum_bounds(x, y)
        print(f"m = {m}, subset {s}: mmd2 {mmd2:.12g} (hip {sym[s, 3]:.12g}), |errors| of the sums " +
              " ".join(f"{abs(sym[s, k] - sums[k]):.2e}/{bs[k]:.2e}" for k in range(3)) + f", of mmd2 {abs(sym[s, 3] - mmd2):.2e}/{bm:.2e}")
        assert mmd2 > MMD2_STATED[m]
        for got in (full, sym):
            for k in range(3):
                assert abs(got[s, k] - sums[k]) <= bs[k], (s, k)
            assert abs(got[s, 3] - mmd2) <= bm
            # the finish's formula on the finish's own sums, operation by operation
            want = (got[s, 0] + got[s, 1]) / (float(m) * float(m - 1)) - (2.0 * got[s, 2]) / (float(m) * float(m))
            assert got[s, 3] == want
        for k in range(3):                                                   # the symmetric shortcut against the full launch
            assert abs(full[s, k] - sym[s, k]) <= bs[k]
        assert abs(full[s, 3] - sym[s, 3]) <= bm
        wrong = dict(diagonal=FR.mmd2(x, y, diagonal=True), divisor=FR.mmd2(x, y, biased_divisor=True), gamma1=FR.mmd2(x, y, gamma=1.0),
                     coef0=FR.mmd2(x, y, coef0=0.0), degree2=FR.mmd2(x, y, degree=2))
        for name, v in wrong.items():
            assert abs(v - mmd2) >= 10 * bm, (name, v, mmd2, bm)


def test_kernel_inception_distance_public_call_and_banks_in_pieces():
    a, b = _sides()
    ag, bg = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    mean, std = fd.kernel_inception_distance(ag, bg, subsets=5, subset_size=70)
    rmean, rstd, v = FR.kid(a, b, 5, 70)
    bm = max(_sum_bounds(a[i].astype(np.float64), b[j].astype(np.float64))[3] for i, j in FR.kid_indices(KID_N, KID_N, 5, 70))
    print(f"kid: hip {mean:.12g} +- {std:.12g}, float64 {rmean:.12g} +- {rstd:.12g}, bound per subset {bm:.2e}")
    assert isinstance(mean, float) and isinstance(std, float)
    assert abs(mean - rmean) <= bm and abs(std - rstd) <= 2 * bm              # a std moves by at most twice what its values move by
    assert rmean > 0.5 and rstd > 0                                           # 0.584 +- 0.068 when written
    # banks: two pieces give the bits of one piece, and the same numbers; a bank and its tensor are the same argument
    one, two = fd.FeatureBank(KID_D, "cuda").append(ag), fd.FeatureBank(KID_D, "cuda").append(ag[:37]).append(ag[37:])
    assert two.n == one.n == KID_N and torch.equal(one.rows(), two.rows()) and torch.equal(one.rows(), ag)
    bb = fd.FeatureBank(KID_D, "cuda").append(bg)
    from frido_amd import pipeline
    assert pipeline.kid(two, bb, subsets=5, subset_size=70) == (mean, std) == pipeline.kid(one, bb, subsets=5, subset_size=70)
    assert fd.kernel_inception_distance(ag, bg, subsets=5, subset_size=70, rng_seed=7) != (mean, std)


# ---- the Inception Score ---------------------------------------------------------------------------------
ISC_CASES = [pytest.param(7, 4, 3, marks=pytest.mark.gate), pytest.param(40, 100, 4, marks=pytest.mark.gate), (40, 1008, 4), (130, 1008, 10)]


def _isc_launch(lg, perm, splits):
    """The four launches into NaN-guarded buffers: (rowstats [N, 2], q [splits, C], kl [N], scores [splits]) as numpy."""
    N, Cn = lg.shape
    pg = torch.from_numpy(perm.astype(np.int32)).cuda()
    bufs = [_out(2 * N), _out(splits * Cn), _out(N), _out(splits)]
    d = fd.isc_desc(lg.data_ptr(), pg.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), N, Cn, splits)
    for step in fd.ISC_STEPS:
        fd.launch(step, d, _stream())
    return [_take(b, n, "frido_isc").numpy() for b, n in zip(bufs, (2 * N, splits * Cn, N, splits))]


@pytest.mark.parametrize("N,Cn,splits", ISC_CASES)
def test_inception_score_against_float64(N, Cn, splits):
    """Logits with a spread of 3.  Wrong variants -- a bias added to the logits, no permutation, q over all rows, ddof 1 -- lie at
    least 10 x outside the bound."""
    l = _normal(f"fidelity:isc:{N}:{Cn}", (N, Cn), 0.0, 3.0)
    lg = torch.from_numpy(l).cuda()
    bound = 64 * Cn * U
    perm = fd.isc_permutation(N)
    rowstats, q, kl, scores = _isc_launch(lg, perm, splits)
    again = _isc_launch(lg, perm, splits)
    assert all(np.array_equal(a, b) for a, b in zip((rowstats, q, kl, scores), again))      # a replay: the same bits
    ref = FR.isc_scores(l, splits)
    rel = np.abs(scores - ref) / ref
    rmean, rstd = FR.isc(l, splits)
    mean, std = fd.inception_score(lg, splits=splits)
    assert (mean, std) == (float(np.mean(scores)), float(np.std(scores)))
    e_mean, e_std = abs(mean - rmean) / rmean, abs(std - rstd) / rstd
    print(f"isc N={N} C={Cn} splits={splits}: score {rmean:.6f} +- {rstd:.6f}; relative errors: splits {rel.max():.2e}, mean {e_mean:.2e}, "
          f"std {e_std:.2e}; bound {bound:.2e}")
    # the intermediate values, against the restatement's own
    lp = FR.log_softmax(l[perm])
    assert np.array_equal(rowstats.reshape(N, 2)[:, 0], l[perm].astype(np.float64).max(axis=1))
    assert np.abs(np.exp(lp).sum(axis=1) - 1.0).max() <= bound
    assert rel.max() <= bound and e_mean <= bound and e_std <= bound
    # shuffled and unshuffled are different scores, and the unshuffled one is right, too
    plain = fd.inception_split_scores(lg, splits=splits, shuffle=False)
    ref_plain = FR.isc_scores(l, splits, shuffle=False)
    assert (np.abs(plain - ref_plain) / ref_plain).max() <= bound
    bias = _normal(f"fidelity:isc:bias:{Cn}", (1, Cn), 0.0, 0.5).astype(np.float64)
    wrong = dict(bias=FR.isc(l.astype(np.float64) + bias, splits), no_permutation=FR.isc(l, splits, shuffle=False),
                 q_over_all=FR.isc(l, splits, marginal_over_all=True), ddof1=FR.isc(l, splits, ddof=1))
    for name, (wm, ws) in wrong.items():
        assert max(abs(wm - rmean) / rmean, abs(ws - rstd) / rstd) >= 10 * bound, (name, wm, ws)


# ---- FIDInceptionV3.logits and the pipeline --------------------------------------------------------------
def test_logits_bit_equal_and_end_to_end_on_the_107_tower():
    """The 107 x 107 tower of tests/test_fid_gpu.py (its weights, nets and float64 features are shared through that module's caches).
    logits: features @ fc.weight.T in the kernel's order, rounded once, bit for bit, from the SAME (device) features; no bias.
    End to end: pipeline.fidelity_features over two batches of 4 images on each of two sides, then inception_score(splits=2) per side
    and kid(subsets=3, subset_size=6), against the restatement on the float64 tower's features and logits.  The bound is propagated
    from the feature bound eps = 8 E32 max |f| like test_fid_statistics_and_fid_end_to_end's: each reference number recomputed with
    every feature of both sides moved by +-eps (the larger change of two draws of signs)."""
    import test_fid_gpu as TF
    from frido_amd import fid, pipeline
    m = TF._net("bf16x3", 107)
    sd = TF._sd()
    W = sd["fc.weight"].double().numpy()
    img, _, _ = TF._tower_case("107")
    f = m(img.cuda())
    lg = m.logits(f)
    assert lg.shape == (img.shape[0], 1008) and lg.dtype == torch.float32 and torch.equal(m(img.cuda()), f)
    want = FR.dot_in_order(f.cpu().numpy(), sd["fc.weight"].numpy()).astype(np.float32)
    assert np.array_equal(lg.cpu().numpy(), want)
    assert not np.array_equal(want, (FR.dot_in_order(f.cpu().numpy(), sd["fc.weight"].numpy()) + sd["fc.bias"].double().numpy()).astype(np.float32))
    assert torch.equal(m.logits(f), lg)

    banks, feats = {}, {}
    for side, gain in (("a", 1.0), ("b", 0.6)):
        batches = [(TF._images(f"fid:e2e:{side}{k}", 4, 40) * gain + (0.2 if side == "b" else 0.0)).clamp(-1, 1) for k in range(2)]
        st, fb, lb = fid.FeatureStatistics(2048, "cuda"), fd.FeatureBank(2048, "cuda"), fd.FeatureBank(1008, "cuda")
        for x in batches:
            out = pipeline.fidelity_features(m, x.cuda(), stats=st, feats=fb, logits=lb)
            assert out[0] is st and out[1] is fb and out[2] is lb
        assert st.n == fb.n == lb.n == 8
        assert pipeline.fidelity_features(m, batches[0].cuda()) == (None, None, None)
        only = pipeline.fid_statistics(m, batches[1].cuda(), pipeline.fid_statistics(m, batches[0].cuda()))
        assert torch.equal(only.s1, st.s1) and torch.equal(only.s2, st.s2)      # the statistics fid_statistics collects, bit for bit
        banks[side] = (fb, lb)
        feats[side] = torch.cat([R.features(sd, x, "pil", 107) for x in batches]).numpy()
    eps = 8.0 * TF._tower_E32() * max(float(np.abs(v).max()) for v in feats.values())

    def numbers(fa, fb):
        return np.array(FR.isc(fa @ W.T, 2) + FR.isc(fb @ W.T, 2) + FR.kid(fa, fb, 3, 6)[:2])

    ref = numbers(feats["a"], feats["b"])
    rng = np.random.default_rng(5)
    moved = np.max([np.abs(numbers(feats["a"] + eps * rng.choice([-1.0, 1.0], feats["a"].shape),
                                   feats["b"] + eps * rng.choice([-1.0, 1.0], feats["b"].shape)) - ref) for _ in range(2)], axis=0)
    got = np.array(pipeline.inception_score(banks["a"][1], splits=2) + pipeline.inception_score(banks["b"][1], splits=2) +
                   pipeline.kid(banks["a"][0], banks["b"][0], subsets=3, subset_size=6))
    names = ("isc a mean", "isc a std", "isc b mean", "isc b std", "kid mean", "kid std")
    for n, g, r, b in zip(names, got, ref, moved):
        print(f"end to end {n}: hip {g:.9g}, float64 reference {r:.9g}, |difference| {abs(g - r):.3e}, bound {b:.3e}")
    assert bool((moved > 0).all()) and bool((np.abs(got - ref) <= moved).all())

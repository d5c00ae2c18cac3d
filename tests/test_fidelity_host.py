"""Host side of the Inception Score and the Kernel Inception Distance (frido_amd/fidelity.py, FIDInceptionV3.logits,
pipeline.fidelity_features / inception_score / kid): the float64 restatement against independent code, the random streams, FeatureBank,
the refusals and the ABI constraints.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fidelity_ref as FR
from frido_amd import _lib, synth
from frido_amd._lib import FridoHipError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _feats(tag, n, D, mean=0.0, scale=1.0):
    return (synth.seeded_normal(tag, (n, D)) * scale + mean).astype(np.float32)


# ---- the restatement against independent code ----------------------------------------------------------------
def test_poly_kernel_and_mmd2_against_sklearn():
    """The Gram matrices against sklearn.metrics.pairwise.polynomial_kernel, and mmd2 written out from them a second time.  Both are
    float64 matrix products of D terms followed by the same few operations: 4 D 2^-53 of the largest entry."""
    from sklearn.metrics.pairwise import polynomial_kernel
    x, y = _feats("fidelity:host:x", 40, 32).astype(np.float64), _feats("fidelity:host:y", 40, 32, 0.3, 1.5).astype(np.float64)
    for degree, gamma, coef0 in ((3, None, 1.0), (2, 0.5, 0.0), (1, None, 2.0), (4, 0.01, 1.0)):
        for a, b in ((x, x), (x, y)):
            ours, ref = FR.poly_kernel(a, b, degree, gamma, coef0), polynomial_kernel(a, b, degree=degree, gamma=gamma, coef0=coef0)
            assert np.abs(ours - ref).max() <= 4 * 32 * 2.0 ** -53 * np.abs(ref).max() * degree
        kxx, kyy, kxy = (polynomial_kernel(a, b, degree=degree, gamma=gamma, coef0=coef0) for a, b in ((x, x), (y, y), (x, y)))
        m = 40
        want = ((kxx.sum() - np.trace(kxx)) + (kyy.sum() - np.trace(kyy))) / (m * (m - 1)) - 2 * kxy.mean()
        scale = (np.abs(kxx).sum() + np.abs(kyy).sum()) / (m * (m - 1)) + 2 * np.abs(kxy).mean()
        assert abs(FR.mmd2(x, y, degree, gamma, coef0) - want) <= 4 * m * m * 2.0 ** -53 * scale
    assert FR.mmd2(x, y) > 0.1 > 0 > FR.mmd2(x, x)      # two sides apart; a set against itself: negative, the cross term keeps its diagonal


def test_in_order_dot_and_poly_are_what_they_say():
    x, y = _feats("fidelity:host:dx", 5, 12), _feats("fidelity:host:dy", 3, 12)
    d = FR.dot_in_order(x, y)
    for a in range(5):
        for b in range(3):
            acc = 0.0
            for k in range(12):
                acc = acc + float(x[a, k]) * float(y[b, k])               # python floats: one rounding per add, the product exact
            assert d[a, b] == acc
    assert np.abs(d - x.astype(np.float64) @ y.astype(np.float64).T).max() <= 12 * 2.0 ** -53 * np.abs(d).max() * 4
    t = d * 0.25 + 1.0
    assert np.array_equal(FR.poly_in_order(d, 0.25, 1.0, 3), (t * t) * t) and np.array_equal(FR.poly_in_order(d, 0.25, 1.0, 1), t)


def test_softmax_and_scores_against_scipy():
    from scipy.special import log_softmax, softmax
    l = (synth.seeded_normal("fidelity:host:l", (30, 50)) * 3).astype(np.float32)
    assert np.abs(FR.log_softmax(l) - log_softmax(l.astype(np.float64), axis=1)).max() <= 8 * 50 * 2.0 ** -53 * np.abs(l).max()
    # the score, a second time from scipy's p, unshuffled, three ragged splits (0, 10, 20, 30 / 30 rows -> equal here; 31 rows below)
    for N in (30, 31):
        ll = l[:N] if N == 30 else np.concatenate([l, l[:1] * 0.5])
        p, logp = softmax(ll.astype(np.float64), axis=1), log_softmax(ll.astype(np.float64), axis=1)
        want = []
        for i in range(3):
            lo, hi = i * N // 3, (i + 1) * N // 3
            q = p[lo:hi].mean(axis=0)
            want.append(np.exp(np.mean([(p[r] * (logp[r] - np.log(q))).sum() for r in range(lo, hi)])))
        got = FR.isc_scores(ll, 3, shuffle=False)
        assert np.abs(got - np.array(want)).max() <= 64 * 50 * 2.0 ** -53 * max(want)
        mean, std = FR.isc(ll, 3, shuffle=False)
        assert mean == float(np.mean(got)) and std == float(np.std(got)) and FR.isc(ll, 3, shuffle=False, ddof=1)[1] > std
    assert 1.0 < FR.isc(l, 3)[0] < 50.0


def test_random_streams_are_the_pinned_ones():
    """np.random.RandomState(2020): the permutation of 10 and the first two subsets of choice(7, 4), choice(9, 4), written out."""
    from frido_amd import fidelity
    assert fidelity.isc_permutation(10).tolist() == [2, 4, 9, 1, 5, 7, 6, 3, 8, 0]
    assert fidelity.isc_permutation(10, shuffle=False).tolist() == list(range(10))
    assert fidelity.isc_permutation(10, rng_seed=1).tolist() != fidelity.isc_permutation(10).tolist()
    i1, i2 = fidelity.kid_subsets(7, 9, 2, 4)
    assert i1.tolist() == [[5, 4, 1, 2], [0, 1, 5, 4]] and i2.tolist() == [[3, 1, 2, 4], [5, 2, 3, 1]]
    ref = FR.kid_indices(7, 9, 2, 4)
    assert [a.tolist() for a, _ in ref] == i1.tolist() and [b.tolist() for _, b in ref] == i2.tolist()
    sig = inspect.signature(fidelity.inception_score).parameters
    assert (sig["splits"].default, sig["shuffle"].default, sig["rng_seed"].default) == (10, True, 2020)
    sig = inspect.signature(fidelity.kernel_inception_distance).parameters
    assert [sig[k].default for k in ("subsets", "subset_size", "degree", "gamma", "coef0", "rng_seed")] == [100, 1000, 3, None, 1.0, 2020]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for k, p in sig.items() if k not in ("f1", "f2"))


# ---- FeatureBank ----------------------------------------------------------------------------------------------
def test_feature_bank_growth_save_load_concat(tmp_path):
    from frido_amd import fidelity
    x = torch.from_numpy(_feats("fidelity:host:bank", 300, 8))
    b = fidelity.FeatureBank(8, "cpu")
    assert b.n == 0 and b.rows().shape == (0, 8)
    caps = []
    for lo, hi in ((0, 1), (1, 64), (64, 65), (65, 200), (200, 300)):
        assert b.append(x[lo:hi]) is b
        caps.append(b.buf.shape[0])
        assert b.n == hi and torch.equal(b.rows(), x[:hi])
    assert caps == [64, 64, 128, 256, 512]                                   # doubling, never shrinking
    assert b.rows().data_ptr() == b.buf.data_ptr()                            # a view
    one = fidelity.FeatureBank(8, "cpu").append(x)
    assert torch.equal(one.rows(), b.rows())                                  # pieces == one piece
    path = tmp_path / "bank.npz"
    b.save(str(path))
    z = np.load(path)
    assert z.files == ["features"] and z["features"].dtype == np.float32 and z["features"].shape == (300, 8)
    back = fidelity.FeatureBank.load(str(path))
    assert back.n == 300 and back.D == 8 and torch.equal(back.rows(), x) and back.device.type == "cpu"
    np.savez(tmp_path / "other.npz", mu=np.zeros(3))
    with pytest.raises(ValueError, match="features"):
        fidelity.FeatureBank.load(str(tmp_path / "other.npz"))
    parts = [fidelity.FeatureBank(8, "cpu").append(x[:7]), fidelity.FeatureBank(8, "cpu"), fidelity.FeatureBank(8, "cpu").append(x[7:100])]
    c = fidelity.FeatureBank.concat(parts)
    assert c.n == 100 and torch.equal(c.rows(), x[:100]) and parts[0].n == 7
    with pytest.raises(ValueError, match="nothing to join"):
        fidelity.FeatureBank.concat([])
    with pytest.raises(ValueError, match="widths differ"):
        fidelity.FeatureBank.concat([fidelity.FeatureBank(8, "cpu"), fidelity.FeatureBank(4, "cpu")])
    for bad in (torch.zeros(2, 4), torch.zeros(8), torch.zeros(2, 8, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="float32"):
            b.append(bad)
    assert b.all_gather_concat() is b                                         # no process group: nothing to gather


GATHER_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
from frido_amd import fidelity
from test_fidelity_host import _feats
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
x = torch.from_numpy(_feats("fidelity:gather", 40, 8))
cut = [0, 17, 40]
mine = fidelity.FeatureBank(8, "cpu").append(x[cut[rank]:cut[rank + 1]])
full = mine.all_gather_concat()
assert full.n == 40 and torch.equal(full.rows(), x), rank                    # rank order, ragged shards
assert mine.n == cut[rank + 1] - cut[rank]
empty = (fidelity.FeatureBank(8, "cpu") if rank == 0 else mine).all_gather_concat()
assert empty.n == 23 and torch.equal(empty.rows(), x[17:]), rank              # a rank without rows
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_all_gather_concat_world_size_2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(GATHER_WORKER % (REPO, REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29537", str(script)],
                         capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 2


# ---- refusals -------------------------------------------------------------------------------------------------
def test_refusals():
    from frido_amd import fidelity, pipeline
    from frido_amd.models import FIDInceptionV3
    l = torch.zeros(20, 12)
    with pytest.raises(ValueError, match="splits"):
        fidelity.inception_score(torch.zeros(5, 12), splits=6)               # N < splits
    with pytest.raises(ValueError, match="splits"):
        fidelity.inception_score(l, splits=0)
    for bad in (torch.zeros(20), torch.zeros(2, 3, 4), torch.zeros(20, 12, dtype=torch.float64), "x"):
        with pytest.raises(ValueError, match="2-D float32"):
            fidelity.inception_score(bad)
        with pytest.raises(ValueError, match="2-D float32"):
            fidelity.kernel_inception_distance(bad, l, subset_size=4)
        with pytest.raises(ValueError, match="2-D float32"):
            fidelity.kernel_inception_distance(l, bad, subset_size=4)
        with pytest.raises(ValueError, match="2-D float32"):
            fidelity.rows_dot(bad, l)
    with pytest.raises(FridoHipError, match="no CPU"):
        fidelity.inception_score(l, splits=2)
    with pytest.raises(FridoHipError, match="no CPU"):
        pipeline.inception_score(fidelity.FeatureBank(12, "cpu").append(l), splits=2)
    a, b = torch.zeros(20, 12), torch.zeros(9, 12)
    for kw in (dict(subset_size=10), dict(subset_size=21), dict(subset_size=1), dict(subset_size=0)):      # above either count, below 2
        with pytest.raises(ValueError, match="subset_size"):
            fidelity.kernel_inception_distance(a, b, **kw)
        with pytest.raises(ValueError, match="subset_size"):
            fidelity.kernel_inception_distance(b, a, **kw)
    for degree in (0, 5, 2.5):
        with pytest.raises(ValueError, match="degree"):
            fidelity.kernel_inception_distance(a, b, subset_size=4, degree=degree)
    with pytest.raises(ValueError, match="multiple of 4"):
        fidelity.kernel_inception_distance(torch.zeros(20, 10), torch.zeros(9, 10), subset_size=4)
    with pytest.raises(ValueError, match="multiple of 4"):
        fidelity.kernel_inception_distance(a, torch.zeros(9, 16), subset_size=4)
    with pytest.raises(ValueError, match="multiple of 4"):
        fidelity.rows_dot(torch.zeros(2, 6), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="subsets"):
        fidelity.kernel_inception_distance(a, b, subset_size=4, subsets=0)
    with pytest.raises(FridoHipError, match="no CPU"):
        fidelity.kernel_inception_distance(a, b, subset_size=4)
    with pytest.raises(FridoHipError, match="no CPU"):
        pipeline.kid(fidelity.FeatureBank(12, "cpu").append(a), fidelity.FeatureBank(12, "cpu").append(b), subset_size=4)
    with pytest.raises(FridoHipError, match="no CPU"):
        fidelity.rows_dot(a, b)
    with pytest.raises(ValueError, match="outside"):
        fidelity.mmd2_subsets(a, b, np.array([[0, 20]]), np.array([[0, 1]]))
    m = FIDInceptionV3()
    for bad in (torch.zeros(2, 1008), torch.zeros(2048), torch.zeros(2, 2048, dtype=torch.float64), torch.zeros(0, 2048), None):
        with pytest.raises(ValueError, match="2-D float32"):
            m.logits(bad)
    with pytest.raises(FridoHipError, match="no CPU fallback"):
        m.logits(torch.zeros(2, 2048))
    with pytest.raises(ValueError, match="FIDInceptionV3"):
        pipeline.fidelity_features(object(), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="FeatureStatistics"):
        pipeline.fidelity_features(m, torch.zeros(1, 3, 8, 8), stats=3)
    with pytest.raises(ValueError, match="FeatureBank"):
        pipeline.fidelity_features(m, torch.zeros(1, 3, 8, 8), feats=torch.zeros(1, 2048))
    with pytest.raises(ValueError, match="FeatureBank"):
        pipeline.fidelity_features(m, torch.zeros(1, 3, 8, 8), logits=[])


def test_forward_signature_and_key_set_unchanged():
    from frido_amd import fid
    from frido_amd.models import FIDInceptionV3
    m = FIDInceptionV3()
    assert list(inspect.signature(m.forward).parameters) == ["images", "quant"]
    assert inspect.signature(m.forward).parameters["quant"].default is None
    assert list(inspect.signature(m.logits).parameters) == ["features"]
    want = {"fc.weight", "fc.bias"}
    for name, *_ in fid.conv_table():
        want |= {f"{name}.conv.weight"} | {f"{name}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(m.state_dict()) == want
    assert tuple(m.fc.weight.shape) == (fidelity_logits(), 2048)
    assert "never run" not in FIDInceptionV3.__doc__ and "logits" in FIDInceptionV3.__doc__
    assert "never run" not in open(os.path.join(REPO, "README.md")).read()


def fidelity_logits():
    from frido_amd import fidelity
    return fidelity.LOGITS


# ---- ABI ------------------------------------------------------------------------------------------------------
def test_descriptors_match_both_builds_and_bad_ones_are_turned_away():
    from frido_amd import fidelity as fd
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        for name, (struct, sizeof) in fd.LAUNCHERS.items():
            assert getattr(L, sizeof)() == C.sizeof(struct), (planes, name)
        fns = fd._fns(planes)
        assert set(fns) == set(fd.LAUNCHERS)

        def refused(name, desc, words):
            assert fns[name](C.byref(desc), None) == -1 and words in L.frido_last_error(), (name, L.frido_last_error())      # FRIDO_EINVAL

        for name, (struct, _) in fd.LAUNCHERS.items():                       # a zeroed descriptor: null pointers
            refused(name, struct(), name.encode() + b": bad arguments")
        store = dict(mode=fd.STORE_F64, out=base, ldo=8)
        summed = dict(mode=fd.SUM_POLY, partials=base, degree=3)
        listed = dict(ix=base, iy=base, S=2, m=5)
        for kw, words in ((dict(store, D=6), b"D must be a multiple of 4"), (dict(store, x=base + 4), b"x and y must be 16-byte"),
                          (dict(store, mode=4), b"mode"), (dict(store, mode=-1), b"mode"), (dict(store, ix=base), b"ix and iy come together"),
                          (dict(store, S=2), b"S, m"), (dict(store, m=3), b"S, m"), (dict(store, **dict(listed, m=0)), b"S, m"),
                          (dict(store, **dict(listed, iy=base + 2)), b"ix and iy must be 4-byte"),
                          (dict(store, mode=fd.STORE_POLY_F64, degree=0), b"degree"), (dict(summed, degree=5), b"degree"),
                          (dict(store, exclude_diag=1), b"exclude_diag"), (dict(summed, exclude_diag=2), b"exclude_diag"),
                          (dict(store, symmetric=1), b"symmetric"), (dict(summed, symmetric=1, y=base + 16), b"symmetric needs"),
                          (dict(summed, symmetric=1, ny=3), b"symmetric needs"), (dict(summed, partials=None), b"partials"),
                          (dict(summed, partials=base + 4), b"partials"), (dict(store, out=None), b"out must be given"),
                          (dict(store, ldo=7), b"out must be given"), (dict(store, out=base + 8), b"out must be 16-byte"),
                          (dict(store, nx=0), b"bad arguments"), (dict(store, y=None), b"bad arguments")):
            kw = dict(kw)
            d = fd.rows_dot_desc(kw.pop("x", base), kw.pop("y", base), kw.pop("nx", 8), kw.pop("ny", 8), kw.pop("D", 8), **kw)
            refused("frido_rows_dot", d, words)
        for kw, words in ((dict(m=1), b"m must be at least 2"), (dict(nxy=0), b"nxx, nyy and nxy"), (dict(S=0), b"bad arguments"),
                          (dict(pyy=None), b"bad arguments"), (dict(out=base + 8), b"aligned"), (dict(pxx=base + 4), b"aligned")):
            d = fd.mmd_finish_desc(base, base, base, base, 2, 4, 1, 1, 1)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_mmd_finish", d, words)
        for name in fd.ISC_STEPS:
            for kw, words in ((dict(splits=0), b"splits must lie in 1 .. N"), (dict(splits=5), b"splits must lie in 1 .. N"), (dict(C=0), b"N and C"),
                              (dict(N=0), b"N and C"), (dict(kl=None), b"bad arguments"), (dict(rowstats=base + 8), b"aligned"), (dict(perm=base + 2), b"aligned")):
                d = fd.isc_desc(base, base, base, base, base, base, 4, 8, 2)
                for k, v in kw.items():
                    setattr(d, k, v)
                refused(name, d, words)
                assert L.frido_last_error().startswith(name.encode() + b": ")
    assert (fd.STORE_F32, fd.STORE_F64, fd.STORE_POLY_F64, fd.SUM_POLY) == (0, 1, 2, 3)
    assert fd.tiles(64) == 1 and fd.tiles(65) == 4 and fd.tiles(65, symmetric=True) == 3 and fd.tiles(130, 64) == 3 and fd.tiles(1000, symmetric=True) == 136


def test_header_makefile_and_source_constraints():
    """frido_hip.h (the op-kind ABI) and frido_fid.h do not know the launches; fidelity.hip includes launch.h alone and sits directly
    behind fid.hip, with vision.hip and lpips.hip still last."""
    from frido_amd import fidelity as fd
    for hdr in ("frido_hip.h", "frido_fid.h"):
        text = open(os.path.join(REPO, "include", hdr)).read()
        for name in ("frido_fidelity", "rows_dot", "mmd_finish", "frido_isc", "FridoIsc", "FridoRowsDot"):
            assert name not in text, (hdr, name)
    assert _lib.ABI_VERSION == 8 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert not [s for s in _lib.EXPORTS if "rows_dot" in s or "mmd" in s or "isc" in s]
    assert not [s for s in _lib.STRUCTS if "RowsDot" in s or "Mmd" in s or "Isc" in s]
    body = _lib._strip_comments(open(os.path.join(REPO, "include", "frido_fidelity.h")).read())
    assert body.split("#include")[1].strip().startswith('"frido_hip.h"')
    assert _lib._parse_structs(body).keys() == {"FridoRowsDot", "FridoMmdFinish", "FridoIsc"}
    assert {fn for fn, _ in fd.LAUNCHERS.values()} == {fd.FridoRowsDot, fd.FridoMmdFinish, fd.FridoIsc}
    assert len({sz for _, sz in fd.LAUNCHERS.values()}) == 3                   # one frido_sizeof_* per descriptor
    assert fd.ROWS_DOT_GRID_CAP == 512
    mk = open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert srcs[-1] == "lpips.hip" and srcs[-2] == "vision.hip"
    assert srcs[srcs.index("patchgan.hip") + 1] == "fid.hip" and srcs[srcs.index("fid.hip") + 1] == "fidelity.hip"
    assert "fidelity.o obj_bf16p/fidelity.o: ../../include/frido_fidelity.h" in mk
    assert "-ffp-contract=on" in mk
    src = open(os.path.join(REPO, "frido_amd", "csrc", "fidelity.hip")).read()
    assert '#include "launch.h"' in src and "common.h" not in src
    low = src.lower()
    for word in ("atomic", "hipmalloc", "hipfree", "synchronize", "status_raise", "frido_x3_f16"):
        assert word not in low, word
    assert "FRIDO_ROWS_DOT_GRID_CAP" in src and "fp contract(off)" in src
    assert src.count("__launch_bounds__(256)") == src.count("__global__") == 6


def test_fid_npy_tool_on_saved_banks(tmp_path):
    """tools/fid_npy.py without --isc / --kid prints what it printed; with them on saved banks and no GPU it names the missing device."""
    from frido_amd import fidelity
    tool = os.path.join(REPO, "tools", "fid_npy.py")
    a = fidelity.FeatureBank(8, "cpu").append(torch.from_numpy(_feats("fidelity:tool:a", 16, 8)))
    pa = tmp_path / "a.npz"
    a.save(str(pa))
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--isc" in out.stdout and "--kid" in out.stdout
    if not torch.cuda.is_available():
        bad = subprocess.run([sys.executable, tool, str(pa), str(pa), "--kid", "--kid-subset-size", "4"], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "HIP device" in bad.stderr

"""Float64 numpy restatement of improved precision and recall and of density and coverage as frido_amd/manifold.py specifies them
(include/frido_manifold.h): the in-order dot, the norms, the clamped squared distance, the radii, the integer counts and the five
numbers; the named WRONG variants the tests must tell from the right one; and the fixtures both test files share.  Shares no code with
the package: tests/test_manifold_host.py holds it against scipy's cdist and scikit-learn's brute-force neighbours,
tests/test_manifold_gpu.py holds the kernels against it, bit for bit and count for count."""
import functools

import numpy as np

# the wrong variants, by name
VARIANTS = ("lt",               # d2 < rad2 where d2 <= rad2 belongs
            "kth",              # the k-th smallest for the (k + 1)-th: the row itself left out of its own set
            "row_radii",        # precision / density counted with the radii of the generated rows (the slab's rows) where the real rows' belong
            "col_radii",        # recall counted with the radii of the real rows (the slab's columns) where the generated rows' belong
            "no_clamp",         # d2 without its max(., 0)
            "pad")              # the real side's padding up to an even (here: by at least one) row count taken as rows of zeros


# ---- the kernel's own order (bit for bit) -----------------------------------------------------------------
def dot_in_order(x, y):
    """[nx, ny] float64: acc = fma((double)x[a, j], (double)y[b, j], acc) for j ascending from 0.0.  The product of two float32 values
    is exact in float64, so a separate multiply and add rounds exactly as the fma does."""
    x64, y64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    acc = np.zeros((x64.shape[0], y64.shape[0]), np.float64)
    for j in range(x64.shape[1]):
        acc = acc + x64[:, j, None] * y64[None, :, j]
    return acc


def sqnorms(x):
    """[n] float64: n(x) = dot(x, x), the same loop."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    acc = np.zeros(x64.shape[0], np.float64)
    for j in range(x64.shape[1]):
        acc = acc + x64[:, j] * x64[:, j]
    return acc


def d2(x, y, clamp=True):
    """[nx, ny] float64: max((n(x) + n(y)) - 2.0 * dot(x, y), 0.0); numpy rounds every operation on its own."""
    v = (sqnorms(x)[:, None] + sqnorms(y)[None, :]) - 2.0 * dot_in_order(x, y)
    return np.maximum(v, 0.0) if clamp else v


def radii2(x, k, clamp=True, self_excluded=False):
    """[n] float64: the (k + 1)-th smallest value, with multiplicity, of every row of d2(x, x) (the k-th with `self_excluded`)."""
    return np.sort(d2(x, x, clamp), axis=1)[:, k - 1 if self_excluded else k]


def scans(real, fake, k, variant=None):
    """The integer and float64 arrays behind the metric: rad2_real [N], rad2_fake [M], cnt [M], cnt_col [N], dmin_col [N]; rows of
    the cross matrix are generated samples, columns real ones."""
    assert variant is None or variant in VARIANTS, variant
    real, fake = np.asarray(real, np.float32), np.asarray(fake, np.float32)
    N = real.shape[0]
    if variant == "pad":
        real = np.concatenate([real, np.zeros((2 - N % 2, real.shape[1]), np.float32)])
    clamp = variant != "no_clamp"
    rr, rg = (radii2(s, k, clamp, self_excluded=variant == "kth") for s in (real, fake))
    d = d2(fake, real, clamp)                                                # [M, N]
    inside = (lambda a, b: a < b) if variant == "lt" else (lambda a, b: a <= b)
    cnt = inside(d, rg[:, None] if variant == "row_radii" else rr[None, :]).sum(axis=1)
    cnt_col = inside(d, rr[None, :] if variant == "col_radii" else rg[:, None]).sum(axis=0)
    dmin_col = d.min(axis=0)
    return dict(rad2_real=rr[:N], rad2_fake=rg, cnt=cnt.astype(np.int64), cnt_col=cnt_col[:N].astype(np.int64), dmin_col=dmin_col[:N],
                inside=inside)


def counts(real, fake, k, variant=None):
    """The four integer counts: precision, density, recall, coverage."""
    s = scans(real, fake, k, variant)
    return dict(precision=int((s["cnt"] > 0).sum()), density=int(s["cnt"].sum()), recall=int((s["cnt_col"] > 0).sum()),
                coverage=int(s["inside"](s["dmin_col"], s["rad2_real"]).sum()))


def prdc(real, fake, k=3, variant=None):
    """{"precision", "recall", "density", "coverage", "f_score": floats, "counts": the four integers}."""
    c = counts(real, fake, k, variant)
    N, M = len(real), len(fake)
    P, R = c["precision"] / M, c["recall"] / N
    return dict(precision=P, recall=R, density=c["density"] / (k * M), coverage=c["coverage"] / N,
                f_score=2.0 * P * R / (P + R) if P + R > 0 else 0.0, counts=c)


# ---- fixtures (computed once, shared, never changed: the arrays are read-only) ----------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# (N, M, D, k): real-valued cases whose precision, recall and coverage lie inside [0.05, 0.95] (test_manifold_host.py asserts it)
REAL_CASES = [(150, 97, 36, 3), (70, 133, 8, 1), (200, 130, 100, 5)]
# saturates at 1.0: serves the bit-level kernel tests only
SATURATED_CASE = (65, 64, 32, 15)
TIE_CASE = (150, 97, 8, 3)


@functools.lru_cache(maxsize=None)
def real_case(N, M, D):
    """Standard-normal real rows against 0.9 * normal + 0.35 generated rows, float32."""
    rng = np.random.RandomState(N * 1000003 + M * 1009 + D)
    return _frozen(rng.standard_normal((N, D)).astype(np.float32), (0.9 * rng.standard_normal((M, D)) + 0.35).astype(np.float32))


@functools.lru_cache(maxsize=None)
def tie_fixture():
    """Half-integer-valued features, round(2 x) / 2, with duplicated rows inside a side and across the sides: every distance is a
    multiple of 0.25 and many are equal, so `<` and `<=` differ."""
    N, M, D, _ = TIE_CASE
    rng = np.random.RandomState(150978)
    R = (np.round(2.0 * rng.standard_normal((N, D))) / 2.0).astype(np.float32)
    G = (np.round(2.0 * (0.9 * rng.standard_normal((M, D)) + 0.35)) / 2.0).astype(np.float32)
    R[10] = R[11] = R[3]
    G[5] = R[7]
    G[6] = G[2]
    return _frozen(R, G)


NEAR_K = 1


@functools.lru_cache(maxsize=None)
def near_duplicate_fixture(n=128, D=2048):
    """n rows of D in groups of four: the rows 4 i + 1 .. 4 i + 3 are row 4 i with ONE coordinate each moved by one ulp, so
    (n(x) + n(y)) - 2 dot(x, y) within a group is a difference of nearly equal numbers and comes out negative for some pairs.  With
    three such neighbours the unclamped radius of a row at k = 1 can itself be negative, which moves counts."""
    rng = np.random.RandomState(2048128)
    x = rng.standard_normal((n, D)).astype(np.float32)
    for i in range(0, n, 4):
        for g in range(1, 4):
            x[i + g] = x[i]
            j = (37 * i + 5 + 101 * g) % D
            x[i + g, j] = np.nextafter(x[i, j], np.float32(np.inf))
    return _frozen(x)[0]


@functools.lru_cache(maxsize=None)
def near_duplicate_sides():
    """(real, generated): the near-duplicate rows, and every third of them again as the generated side."""
    x = near_duplicate_fixture()
    return _frozen(x, x[1::3].copy())


def sides(name):
    """The (real, generated) rows and k of a fixture: name = a tuple (N, M, D, k), "tie" or "near"."""
    if name == "tie":
        return tie_fixture() + (TIE_CASE[3],)
    if name == "near":
        return near_duplicate_sides() + (NEAR_K,)
    return real_case(*name[:3]) + (name[3],)


@functools.lru_cache(maxsize=None)
def reference(name, variant=None):
    """prdc of a fixture (see sides) in the restatement, or in one of its wrong variants."""
    R, G, k = sides(name)
    return prdc(R, G, k, variant)


@functools.lru_cache(maxsize=None)
def reference_scans(name):
    R, G, k = sides(name)
    s = scans(R, G, k)
    s.pop("inside")
    _frozen(*s.values())
    return s

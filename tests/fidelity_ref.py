"""Float64 numpy restatement of the Inception Score and the Kernel Inception Distance as frido_amd/fidelity.py specifies them, and of the
in-order dot product of csrc/fidelity.hip.  Shares no code with the package: tests/test_fidelity_host.py holds it against scikit-learn's
polynomial kernel and scipy's log_softmax / softmax, tests/test_fidelity_gpu.py holds the kernels against it."""
import numpy as np


# ---- the kernel's own order (bit for bit) -----------------------------------------------------------------
def dot_in_order(x, y):
    """[nx, ny] float64: acc = fma((double)x[a, k], (double)y[b, k], acc) for k ascending from 0.0.  The product of two float32 values
    is exact in float64, so a separate multiply and add rounds exactly as the fma does."""
    x64, y64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    acc = np.zeros((x64.shape[0], y64.shape[0]), np.float64)
    for k in range(x64.shape[1]):
        acc = acc + x64[:, k, None] * y64[None, :, k]
    return acc


def poly_in_order(dot, gamma, coef0, degree):
    """((t * t) * t) * t with t = dot * gamma + coef0: numpy rounds every operation on its own."""
    t = np.asarray(dot, np.float64) * np.float64(gamma) + np.float64(coef0)
    r = t
    for _ in range(degree - 1):
        r = r * t
    return r


# ---- KID ----------------------------------------------------------------------------------------------------
def poly_kernel(x, y, degree=3, gamma=None, coef0=1.0):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    return (x @ y.T * gamma + coef0) ** degree


def gram_sums(x, y, degree=3, gamma=None, coef0=1.0, diagonal=False):
    """(sum K_XX, sum K_YY, sum K_XY) and (sum |K_XX|, ...) of one subset; K_XX and K_YY without their diagonals unless `diagonal`."""
    kxx, kyy, kxy = (poly_kernel(a, b, degree, gamma, coef0) for a, b in ((x, x), (y, y), (x, y)))
    if not diagonal:
        kxx, kyy = kxx - np.diag(np.diag(kxx)), kyy - np.diag(np.diag(kyy))
    return tuple(float(k.sum()) for k in (kxx, kyy, kxy)), tuple(float(np.abs(k).sum()) for k in (kxx, kyy, kxy))


def mmd2(x, y, degree=3, gamma=None, coef0=1.0, diagonal=False, biased_divisor=False):
    m = x.shape[0]
    (sxx, syy, sxy), _ = gram_sums(x, y, degree, gamma, coef0, diagonal)
    return (sxx + syy) / (m * m if biased_divisor else m * (m - 1)) - 2.0 * sxy / (m * m)


def kid_indices(n1, n2, subsets, subset_size, rng_seed=2020):
    rng = np.random.RandomState(rng_seed)
    out = []
    for _ in range(subsets):
        a = rng.choice(n1, subset_size, replace=False)
        out.append((a, rng.choice(n2, subset_size, replace=False)))
    return out


def kid(f1, f2, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, rng_seed=2020, **variant):
    """(mean, std, the subsets' mmd2)."""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    v = np.array([mmd2(f1[a], f2[b], degree, gamma, coef0, **variant) for a, b in kid_indices(len(f1), len(f2), subsets, subset_size, rng_seed)])
    return float(v.mean()), float(v.std()), v


# ---- Inception Score ----------------------------------------------------------------------------------------
def log_softmax(l):
    l = np.asarray(l, np.float64)
    z = l - l.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def isc_scores(logits, splits=10, shuffle=True, rng_seed=2020, marginal_over_all=False):
    """The split scores, float64 [splits]."""
    l = np.asarray(logits, np.float64)
    N = l.shape[0]
    if shuffle:
        l = l[np.random.RandomState(rng_seed).permutation(N)]
    logp = log_softmax(l)
    p = np.exp(logp)
    out = []
    for i in range(splits):
        lo, hi = i * N // splits, (i + 1) * N // splits
        q = (p if marginal_over_all else p[lo:hi]).mean(axis=0, keepdims=True)
        out.append(np.exp((p[lo:hi] * (logp[lo:hi] - np.log(q))).sum(axis=1).mean()))
    return np.array(out)


def isc(logits, splits=10, shuffle=True, rng_seed=2020, ddof=0, **variant):
    s = isc_scores(logits, splits, shuffle, rng_seed, **variant)
    return float(s.mean()), float(s.std(ddof=ddof))

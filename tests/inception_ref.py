"""Float64 restatement of the Fréchet Inception Distance, written from the layer table of Inception-v3 (torchvision's names) and the
formulas of include/frido_fid.h with torch's own convolutions and pools: the input transform, the pools, the tower, the global pool,
the statistics and the distance.  Nothing here imports frido_amd.fid: the tests hold the HIP path, its tables included, to this file.

`dtype` switches every function between float64 (the reference) and float32 (the restatement's own rounding error, which the GPU
tests' bounds are multiples of)."""
import numpy as np
import torch
import torch.nn.functional as F

PREFIX = "fid."          # the filler's key prefix
BN_EPS = 1e-3
S = 299


# ---- the input transform --------------------------------------------------------------------------------
def quantise(x, quant):
    """custom_to_pil / custom_to_np of scripts/sample_diffusion.py:103-121 on a float tensor in the tensor's own precision, truncated,
    as a float holding an integer."""
    if quant == "pil":
        u = 255 * ((torch.clamp(x, -1., 1.) + 1.) / 2.)
    else:
        u = ((x + 1) * 127.5).clamp(0, 255)
    return torch.trunc(u)


def resize_axis(n_in, n_out, dtype, centres="legacy"):
    """(i0, i1, f) of the bilinear resize along one axis.  "legacy": TF1 without half-pixel centres, src = dst * in / out; the other
    two are the WRONG variants the tests must tell apart: "half" (half-pixel centres) and "corners" (align_corners=True)."""
    d = torch.arange(n_out, dtype=dtype)
    if centres == "legacy":
        src = d * (torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype))
    elif centres == "half":
        src = ((d + 0.5) * (torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)) - 0.5).clamp_min(0)
    else:
        src = d * (torch.tensor(max(n_in - 1, 0), dtype=dtype) / torch.tensor(max(n_out - 1, 1), dtype=dtype))
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(dtype)


def preprocess(q, s=S, dtype=torch.float64, centres="legacy", divisor=128.0):
    """q: [B, 3, H, W] floats holding integers 0 .. 255 -> [B, 3, s, s]: rows first lerped in x, then in y, then (v - 128) / 128."""
    q = q.to(dtype)
    y0, y1, fy = resize_axis(q.shape[2], s, dtype, centres)
    x0, x1, fx = resize_axis(q.shape[3], s, dtype, centres)
    top, bot = q[:, :, y0], q[:, :, y1]
    top = top[..., x0] + (top[..., x1] - top[..., x0]) * fx
    bot = bot[..., x0] + (bot[..., x1] - bot[..., x0]) * fx
    v = top + (bot - top) * fy[:, None]
    return (v - 128.0) / divisor


def to_q(images, quant="pil", dtype=torch.float64, rounding="trunc"):
    """Either input layout -> [B, 3, H, W] integers as floats.  A float image is quantised in FLOAT32 whatever `dtype` is: the 8-bit
    value is the specification's input, not a quantity with a rounding error."""
    if images.dtype == torch.uint8:
        return images.permute(0, 3, 1, 2).to(dtype)
    x = images.float()
    if rounding == "nearest":      # a WRONG variant for the tests
        u = 255 * ((torch.clamp(x, -1., 1.) + 1.) / 2.) if quant == "pil" else ((x + 1) * 127.5).clamp(0, 255)
        return torch.round(u).to(dtype)
    return quantise(x, quant).to(dtype)


# ---- pools ----------------------------------------------------------------------------------------------
def avg_pool_in_order(x):
    """3 x 3, stride 1, padding 1, the padding left out of the divisor, in the kernel's order: the taps inside the plane added in
    (ky, kx) order in the tensor's precision, then ONE division by their count.  x: [B, C, H, W]."""
    B, C, H, W = x.shape
    acc = torch.zeros_like(x)
    cnt = torch.zeros(H, W, dtype=x.dtype)
    first = torch.ones(H, W, dtype=torch.bool)
    for ky in (-1, 0, 1):
        for kx in (-1, 0, 1):
            ys = slice(max(0, -ky), min(H, H - ky))
            xs = slice(max(0, -kx), min(W, W - kx))
            yd = slice(ys.start + ky, ys.stop + ky)
            xd = slice(xs.start + kx, xs.stop + kx)
            tap = x[:, :, yd, xd]
            f = first[ys, xs]
            acc[:, :, ys, xs] = torch.where(f, tap, acc[:, :, ys, xs] + tap)
            first[ys, xs] = False
            cnt[ys, xs] += 1
    return acc / cnt


def avg_pool(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def max_pool_s2(x):
    return F.max_pool2d(x, 3, stride=2)


def max_pool_s1(x):
    return F.max_pool2d(x, 3, stride=1, padding=1)


# ---- the tower ------------------------------------------------------------------------------------------
class Net:
    """The tower over a state_dict with torchvision's names.  `fold`: conv + BatchNorm as one conv with the folded weights (what the
    HIP path runs), else the conv and F.batch_norm apart.  `record`: a dict that receives every post-ReLU output by conv name."""

    def __init__(self, sd, dtype=torch.float64, fold=False, record=None):
        self.sd, self.dtype, self.fold, self.record = sd, dtype, fold, record

    def bc(self, x, name, stride=1, padding=0):
        g = lambda k: self.sd[f"{name}.{k}"]      # noqa: E731
        w = g("conv.weight").double()
        if self.fold:
            a = g("bn.weight").double() / torch.sqrt(g("bn.running_var").double() + BN_EPS)
            wf = (w * a.view(-1, 1, 1, 1)).float().to(self.dtype)      # rounded to float32 once, like the operand the kernel is given
            bf = (g("bn.bias").double() - g("bn.running_mean").double() * a).float().to(self.dtype)
            y = F.conv2d(x, wf, bf, stride=stride, padding=padding)
        else:
            y = F.conv2d(x, w.to(self.dtype), None, stride=stride, padding=padding)
            y = F.batch_norm(y, g("bn.running_mean").to(self.dtype), g("bn.running_var").to(self.dtype), g("bn.weight").to(self.dtype),
                             g("bn.bias").to(self.dtype), False, 0.0, BN_EPS)
        y = F.relu(y)
        if self.record is not None:
            self.record[name] = y
        return y

    def stem(self, x):
        x = self.bc(x, "Conv2d_1a_3x3", stride=2)
        x = self.bc(x, "Conv2d_2a_3x3")
        x = self.bc(x, "Conv2d_2b_3x3", padding=1)
        x = max_pool_s2(x)
        x = self.bc(x, "Conv2d_3b_1x1")
        x = self.bc(x, "Conv2d_4a_3x3")
        return max_pool_s2(x)

    def block_a(self, x, n):
        b1 = self.bc(x, n + ".branch1x1")
        b5 = self.bc(self.bc(x, n + ".branch5x5_1"), n + ".branch5x5_2", padding=2)
        b3 = self.bc(x, n + ".branch3x3dbl_1")
        b3 = self.bc(b3, n + ".branch3x3dbl_2", padding=1)
        b3 = self.bc(b3, n + ".branch3x3dbl_3", padding=1)
        bp = self.bc(avg_pool(x), n + ".branch_pool")
        return [b1, b5, b3, bp]

    def block_b(self, x, n):
        b3 = self.bc(x, n + ".branch3x3", stride=2)
        bd = self.bc(x, n + ".branch3x3dbl_1")
        bd = self.bc(bd, n + ".branch3x3dbl_2", padding=1)
        bd = self.bc(bd, n + ".branch3x3dbl_3", stride=2)
        return [b3, bd, max_pool_s2(x)]

    def block_c(self, x, n):
        b1 = self.bc(x, n + ".branch1x1")
        b7 = self.bc(x, n + ".branch7x7_1")
        b7 = self.bc(b7, n + ".branch7x7_2", padding=(0, 3))
        b7 = self.bc(b7, n + ".branch7x7_3", padding=(3, 0))
        bd = self.bc(x, n + ".branch7x7dbl_1")
        bd = self.bc(bd, n + ".branch7x7dbl_2", padding=(3, 0))
        bd = self.bc(bd, n + ".branch7x7dbl_3", padding=(0, 3))
        bd = self.bc(bd, n + ".branch7x7dbl_4", padding=(3, 0))
        bd = self.bc(bd, n + ".branch7x7dbl_5", padding=(0, 3))
        bp = self.bc(avg_pool(x), n + ".branch_pool")
        return [b1, b7, bd, bp]

    def block_d(self, x, n):
        b3 = self.bc(self.bc(x, n + ".branch3x3_1"), n + ".branch3x3_2", stride=2)
        b7 = self.bc(x, n + ".branch7x7x3_1")
        b7 = self.bc(b7, n + ".branch7x7x3_2", padding=(0, 3))
        b7 = self.bc(b7, n + ".branch7x7x3_3", padding=(3, 0))
        b7 = self.bc(b7, n + ".branch7x7x3_4", stride=2)
        return [b3, b7, max_pool_s2(x)]

    def block_e(self, x, n, pool):
        b1 = self.bc(x, n + ".branch1x1")
        b3 = self.bc(x, n + ".branch3x3_1")
        b3 = torch.cat([self.bc(b3, n + ".branch3x3_2a", padding=(0, 1)), self.bc(b3, n + ".branch3x3_2b", padding=(1, 0))], 1)
        bd = self.bc(self.bc(x, n + ".branch3x3dbl_1"), n + ".branch3x3dbl_2", padding=1)
        bd = torch.cat([self.bc(bd, n + ".branch3x3dbl_3a", padding=(0, 1)), self.bc(bd, n + ".branch3x3dbl_3b", padding=(1, 0))], 1)
        bp = self.bc(pool(x), n + ".branch_pool")
        return [b1, b3, bd, bp]

    def block(self, x, n):
        """The branch outputs of block `n` in concat order."""
        if n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            return self.block_a(x, n)
        if n == "Mixed_6a":
            return self.block_b(x, n)
        if n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            return self.block_c(x, n)
        if n == "Mixed_7a":
            return self.block_d(x, n)
        return self.block_e(x, n, avg_pool if n == "Mixed_7b" else max_pool_s1)

    def tower(self, x, inputs=None):
        """[B, 3, s, s] preprocessed images -> [B, 2048]; `inputs` receives every block's input by name."""
        x = self.stem(x.to(self.dtype))
        for n in BLOCK_NAMES:
            if inputs is not None:
                inputs[n] = x
            x = torch.cat(self.block(x, n), 1)
        return gap(x)


BLOCK_NAMES = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")


def gap(x):
    """[B, C, H, W] -> [B, C]: the pixels added in index order in float64, one division, rounded to the tensor's precision."""
    B, C, H, W = x.shape
    flat = x.reshape(B, C, H * W).double()
    acc = torch.zeros(B, C, dtype=torch.float64)
    for p in range(H * W):
        acc = acc + flat[:, :, p]
    return (acc / (H * W)).to(x.dtype)


def features(sd, images, quant="pil", s=S, dtype=torch.float64, fold=True):
    return Net(sd, dtype, fold).tower(preprocess(to_q(images, quant, dtype), s, dtype))


# ---- weights --------------------------------------------------------------------------------------------
def filled_state_dict(module, prefix=PREFIX):
    """The module's state_dict (parameters AND the BatchNorm buffers) from the "inception" filler, keyed by prefix + name."""
    from frido_amd.synth import fill_tensor
    out = {}
    for k, v in module.state_dict().items():
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros((), dtype=torch.long)
        else:
            out[k] = torch.from_numpy(fill_tensor(prefix + k, v.shape, "inception").copy())
    return out


def fill(module, prefix=PREFIX):
    sd = filled_state_dict(module, prefix)
    module.load_state_dict(sd)
    return sd


# ---- statistics and the distance ------------------------------------------------------------------------
def accumulate(x, s1=None, s2=None):
    """The in-order float64 sums of the rows of x [B, D] float32: s1 += x_b, s2 += x_b x_b^T, b ascending (products exact)."""
    x = x.double()
    D = x.shape[1]
    s1 = torch.zeros(D, dtype=torch.float64) if s1 is None else s1.clone()
    s2 = torch.zeros(D, D, dtype=torch.float64) if s2 is None else s2.clone()
    for b in range(x.shape[0]):
        s1 = s1 + x[b]
        s2 = s2 + torch.outer(x[b], x[b])
    return s1, s2


def mean_cov(x):
    x = np.asarray(x, dtype=np.float64)
    return x.mean(0), np.cov(x, rowvar=False)


def frechet_sqrtm(mu1, s1, mu2, s2):
    """torch-fidelity's formula: scipy.linalg.sqrtm of the unsymmetric product (full-rank inputs only: no eps branch)."""
    import scipy.linalg
    covmean, _ = scipy.linalg.sqrtm(np.asarray(s1).dot(np.asarray(s2)), disp=False)
    covmean = covmean.real
    diff = np.asarray(mu1) - np.asarray(mu2)
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def frechet_from_features(fa, fb):
    """The reference's distance from two feature sets [N, D], float64 all the way, by a route of its own: with A, B the centred
    features over sqrt(N - 1), sigma1 = A^T A and sigma2 = B^T B, and the non-zero eigenvalues of sigma1 sigma2 = A^T (A B^T) B are
    those of (A B^T)(A B^T)^T -- so tr sqrt(sigma1 sigma2) is the sum of the singular values of the N x N matrix A B^T.  No D x D
    matrix is formed and a covariance of rank N - 1 << D costs no accuracy."""
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    ma, mb = fa.mean(0), fb.mean(0)
    A, B = (fa - ma) / np.sqrt(fa.shape[0] - 1), (fb - mb) / np.sqrt(fb.shape[0] - 1)
    diff = ma - mb
    return float(diff @ diff + (A * A).sum() + (B * B).sum() - 2.0 * np.linalg.svd(A @ B.T, compute_uv=False).sum())

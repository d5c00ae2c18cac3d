"""Fréchet Inception Distance on the HIP engine: the ctypes binding of include/frido_fid.h (csrc/fid.hip: the input transform, the 3 x 3
pools, the global average pool, the float64 feature statistics), the table of Inception-v3's 94 convolutions, InceptionPlan -- the
compiled tower of one input shape --, FeatureStatistics and frechet_distance.

Bound beside `_lib`, not inside it, like frido_amd/lpips.py: these four launches are no op kinds.  The descriptors are parsed from their
own header with `_lib`'s parser, the functions are taken from the handle `_lib.lib()` returns for the active plane format (the code is
the same in both builds: f32 / f64 only), and every descriptor's size is compared with the library's at first use.  A library without the
symbols is a stale build and is named as one: there is no fallback.

The network is the FID variant of torchvision's Inception-v3 that torch-fidelity's FeatureExtractorInceptionV3 runs (its feature
'2048'): every average pool leaves the padding out of its divisor and Mixed_7c pools with a maximum.  The input transform's formula is
written at FridoFidPreprocess; it IS the specification here -- torch-fidelity is not installed to pin it against."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import FridoHipError
from .builder import ACT_RELU

HEADER = os.path.join(_lib.REPO, "include", "frido_fid.h")
_src = _lib._strip_comments(open(HEADER).read())
_structs = _lib._parse_structs(_src)
FridoFidPreprocess = type("FridoFidPreprocess", (C.Structure,), {"_fields_": _structs["FridoFidPreprocess"]})
FridoPool3 = type("FridoPool3", (C.Structure,), {"_fields_": _structs["FridoPool3"]})
FridoGap = type("FridoGap", (C.Structure,), {"_fields_": _structs["FridoGap"]})
FridoFeatAccum = type("FridoFeatAccum", (C.Structure,), {"_fields_": _structs["FridoFeatAccum"]})

# launcher -> (descriptor, the library's sizeof function)
LAUNCHERS = {"frido_fid_preprocess": (FridoFidPreprocess, "frido_sizeof_fid_preprocess"), "frido_pool3": (FridoPool3, "frido_sizeof_pool3"),
             "frido_gap": (FridoGap, "frido_sizeof_gap"), "frido_feat_accum": (FridoFeatAccum, "frido_sizeof_feat_accum")}

SRC_U8_HWC, SRC_F32_NCHW = 0, 1                      # FRIDO_FID_SRC_*
QUANT = {"pil": 2, "np": 1}                          # FRIDO_FID_QUANT_*: custom_to_pil / custom_to_np of scripts/sample_diffusion.py:103-121
POOL_MAX_S2, POOL_MAX_S1P1, POOL_AVG_S1P1 = 0, 1, 2  # FRIDO_POOL3_*
RESOLUTION = 299
FEATURES = 2048
BN_EPS = 1e-3                                        # BasicConv2d's BatchNorm2d(eps=0.001)
FC_SHAPE = (1008, 2048)                              # the checkpoint's fc: FIDInceptionV3.logits runs its weight (no bias), forward never
MIN_SIDE = 1                                         # the resize takes any source size

_bound = {}      # plane format -> {launcher name: function of that build}


def _fns(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        fns = {}
        for name, (struct, sizeof) in LAUNCHERS.items():
            for sym in (name, sizeof):
                if not hasattr(L, sym):
                    raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {sym}: a stale build from before csrc/fid.hip "
                                        "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
            c_sz = getattr(L, sizeof)()
            if c_sz != C.sizeof(struct):
                raise FridoHipError(f"ABI mismatch: sizeof({struct.__name__}) C={c_sz} py={C.sizeof(struct)} "
                                    "(include/frido_fid.h and the build disagree: stale build?)")
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


def preprocess_desc(src_ptr, dst_ptr, B, H, W, S=RESOLUTION, *, src_kind, quant="pil"):
    """A filled FridoFidPreprocess: uint8 [B][H][W][3] or f32 [B][3][H][W] -> dst [B * S * S][3] f32."""
    return FridoFidPreprocess(src=src_ptr, dst=dst_ptr, B=B, H=H, W=W, S=S, src_kind=src_kind, quant=QUANT[quant])


def pool_desc(src_ptr, dst_ptr, B, H, W, Cn, mode, ldd=None, c0=0):
    return FridoPool3(src=src_ptr, dst=dst_ptr, B=B, H=H, W=W, C=Cn, ldd=Cn if ldd is None else ldd, c0=c0, mode=mode)


def gap_desc(src_ptr, dst_ptr, B, HW, Cn):
    return FridoGap(src=src_ptr, dst=dst_ptr, B=B, HW=HW, C=Cn)


def accum_desc(x_ptr, s1_ptr, s2_ptr, B, D):
    return FridoFeatAccum(x=x_ptr, s1=s1_ptr, s2=s2_ptr, B=B, D=D)


def pool_out(h, mode):
    """Output side of a 3 x 3 pool: stride 2 without padding (floor), or stride 1 with padding 1."""
    return (h - 3) // 2 + 1 if mode == POOL_MAX_S2 else h


# ---- the net's shape ------------------------------------------------------------------------------------
def _c(name, cout, kh=1, kw=1, stride=1, pad=0, padx=None):
    return (name, cout, kh, kw, stride, pad, pad if padx is None else padx)


STEM = (_c("Conv2d_1a_3x3", 32, 3, 3, 2), _c("Conv2d_2a_3x3", 32, 3, 3), _c("Conv2d_2b_3x3", 64, 3, 3, pad=1), "pool",
        _c("Conv2d_3b_1x1", 80), _c("Conv2d_4a_3x3", 192, 3, 3), "pool")
# name -> (kind, input channels, the kind's parameter): A's pool features, C's c7, E's pool ("avg" in Mixed_7b, "max" in Mixed_7c)
BLOCKS = {"Mixed_5b": ("A", 192, 32), "Mixed_5c": ("A", 256, 64), "Mixed_5d": ("A", 288, 64), "Mixed_6a": ("B", 288, None),
          "Mixed_6b": ("C", 768, 128), "Mixed_6c": ("C", 768, 160), "Mixed_6d": ("C", 768, 160), "Mixed_6e": ("C", 768, 192),
          "Mixed_7a": ("D", 768, None), "Mixed_7b": ("E", 1280, "avg"), "Mixed_7c": ("E", 2048, "max")}


def _r17(name, cout):      # (1, 7), padding (0, 3)
    return _c(name, cout, 1, 7, pad=0, padx=3)


def _r71(name, cout):      # (7, 1), padding (3, 0)
    return _c(name, cout, 7, 1, pad=3, padx=0)


def block_branches(kind, param):
    """The branches of one block in concat order: (pool in front of the branch or None, the chain of convs, the convs that all read the
    chain's end and are concatenated).  A branch without convs is its pool alone, written straight into the concat."""
    if kind == "A":
        return [(None, [_c("branch1x1", 64)], []),
                (None, [_c("branch5x5_1", 48), _c("branch5x5_2", 64, 5, 5, pad=2)], []),
                (None, [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, 3, 3, pad=1), _c("branch3x3dbl_3", 96, 3, 3, pad=1)], []),
                (POOL_AVG_S1P1, [_c("branch_pool", param)], [])]
    if kind == "B":
        return [(None, [_c("branch3x3", 384, 3, 3, 2)], []),
                (None, [_c("branch3x3dbl_1", 64), _c("branch3x3dbl_2", 96, 3, 3, pad=1), _c("branch3x3dbl_3", 96, 3, 3, 2)], []),
                (POOL_MAX_S2, [], [])]
    if kind == "C":
        c7 = param
        return [(None, [_c("branch1x1", 192)], []),
                (None, [_c("branch7x7_1", c7), _r17("branch7x7_2", c7), _r71("branch7x7_3", 192)], []),
                (None, [_c("branch7x7dbl_1", c7), _r71("branch7x7dbl_2", c7), _r17("branch7x7dbl_3", c7), _r71("branch7x7dbl_4", c7),
                        _r17("branch7x7dbl_5", 192)], []),
                (POOL_AVG_S1P1, [_c("branch_pool", 192)], [])]
    if kind == "D":
        return [(None, [_c("branch3x3_1", 192), _c("branch3x3_2", 320, 3, 3, 2)], []),
                (None, [_c("branch7x7x3_1", 192), _r17("branch7x7x3_2", 192), _r71("branch7x7x3_3", 192), _c("branch7x7x3_4", 192, 3, 3, 2)], []),
                (POOL_MAX_S2, [], [])]
    if kind == "E":
        def pair(stem):
            return [_c(stem + "a", 384, 1, 3, pad=0, padx=1), _c(stem + "b", 384, 3, 1, pad=1, padx=0)]
        return [(None, [_c("branch1x1", 320)], []),
                (None, [_c("branch3x3_1", 384)], pair("branch3x3_2")),
                (None, [_c("branch3x3dbl_1", 448), _c("branch3x3dbl_2", 384, 3, 3, pad=1)], pair("branch3x3dbl_3")),
                (POOL_AVG_S1P1 if param == "avg" else POOL_MAX_S1P1, [_c("branch_pool", 192)], [])]
    raise ValueError(f"unknown Inception block kind {kind!r}")


def block_widths(name):
    """Output channels of each branch of the block `name`, in concat order."""
    kind, cin, param = BLOCKS[name]
    out = []
    for pool, chain, tails in block_branches(kind, param):
        out.append(sum(t[1] for t in tails) if tails else chain[-1][1] if chain else cin)
    return out


def conv_table():
    """[(dotted name, cin, cout, kh, kw, stride, pad, padx)] of the 94 convolutions, in the order they run."""
    rows, cin = [], 3
    for spec in STEM:
        if spec == "pool":
            continue
        rows.append((spec[0], cin) + spec[1:])
        cin = spec[1]
    for name, (kind, bc, param) in BLOCKS.items():
        for pool, chain, tails in block_branches(kind, param):
            c = bc
            for spec in chain:
                rows.append((f"{name}.{spec[0]}", c) + spec[1:])
                c = spec[1]
            for spec in tails:
                rows.append((f"{name}.{spec[0]}", c) + spec[1:])
    return rows


def tower_planes(S=RESOLUTION):
    """The plane side in front of each block and behind the last one, {"Mixed_5b": 35, ..., "head": 8} at S = 299; None where a conv or
    a pool is left without an output pixel."""
    h = S
    for spec in STEM:
        h = pool_out(h, POOL_MAX_S2) if spec == "pool" else (h + 2 * spec[5] - spec[2]) // spec[4] + 1
        if h < 1:
            return None
    out = {}
    for name, (kind, _, _) in BLOCKS.items():
        out[name] = h
        if kind in ("B", "D"):
            h = pool_out(h, POOL_MAX_S2)
            if h < 1:
                return None
    out["head"] = h
    return out


# ---- BatchNorm, folded into the conv on the host in float64 and rounded once ----------------------------
def fold_conv_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) + eval-mode BatchNorm2d as ONE conv:  a = gamma / sqrt(var + eps),  w' = w a,  b' = beta - mean a."""
    a = gamma.detach().cpu().double() / torch.sqrt(var.detach().cpu().double() + eps)
    wf = w.detach().cpu().double() * a.view(-1, 1, 1, 1)
    bf = beta.detach().cpu().double() - mean.detach().cpu().double() * a
    return wf.float(), bf.float()


def folded_weights(sd, device):
    """{name.weight, name.bias} float32 on `device` for the 94 convolutions, from a state_dict with torchvision's names."""
    out = {}
    for row in conv_table():
        n = row[0]
        wf, bf = fold_conv_bn(sd[n + ".conv.weight"], sd[n + ".bn.weight"], sd[n + ".bn.bias"], sd[n + ".bn.running_mean"],
                              sd[n + ".bn.running_var"])
        out[n + ".weight"], out[n + ".bias"] = wf.contiguous().to(device), bf.contiguous().to(device)
    return out


# ---- emission -------------------------------------------------------------------------------------------
class Cols:
    """Columns c0 .. of an f32 activation [rows][C]: what Builder.conv's out=("f32", view) writes with the activation's own leading
    dimension, so that a branch's last conv lands in its range of the block's concat."""

    def __init__(self, act, c0):
        self.ptr, self.C, self.rows = act.ptr + 4 * c0, act.C, act.rows


def _conv(b, a, B, h, w, prefix, spec, out):
    name, cout, kh, kw, stride, pad, padx = spec
    return b.conv(a, B, h, w, prefix + name, stride=stride, pad=pad, padx=None if padx == pad else padx, act=ACT_RELU, out=out)


def _chain(b, a, B, h, w, prefix, specs, last_out):
    """The convs `specs` in a row from the operand `a` (not freed here); every output an operand where Cout % 32 == 0, else f32 + PACK
    (the 48- and 80-channel ones); the last one goes to `last_out` (an out= of Builder.conv).  Returns (result, h, w)."""
    cur = a
    for i, spec in enumerate(specs):
        _, cout, kh, kw, stride, pad, padx = spec
        last = i == len(specs) - 1
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * padx - kw) // stride + 1
        if last:
            o = _conv(b, cur, B, h, w, prefix, spec, last_out)
        elif cout % 32 == 0:
            o = _conv(b, cur, B, h, w, prefix, spec, "op")
        else:
            f = _conv(b, cur, B, h, w, prefix, spec, "f32_strict")
            o = b.pack(f.ptr, 1, B * ho * wo, cout, 0, cout)
            f.free()
        if cur is not a:
            cur.free()
        cur, h, w = o, ho, wo
    return cur, h, w


def emit_block(b, name, a_in, B, h, w):
    """One Mixed_* block on the builder's current program.  a_in: the block's f32 input [B * h * w][Cin] (anything with .ptr and .C; it is
    read by the pool launch and by the program's PACK, the caller frees it).  Returns (pool, out, ho, wo): the filled FridoPool3 that has
    to be launched BEFORE the program, and the block's f32 output [B * ho * wo][Ctot] with the branches in torchvision's concat order.
    Every branch's last conv writes its column range of `out` itself; B and D blocks pool straight into the last range."""
    kind, cin, param = BLOCKS[name]
    assert a_in.C == cin, (name, a_in.C, cin)
    branches = block_branches(kind, param)
    widths = block_widths(name)
    reduce = kind in ("B", "D")
    ho, wo = (pool_out(h, POOL_MAX_S2), pool_out(w, POOL_MAX_S2)) if reduce else (h, w)
    out = b.f32_strict(B * ho * wo, sum(widths))
    # The pool launch runs BEFORE this program, so what it writes must not be a buffer the program uses earlier for something else:
    # `out` and `pooled` are taken from the pool before anything of this block is released into it.
    pooled = None if reduce else b.f32_strict(B * h * w, cin)
    x = b.pack(a_in.ptr, 1, B * h * w, cin, 0, cin)
    pool, c0 = None, 0
    for (mode, chain, tails), width in zip(branches, widths):
        if mode is not None and not chain:                      # B, D: the pooled input IS the branch
            pool = pool_desc(a_in.ptr, out.ptr, B, h, w, cin, mode, ldd=out.C, c0=c0)
        elif mode is not None:                                  # A, C, E: pool -> PACK -> branch_pool's 1 x 1
            pool = pool_desc(a_in.ptr, pooled.ptr, B, h, w, cin, mode)
            px = b.pack(pooled.ptr, 1, B * h * w, cin, 0, cin)
            _chain(b, px, B, h, w, name + ".", chain, ("f32", Cols(out, c0)))
            px.free()
            pooled.free()
        elif tails:                                             # E: two convs on the chain's end, side by side
            mid, mh, mw = _chain(b, x, B, h, w, name + ".", chain, "op")
            t0 = c0
            for spec in tails:
                _conv(b, mid, B, mh, mw, name + ".", spec, ("f32", Cols(out, t0)))
                t0 += spec[1]
            mid.free()
        else:
            _chain(b, x, B, h, w, name + ".", chain, ("f32", Cols(out, c0)))
        c0 += width
    x.free()
    return pool, out, ho, wo


class InceptionPlan:
    """The tower of one input shape (B, H, W, dtype) on a Builder over the FOLDED weights (folded_weights):

        frido_fid_preprocess(x_in)                                   [B * 299 * 299][3] f32 NHWC (csrc/fid.hip)
        stem program 1:     PACK -> Conv2d_1a, 2a, 2b                conv + bias + ReLU launches of the implicit GEMM, operand to operand
        frido_pool3 (max, stride 2)
        stem program 2:     PACK -> Conv2d_3b -> PACK -> Conv2d_4a   (80 channels are no operand width: f32 and PACK)
        frido_pool3 (max, stride 2)
        eleven times:       frido_pool3, then the block's program    emit_block
        frido_gap                                                    out [B][2048]

    The pools and the head are no op kinds, so they sit BETWEEN the programs; `launch` issues everything in order on one stream and the
    caller captures that as one graph.  `x_in` and `out` are fixed buffers."""

    def __init__(self, b, *, B, H, W, uint8, quant="pil", S=RESOLUTION):
        self.b = b
        dev = b.device
        planes = tower_planes(S)
        assert planes is not None, S
        self.x_in = (torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev) if uint8 else
                     torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev))
        self.out = torch.zeros(B, FEATURES, dtype=torch.float32, device=dev)
        self.pre = b.persistent_f32(B * S * S, 3)
        self.steps = [("frido_fid_preprocess", preprocess_desc(self.x_in.data_ptr(), self.pre.data_ptr(), B, H, W, S,
                                                               src_kind=SRC_U8_HWC if uint8 else SRC_F32_NCHW, quant=quant))]
        self.progs = []
        src_ptr, cin, h = self.pre.data_ptr(), 3, S
        act, group = None, []
        for spec in STEM:
            if spec != "pool":
                group.append(spec)
                continue
            prog = b.new_prog()
            a = b.pack(src_ptr, 1, B * h * h, cin, 0, cin)
            if act is not None:
                act.free()
            o, h, _ = _chain(b, a, B, h, h, "", group, "f32_strict")
            a.free()
            self.progs.append(prog)
            self.steps.append(("prog", prog))
            hp = pool_out(h, POOL_MAX_S2)
            act = b.f32_strict(B * hp * hp, o.C)
            self.steps.append(("frido_pool3", pool_desc(o.ptr, act.ptr, B, h, h, o.C, POOL_MAX_S2)))
            o.free()
            src_ptr, cin, h, group = act.ptr, act.C, hp, []
        w = h
        for name in BLOCKS:
            assert h == planes[name], (name, h, planes[name])
            prog = b.new_prog()
            pool, o, ho, wo = emit_block(b, name, act, B, h, w)
            act.free()
            self.progs.append(prog)
            self.steps.append(("frido_pool3", pool))
            self.steps.append(("prog", prog))
            act, h, w = o, ho, wo
        self.last = act               # the head's input (a pool buffer, never freed)
        self.steps.append(("frido_gap", gap_desc(act.ptr, self.out.data_ptr(), B, h * w, act.C)))
        self.graph = None

    def launch(self, stream):
        """Every launch of the plan in order on `stream` (directly, or inside a capture)."""
        for name, what in self.steps:
            if name == "prog":
                what.run(stream)
            else:
                launch(name, what, stream)


# ---- statistics and the distance ------------------------------------------------------------------------
class FeatureStatistics:
    """Streaming first and second moments of [*, D] float32 features in float64: `n` (a host int), `s1` [D] = sum x and `s2` [D][D] =
    sum x x^T on the device.  update() is one launch of frido_feat_accum (b ascending, products exact: one defined value, bitwise
    symmetric, the same bits for the same rows however they are batched); mean() and cov() are float64 torch expressions on the device."""

    def __init__(self, D=FEATURES, device="cuda"):
        self.D, self.device, self.n = int(D), torch.device(device), 0
        self.s1 = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.s2 = torch.zeros(self.D, self.D, dtype=torch.float64, device=self.device)

    @_lib.with_planes
    def update(self, features):
        from .engine import current_stream_ptr, require_gpu
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != self.D or features.dtype != torch.float32:
            got = (tuple(features.shape), features.dtype) if torch.is_tensor(features) else type(features).__name__
            raise ValueError(f"FeatureStatistics.update: features must be a float32 [B, {self.D}] tensor, got {got}")
        if features.device.type != "cuda" or self.device.type != "cuda":
            raise FridoHipError(f"FeatureStatistics.update: features on '{features.device}', sums on '{self.device}', but the accumulation "
                                "runs only on an MI355X HIP device; there is no CPU fallback")
        if features.shape[0] == 0:
            return self
        require_gpu(self.device)
        x = features.detach().contiguous()
        launch("frido_feat_accum", accum_desc(x.data_ptr(), self.s1.data_ptr(), self.s2.data_ptr(), x.shape[0], self.D),
               current_stream_ptr(self.device))
        x.record_stream(torch.cuda.current_stream(self.device))
        self.n += int(x.shape[0])
        return self

    def mean(self):
        if self.n < 1:
            raise ValueError("FeatureStatistics.mean: no features were added")
        return self.s1 / self.n

    def cov(self):
        """The unbiased covariance (s2 - n mu mu^T) / (n - 1), float64 [D][D]."""
        if self.n < 2:
            raise ValueError(f"FeatureStatistics.cov: a covariance needs at least 2 samples, got {self.n}")
        mu = self.s1 / self.n
        return (self.s2 - self.n * torch.outer(mu, mu)) / (self.n - 1)

    def save(self, path):
        """An .npz with mu, sigma, n: the form precomputed reference statistics are passed around in."""
        with open(path, "wb") as f:      # a file object: numpy appends no suffix of its own
            np.savez(f, mu=self.mean().cpu().numpy(), sigma=self.cov().cpu().numpy(), n=np.int64(self.n))

    @classmethod
    def load(cls, path, device="cpu"):
        """The statistics a save() wrote: the sums are restored from mu, sigma and n (s1 = n mu, s2 = (n - 1) sigma + n mu mu^T)."""
        z = np.load(path)
        mu, sigma, n = torch.from_numpy(z["mu"]).double(), torch.from_numpy(z["sigma"]).double(), int(z["n"])
        if mu.dim() != 1 or sigma.shape != (mu.shape[0], mu.shape[0]) or n < 2:
            raise ValueError(f"FeatureStatistics.load: {path} holds mu {tuple(mu.shape)}, sigma {tuple(sigma.shape)}, n {n}")
        st = cls(mu.shape[0], device)
        st.n = n
        st.s1 = (n * mu).to(st.device)
        st.s2 = ((n - 1) * sigma + n * torch.outer(mu, mu)).to(st.device)
        return st

    @classmethod
    def merge(cls, parts):
        """The statistics of all samples of `parts`: n, s1, s2 added in list order (float64 sums in a fixed order)."""
        parts = list(parts)
        if not parts:
            raise ValueError("FeatureStatistics.merge: nothing to merge")
        if any(p.D != parts[0].D for p in parts):
            raise ValueError(f"FeatureStatistics.merge: feature widths differ: {[p.D for p in parts]}")
        st = cls(parts[0].D, parts[0].device)
        for p in parts:
            st.n += p.n
            st.s1 = st.s1 + p.s1.to(st.device)
            st.s2 = st.s2 + p.s2.to(st.device)
        return st

    def all_gather_merge(self, group=None):
        """The statistics over every rank's samples: the sums are GATHERED and added in rank order on every rank (an all-reduce adds in
        an order of its own, which would not be reproducible bit for bit).  Without an initialised process group: self."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        world = dist.get_world_size(group)
        on_host = dist.get_backend(group) == "gloo"
        dev = torch.device("cpu") if on_host else self.device
        flat = torch.cat([torch.tensor([float(self.n)], dtype=torch.float64, device=dev), self.s1.to(dev), self.s2.to(dev).flatten()])
        got = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(got, flat, group=group)
        parts = []
        for g in got:
            p = FeatureStatistics(self.D, self.device)
            p.n = int(g[0].item())
            p.s1 = g[1:1 + self.D].to(self.device)
            p.s2 = g[1 + self.D:].view(self.D, self.D).to(self.device)
            parts.append(p)
        return FeatureStatistics.merge(parts)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr(sigma1) + tr(sigma2) - 2 tr sqrt(sigma1 sigma2) as a float, in float64 on the host.  The last term by the
    symmetric route: sqrt(sigma1 sigma2) has the eigenvalues of r sigma2 r with r = sqrt(sigma1) (symmetric, from eigh with the
    eigenvalues clamped at 0), so the trace is the sum of the clamped square roots of eigvalsh(r sigma2 r) -- no scipy.linalg.sqrtm of an
    unsymmetric product and no eps offset for singular covariances, which is what torch-fidelity does.  The result is not clamped: a
    distance of a distribution to itself comes out as rounding noise of either sign."""
    def host(t):
        return (t.detach() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).to("cpu", torch.float64)
    mu1, sigma1, mu2, sigma2 = host(mu1), host(sigma1), host(mu2), host(sigma2)
    D = mu1.shape[0]
    if mu1.dim() != 1 or mu2.shape != (D,) or sigma1.shape != (D, D) or sigma2.shape != (D, D):
        raise ValueError(f"frechet_distance: mu {tuple(mu1.shape)} / {tuple(mu2.shape)} and sigma {tuple(sigma1.shape)} / "
                         f"{tuple(sigma2.shape)} are not two [D] means with two [D, D] covariances of one D")
    lam, q = torch.linalg.eigh((sigma1 + sigma1.T) / 2)
    r = (q * lam.clamp_min(0).sqrt()) @ q.T
    m = r @ ((sigma2 + sigma2.T) / 2) @ r
    ev = torch.linalg.eigvalsh((m + m.T) / 2)
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(sigma1) + torch.trace(sigma2) - 2 * ev.clamp_min(0).sqrt().sum())

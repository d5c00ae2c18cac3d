"""ctypes binding of include/frido_patchgan.h (csrc/patchgan.hip: the discriminator's stem, the folded norm + LeakyReLU, the one-channel
head, the GAN terms and their finish), the host-side folding of the two norm kinds, and PatchGanPlan, the compiled discriminator of one
input shape.

Bound beside `_lib`, not inside it, like frido_amd/lpips.py: these five launches are no op kinds.  The descriptors are parsed from their
own header with `_lib`'s parser, the functions are taken from the handle `_lib.lib()` returns for the active plane format (the code is
the same in both builds: f32 / f64 only), and every descriptor's size is compared with the library's at first use.  A library without the
symbols is a stale build and is named as one: there is no fallback."""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import FridoHipError

HEADER = os.path.join(_lib.REPO, "include", "frido_patchgan.h")
_structs = _lib._parse_structs(_lib._strip_comments(open(HEADER).read()))
FridoDiscStem = type("FridoDiscStem", (C.Structure,), {"_fields_": _structs["FridoDiscStem"]})
FridoAffineLeaky = type("FridoAffineLeaky", (C.Structure,), {"_fields_": _structs["FridoAffineLeaky"]})
FridoDiscHead = type("FridoDiscHead", (C.Structure,), {"_fields_": _structs["FridoDiscHead"]})
FridoGanTerms = type("FridoGanTerms", (C.Structure,), {"_fields_": _structs["FridoGanTerms"]})
FridoGanFinish = type("FridoGanFinish", (C.Structure,), {"_fields_": _structs["FridoGanFinish"]})

# launcher -> (descriptor, the library's sizeof function)
LAUNCHERS = {"frido_disc_stem": (FridoDiscStem, "frido_sizeof_disc_stem"), "frido_affine_leaky": (FridoAffineLeaky, "frido_sizeof_affine_leaky"),
             "frido_disc_head": (FridoDiscHead, "frido_sizeof_disc_head"), "frido_gan_terms": (FridoGanTerms, "frido_sizeof_gan_terms"),
             "frido_gan_finish": (FridoGanFinish, "frido_sizeof_gan_finish")}

SLOPE = 0.2               # nn.LeakyReLU(0.2, True), discriminator/model.py:41,50,58
KW, PADW = 4, 1           # model.py:39-40
MAX_INPUT_NC = 8          # frido_disc_stem: Cin <= 8
STEM_MAX_WEIGHTS = 512    # ndf * Cin: the stem's weights in 32 KB of LDS
BN_EPS = 1e-5             # nn.BatchNorm2d's default
OUT_NAMES = ("logits_real", "logits_fake", "g_loss", "hinge", "vanilla")      # FridoGanFinish.out

_bound = {}      # plane format -> {launcher name: function of that build}


def _fns(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        fns = {}
        for name, (struct, sizeof) in LAUNCHERS.items():
            for sym in (name, sizeof):
                if not hasattr(L, sym):
                    raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {sym}: a stale build from before csrc/patchgan.hip "
                                        "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
            c_sz = getattr(L, sizeof)()
            if c_sz != C.sizeof(struct):
                raise FridoHipError(f"ABI mismatch: sizeof({struct.__name__}) C={c_sz} py={C.sizeof(struct)} "
                                    "(include/frido_patchgan.h and the build disagree: stale build?)")
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


def stem_desc(x_ptr, y_ptr, w_ptr, bias_ptr, dst_ptr, B, Cin, H, W, ndf, slope=SLOPE):
    """A filled FridoDiscStem: x, y [B][Cin][H][W] f32 (y may be None) -> dst [S * Ho * Wo][ndf] f32, x's samples first."""
    return FridoDiscStem(x=x_ptr, y=y_ptr, w=w_ptr, bias=bias_ptr, dst=dst_ptr, B=B, Cin=Cin, H=H, W=W, ndf=ndf, slope=slope)


def affine_desc(src_ptr, a_ptr, b_ptr, dst_ptr, rows, Cn, slope=SLOPE):
    return FridoAffineLeaky(src=src_ptr, a=a_ptr, b=b_ptr, dst=dst_ptr, rows=rows, C=Cn, slope=slope)


def head_desc(src_ptr, w_ptr, logits_ptr, S, H, W, Cn, bias):
    return FridoDiscHead(src=src_ptr, w=w_ptr, logits=logits_ptr, S=S, H=H, W=W, C=Cn, bias=bias)


def terms_desc(logits_ptr, sums_ptr, S, n):
    return FridoGanTerms(logits=logits_ptr, sums=sums_ptr, S=S, n=n)


def finish_desc(sums_ptr, out_ptr, per_sample_ptr, B, n):
    return FridoGanFinish(sums=sums_ptr, out=out_ptr, per_sample=per_sample_ptr, B=B, n=n)


# ---- the net's shape ------------------------------------------------------------------------------------
def layer_table(input_nc, ndf, n_layers):
    """[(index of the conv in `main`, index of its norm or None, cin, cout, stride)] of discriminator/model.py:41-62: the stem, the
    n_layers - 1 stride-2 convs, the stride-1 conv, the one-channel head."""
    rows = [(0, None, input_nc, ndf, 2)]
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        rows.append((3 * n - 1, 3 * n, ndf * prev, ndf * mult, 2))
    prev, mult = mult, min(2 ** n_layers, 8)
    rows.append((3 * n_layers - 1, 3 * n_layers, ndf * prev, ndf * mult, 1))
    rows.append((3 * n_layers + 2, None, ndf * mult, 1, 1))
    return rows


def conv_out(h, stride):
    """Output side of a 4 x 4 conv with padding 1 (floor division, like torch)."""
    return (h + 2 * PADW - KW) // stride + 1


def plane_sizes(H, W, n_layers):
    """(h, w) after each of the n_layers + 2 convs; None when some conv is left without an output pixel."""
    out = []
    for stride in [2] * n_layers + [1, 1]:
        if H + 2 * PADW < KW or W + 2 * PADW < KW:
            return None
        H, W = conv_out(H, stride), conv_out(W, stride)
        if H < 1 or W < 1:
            return None
        out.append((H, W))
    return out


# ---- the norms, folded on the host in float64 and rounded once ------------------------------------------
def fold_batchnorm(weight, bias, running_mean, running_var, eps=BN_EPS):
    """Eval-mode BatchNorm2d as v = a x + b:  a = gamma / sqrt(running_var + eps),  b = beta - running_mean a."""
    a = weight.detach().cpu().double() / torch.sqrt(running_var.detach().cpu().double() + eps)
    b = bias.detach().cpu().double() - running_mean.detach().cpu().double() * a
    return a.float(), b.float()


def fold_actnorm(loc, scale, conv_bias):
    """ActNorm (taming/modules/util.py:58, h = scale (x + loc)) behind a biased conv as v = a x + b:  a = scale,  b = scale (bias + loc)."""
    a = scale.detach().cpu().double().flatten()
    b = a * (conv_bias.detach().cpu().double().flatten() + loc.detach().cpu().double().flatten())
    return a.float(), b.float()


def fold_norm(sd, prefix, conv_idx, norm_idx, use_actnorm):
    """(a, b) float32 [C] of the norm main.<norm_idx> behind the conv main.<conv_idx>, from a state_dict with the reference's names."""
    p = f"{prefix}main.{norm_idx}."
    if use_actnorm:
        return fold_actnorm(sd[p + "loc"], sd[p + "scale"], sd[f"{prefix}main.{conv_idx}.bias"])
    return fold_batchnorm(sd[p + "weight"], sd[p + "bias"], sd[p + "running_mean"], sd[p + "running_var"])


def repack_stem_weight(w):
    """main.0.weight [ndf][Cin][4][4] -> [ndf][4][4][Cin] float32, contiguous."""
    return w.detach().float().permute(0, 2, 3, 1).contiguous()


def repack_head_weight(w):
    """The last conv's weight [1][C][4][4] -> [4][4][C] float32, contiguous."""
    return w.detach().float()[0].permute(1, 2, 0).contiguous()


class PatchGanPlan:
    """NLayerDiscriminator.forward (discriminator/model.py:65-67) of one input shape (B, H, W) on a Builder over the module's weights; with
    `pair` the real and the fake images go through the net together as ONE batch of S = 2B (eval-mode norms are per-sample: no value
    changes), followed by the GAN terms:

        frido_disc_stem(x_in, y_in)                                  [S * h1 * w1][ndf] f32 NHWC (csrc/patchgan.hip)
        per middle conv:    PACK -> 4 x 4 conv GEMM (f32 out, no bias, no activation), then frido_affine_leaky in place
        frido_disc_head                                              logits [S][Ho][Wo]
        pair only:          frido_gan_terms, frido_gan_finish        sums [S][5] f64, out [5], per_sample [S]

    The stem, the affines and the head are no op kinds, so they sit BETWEEN the slice programs; `launch` issues everything in order on
    one stream and the caller captures that as one graph.  `x_in`, `y_in`, `logits`, `out`, `per_sample` are fixed buffers."""

    def __init__(self, b, *, B, H, W, pair, input_nc, ndf, n_layers, consts):
        self.b, self.pair = b, pair
        dev = b.device
        S = 2 * B if pair else B
        table = layer_table(input_nc, ndf, n_layers)
        self.planes_hw = plane_sizes(H, W, n_layers)
        assert self.planes_hw is not None, (H, W, n_layers)
        self.x_in = torch.zeros(B, input_nc, H, W, dtype=torch.float32, device=dev)
        self.y_in = torch.zeros(B, input_nc, H, W, dtype=torch.float32, device=dev) if pair else None
        Ho, Wo = self.planes_hw[-1]
        self.logits = b.persistent_f32(S, 1, Ho, Wo, zero=True)
        h, w = self.planes_hw[0]
        act = b.f32_strict(S * h * w, ndf)
        self.steps = [("frido_disc_stem", stem_desc(self.x_in.data_ptr(), self.y_in.data_ptr() if pair else None, consts["stem_w"].data_ptr(),
                                                    consts["stem_b"].data_ptr(), act.ptr, B, input_nc, H, W, ndf))]
        self.progs = []
        for li, (ci, ni, cin, cout, stride) in enumerate(table[1:-1], start=1):
            ho, wo = self.planes_hw[li]
            prog = b.new_prog()
            a = b.pack(act.ptr, 1, S * h * w, cin, 0, cin)          # channels zero-padded to the operand's multiple of 32 here
            o = b.conv(a, S, h, w, f"main.{ci}", stride=stride, pad=PADW, bias=False, out="f32_strict")
            a.free()
            act.free()                # read by this program's PACK only; later programs may reuse it (one stream, in order)
            av, bv = consts["affine"][ni]
            self.progs.append(prog)
            self.steps.append(("prog", prog))
            self.steps.append(("frido_affine_leaky", affine_desc(o.ptr, av.data_ptr(), bv.data_ptr(), o.ptr, S * ho * wo, cout)))
            act, h, w = o, ho, wo
        self.last = act               # the head's input (a pool buffer, never freed)
        self.steps.append(("frido_disc_head", head_desc(act.ptr, consts["head_w"].data_ptr(), self.logits.data_ptr(), S, h, w, table[-1][2],
                                                        consts["head_b"])))
        if pair:
            self.sums = torch.zeros(S, 5, dtype=torch.float64, device=dev)
            self.out = torch.zeros(5, dtype=torch.float32, device=dev)
            self.per_sample = torch.zeros(S, dtype=torch.float32, device=dev)
            self.steps.append(("frido_gan_terms", terms_desc(self.logits.data_ptr(), self.sums.data_ptr(), S, Ho * Wo)))
            self.steps.append(("frido_gan_finish", finish_desc(self.sums.data_ptr(), self.out.data_ptr(), self.per_sample.data_ptr(), B, Ho * Wo)))
        self.graph = None

    def launch(self, stream):
        """Every launch of the plan in order on `stream` (directly, or inside a capture)."""
        for name, what in self.steps:
            if name == "prog":
                what.run(stream)
            else:
                launch(name, what, stream)

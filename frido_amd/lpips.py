"""ctypes binding of include/frido_lpips.h (csrc/lpips.hip: the ScalingLayer, the 2 x 2 max pool, one LPIPS feature layer, the sum over
the layers) and LpipsPlan, the compiled LPIPS of one input shape.

Bound beside `_lib`, not inside it, like frido_amd/vision.py: `_lib.EXPORTS`, `_lib.OP_KINDS` and `_lib.KIND_STRUCT` are read off
include/frido_hip.h, the op-kind ABI, and these four launches are no op kinds.  The descriptors are parsed from their own header with the
same parser, the functions are taken from the handle `_lib.lib()` returns for the active plane format (the code is the same in both
builds: f32 / f64 only), and every descriptor's size is compared with the library's at first use.  A library without the symbols is a
stale build and is named as one: there is no fallback."""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import FridoHipError
from .builder import ACT_RELU

HEADER = os.path.join(_lib.REPO, "include", "frido_lpips.h")
_structs = _lib._parse_structs(_lib._strip_comments(open(HEADER).read()))
FridoLpipsScale = type("FridoLpipsScale", (C.Structure,), {"_fields_": _structs["FridoLpipsScale"]})
FridoMaxPool2 = type("FridoMaxPool2", (C.Structure,), {"_fields_": _structs["FridoMaxPool2"]})
FridoLpipsLayer = type("FridoLpipsLayer", (C.Structure,), {"_fields_": _structs["FridoLpipsLayer"]})
FridoLpipsFinish = type("FridoLpipsFinish", (C.Structure,), {"_fields_": _structs["FridoLpipsFinish"]})

# launcher -> (descriptor, the library's sizeof function)
LAUNCHERS = {"frido_lpips_scale": (FridoLpipsScale, "frido_sizeof_lpips_scale"), "frido_maxpool2": (FridoMaxPool2, "frido_sizeof_maxpool2"),
             "frido_lpips_layer": (FridoLpipsLayer, "frido_sizeof_lpips_layer"), "frido_lpips_finish": (FridoLpipsFinish, "frido_sizeof_lpips_finish")}

SHIFT = (-.030, -.088, -.188)      # ScalingLayer, taming/modules/losses/lpips.py:60-61
SCALE = (.458, .448, .450)
CHNS = (64, 128, 256, 512, 512)    # lpips.py:16
# torchvision's vgg16 `features` (configuration D) cut where lpips.py:86-95 cuts it: per slice the conv layers' indices and widths.  A slice
# ends at relu1_2 / relu2_2 / relu3_3 / relu4_3 / relu5_3; slices 2 .. 5 begin with the max pool (indices 4, 9, 16, 23).
VGG_SLICES = (((0, 64), (2, 64)), ((5, 128), (7, 128)), ((10, 256), (12, 256), (14, 256)), ((17, 512), (19, 512), (21, 512)),
              ((24, 512), (26, 512), (28, 512)))
MIN_SIDE = 16                      # four floor-mode pools leave at least one pixel
LAYER_PIXELS_PER_BLOCK = 32        # pixels one workgroup of frido_lpips_layer sums, until LAYER_MAX_BLOCKS workgroups per sample are reached
LAYER_MAX_BLOCKS = 256

_bound = {}      # plane format -> {launcher name: function of that build}


def _fns(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        fns = {}
        for name, (struct, sizeof) in LAUNCHERS.items():
            for sym in (name, sizeof):
                if not hasattr(L, sym):
                    raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {sym}: a stale build from before csrc/lpips.hip "
                                        "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
            c_sz = getattr(L, sizeof)()
            if c_sz != C.sizeof(struct):
                raise FridoHipError(f"ABI mismatch: sizeof({struct.__name__}) C={c_sz} py={C.sizeof(struct)} "
                                    "(include/frido_lpips.h and the build disagree: stale build?)")
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


def scale_desc(x_ptr, y_ptr, dst_ptr, B, H, W, shift=SHIFT, scale=SCALE):
    """A filled FridoLpipsScale: x, y [B][3][H][W] f32 -> dst [2B * H * W][3] f32, x's samples first."""
    d = FridoLpipsScale(x=x_ptr, y=y_ptr, dst=dst_ptr, B=B, H=H, W=W)
    for c in range(3):      # as the float32 values of the module's buffers, whatever precision the caller wrote them in
        d.shift[c] = shift[c]
        d.scale[c] = scale[c]
    return d


def maxpool_desc(src_ptr, dst_ptr, B, H, W, Cn):
    return FridoMaxPool2(src=src_ptr, dst=dst_ptr, B=B, H=H, W=W, C=Cn)


def layer_blocks(HW):
    """Workgroups per sample the plan gives frido_lpips_layer for a plane of HW pixels (1 .. HW)."""
    return max(1, min(LAYER_MAX_BLOCKS, -(-HW // LAYER_PIXELS_PER_BLOCK)))


def layer_desc(f0_ptr, f1_ptr, w_ptr, partials_ptr, B, HW, Cn, nblk):
    return FridoLpipsLayer(f0=f0_ptr, f1=f1_ptr, w=w_ptr, partials=partials_ptr, B=B, HW=HW, C=Cn, nblk=nblk)


def finish_desc(partials_ptr, per_layer_ptr, out_ptr, B, nblk, HW):
    d = FridoLpipsFinish(partials=partials_ptr, per_layer=per_layer_ptr, out=out_ptr, B=B)
    for l in range(5):
        d.nblk[l] = nblk[l]
        d.HW[l] = HW[l]
    return d


def plane_sizes(H, W):
    """(h, w) of the five feature planes of an H x W image: four floor-mode 2 x 2 pools."""
    out = []
    for _ in range(5):
        out.append((H, W))
        H, W = H // 2, W // 2
    return out


class LpipsPlan:
    """LPIPS (taming/modules/losses/lpips.py:41-54) of one input shape (B, H, W) on a Builder over the module's weights.  The VGG16 tower runs
    ONCE at batch 2B -- input and target together, so the weights are read once:

        s = frido_lpips_scale(x_in, y_in)                            [2B * H * W][3] f32 NHWC (csrc/lpips.hip)
        slice 1:            PACK(s) -> conv1_1 -> conv1_2            3 x 3 conv + bias + ReLU launches, operand to operand; the slice's last
        slices 2 .. 5:      frido_maxpool2, then PACK -> the convs   conv writes f32 (for the layer kernel, the pool and the next PACK)
        frido_lpips_layer x 5                                        per workgroup one f64 partial sum of sum_c w (f0 / n0 - f1 / n1)^2
        frido_lpips_finish                                           per_layer [B][5], out [B]

    The pools and the layer kernels are no op kinds, so they sit BETWEEN the five slice programs; `launch` issues everything in order on
    one stream and the caller captures that as one graph.  `x_in`, `y_in`, `out`, `per_layer` are fixed buffers."""

    def __init__(self, b, *, B, H, W, shift, scale, lin_names):
        self.b = b
        dev = b.device
        B2 = 2 * B
        self.x_in = torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        self.y_in = torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        self.out = torch.zeros(B, dtype=torch.float32, device=dev)
        self.per_layer = torch.zeros(B, 5, dtype=torch.float32, device=dev)
        self.scaled = b.persistent_f32(B2 * H * W, 3)
        self.steps = [("frido_lpips_scale", scale_desc(self.x_in.data_ptr(), self.y_in.data_ptr(), self.scaled.data_ptr(), B, H, W, shift, scale))]
        self.planes_hw = plane_sizes(H, W)
        self.progs, self.feats = [], []      # the slice programs; the five f32 feature maps [2B * h * w][C] (pool buffers, never freed)
        src_ptr, Cn = self.scaled.data_ptr(), 3
        for si, convs in enumerate(VGG_SLICES):
            h, w = self.planes_hw[si]
            pooled = None
            if si > 0:
                ph, pw = self.planes_hw[si - 1]
                pooled = b.f32_strict(B2 * h * w, Cn)
                self.steps.append(("frido_maxpool2", maxpool_desc(self.feats[-1].ptr, pooled.ptr, B2, ph, pw, Cn)))
                src_ptr = pooled.ptr
            prog = b.new_prog()
            a = b.pack(src_ptr, 1, B2 * h * w, Cn, 0, Cn)      # conv1_1's three channels are zero-padded to the operand's 32 here
            for j, (idx, cout) in enumerate(convs):
                o = b.conv(a, B2, h, w, f"net.slice{si + 1}.{idx}", act=ACT_RELU, out="f32_strict" if j == len(convs) - 1 else "op")
                a.free()
                a, Cn = o, cout
            if pooled is not None:
                pooled.free()      # read by this program's PACK only; later programs may reuse it (one stream, in order)
            self.feats.append(a)
            self.progs.append(prog)
            self.steps.append(("prog", prog))
        self.nblk = [layer_blocks(h * w) for h, w in self.planes_hw]
        self.partials = torch.zeros(B * sum(self.nblk), dtype=torch.float64, device=dev)      # [layer][b][blk]
        off = 0
        for l, (f, (h, w)) in enumerate(zip(self.feats, self.planes_hw)):
            wl = b.dev_f32(lin_names[l])
            assert wl.numel() == CHNS[l] == f.C, (lin_names[l], tuple(wl.shape), f.C)
            self.steps.append(("frido_lpips_layer", layer_desc(f.ptr, f.ptr + 4 * B * h * w * f.C, wl.data_ptr(), self.partials.data_ptr() + 8 * off,
                                                               B, h * w, f.C, self.nblk[l])))
            off += B * self.nblk[l]
        self.steps.append(("frido_lpips_finish", finish_desc(self.partials.data_ptr(), self.per_layer.data_ptr(), self.out.data_ptr(), B,
                                                             self.nblk, [h * w for h, w in self.planes_hw])))
        self.graph = None

    def launch(self, stream):
        """Every launch of the plan in order on `stream` (directly, or inside a capture)."""
        for name, what in self.steps:
            if name == "prog":
                what.run(stream)
            else:
                launch(name, what, stream)

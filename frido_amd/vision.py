"""ctypes binding of include/frido_vision.h: the one launch in front of the CLIP image tower's program (csrc/vision.hip).

It is bound beside `_lib`, not inside it: `_lib.EXPORTS`, `_lib.OP_KINDS` and `_lib.KIND_STRUCT` are read off include/frido_hip.h, the op-kind
ABI, and this launch is no op kind.  The descriptor is parsed from its own header with the same parser, the function is taken from the
handle `_lib.lib()` returns for the active plane format (the code is the same in both builds: f32 only), and the descriptor's size is
compared with the library's at first use.  A library without the symbol is a stale build and is named as one: there is no fallback."""
import ctypes as C
import os

from . import _lib
from ._lib import FridoHipError

HEADER = os.path.join(_lib.REPO, "include", "frido_vision.h")
_fields = _lib._parse_structs(_lib._strip_comments(open(HEADER).read()))["FridoClipPreprocess"]
FridoClipPreprocess = type("FridoClipPreprocess", (C.Structure,), {"_fields_": _fields})

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)      # encoders/modules.py:239-240
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

_bound = {}      # plane format -> frido_clip_preprocess of that build


def _fn(planes=None):
    planes = planes or _lib.active_planes()
    if planes not in _bound:
        L = _lib.lib(planes)
        for name in ("frido_clip_preprocess", "frido_sizeof_clip_preprocess"):
            if not hasattr(L, name):
                raise FridoHipError(f"{_lib.LIB_PATHS[planes]} does not export {name}: a stale build from before csrc/vision.hip "
                                    "(rebuild with `python -c 'import __graft_entry__ as g; g.build()'`)")
        c_sz = L.frido_sizeof_clip_preprocess()
        if c_sz != C.sizeof(FridoClipPreprocess):
            raise FridoHipError(f"ABI mismatch: sizeof(FridoClipPreprocess) C={c_sz} py={C.sizeof(FridoClipPreprocess)} "
                                "(include/frido_vision.h and the build disagree: stale build?)")
        L.frido_clip_preprocess.argtypes = [C.c_void_p, C.c_void_p]
        _bound[planes] = L.frido_clip_preprocess
    return _bound[planes]


def preprocess_desc(src_ptr, dst_ptr, B, H, W, res, P, mean=CLIP_MEAN, std=CLIP_STD):
    """A filled FridoClipPreprocess: src [B][3][H][W] f32 in [-1, 1] -> dst [B * (res / P)^2][3 * P * P] f32."""
    d = FridoClipPreprocess(src=src_ptr, dst=dst_ptr, B=B, H=H, W=W, res=res, P=P)
    for c in range(3):      # mean / std as the float32 values of the module's buffers, whatever precision the caller wrote them in
        d.mean[c] = mean[c]
        d.rstd[c] = 1.0 / C.c_float(std[c]).value
    return d


def clip_preprocess(desc, stream):
    """Launch frido_clip_preprocess(desc) on `stream` (a hipStream_t handle); a refused descriptor raises with the library's message."""
    rc = _fn()(C.byref(desc), stream)
    if rc != 0:
        raise FridoHipError(f"frido_clip_preprocess failed (rc={rc}): {_lib.lib().frido_last_error().decode()}")

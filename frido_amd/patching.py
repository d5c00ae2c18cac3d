"""Patch-wise ("convolutional") mode of FridoDiffusion: what the reference does once `model.split_input_params` is set
(frido/models/diffusion/frido.py:677-764 get_fold_unfold / get_weighting / delta_border, :1076-1152 apply_model, :840-877
decode_first_stage, :963-993 encode_first_stage).

The tensor is cut into overlapping crops (frido_unfold), the model runs on all crops as ONE batch, and the results are stitched with
a border-distance weighting and divided by the folded weighting (frido_fold).  This module owns the geometry: the crop grid, the
`weighting` / `normalization` tables (torch float32 on the host, once per geometry, bit-equal to the reference's tensors, uploaded) and the descriptors of the two kernels (op kinds FRIDO_OP_UNFOLD / FRIDO_OP_FOLD).

Batch layout of the crop tensor (include/frido_hip.h): crop l of sample b is entry b * L + l, so per-sample inputs of the model
(timesteps, context, labels) are repeated with `repeat_interleave(L)`.
"""
import ctypes as C

import torch

from . import _lib

MODEL, DECODE, ENCODE = "model", "decode", "encode"
PARAM_KEYS = ("ks", "stride", "vqf", "patch_distributed_vq", "tie_braker", "clip_min_weight", "clip_max_weight", "clip_min_tie_weight",
              "clip_max_tie_weight")
# cond_stage_key values for which the reference unfolds the CONDITIONING as well (frido.py:1091-1101) / rebuilds it per crop (:1103-1137)
UNFOLDED_COND_KEYS = ("image", "LR_image", "segmentation", "bbox_img")


def refuse(what):
    return NotImplementedError(f"{what} is not built for the patch-wise mode (split_input_params is set on the model; delete the attribute "
                               "to run on the whole latent)")


def params_of(model):
    """The model's split_input_params (looked up on every call, like the reference's hasattr), or None."""
    return getattr(model, "split_input_params", None)


def check_conditioning(model, cond):
    """The conditioning forms the reference would treat differently per crop are refused, never ignored."""
    if isinstance(cond, (dict, list)):
        raise refuse("a dict / list conditioning")
    if model.cond_stage_key in UNFOLDED_COND_KEYS and model.model.conditioning_key:
        raise refuse(f"cond_stage_key={model.cond_stage_key!r} with a conditioning key (the reference unfolds the conditioning itself, frido.py:1091-1101)")
    if model.cond_stage_key == "coordinates_bbox":
        raise refuse("cond_stage_key='coordinates_bbox' (per-crop bounding-box tokens, frido.py:1103-1137)")
    if model.model.conditioning_key in ("concat", "hybrid"):
        # beyond the reference's own list: it would hand the full-size c_concat to every crop and fail on the channel concat
        raise refuse(f"conditioning_key={model.model.conditioning_key!r} (a full-size c_concat does not fit the crops)")


# ---- the stitching weights: same float32 operations as the reference's get_weighting (frido.py:684-712), in this project's terms -------
def border_distance(n, m):
    """[n][m] float32: how far each cell of an n x m grid is from the nearest edge, on axes normalised to [0, 1] (0 on the border, 0.5 in
    the centre).  A one-cell axis has no extent: 0 / 0, NaN -- PatchGeometry turns that into an error."""
    rows = torch.arange(n, dtype=torch.float32) / torch.tensor(float(n - 1))
    cols = torch.arange(m, dtype=torch.float32) / torch.tensor(float(m - 1))
    return torch.minimum(torch.minimum(rows, 1 - rows)[:, None], torch.minimum(cols, 1 - cols)[None, :])      # minimum keeps a NaN


def weighting_tables(kh, kw, sy, sx, H, W, *, tie, clip, clip_tie):
    """(weighting [kh * kw][L], normalization [H][W]) for crops kh x kw at stride (sy, sx) of an H x W map: a crop pixel weighs its clipped
    border distance, with `tie` times the clipped border distance of the crop within the Ly x Lx crop grid; the normalization is the sum
    of the weights that land on each pixel (nn.Fold of the weights -- the same summation the reference's normalization comes from)."""
    Ly, Lx = (H - kh) // sy + 1, (W - kw) // sx + 1
    per_pixel = border_distance(kh, kw).clamp(clip[0], clip[1]).reshape(kh * kw, 1)
    if tie:
        per_crop = border_distance(Ly, Lx).clamp(clip_tie[0], clip_tie[1]).reshape(1, Ly * Lx)
        weighting = per_pixel * per_crop
    else:
        weighting = per_pixel.expand(kh * kw, Ly * Lx)
    weighting = weighting.contiguous()
    normalization = torch.nn.functional.fold(weighting[None], output_size=(H, W), kernel_size=(kh, kw), stride=(sy, sx))
    return weighting, normalization.reshape(H, W).contiguous()


class PatchGeometry:
    """Crop grid of one tensor shape.  `src`: (H, W, kh, kw, sy, sx) of the tensor that is unfolded; `out`: the same six numbers of the
    tensor that is folded (equal to src for the denoiser; src times vqf for decode, src over vqf for encode).  wt / norm: the fold side's
    tables on the device (None on a host-only geometry: device=None)."""

    def __init__(self, src, out, *, tie, clip, clip_tie, device):
        self.src, self.out = tuple(src), tuple(out)
        H, W, kh, kw, sy, sx = self.src
        self.Ly, self.Lx = (H - kh) // sy + 1, (W - kw) // sx + 1
        self.L = self.Ly * self.Lx
        Ho, Wo, kho, kwo, syo, sxo = self.out
        self.weighting, self.normalization = weighting_tables(kho, kwo, syo, sxo, Ho, Wo, tie=tie, clip=clip, clip_tie=clip_tie)
        if not (bool(torch.isfinite(self.weighting).all()) and bool((self.normalization > 0).all())):
            raise ValueError(f"split_input_params: the weighting of {self.Ly} x {self.Lx} crops of {kho} x {kwo} is not finite and positive "
                             "(tie_braker on a one-crop axis, or a one-pixel crop axis: the border distance is 0 / 0) -- the reference returns NaN here")
        self.max_cover = -(-kho // syo) * -(-kwo // sxo)          # most crops over one pixel
        self.wt = self.weighting.to(device) if device is not None else None
        self.norm = self.normalization.to(device) if device is not None else None

    def origins(self):
        """(y0, x0) of every crop of the unfolded tensor, in crop order l = ly * Lx + lx."""
        _, _, _, _, sy, sx = self.src
        return [(ly * sy, lx * sx) for ly in range(self.Ly) for lx in range(self.Lx)]

    def unfold_desc(self, src_ptr, dst_ptr, B, Cn):
        H, W, kh, kw, sy, sx = self.src
        return _lib.STRUCTS["FridoUnfold"](src=src_ptr, dst=dst_ptr, B=B, H=H, W=W, C=Cn, kh=kh, kw=kw, sy=sy, sx=sx)

    def fold_desc(self, crops_ptr, out_ptr, B, Cn, out_u8=None, u8_mode=0):
        H, W, kh, kw, sy, sx = self.out
        return _lib.STRUCTS["FridoFold"](crops=crops_ptr, out=out_ptr, wt=self.wt.data_ptr(), norm=self.norm.data_ptr(), out_u8=out_u8,
                                         B=B, H=H, W=W, C=Cn, kh=kh, kw=kw, sy=sy, sx=sx, u8_mode=u8_mode)


def launch_unfold(desc, stream):
    _lib.check(_lib.lib().frido_unfold(C.byref(desc), stream), "frido_unfold")


def launch_fold(desc, stream):
    _lib.check(_lib.lib().frido_fold(C.byref(desc), stream), "frido_fold")


_GEOMETRIES = {}
GEOMETRY_CACHE_SIZE = 16


def _pair(v, name):
    v = tuple(int(a) for a in v)
    if len(v) != 2 or min(v) <= 0:
        raise ValueError(f"split_input_params[{name!r}] must be two positive integers, got {v}")
    return v


def geometry(params, H, W, mode, device):
    """The PatchGeometry of an H x W tensor under `params` (a split_input_params dict), cached per (H, W, kh, kw, sy, sx, scale, tie and
    clip values, device).  mode: MODEL (the denoiser on latent crops), DECODE (latent crops -> image, fold at vqf x) or ENCODE (image
    crops -> latent, fold at 1 / vqf)."""
    missing = [k for k in PARAM_KEYS if k not in params and not (k == "patch_distributed_vq" and mode == MODEL)]
    if missing:
        raise KeyError(f"split_input_params lacks {missing}")
    (kh, kw), (sy, sx) = _pair(params["ks"], "ks"), _pair(params["stride"], "stride")
    f = 1 if mode == MODEL else int(params["vqf"])
    if mode == MODEL:
        if kh > H or kw > W:
            raise ValueError(f"split_input_params: ks {(kh, kw)} is larger than the {H} x {W} latent")
    else:
        if kh > H or kw > W:                           # frido.py:846-852 / :970-976 ("reducing Kernel" / "reducing stride")
            kh, kw = min(kh, H), min(kw, W)
        if sy > H or sx > W:
            sy, sx = min(sy, H), min(sx, W)
        if kh != kw:
            raise ValueError(f"split_input_params: decode / encode need a square ks, got {(kh, kw)} (the reference builds its second fold from "
                             "ks[0] twice, frido.py:739,752)")
    if (H - kh) % sy or (W - kw) % sx:
        raise ValueError(f"split_input_params: crops of {(kh, kw)} at stride {(sy, sx)} do not tile a {H} x {W} tensor exactly "
                         "((H - kh) % sy, (W - kw) % sx must be 0): the reference's normalization is 0 on the uncovered border and it "
                         "divides 0 by 0 there, returning NaN")
    src = (H, W, kh, kw, sy, sx)
    if mode == DECODE:
        out = tuple(v * f for v in src)
    elif mode == ENCODE:
        if any(v % f for v in src):
            raise ValueError(f"split_input_params: image size, ks and stride {src} must be multiples of vqf = {f} for a patch-wise encode")
        out = tuple(v // f for v in src)
    else:
        out = src
    tie = bool(params["tie_braker"])
    clip = (float(params["clip_min_weight"]), float(params["clip_max_weight"]))
    clip_tie = (float(params["clip_min_tie_weight"]), float(params["clip_max_tie_weight"]))
    key = (src, out, tie, clip, clip_tie if tie else None, str(device))
    if key in _GEOMETRIES:
        _GEOMETRIES[key] = _GEOMETRIES.pop(key)
    else:
        while len(_GEOMETRIES) >= GEOMETRY_CACHE_SIZE:
            _GEOMETRIES.pop(next(iter(_GEOMETRIES)))
        _GEOMETRIES[key] = PatchGeometry(src, out, tie=tie, clip=clip, clip_tie=clip_tie, device=device)
    return _GEOMETRIES[key]


def geometry_key(params):
    """What of split_input_params a compiled sampler engine depends on (part of its cache key)."""
    return (tuple(int(v) for v in params["ks"]), tuple(int(v) for v in params["stride"]), bool(params["tie_braker"]),
            float(params["clip_min_weight"]), float(params["clip_max_weight"]), float(params["clip_min_tie_weight"]),
            float(params["clip_max_tie_weight"]))

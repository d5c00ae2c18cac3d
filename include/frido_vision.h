/* The front of the CLIP image tower (FrozenClipImageEmbedder.preprocess, frido/modules/encoders/modules.py:242-250, and the
 * patch cut of clip/model.py VisionTransformer.conv1): ONE launcher beside the op table of frido_hip.h.
 *
 * A header of its own on purpose: frido_hip.h is the op-kind ABI (FRIDO_ABI_VERSION, the FridoOpKind enum, one launcher per kind,
 * every prototype an export that frido_amd/_lib.py requires of a build).  This launch is no op kind -- it is the first node of the
 * image tower's captured graph, in front of the tower's program -- so nothing of that ABI moves: frido_amd/vision.py binds it from
 * the same shared library, cross-checks the descriptor's size, and names a stale build if the symbol is missing.
 * Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with frido_last_error(). */
#ifndef FRIDO_VISION_H
#define FRIDO_VISION_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bicubic resize (align_corners = True, no antialias) of an image batch to res x res, CLIP's normalisation, and the cut into
 * P x P patches as GEMM rows, all in f32:
 *   v   = bicubic(src[b][c])(oy, ox)          separable Keys cubic, A = -0.75, 16 taps: source coordinate s = o * (n_in - 1) / (n_out - 1)
 *                                             (0 when n_out == 1), i0 = floor(s), t = s - i0, taps i0 - 1 .. i0 + 2 clamped to [0, n_in - 1]
 *                                             (torch.nn.functional.interpolate(mode="bicubic", align_corners=True))
 *   out = ((v + 1) / 2 - mean[c]) * rstd[c]
 *   dst[(b * g + oy / P) * g + ox / P][(c * P + oy % P) * P + ox % P] = out,   g = res / P
 * i.e. row = patch, column = (c, py, px): the order of conv1.weight.reshape(width, 3 * P * P). */
typedef struct FridoClipPreprocess {
    const float* src;      /* [B][3][H][W] f32, NCHW, values in [-1, 1] (what FrozenClipImageEmbedder.forward takes) */
    float* dst;            /* [B * g * g][3 * P * P] f32, g = res / P; column (c, py, px) = conv1.weight.reshape(width, -1)'s order */
    int32_t B, H, W, res, P;
    float mean[3], rstd[3];
} FridoClipPreprocess;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_clip_preprocess(const FridoClipPreprocess* d, frido_stream_t s);
int frido_sizeof_clip_preprocess(void);

#ifdef __cplusplus
}
#endif
#endif

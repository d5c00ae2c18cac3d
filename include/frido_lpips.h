/* The memory-bound part of LPIPS (taming/modules/losses/lpips.py:11-122) around the VGG16 convolutions: the ScalingLayer, the
 * 2 x 2 max pools between the five feature slices, the per-pixel channel normalisation + 1 x 1 projection + spatial sum of one
 * feature layer, and the sum over the layers.  FOUR launchers beside the op table of frido_hip.h.
 *
 * A header of its own for the reason frido_vision.h has one: frido_hip.h is the op-kind ABI (FRIDO_ABI_VERSION, the FridoOpKind
 * enum, one launcher per kind, every prototype an export that frido_amd/_lib.py requires of a build).  These launches are no op
 * kinds -- they sit between the slice programs of the LPIPS graph -- so nothing of that ABI moves: frido_amd/lpips.py binds them
 * from the same shared library, cross-checks each descriptor's size, and names a stale build if a symbol is missing.
 * Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with frido_last_error().
 * The element-wise arithmetic is f32 (real divisions, every operation rounded on its own), the channel and spatial sums are f64; no
 * atomics and a fixed summation order: a replay returns the same bits. */
#ifndef FRIDO_LPIPS_H
#define FRIDO_LPIPS_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ScalingLayer (lpips.py:57-64) of the two images of a pair, NCHW -> NHWC, x's samples first and then y's:
 *   dst[(s * H * W + p) * 3 + c] = (src_s[c * H * W + p] - shift[c]) / scale[c]      s = 0 .. 2B-1, src_s = x[s] or y[s - B]
 * A real division, every operation rounded on its own. */
typedef struct FridoLpipsScale {
    const float* x;        /* [B][3][H][W] f32 NCHW: `input` */
    const float* y;        /* [B][3][H][W] f32 NCHW: `target` */
    float* dst;            /* [2B * H * W][3] f32 NHWC */
    int32_t B, H, W;
    float shift[3], scale[3];      /* the float32 values of the module's buffers */
} FridoLpipsScale;

/* nn.MaxPool2d(kernel_size=2, stride=2) on NHWC f32: floor mode, an odd last row or column is dropped.
 *   dst[b][oy][ox][c] = max over dy, dx in {0, 1} of src[b][2 oy + dy][2 ox + dx][c],   oy < H / 2, ox < W / 2 */
typedef struct FridoMaxPool2 {
    const float* src;      /* [B][H][W][C] f32 */
    float* dst;            /* [B][H / 2][W / 2][C] f32 */
    int32_t B, H, W, C;    /* C % 4 == 0, H >= 2, W >= 2 */
} FridoMaxPool2;

/* One feature layer (lpips.py:46-50, 116-118).  Per pixel p of sample b, over the channels c:
 *   n0 = sqrt(sum f0^2) + 1e-10,  n1 likewise (eps OUTSIDE the root),   d[b][p] = sum_c w[c] * (f0[c] / n0 - f1[c] / n1)^2
 * a pixel whose features are all zero gives 0 / 1e-10 = 0, not NaN.  Workgroup (blk, b) owns the pixels
 * blk * per .. min((blk + 1) * per, HW) - 1 with per = ceil(HW / nblk) and writes the ONE f64 sum of their d to partials[b][blk]
 * (0 for a block past the last pixel); nothing is added across workgroups here. */
typedef struct FridoLpipsLayer {
    const float* f0;       /* [B * HW][C] f32: the rows of `input` */
    const float* f1;       /* [B * HW][C] f32: the rows of `target` */
    const float* w;        /* [C] f32: linK.model[-1].weight */
    double* partials;      /* [B][nblk] f64 */
    int32_t B, HW, C;      /* C % 4 == 0 */
    int32_t nblk;          /* 1 .. HW workgroups per sample: the caller's choice (it sizes `partials`) */
} FridoLpipsLayer;

/* The spatial means and the sum over the five layers (lpips.py:50-54).  One workgroup per sample:
 *   r[l] = (float)((partials_l[b][0] + partials_l[b][1] + ... in index order, f64) / HW[l])        per_layer[b][l] = r[l]
 *   out[b] = ((((r[0] + r[1]) + r[2]) + r[3]) + r[4])   in f32: the reference's `val += res[l]`
 * partials_l = partials + B * (nblk[0] + ... + nblk[l - 1]): the layers' blocks lie back to back. */
typedef struct FridoLpipsFinish {
    const double* partials;      /* [5 layers][B][nblk[l]] f64 */
    float* per_layer;            /* [B][5] f32 */
    float* out;                  /* [B] f32 */
    int32_t B;
    int32_t nblk[5], HW[5];
} FridoLpipsFinish;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_lpips_scale(const FridoLpipsScale* d, frido_stream_t s);
int frido_maxpool2(const FridoMaxPool2* d, frido_stream_t s);
int frido_lpips_layer(const FridoLpipsLayer* d, frido_stream_t s);
int frido_lpips_finish(const FridoLpipsFinish* d, frido_stream_t s);
int frido_sizeof_lpips_scale(void);
int frido_sizeof_maxpool2(void);
int frido_sizeof_lpips_layer(void);
int frido_sizeof_lpips_finish(void);

#ifdef __cplusplus
}
#endif
#endif

/* The launches of the Fréchet Inception Distance around the Inception-v3 tower's convolutions: the input transform of torch-fidelity's
 * FeatureExtractorInceptionV3 (quantise, TF1-legacy bilinear resize to 299 x 299, (v - 128) / 128), the tower's 3 x 3 pools, its global
 * average pool, and the float64 accumulation of the feature statistics.  FOUR launchers beside the op table of frido_hip.h.
 *
 * A header of its own for the reason frido_lpips.h has one: frido_hip.h is the op-kind ABI, and these launches are no op kinds --
 * they sit between the programs of the tower's graph -- so nothing of that ABI moves: frido_amd/fid.py binds them from the same
 * shared library, cross-checks each descriptor's size, and names a stale build if a symbol is missing.
 * Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with frido_last_error().
 * Element-wise arithmetic is f32 with every operation rounded on its own (nothing is contracted into an fma); the sums of the global
 * pool and of the statistics are f64 in a fixed order.  No atomics: a replay returns the same bits. */
#ifndef FRIDO_FID_H
#define FRIDO_FID_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FRIDO_FID_SRC_U8_HWC = 0,        /* uint8 [B][H][W][3]: what pipeline.sample_images gathers */
       FRIDO_FID_SRC_F32_NCHW = 1 };    /* float32 [B][3][H][W] in [-1, 1]: what the decoders return */
enum { FRIDO_FID_QUANT_PIL = 2,         /* custom_to_pil: FridoGemm.u8_mode 2 (the PNG writer's formula) */
       FRIDO_FID_QUANT_NP = 1 };        /* custom_to_np:  FridoGemm.u8_mode 1 */

/* Source image -> f32 NHWC [B * S * S][3].  q = the pixel as a float holding an integer 0 .. 255: the uint8 value itself, or the float
 * source put through one of FridoGemm.out_u8's two conversions (frido_hip.h: u8_mode), truncated.  Then the TF1-legacy bilinear resize
 * (no half-pixel offset, corners not aligned), with sy = (float)H / (float)S, sx = (float)W / (float)S:
 *   fy = (float)oy * sy;  y0 = (int)floorf(fy);  y1 = min(y0 + 1, H - 1);  ty = fy - (float)y0;           likewise x0, x1, tx
 *   top = q[y0][x0] + (q[y0][x1] - q[y0][x0]) * tx;    bot = q[y1][x0] + (q[y1][x1] - q[y1][x0]) * tx
 *   v = top + (bot - top) * ty;    dst[(b * S + oy) * S + ox][c] = (v - 128) / 128
 * every operation a separate f32 rounding.  With H == W == S every t is 0 and dst is exactly (q - 128) / 128. */
typedef struct FridoFidPreprocess {
    const void* src;       /* uint8 [B][H][W][3] or f32 [B][3][H][W] */
    float* dst;            /* [B * S * S][3] f32 NHWC */
    int32_t B, H, W, S;    /* S >= 1: 299 in the tower; the tests use others */
    int32_t src_kind;      /* FRIDO_FID_SRC_* */
    int32_t quant;         /* FRIDO_FID_QUANT_* (float sources only) */
} FridoFidPreprocess;

enum { FRIDO_POOL3_MAX_S2 = 0,          /* max, kernel 3, stride 2, no padding: Ho = (H - 3) / 2 + 1 (floor) */
       FRIDO_POOL3_MAX_S1P1 = 1,        /* max, kernel 3, stride 1, padding 1 (the padding never wins): Ho = H */
       FRIDO_POOL3_AVG_S1P1 = 2 };      /* average, kernel 3, stride 1, padding 1, the padding EXCLUDED from the divisor: Ho = H */

/* 3 x 3 pool on f32 NHWC, four channels per thread.  dst row (b, oy, ox) starts at dst + ((b * Ho + oy) * Wo + ox) * ldd + c0: the
 * destination may be a column range of a wider (concatenated) tensor.  The average adds the taps inside the plane in (ky, kx) order in
 * f32, starting from the first such tap, and divides by their count (a true division). */
typedef struct FridoPool3 {
    const float* src;      /* [B][H][W][C] f32 */
    float* dst;            /* [B * Ho * Wo][ldd] f32, columns c0 .. c0 + C - 1 are written */
    int32_t B, H, W, C;    /* C % 4 == 0; H, W >= 3 in mode MAX_S2 */
    int32_t ldd, c0;       /* ldd % 4 == 0, c0 % 4 == 0, c0 + C <= ldd */
    int32_t mode;          /* FRIDO_POOL3_* */
} FridoPool3;

/* Global average pool: dst[b][c] = (float)((sum_{p = 0 .. HW-1, in this order, f64} src[b][p][c]) / (double)HW). */
typedef struct FridoGap {
    const float* src;      /* [B][HW][C] f32 */
    float* dst;            /* [B][C] f32 */
    int32_t B, HW, C;      /* C % 4 == 0 */
} FridoGap;

/* Feature statistics: s1[i] += sum_b x[b][i] and s2[i][j] += sum_b x[b][i] * x[b][j] in f64, b ascending; the product of two f32
 * values is exact in f64, so each element has ONE defined value (acc = acc + (double)xi * (double)xj, starting from the stored s2)
 * and s2 stays bitwise symmetric.  One workgroup owns a 64 x 64 tile of s2 (4 x 4 elements per thread) and loops over the rows. */
typedef struct FridoFeatAccum {
    const float* x;        /* [B][D] f32 */
    double* s1;            /* [D] f64, read and written */
    double* s2;            /* [D][D] f64, read and written */
    int32_t B, D;
} FridoFeatAccum;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_fid_preprocess(const FridoFidPreprocess* d, frido_stream_t s);
int frido_pool3(const FridoPool3* d, frido_stream_t s);
int frido_gap(const FridoGap* d, frido_stream_t s);
int frido_feat_accum(const FridoFeatAccum* d, frido_stream_t s);
int frido_sizeof_fid_preprocess(void);
int frido_sizeof_pool3(void);
int frido_sizeof_gap(void);
int frido_sizeof_feat_accum(void);

#ifdef __cplusplus
}
#endif
#endif

/* The ends of the PatchGAN discriminator (taming/modules/discriminator/model.py:17-67) around its middle convolutions, and the
 * reductions of the GAN terms of VQLPIPSWithDiscriminator (taming/modules/losses/vqperceptual.py:22-33, 102-150).  FIVE launchers
 * beside the op table of frido_hip.h.
 *
 * A header of its own for the reason frido_lpips.h has one: frido_hip.h is the op-kind ABI, and these launches are no op kinds --
 * they sit between the slice programs of the discriminator's graph -- so nothing of that ABI moves: frido_amd/patchgan.py binds
 * them from the same shared library, cross-checks each descriptor's size, and names a stale build if a symbol is missing.
 * Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with frido_last_error().
 * Element-wise arithmetic is f32; the dot products of the stem and the head are f32 FUSED multiply-adds (fmaf) in the order written
 * at each struct; the sums over logits are f64.  No atomics and a fixed summation order: a replay returns the same bits. */
#ifndef FRIDO_PATCHGAN_H
#define FRIDO_PATCHGAN_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The first layer: conv 4 x 4, stride 2, zero padding 1, bias, LeakyReLU, straight from the NCHW images of a pair to one NHWC block,
 * x's samples (real) first and then y's (fake):
 *   acc = 0;  for ky, kx, c in this order:  acc = fmaf(w[n][ky][kx][c], src_s[c][2 oy + ky - 1][2 ox + kx - 1], acc)   (0 outside)
 *   v = acc + bias[n];   dst[(s * Ho * Wo + oy * Wo + ox)][n] = v >= 0 ? v : slope * v
 * s = 0 .. S-1, S = 2B (src_s = x[s] or y[s - B]) or S = B when y is NULL.  Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1 (floor).
 * The weights are staged in LDS once per workgroup: ndf * 16 * Cin * 4 bytes <= 32 KB. */
typedef struct FridoDiscStem {
    const float* x;        /* [B][Cin][H][W] f32 NCHW: the real images */
    const float* y;        /* [B][Cin][H][W] f32 NCHW: the fake images, or NULL */
    const float* w;        /* [ndf][4][4][Cin] f32: main.0.weight, repacked by the host */
    const float* bias;     /* [ndf] f32 */
    float* dst;            /* [S * Ho * Wo][ndf] f32 NHWC */
    int32_t B, Cin, H, W;  /* Cin <= 8, H >= 2, W >= 2 */
    int32_t ndf;           /* ndf % 4 == 0, ndf * Cin <= 512 */
    float slope;
} FridoDiscStem;

/* Per-channel affine + LeakyReLU on f32 NHWC rows (an eval-mode BatchNorm2d or an ActNorm with the conv's bias, folded by the host):
 *   v = fmaf(a[c], x, b[c]);   dst = v >= 0 ? v : slope * v            dst may be src */
typedef struct FridoAffineLeaky {
    const float* src;      /* [rows][C] f32 */
    const float* a;        /* [C] f32 */
    const float* b;        /* [C] f32 */
    float* dst;            /* [rows][C] f32 */
    int64_t rows;
    int32_t C;             /* C % 4 == 0 */
    float slope;
} FridoAffineLeaky;

/* The last layer: conv 4 x 4, stride 1, zero padding 1, ONE output channel, bias, on NHWC f32.  Ho = H - 1, Wo = W - 1.
 * One wave per output pixel; lane l owns the float4 columns l, l + 64, ... of every tap:
 *   part_l = 0;  for ky, kx, then the lane's columns in index order, then the four channels of a column:
 *                part_l = fmaf(w[ky][kx][c], src[s][oy + ky - 1][ox + kx - 1][c], part_l)                    (0 outside)
 *   logits[s][oy][ox] = (xor-shuffle tree over the 64 lanes, offsets 32, 16, .. 1) + bias */
typedef struct FridoDiscHead {
    const float* src;      /* [S][H][W][C] f32 NHWC */
    const float* w;        /* [4][4][C] f32: the last conv's weight, repacked by the host */
    float* logits;         /* [S][Ho][Wo] f32 */
    int32_t S, H, W, C;    /* C % 4 == 0, H >= 2, W >= 2 */
    float bias;
} FridoDiscHead;

/* Five sums over the n logits of each sample, ONE wave per sample: lane l adds the elements l, l + 64, ... in index order in f64,
 * then the xor-shuffle tree (offsets 32 .. 1).  The terms are evaluated element-wise in f32:
 *   sums[s] = { sum l,  sum relu(1 - l),  sum relu(1 + l),  sum softplus(-l),  sum softplus(l) }
 *   softplus(x) = x > 20 ? x : (float)log1p(exp((double)x))       (torch.nn.functional.softplus, beta 1, threshold 20; the f32 value
 *                                                                  is rounded once from the f64 evaluation) */
typedef struct FridoGanTerms {
    const float* logits;   /* [S][n] f32 */
    double* sums;          /* [S][5] f64 */
    int32_t S, n;
} FridoGanTerms;

/* The scalars of vqperceptual.py:111, 22-33, 146-148 from the sums of 2B samples, real first.  One wave; the samples are added in
 * index order in f64, each result rounded to f32 once.  N = B * n:
 *   out[0] = mean(logits_real) = (sum_{s < B} sums[s][0]) / N          out[1] = mean(logits_fake) = (sum_{s >= B} sums[s][0]) / N
 *   out[2] = g_loss = -mean(logits_fake)
 *   out[3] = hinge   = 0.5 * ((sum_{s < B} sums[s][1]) / N + (sum_{s >= B} sums[s][2]) / N)
 *   out[4] = vanilla = 0.5 * ((sum_{s < B} sums[s][3]) / N + (sum_{s >= B} sums[s][4]) / N)
 *   per_sample[s] = sums[s][0] / n                                      s = 0 .. 2B-1 */
typedef struct FridoGanFinish {
    const double* sums;    /* [2B][5] f64 */
    float* out;            /* [5] f32 */
    float* per_sample;     /* [2B] f32 */
    int32_t B, n;
} FridoGanFinish;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_disc_stem(const FridoDiscStem* d, frido_stream_t s);
int frido_affine_leaky(const FridoAffineLeaky* d, frido_stream_t s);
int frido_disc_head(const FridoDiscHead* d, frido_stream_t s);
int frido_gan_terms(const FridoGanTerms* d, frido_stream_t s);
int frido_gan_finish(const FridoGanFinish* d, frido_stream_t s);
int frido_sizeof_disc_stem(void);
int frido_sizeof_affine_leaky(void);
int frido_sizeof_disc_head(void);
int frido_sizeof_gan_terms(void);
int frido_sizeof_gan_finish(void);

#ifdef __cplusplus
}
#endif
#endif

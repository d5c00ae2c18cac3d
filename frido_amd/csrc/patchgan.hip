// The ends of the PatchGAN discriminator around its middle convolutions (include/frido_patchgan.h): the 4 x 4 stride-2 stem straight from
// the NCHW images of a pair, the per-channel affine + LeakyReLU that an eval-mode BatchNorm2d / ActNorm folds to, the one-channel 4 x 4
// head, and the reductions of the GAN terms.  Plain f32 arithmetic with f64 sums over the logits: no operand planes, so no status word
// (launch.h alone, like lpips.hip) and the two builds of the library compile the same code.  The launches sit between the slice programs
// of the discriminator's graph, they are no op kinds.  No atomics anywhere and every sum in a fixed order: a replay returns the same bits.
// The stem and the affine are bandwidth kernels (16-byte stores / accesses); the head is one wave per logit with the channels of a tap
// across the lanes, its sum a wave64 xor-shuffle tree.
#include "launch.h"
#include "frido_patchgan.h"

namespace {

constexpr int PG_GRID_CAP = 1024;         // 4 workgroups per CU; larger problems take further trips of the grid-stride loops
constexpr int STEM_LDS_FLOATS = 8192;     // 32 KB of weights

__device__ __forceinline__ float leaky(float v, float slope) { return v >= 0.0f ? v : __fmul_rn(slope, v); }

constexpr int STEM_PIX = 4;               // output pixels per thread: one LDS read of four weights serves four pixels

// Workgroup = tiles of STEM_PIX * pps output pixels, pps = 256 / (ndf / 4) pixel slots; thread (slot, q) owns the output channels
// 4 q .. 4 q + 3 of the pixels slot, slot + pps, slot + 2 pps, slot + 3 pps of the tile: per pixel one 16-byte store, the lanes of a pixel
// writing one contiguous row and consecutive slots consecutive rows.  LDS holds the weights transposed, [k][ndf] with
// k = (ky * 4 + kx) * Cin + c: the four weights of a thread are one 16-byte read (consecutive lanes read consecutive slots: no bank
// conflict) that all STEM_PIX pixels use, and the source value of a tap is the same address in all lanes of a pixel (a broadcast).
// Every stored pixel index is < P = S * Ho * Wo; every source index is bounds-checked (zero padding); a thread's pixels past P read
// nothing and store nothing.
__global__ __launch_bounds__(256) void disc_stem_kernel(const FridoDiscStem d, int Ho, int Wo, int64_t P, int pps, int64_t ntiles) {
    __shared__ __attribute__((aligned(16))) float sw[STEM_LDS_FLOATS];
    const int K = 16 * d.Cin, NQ = d.ndf >> 2;
    for (int i = threadIdx.x; i < d.ndf * K; i += 256) {
        const int n = i / K, k = i - n * K;
        sw[k * d.ndf + n] = d.w[i];
    }
    __syncthreads();
    const int slot = threadIdx.x / NQ, q = threadIdx.x - slot * NQ;
    if (slot >= pps) return;                                   // after the only barrier
    const int64_t HW = (int64_t)d.H * d.W, HoWo = (int64_t)Ho * Wo;
    float bias[4];
    load_vec<4>(d.bias + 4 * q, bias);
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t p0 = t * pps * STEM_PIX + slot;
        const float* src[STEM_PIX];
        int y0[STEM_PIX], x0[STEM_PIX];                        // 2 oy - 1, 2 ox - 1
        bool live[STEM_PIX];
        float acc[STEM_PIX][4];
#pragma unroll
        for (int j = 0; j < STEM_PIX; ++j) {
            const int64_t p = p0 + (int64_t)j * pps;
            live[j] = p < P;
            const int64_t pp = live[j] ? p : 0;
            const int64_t s = pp / HoWo, r = pp - s * HoWo;
            const int oy = (int)(r / Wo), ox = (int)(r - (int64_t)oy * Wo);
            src[j] = s < d.B ? d.x + s * d.Cin * HW : d.y + (s - d.B) * d.Cin * HW;
            y0[j] = 2 * oy - 1;
            x0[j] = 2 * ox - 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = 0.0f;
        }
        for (int ky = 0; ky < 4; ++ky) {
            for (int kx = 0; kx < 4; ++kx) {
                bool in[STEM_PIX];
                int64_t off[STEM_PIX];
#pragma unroll
                for (int j = 0; j < STEM_PIX; ++j) {
                    const int iy = y0[j] + ky, ix = x0[j] + kx;
                    in[j] = live[j] && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                    off[j] = in[j] ? (int64_t)iy * d.W + ix : 0;
                }
                const float* wp = sw + (ky * 4 + kx) * d.Cin * d.ndf + 4 * q;
                for (int c = 0; c < d.Cin; ++c) {
                    float w[4];
                    load_vec<4>(wp + c * d.ndf, w);
#pragma unroll
                    for (int j = 0; j < STEM_PIX; ++j) {
                        const float v = in[j] ? src[j][off[j] + c * HW] : 0.0f;
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[j][k] = fmaf(w[k], v, acc[j][k]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < STEM_PIX; ++j) {
            if (!live[j]) continue;
            float o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = leaky(__fadd_rn(acc[j][k], bias[k]), d.slope);
            store_vec<4>(d.dst + (p0 + (int64_t)j * pps) * d.ndf + 4 * q, o);
        }
    }
}

// One thread per four channels of a row: unit i IS the four consecutive floats 4 i .. 4 i + 3 of src and dst.
__global__ __launch_bounds__(256) void affine_leaky_kernel(const FridoAffineLeaky d, int64_t units) {
    const int C4 = d.C >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        float x[4], a[4], b[4], o[4];
        load_vec<4>(d.src + 4 * i, x);
        load_vec<4>(d.a + 4 * c4, a);
        load_vec<4>(d.b + 4 * c4, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = leaky(fmaf(a[j], x[j], b[j]), d.slope);
        store_vec<4>(d.dst + 4 * i, o);
    }
}

// sum over the 64 lanes of a wave: every lane ends with the same value
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Four waves per workgroup, one wave per output pixel and trip (the pixel index is wave-uniform: every lane takes part in the shuffles).
__global__ __launch_bounds__(256) void disc_head_kernel(const FridoDiscHead d, int Ho, int Wo, int64_t P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C4 = d.C >> 2;
    const int64_t HoWo = (int64_t)Ho * Wo;
    for (int64_t p = (int64_t)blockIdx.x * 4 + wave; p < P; p += (int64_t)gridDim.x * 4) {
        const int64_t s = p / HoWo, r = p - s * HoWo;
        const int oy = (int)(r / Wo), ox = (int)(r - (int64_t)oy * Wo);
        float part = 0.0f;
        for (int ky = 0; ky < 4; ++ky) {
            const int iy = oy + ky - 1;
            if (iy < 0 || iy >= d.H) continue;                 // a zero tap adds nothing to the fused sum
            for (int kx = 0; kx < 4; ++kx) {
                const int ix = ox + kx - 1;
                if (ix < 0 || ix >= d.W) continue;
                const float* sp = d.src + ((s * d.H + iy) * d.W + ix) * (int64_t)d.C;
                const float* wp = d.w + (ky * 4 + kx) * d.C;
                for (int c4 = lane; c4 < C4; c4 += 64) {
                    float x[4], w[4];
                    load_vec<4>(sp + 4 * c4, x);
                    load_vec<4>(wp + 4 * c4, w);
#pragma unroll
                    for (int j = 0; j < 4; ++j) part = fmaf(w[j], x[j], part);
                }
            }
        }
        part = wave_sum(part);
        if (lane == 0) d.logits[p] = __fadd_rn(part, d.bias);
    }
}

// torch's softplus (beta 1, threshold 20) as an f32 value: log1p(exp(x)) is evaluated in f64 and rounded ONCE (log1pf(expf(x)) would round
// twice; the logits are few, the f64 rate does not matter here)
__device__ __forceinline__ float softplus(float x) { return x > 20.0f ? x : (float)log1p(exp((double)x)); }

// One wave per sample.
__global__ __launch_bounds__(64) void gan_terms_kernel(const FridoGanTerms d) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const float* l = d.logits + (int64_t)s * d.n;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < d.n; i += 64) {
        const float v = l[i];
        a[0] += (double)v;
        a[1] += (double)fmaxf(__fsub_rn(1.0f, v), 0.0f);
        a[2] += (double)fmaxf(__fadd_rn(1.0f, v), 0.0f);
        a[3] += (double)softplus(-v);
        a[4] += (double)softplus(v);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] = wave_sum(a[k]);
    if (lane < 5) {
        double v = a[0];
#pragma unroll
        for (int k = 1; k < 5; ++k) v = lane == k ? a[k] : v;
        d.sums[(int64_t)s * 5 + lane] = v;
    }
}

// One wave: lane 0 adds the samples in index order; the lanes share the per-sample means.
__global__ __launch_bounds__(64) void gan_finish_kernel(const FridoGanFinish d) {
    const int lane = threadIdx.x;
    for (int s = lane; s < 2 * d.B; s += 64) d.per_sample[s] = (float)(d.sums[(int64_t)s * 5] / (double)d.n);
    if (lane != 0) return;
    const double N = (double)d.B * (double)d.n;
    double lr = 0.0, lf = 0.0, hr = 0.0, hf = 0.0, vr = 0.0, vf = 0.0;
    for (int s = 0; s < d.B; ++s) {
        const double* r = d.sums + (int64_t)s * 5;
        const double* f = d.sums + (int64_t)(s + d.B) * 5;
        lr += r[0];
        hr += r[1];
        vr += r[3];
        lf += f[0];
        hf += f[2];
        vf += f[4];
    }
    d.out[0] = (float)(lr / N);
    d.out[1] = (float)(lf / N);
    d.out[2] = (float)(-(lf / N));
    d.out[3] = (float)(0.5 * (hr / N + hf / N));
    d.out[4] = (float)(0.5 * (vr / N + vf / N));
}

}  // namespace

extern "C" int frido_sizeof_disc_stem(void) { return (int)sizeof(FridoDiscStem); }
extern "C" int frido_sizeof_affine_leaky(void) { return (int)sizeof(FridoAffineLeaky); }
extern "C" int frido_sizeof_disc_head(void) { return (int)sizeof(FridoDiscHead); }
extern "C" int frido_sizeof_gan_terms(void) { return (int)sizeof(FridoGanTerms); }
extern "C" int frido_sizeof_gan_finish(void) { return (int)sizeof(FridoGanFinish); }

extern "C" int frido_disc_stem(const FridoDiscStem* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->w && d->bias && d->dst && d->B > 0, "bad arguments");
    FRIDO_REQUIRE(d->Cin >= 1 && d->Cin <= 8, "1 .. 8 input channels");
    FRIDO_REQUIRE(d->H >= 2 && d->W >= 2, "the image must hold one output pixel");
    FRIDO_REQUIRE(d->ndf >= 4 && d->ndf % 4 == 0, "ndf must be a multiple of 4");
    FRIDO_REQUIRE(d->ndf * 16 * d->Cin <= STEM_LDS_FLOATS, "the weights must fit 32 KB of LDS (ndf * Cin <= 512)");
    FRIDO_REQUIRE(aligned16(d->bias) && aligned16(d->dst), "bias and dst must be 16-byte aligned");
    const int Ho = (d->H - 2) / 2 + 1, Wo = (d->W - 2) / 2 + 1;
    const int64_t P = (int64_t)(d->y ? 2 : 1) * d->B * Ho * Wo;
    const int pps = 256 / (d->ndf / 4);
    const int64_t tile = (int64_t)pps * STEM_PIX, ntiles = (P + tile - 1) / tile;
    const int grid = (int)(ntiles < PG_GRID_CAP ? ntiles : PG_GRID_CAP);
    hipLaunchKernelGGL(disc_stem_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d, Ho, Wo, P, pps, ntiles);
    return frido_check_launch("disc_stem");
}

extern "C" int frido_affine_leaky(const FridoAffineLeaky* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->a && d->b && d->dst && d->rows > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->C % 4 == 0, "C must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->src) && aligned16(d->dst) && aligned16(d->a) && aligned16(d->b), "src, dst, a and b must be 16-byte aligned");
    const int64_t units = d->rows * (d->C / 4);
    hipLaunchKernelGGL(affine_leaky_kernel, dim3(grid_for(units, PG_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, units);
    return frido_check_launch("affine_leaky");
}

extern "C" int frido_disc_head(const FridoDiscHead* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->w && d->logits && d->S > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->H >= 2 && d->W >= 2, "the plane must hold one output pixel");
    FRIDO_REQUIRE(d->C % 4 == 0, "C must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->src) && aligned16(d->w), "src and w must be 16-byte aligned");
    const int Ho = d->H - 1, Wo = d->W - 1;
    const int64_t P = (int64_t)d->S * Ho * Wo;
    const int64_t blocks = (P + 3) / 4;
    const int grid = (int)(blocks < PG_GRID_CAP ? blocks : PG_GRID_CAP);
    hipLaunchKernelGGL(disc_head_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d, Ho, Wo, P);
    return frido_check_launch("disc_head");
}

extern "C" int frido_gan_terms(const FridoGanTerms* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->logits && d->sums && d->S > 0 && d->n > 0, "bad arguments");
    FRIDO_REQUIRE(((uintptr_t)d->sums & 7) == 0, "sums must be 8-byte aligned");
    hipLaunchKernelGGL(gan_terms_kernel, dim3(d->S), dim3(64), 0, (hipStream_t)s, *d);
    return frido_check_launch("gan_terms");
}

extern "C" int frido_gan_finish(const FridoGanFinish* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->sums && d->out && d->per_sample && d->B > 0 && d->n > 0, "bad arguments");
    FRIDO_REQUIRE(((uintptr_t)d->sums & 7) == 0, "sums must be 8-byte aligned");
    hipLaunchKernelGGL(gan_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, *d);
    return frido_check_launch("gan_finish");
}

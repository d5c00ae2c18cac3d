// The launches of the Fréchet Inception Distance around the Inception-v3 tower's convolutions (include/frido_fid.h): the input transform
// (quantise, TF1-legacy bilinear resize, (v - 128) / 128), the 3 x 3 pools, the global average pool, the f64 feature statistics.  Plain
// f32 / f64 arithmetic: no operand planes, so no status word (launch.h alone, like lpips.hip and patchgan.hip) and the two builds of the
// library compile the same code.  The launches sit between the programs of the tower's graph, they are no op kinds.  Nothing is added
// across threads and every sum has a fixed order: a replay returns the same bits.  The build contracts a * b + c into an fma
// (-ffp-contract=on); where the header promises separately rounded operations the __f*_rn intrinsics keep them apart, as in fold.hip.
// All four are bandwidth kernels except the statistics, 2 B D^2 f64 FMAs on the vector pipe (0.27 GFLOP at B = 64, D = 2048).
#include "launch.h"
#include "frido_fid.h"

namespace {

constexpr int FID_GRID_CAP = 1024;        // 4 workgroups per CU; larger problems take further trips of the grid-stride loops

// FridoGemm.out_u8's two conversions (igemm_shared.h, fold.hip), expression for expression, kept as the float that holds the integer
__device__ __forceinline__ float quantise(float x, int mode) {
    float u;
    if (mode == FRIDO_FID_QUANT_PIL) u = __fmul_rn(255.0f, __fmul_rn(__fadd_rn(fminf(fmaxf(x, -1.0f), 1.0f), 1.0f), 0.5f));
    else u = fminf(fmaxf(__fmul_rn(__fadd_rn(x, 1.0f), 127.5f), 0.0f), 255.0f);
    return truncf(u);
}

// a + (b - a) * t, three roundings
__device__ __forceinline__ float lerp3(float a, float b, float t) { return __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), t)); }

// One thread per FOUR consecutive output pixels: their 12 floats are three 16-byte stores (dst is 16-byte aligned and 4 pixels are 48
// bytes); the last unit of a pixel count that is no multiple of 4 stores scalars.  Every source index is clamped into the plane.
__global__ __launch_bounds__(256) void fid_preprocess_kernel(const FridoFidPreprocess d, float sy, float sx, int64_t P, int64_t units) {
    const int64_t HW = (int64_t)d.H * d.W, SS = (int64_t)d.S * d.S;
    const uint8_t* s8 = static_cast<const uint8_t*>(d.src);
    const float* sf = static_cast<const float*>(d.src);
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        float o[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t p = 4 * u + j < P ? 4 * u + j : P - 1;
            const int64_t b = p / SS, r = p - b * SS;
            const int oy = (int)(r / d.S), ox = (int)(r - (int64_t)oy * d.S);
            const float fy = __fmul_rn((float)oy, sy), fx = __fmul_rn((float)ox, sx);
            int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
            y0 = y0 < d.H - 1 ? y0 : d.H - 1;
            x0 = x0 < d.W - 1 ? x0 : d.W - 1;
            const int y1 = y0 + 1 < d.H - 1 ? y0 + 1 : d.H - 1, x1 = x0 + 1 < d.W - 1 ? x0 + 1 : d.W - 1;
            const float ty = __fsub_rn(fy, (float)y0), tx = __fsub_rn(fx, (float)x0);
            const int64_t i00 = (int64_t)y0 * d.W + x0, i01 = (int64_t)y0 * d.W + x1, i10 = (int64_t)y1 * d.W + x0, i11 = (int64_t)y1 * d.W + x1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float q00, q01, q10, q11;
                if (d.src_kind == FRIDO_FID_SRC_U8_HWC) {
                    const uint8_t* im = s8 + b * HW * 3 + c;
                    q00 = (float)im[i00 * 3];
                    q01 = (float)im[i01 * 3];
                    q10 = (float)im[i10 * 3];
                    q11 = (float)im[i11 * 3];
                } else {
                    const float* im = sf + (b * 3 + c) * HW;
                    q00 = quantise(im[i00], d.quant);
                    q01 = quantise(im[i01], d.quant);
                    q10 = quantise(im[i10], d.quant);
                    q11 = quantise(im[i11], d.quant);
                }
                const float v = lerp3(lerp3(q00, q01, tx), lerp3(q10, q11, tx), ty);
                o[3 * j + c] = __fdiv_rn(__fsub_rn(v, 128.0f), 128.0f);
            }
        }
        float* dp = d.dst + 12 * u;
        if (4 * u + 4 <= P) {
            store_vec<4>(dp, o);
            store_vec<4>(dp + 4, o + 4);
            store_vec<4>(dp + 8, o + 8);
        } else {
            const int n = (int)(P - 4 * u) * 3;
            for (int k = 0; k < n; ++k) dp[k] = o[k];
        }
    }
}

// torch's max pool keeps a NaN (max_pool2d: `val > maxval || isnan(val)`)
__device__ __forceinline__ float max_keep_nan(float m, float v) { return (v > m || v != v) ? v : m; }

// One thread per four channels of an output pixel: one 16-byte load per tap inside the plane, one 16-byte store.
__global__ __launch_bounds__(256) void pool3_kernel(const FridoPool3 d, int Ho, int Wo, int64_t units) {
    const int C4 = d.C >> 2;
    const int stride = d.mode == FRIDO_POOL3_MAX_S2 ? 2 : 1, pad = d.mode == FRIDO_POOL3_MAX_S2 ? 0 : 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        const int64_t p = i / C4;                               // (b, oy, ox)
        const int ox = (int)(p % Wo);
        const int64_t q = p / Wo;
        const int oy = (int)(q % Ho);
        const int64_t b = q / Ho;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int n = 0;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * stride + ky - pad;
            if (iy < 0 || iy >= d.H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * stride + kx - pad;
                if (ix < 0 || ix >= d.W) continue;
                float v[4];
                load_vec<4>(d.src + ((b * d.H + iy) * d.W + ix) * (int64_t)d.C + 4 * c4, v);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (n == 0) acc[k] = v[k];
                    else if (d.mode == FRIDO_POOL3_AVG_S1P1) acc[k] = __fadd_rn(acc[k], v[k]);
                    else acc[k] = max_keep_nan(acc[k], v[k]);
                }
                ++n;
            }
        }
        if (d.mode == FRIDO_POOL3_AVG_S1P1) {
            const float cnt = (float)n;                         // n >= 4: the centre tap and its neighbours inside a plane of H, W >= 2; >= 1 always
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = __fdiv_rn(acc[k], cnt);
        }
        store_vec<4>(d.dst + p * d.ldd + d.c0 + 4 * c4, acc);
    }
}

// One thread per four channels of a sample, the pixels in index order.
__global__ __launch_bounds__(256) void gap_kernel(const FridoGap d, int64_t units) {
    const int C4 = d.C >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        const int64_t b = i / C4;
        const float* sp = d.src + b * d.HW * (int64_t)d.C + 4 * c4;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = 0; p < d.HW; ++p) {
            float v[4];
            load_vec<4>(sp + (int64_t)p * d.C, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] += (double)v[k];
        }
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (float)(a[k] / (double)d.HW);
        store_vec<4>(d.dst + b * d.C + 4 * c4, o);
    }
}

// Workgroup = one 64 x 64 tile of s2 per trip; thread (ty, tx) = (t / 16, t % 16) owns rows i0 + 4 ty .. + 3 and columns j0 + 4 tx .. + 3,
// sixteen f64 accumulators that start from the stored values.  D % 4 == 0, so a thread's four rows (columns) are inside D together or
// not at all.  A product of two f32 values is exact in f64: the fma below rounds once, exactly as a separate multiply and add would.
// The first tile column's threads with tx == 0 also own s1 of their rows.  All of a wave's loads of a row are two float4 per lane from
// at most 128 distinct bytes + 16 bytes: served by the L1.
__global__ __launch_bounds__(256) void feat_accum_kernel(const FridoFeatAccum d, int nt, int64_t ntiles) {
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ti = (int)(t / nt), tj = (int)(t - (int64_t)ti * nt);
        const int i = ti * 64 + 4 * ty, j = tj * 64 + 4 * tx;
        if (i >= d.D || j >= d.D) continue;                    // no barrier in this kernel
        double acc[4][4], a1[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = d.s2[(int64_t)(i + a) * d.D + j + c];
        }
        const bool own1 = tj == 0 && tx == 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) a1[a] = own1 ? d.s1[i + a] : 0.0;
        for (int b = 0; b < d.B; ++b) {
            const float* row = d.x + (int64_t)b * d.D;
            float xi[4], xj[4];
            load_vec<4>(row + i, xi);
            load_vec<4>(row + j, xj);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                a1[a] += (double)xi[a];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma((double)xi[a], (double)xj[c], acc[a][c]);
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) d.s2[(int64_t)(i + a) * d.D + j + c] = acc[a][c];
        }
        if (own1) {
#pragma unroll
            for (int a = 0; a < 4; ++a) d.s1[i + a] = a1[a];
        }
    }
}

}  // namespace

extern "C" int frido_sizeof_fid_preprocess(void) { return (int)sizeof(FridoFidPreprocess); }
extern "C" int frido_sizeof_pool3(void) { return (int)sizeof(FridoPool3); }
extern "C" int frido_sizeof_gap(void) { return (int)sizeof(FridoGap); }
extern "C" int frido_sizeof_feat_accum(void) { return (int)sizeof(FridoFeatAccum); }

extern "C" int frido_fid_preprocess(const FridoFidPreprocess* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->H > 0 && d->W > 0 && d->S > 0, "bad arguments");
    FRIDO_REQUIRE(d->src_kind == FRIDO_FID_SRC_U8_HWC || d->src_kind == FRIDO_FID_SRC_F32_NCHW, "src_kind: uint8 HWC (0) or f32 NCHW (1)");
    FRIDO_REQUIRE(d->src_kind == FRIDO_FID_SRC_U8_HWC || d->quant == FRIDO_FID_QUANT_PIL || d->quant == FRIDO_FID_QUANT_NP,
                  "quant: 2 (custom_to_pil) or 1 (custom_to_np)");
    FRIDO_REQUIRE(d->H < (1 << 24) && d->W < (1 << 24) && d->S < (1 << 24), "sides must be exact as f32");
    FRIDO_REQUIRE(aligned16(d->dst), "dst must be 16-byte aligned");
    const int64_t P = (int64_t)d->B * d->S * d->S, units = (P + 3) / 4;
    hipLaunchKernelGGL(fid_preprocess_kernel, dim3(grid_for(units, FID_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d,
                       (float)d->H / (float)d->S, (float)d->W / (float)d->S, P, units);
    return frido_check_launch("fid_preprocess");
}

extern "C" int frido_pool3(const FridoPool3* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->H > 0 && d->W > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->mode == FRIDO_POOL3_MAX_S2 || d->mode == FRIDO_POOL3_MAX_S1P1 || d->mode == FRIDO_POOL3_AVG_S1P1,
                  "mode: max s2 (0), max s1 p1 (1) or average s1 p1 (2)");
    FRIDO_REQUIRE(d->mode != FRIDO_POOL3_MAX_S2 || (d->H >= 3 && d->W >= 3), "the plane must hold one 3 x 3 window");
    FRIDO_REQUIRE(d->C % 4 == 0 && d->ldd % 4 == 0 && d->c0 % 4 == 0, "C, ldd and c0 must be multiples of 4");
    FRIDO_REQUIRE(d->c0 >= 0 && d->c0 + d->C <= d->ldd, "the columns c0 .. c0 + C must lie inside ldd");
    FRIDO_REQUIRE(aligned16(d->src) && aligned16(d->dst), "src and dst must be 16-byte aligned");
    const int Ho = d->mode == FRIDO_POOL3_MAX_S2 ? (d->H - 3) / 2 + 1 : d->H, Wo = d->mode == FRIDO_POOL3_MAX_S2 ? (d->W - 3) / 2 + 1 : d->W;
    const int64_t units = (int64_t)d->B * Ho * Wo * (d->C / 4);
    hipLaunchKernelGGL(pool3_kernel, dim3(grid_for(units, FID_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, Ho, Wo, units);
    return frido_check_launch("pool3");
}

extern "C" int frido_gap(const FridoGap* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->HW > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->C % 4 == 0, "C must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->src) && aligned16(d->dst), "src and dst must be 16-byte aligned");
    const int64_t units = (int64_t)d->B * (d->C / 4);
    hipLaunchKernelGGL(gap_kernel, dim3(grid_for(units, FID_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, units);
    return frido_check_launch("gap");
}

extern "C" int frido_feat_accum(const FridoFeatAccum* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->s1 && d->s2 && d->B > 0 && d->D > 0, "bad arguments");
    FRIDO_REQUIRE(d->D % 4 == 0, "D must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->x) && ((uintptr_t)d->s1 & 7) == 0 && ((uintptr_t)d->s2 & 7) == 0, "x must be 16-byte, s1 and s2 8-byte aligned");
    const int nt = (d->D + 63) / 64;
    const int64_t ntiles = (int64_t)nt * nt;
    const int grid = (int)(ntiles < 2 * FID_GRID_CAP ? ntiles : 2 * FID_GRID_CAP);
    hipLaunchKernelGGL(feat_accum_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, *d, nt, ntiles);
    return frido_check_launch("feat_accum");
}

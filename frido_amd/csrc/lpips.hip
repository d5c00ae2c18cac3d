// The memory-bound part of LPIPS around the VGG16 convolutions (include/frido_lpips.h): the ScalingLayer of an image pair into one NHWC
// block, the 2 x 2 max pool between the feature slices, one feature layer's normalise / project / spatial sum, and the sum over the layers.
// Plain f32 arithmetic with f64 sums: no operand planes, so no status word (launch.h alone, like vision.hip) and the two builds of
// the library compile the same code.  The launches sit between the slice programs of the LPIPS graph, they are no op kinds: nothing of
// frido_hip.h's op table knows them.  No atomics anywhere and every sum in a fixed order, so a replay returns the same bits.
// These are bandwidth kernels: 16-byte accesses wherever the shape allows them, and the per-pixel channel sums stay in registers
// (wave64 xor-shuffles), the features are read from memory once.
#include "launch.h"
#include "frido_lpips.h"

namespace {

constexpr int LPIPS_GRID_CAP = 1024;      // 4 workgroups per CU; larger problems take further trips of the grid-stride loop

// V consecutive pixels of one sample per thread: three plane loads, one contiguous run of 3 V floats out (16-byte accesses for V == 4:
// a sample's plane is then a whole number of vectors).  Every unit index is < units = 2B * HW / V.
template <int V>
__global__ __launch_bounds__(256) void lpips_scale_kernel(const FridoLpipsScale d, int64_t units) {
    const int64_t HW = (int64_t)d.H * d.W, per = HW / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int64_t s = i / per, p = (i % per) * V;
        const float* src = (s < d.B ? d.x + s * 3 * HW : d.y + (s - d.B) * 3 * HW) + p;
        float o[3 * V];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[V];
            load_vec<V>(src + c * HW, v);
#pragma unroll
            for (int k = 0; k < V; ++k) o[k * 3 + c] = __fdiv_rn(__fsub_rn(v[k], d.shift[c]), d.scale[c]);
        }
        float* dst = d.dst + (s * HW + p) * 3;
        if constexpr (V == 4) {
#pragma unroll
            for (int j = 0; j < 3; ++j) store_vec<4>(dst + 4 * j, o + 4 * j);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) dst[j] = o[j];
        }
    }
}

// One thread owns four channels of one output pixel: four 16-byte loads (rows 2 oy, 2 oy + 1 <= H - 1; columns 2 ox, 2 ox + 1 <= W - 1),
// one 16-byte store.
__global__ __launch_bounds__(256) void maxpool2_kernel(const FridoMaxPool2 d, int64_t units) {
    const int C4 = d.C >> 2, Ho = d.H >> 1, Wo = d.W >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        int64_t r = i / C4;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const int64_t b = r / Ho;
        const float* p = d.src + (((b * d.H + 2 * oy) * d.W + 2 * ox) * (int64_t)d.C + 4 * c4);
        float a[4], q[4], m[4];
        load_vec<4>(p, a);
        load_vec<4>(p + d.C, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = fmaxf(a[k], q[k]);
        load_vec<4>(p + (int64_t)d.W * d.C, a);
        load_vec<4>(p + (int64_t)d.W * d.C + d.C, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = fmaxf(m[k], fmaxf(a[k], q[k]));
        store_vec<4>(d.dst + i * 4, m);                    // unit i IS four consecutive floats of dst: (b, oy, ox, c4) in storage order
    }
}

// sum over the LP lanes of a pixel (LP = 16 / 32 / 64 consecutive lanes): every lane of the group ends with the same value
template <int LP>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = LP >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sqrt(sum f^2) + eps, eps OUTSIDE the root (lpips.py:116-118), from the f64 channel sum
__device__ __forceinline__ float norm_of(double s) { return __fadd_rn(sqrtf((float)s), 1e-10f); }
// one channel's w (f0 / n0 - f1 / n1)^2: real divisions, every f32 operation rounded on its own
__device__ __forceinline__ double term(float a0, float a1, float n0, float n1, float w) {
    const float t = __fsub_rn(__fdiv_rn(a0, n0), __fdiv_rn(a1, n1));
    return (double)__fmul_rn(__fmul_rn(t, t), w);
}

// Workgroup (blk, b): the pixels blk * per .. of sample b, four waves, 64 / LP pixels per wave and trip, LP lanes across the channels of a
// pixel, each with the float4 columns sub, sub + LP, ...  NV > 0: a lane's columns (at most NV per tensor, C <= 4 LP NV) stay in registers
// between the norm pass and the difference pass; NV == 0: any C, the second pass reads the row again (from the caches).
// Order of the sums: a lane's elements in index order, the xor tree over the group, the pixels of a lane slot in index order in f64,
// the slots of a wave in order, the waves in order.
template <int LP, int NV>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const FridoLpipsLayer d, int per) {
    constexpr int PPW = 64 / LP;
    __shared__ double wave_sum[4];
    const int b = blockIdx.y, blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LP, slot = lane / LP;
    const int C4 = d.C >> 2;
    const int64_t p0 = (int64_t)blk * per;
    const int64_t p1 = p0 + per < d.HW ? p0 + per : d.HW;
    double acc = 0.0;
    for (int64_t g = p0 + wave * PPW; g < p1; g += 4 * PPW) {      // wave-uniform: every lane takes part in the shuffles
        const int64_t p = g + slot;
        const bool live = p < p1;
        const int64_t row = ((int64_t)b * d.HW + (live ? p : p0)) * d.C;
        const float* r0 = d.f0 + row;
        const float* r1 = d.f1 + row;
        double s0 = 0.0, s1 = 0.0, dd = 0.0;      // the elements are f32, their products exact in f64; the sums carry no f32 rounding
        if constexpr (NV > 0) {
            float a0[NV][4], a1[NV][4];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c4 = sub + j * LP;
                if (live && c4 < C4) {
                    load_vec<4>(r0 + 4 * c4, a0[j]);
                    load_vec<4>(r1 + 4 * c4, a1[j]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) a0[j][k] = a1[j][k] = 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s0 = fma((double)a0[j][k], (double)a0[j][k], s0);
                    s1 = fma((double)a1[j][k], (double)a1[j][k], s1);
                }
            }
            const float n0 = norm_of(group_sum<LP>(s0)), n1 = norm_of(group_sum<LP>(s1));
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c4 = sub + j * LP;
                if (c4 < C4) {
                    float w[4];
                    load_vec<4>(d.w + 4 * c4, w);
#pragma unroll
                    for (int k = 0; k < 4; ++k) dd += term(a0[j][k], a1[j][k], n0, n1, w[k]);
                }
            }
        } else {
            if (live)
                for (int c4 = sub; c4 < C4; c4 += LP) {
                    float a0[4], a1[4];
                    load_vec<4>(r0 + 4 * c4, a0);
                    load_vec<4>(r1 + 4 * c4, a1);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        s0 = fma((double)a0[k], (double)a0[k], s0);
                        s1 = fma((double)a1[k], (double)a1[k], s1);
                    }
                }
            const float n0 = norm_of(group_sum<LP>(s0)), n1 = norm_of(group_sum<LP>(s1));
            if (live)
                for (int c4 = sub; c4 < C4; c4 += LP) {
                    float a0[4], a1[4], w[4];
                    load_vec<4>(r0 + 4 * c4, a0);
                    load_vec<4>(r1 + 4 * c4, a1);
                    load_vec<4>(d.w + 4 * c4, w);
#pragma unroll
                    for (int k = 0; k < 4; ++k) dd += term(a0[k], a1[k], n0, n1, w[k]);
                }
        }
        dd = group_sum<LP>(dd);
        if (live) acc += dd;                                // the same value in every lane of the group; lane sub == 0 is the one read below
    }
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < PPW; ++s) tot += __shfl(acc, s * LP);
    if (lane == 0) wave_sum[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) d.partials[(int64_t)b * d.nblk + blk] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// One wave per sample: lane l < 5 adds layer l's partials of the sample in index order, lane 0 forms the total.
__global__ __launch_bounds__(64) void lpips_finish_kernel(const FridoLpipsFinish d) {
    __shared__ float r[5];
    const int b = blockIdx.x, l = threadIdx.x;
    if (l < 5) {
        int64_t off = 0;
        for (int j = 0; j < l; ++j) off += (int64_t)d.B * d.nblk[j];
        const double* p = d.partials + off + (int64_t)b * d.nblk[l];
        double s = 0.0;
        for (int k = 0; k < d.nblk[l]; ++k) s += p[k];
        r[l] = (float)(s / (double)d.HW[l]);
        d.per_layer[b * 5 + l] = r[l];
    }
    __syncthreads();
    if (l == 0) d.out[b] = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), r[2]), r[3]), r[4]);
}

}  // namespace

extern "C" int frido_sizeof_lpips_scale(void) { return (int)sizeof(FridoLpipsScale); }
extern "C" int frido_sizeof_maxpool2(void) { return (int)sizeof(FridoMaxPool2); }
extern "C" int frido_sizeof_lpips_layer(void) { return (int)sizeof(FridoLpipsLayer); }
extern "C" int frido_sizeof_lpips_finish(void) { return (int)sizeof(FridoLpipsFinish); }

extern "C" int frido_lpips_scale(const FridoLpipsScale* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->x && d->y && d->dst && d->B > 0 && d->H > 0 && d->W > 0, "bad arguments");
    FRIDO_REQUIRE(d->scale[0] != 0.0f && d->scale[1] != 0.0f && d->scale[2] != 0.0f, "a zero scale");
    const int64_t HW = (int64_t)d->H * d->W, pixels = 2 * (int64_t)d->B * HW;
    // 16-byte accesses where every plane of every sample starts on a vector (HW % 4 == 0, aligned tensors); one pixel per thread otherwise
    if (HW % 4 == 0 && aligned16(d->x) && aligned16(d->y) && aligned16(d->dst))
        hipLaunchKernelGGL(lpips_scale_kernel<4>, dim3(grid_for(pixels / 4, LPIPS_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, pixels / 4);
    else
        hipLaunchKernelGGL(lpips_scale_kernel<1>, dim3(grid_for(pixels, LPIPS_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, pixels);
    return frido_check_launch("lpips_scale");
}

extern "C" int frido_maxpool2(const FridoMaxPool2* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->H >= 2 && d->W >= 2, "the plane must hold one 2 x 2 window");
    FRIDO_REQUIRE(d->C % 4 == 0, "C must be a multiple of 4");
    FRIDO_REQUIRE(aligned16(d->src) && aligned16(d->dst), "src and dst must be 16-byte aligned");
    const int64_t units = (int64_t)d->B * (d->H / 2) * (d->W / 2) * (d->C / 4);
    hipLaunchKernelGGL(maxpool2_kernel, dim3(grid_for(units, LPIPS_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, units);
    return frido_check_launch("maxpool2");
}

extern "C" int frido_lpips_layer(const FridoLpipsLayer* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->f0 && d->f1 && d->w && d->partials && d->HW > 0 && d->C > 0, "bad arguments");
    FRIDO_REQUIRE(d->B > 0 && d->B <= 65535, "1 .. 65535 samples (the grid's second dimension)");
    FRIDO_REQUIRE(d->C % 4 == 0, "C must be a multiple of 4");
    FRIDO_REQUIRE(d->nblk >= 1 && d->nblk <= d->HW, "1 .. HW workgroups per sample");
    FRIDO_REQUIRE(aligned16(d->f0) && aligned16(d->f1) && aligned16(d->w), "f0, f1 and w must be 16-byte aligned");
    FRIDO_REQUIRE(((uintptr_t)d->partials & 7) == 0, "partials must be 8-byte aligned");
    const int per = (d->HW + d->nblk - 1) / d->nblk, C4 = d->C / 4;
    const dim3 grid(d->nblk, d->B);
#define LPIPS_LAYER(LP, NV) hipLaunchKernelGGL((lpips_layer_kernel<LP, NV>), grid, dim3(256), 0, (hipStream_t)s, *d, per)
    if (C4 <= 16) LPIPS_LAYER(16, 1);           // relu1_2: four pixels per wave and trip
    else if (C4 <= 32) LPIPS_LAYER(32, 1);      // relu2_2
    else if (C4 <= 64) LPIPS_LAYER(64, 1);      // relu3_3
    else if (C4 <= 128) LPIPS_LAYER(64, 2);     // relu4_3, relu5_3
    else LPIPS_LAYER(64, 0);
#undef LPIPS_LAYER
    return frido_check_launch("lpips_layer");
}

extern "C" int frido_lpips_finish(const FridoLpipsFinish* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->partials && d->per_layer && d->out && d->B > 0, "bad arguments");
    for (int l = 0; l < 5; ++l) FRIDO_REQUIRE(d->nblk[l] >= 1 && d->HW[l] >= 1, "every layer needs a block count and a pixel count");
    FRIDO_REQUIRE(((uintptr_t)d->partials & 7) == 0, "partials must be 8-byte aligned");
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(d->B), dim3(64), 0, (hipStream_t)s, *d);
    return frido_check_launch("lpips_finish");
}

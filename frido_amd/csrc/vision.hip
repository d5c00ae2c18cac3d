// The front of the CLIP image tower (include/frido_vision.h): bicubic resize to the tower's resolution, CLIP's mean / std, and the
// cut into P x P patches laid out as the rows of the patch-embedding GEMM -- one launch, f32 in, f32 out.
// Plain f32 arithmetic: no operand planes, so no status word (launch.h alone, like fold.hip) and the two builds of the library compile the
// same code.  The launch is the first node of the tower's graph, not an op kind: nothing of frido_hip.h's op table knows it.
// A few hundred KB per image, read once through the caches; the cost is the 16 taps per output element, not the bytes.
#include "launch.h"
#include "frido_vision.h"

namespace {

constexpr int CLIP_PRE_GRID_CAP = 1024;      // 4 workgroups per CU; larger batches take further trips of the grid-stride loop

// Keys cubic convolution weights for the taps i0 - 1 .. i0 + 2 at fraction t (A = -0.75: torch's upsample_bicubic2d).  Every operation
// is rounded on its own, so t = 0 gives exactly {0, 1, 0, 0} and an identity resize returns its input.
__device__ __forceinline__ float cubic_near(float x) {      // |x| <= 1:  ((A + 2) x - (A + 3)) x x + 1
    constexpr float A = -0.75f;
    return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2.0f, x), A + 3.0f), x), x), 1.0f);
}
__device__ __forceinline__ float cubic_far(float x) {       // 1 < |x| < 2:  ((A x - 5A) x + 8A) x - 4A
    constexpr float A = -0.75f;
    return __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, x), 5.0f * A), x), 8.0f * A), x), 4.0f * A);
}
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
    w[0] = cubic_far(__fadd_rn(t, 1.0f));
    w[1] = cubic_near(t);
    w[2] = cubic_near(__fsub_rn(1.0f, t));
    w[3] = cubic_far(__fsub_rn(2.0f, t));
}
// taps of output coordinate o along an axis of n source samples: clamped source indices and weights
__device__ __forceinline__ void taps(int o, float scale, int n, int idx[4], float w[4]) {
    const float s = __fmul_rn((float)o, scale);
    const float f = floorf(s);
    const int i0 = (int)f;
    cubic_weights(__fsub_rn(s, f), w);
#pragma unroll
    for (int j = 0; j < 4; ++j) idx[j] = min(max(i0 - 1 + j, 0), n - 1);
}

// One thread owns V consecutive px of one (b, patch, c, py): the four source rows and the vertical weights are shared by the V
// outputs, the store is one 16-byte access (V == 4).  Every source index is clamped to the plane, every unit index is < units.
template <int V>
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const FridoClipPreprocess d, float sy_scale, float sx_scale, int64_t units) {
    const int g = d.res / d.P, pv = d.P / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        const int pxv = (int)(i % pv);
        int64_t r = i / pv;
        const int py = (int)(r % d.P);
        r /= d.P;
        const int c = (int)(r % 3);
        r /= 3;                                             // patch row of dst: (b * g + gy) * g + gx
        const int gx = (int)(r % g), gy = (int)((r / g) % g);
        const int64_t b = r / ((int64_t)g * g);
        const int oy = gy * d.P + py, ox0 = gx * d.P + pxv * V;
        int iy[4];
        float wy[4];
        taps(oy, sy_scale, d.H, iy, wy);
        const float* plane = d.src + (b * 3 + c) * ((int64_t)d.H * d.W);
        const float mean = d.mean[c], rstd = d.rstd[c];
        float out[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int ix[4];
            float wx[4];
            taps(ox0 + k, sx_scale, d.W, ix, wx);
            float rows[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                   // horizontal pass of source row iy[j], then the vertical pass: torch's order
                const float* row = plane + (int64_t)iy[j] * d.W;
                rows[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(row[ix[0]], wx[0]), __fmul_rn(row[ix[1]], wx[1])), __fmul_rn(row[ix[2]], wx[2])),
                                    __fmul_rn(row[ix[3]], wx[3]));
            }
            const float v = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(rows[0], wy[0]), __fmul_rn(rows[1], wy[1])), __fmul_rn(rows[2], wy[2])),
                                      __fmul_rn(rows[3], wy[3]));
            out[k] = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(v, 1.0f), 0.5f), mean), rstd);
        }
        store_vec<V>(d.dst + i * V, out);                   // unit i IS V consecutive floats of dst: (row, c, py, pxv) in storage order
    }
}

// (n_in - 1) / (n_out - 1), 0 for a single output sample: area_pixel_compute_scale with align_corners
inline float axis_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.0f; }

}  // namespace

extern "C" int frido_sizeof_clip_preprocess(void) { return (int)sizeof(FridoClipPreprocess); }

extern "C" int frido_clip_preprocess(const FridoClipPreprocess* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->src && d->dst && d->B > 0 && d->H > 0 && d->W > 0, "bad arguments");
    FRIDO_REQUIRE(d->res > 0 && d->P > 0 && d->res % d->P == 0, "the resolution must be a whole number of patches");
    FRIDO_REQUIRE(aligned16(d->dst), "dst must be 16-byte aligned");
    const int64_t floats = (int64_t)d->B * 3 * d->res * d->res;
    const float sy = axis_scale(d->H, d->res), sx = axis_scale(d->W, d->res);
    // 16-byte stores where a patch row is a whole number of vectors (ViT-B: P = 32 / 16); one float at a time otherwise (ViT-L: P = 14)
    if (d->P % 4 == 0)
        hipLaunchKernelGGL(clip_preprocess_kernel<4>, dim3(grid_for(floats / 4, CLIP_PRE_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, sy, sx, floats / 4);
    else
        hipLaunchKernelGGL(clip_preprocess_kernel<1>, dim3(grid_for(floats, CLIP_PRE_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, sy, sx, floats);
    return frido_check_launch("clip_preprocess");
}

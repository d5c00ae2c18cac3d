// Composed guidance (Liu et al. 2022: several weighted conditionings against one unconditional evaluation; a negative weight negates)
// with the guidance rescale of Lin et al. 2024, not in the reference: FridoGuidanceCompose in include/frido_hip.h.  eps holds n + 1 slots
// of B * per_sample floats -- the conditionings' eps first, the unconditional one last -- and w[0 .. n) the weights, w[n] = phi, on the device:
//   acc = e_u;   for i = 0 .. n - 1, in this order:   acc = acc + w_i * (e_i - e_u)
//        -- per term guided_eps's operations (launch.h): __fadd_rn(acc, __fmul_rn(w_i, __fsub_rn(e_i, e_u))); n = 1 is its mix, bit for bit
//   plain form:     out = acc
//   rescaled form:  out = acc * f_b,   f_b = phi * sigma(e_0) / sigma(acc) + (1 - phi)   per sample b over its per_sample elements
// in plain f32, every product and sum rounded on its own (no FMA contraction), so the two builds of the library compile the same kernels;
// common.h is included for the sticky status word only (a non-finite out raises FRIDO_STATUS_NONFINITE).  out may alias slot 0: a thread
// reads every slot of its elements before it writes them, and the rescaled form's second pass re-reads only what the same thread wrote.
// The statistics are float64 sums of the fp32 values in a fixed order (per-thread strided partials, a wave shuffle tree, the waves'
// partials added in index order through LDS; no atomics, vqloss.hip's discipline): the same bits on every launch.  The rescaled form reads
// scalars whatever the alignment, so that the order of its sums -- and the result -- depends on the inputs alone.
// Bandwidth-bound and tiny next to the n + 1 denoiser evaluations in front of it: its job is to make guidance a step of its own inside the
// captured step body, in front of whichever update kernel follows.
#include "common.h"

namespace {

constexpr int GUIDE_MAX = 8;            // conditionings per launch
constexpr int GUIDE_GRID_CAP = 2048;

// The weights in registers: statically indexed (the loops over them are fully unrolled under `i < n`), so nothing spills.
struct Weights { float w[GUIDE_MAX]; };
__device__ __forceinline__ Weights load_weights(const float* w, int n) {
    Weights r;
#pragma unroll
    for (int i = 0; i < GUIDE_MAX; ++i) r.w[i] = i < n ? w[i] : 0.0f;
    return r;
}

// acc of V consecutive elements at offset o of every slot (`stride` floats apart); e0: slot 0's values, for the rescaled form's statistics.
template <int V>
__device__ __forceinline__ void compose(const float* eps, int64_t stride, int64_t o, int n, const Weights& wt, float acc[V], float e0[V]) {
    float eu[V];
    load_vec<V>(eps + (int64_t)n * stride + o, eu);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = eu[k];
#pragma unroll
    for (int i = 0; i < GUIDE_MAX; ++i) {
        if (i < n) {      // uniform
            float e[V];
            load_vec<V>(eps + (int64_t)i * stride + o, e);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (i == 0) e0[k] = e[k];
                acc[k] = __fadd_rn(acc[k], __fmul_rn(wt.w[i], __fsub_rn(e[k], eu[k])));
            }
        }
    }
}

// Plain form.  One unit = V consecutive elements; V == 4 when B * per_sample is a multiple of 4 and both bases are 16-byte aligned (every
// slot then is), V == 1 otherwise.
template <int V>
__global__ __launch_bounds__(256) void guidance_compose_kernel(const FridoGuidanceCompose d, int64_t units) {
    const int64_t stride = (int64_t)d.B * d.per_sample;
    const Weights wt = load_weights(d.weights, d.n);
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
        float acc[V], e0[V];
        compose<V>(d.eps, stride, i * V, d.n, wt, acc, e0);
#pragma unroll
        for (int k = 0; k < V; ++k) bad |= nonfinite(acc[k]);
        store_vec<V>(d.out + i * V, acc);
    }
    status_raise(false, bad);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;      // lane 0 holds the sum
}

// Rescaled form: workgroup b owns sample b; thread t owns its elements t, t + 256, ...
__global__ __launch_bounds__(256) void guidance_rescale_kernel(const FridoGuidanceCompose d) {
    __shared__ double part[4][4];      // [wave][sum e0, sum e0^2, sum acc, sum acc^2]
    __shared__ float f_sh;
    const int64_t stride = (int64_t)d.B * d.per_sample;
    const int64_t base = (int64_t)blockIdx.x * d.per_sample;
    const Weights wt = load_weights(d.weights, d.n);
    double s_e = 0.0, s_ee = 0.0, s_a = 0.0, s_aa = 0.0;
    for (int64_t j = threadIdx.x; j < d.per_sample; j += 256) {
        float acc[1], e0[1];
        compose<1>(d.eps, stride, base + j, d.n, wt, acc, e0);
        d.out[base + j] = acc[0];
        const double e = (double)e0[0], a = (double)acc[0];
        s_e += e; s_ee += e * e; s_a += a; s_aa += a * a;
    }
    s_e = wave_sum(s_e); s_ee = wave_sum(s_ee); s_a = wave_sum(s_a); s_aa = wave_sum(s_aa);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = s_e; part[wave][1] = s_ee; part[wave][2] = s_a; part[wave][3] = s_aa;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4];
        for (int q = 0; q < 4; ++q) t[q] = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
        const double N = (double)d.per_sample, phi = (double)d.weights[d.n];
        const double ve = t[1] - t[0] * t[0] / N, va = t[3] - t[2] * t[2] / N;      // N * variance: the divisor cancels in the ratio
        double f = 1.0;
        if (va > 0.0) f = phi * sqrt((ve > 0.0 ? ve : 0.0) / va) + (1.0 - phi);
        f_sh = (float)f;
    }
    __syncthreads();
    const float f = f_sh;
    bool bad = false;
    for (int64_t j = threadIdx.x; j < d.per_sample; j += 256) {
        const float o = __fmul_rn(d.out[base + j], f);
        bad |= nonfinite(o);
        d.out[base + j] = o;
    }
    status_raise(false, bad);
}

}  // namespace

extern "C" int frido_guidance_compose(const FridoGuidanceCompose* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->eps && d->out && d->weights, "null pointer");
    FRIDO_REQUIRE(d->n >= 1 && d->n <= GUIDE_MAX, "1 to 8 conditionings");
    FRIDO_REQUIRE(d->B > 0 && d->per_sample > 0, "B and per_sample must be positive");
    const int64_t total = (int64_t)d->B * d->per_sample;
    // out may BE slot 0; any other overlap with the slots would let one thread's result reach another thread's input
    const float* lo = d->eps + (d->out == d->eps ? total : 0);
    const float* hi = d->eps + (int64_t)(d->n + 1) * total;
    FRIDO_REQUIRE(d->out + total <= lo || d->out >= hi, "out may alias slot 0 exactly and must not overlap any other slot");
    if (d->rescale) {
        hipLaunchKernelGGL(guidance_rescale_kernel, dim3(d->B), dim3(256), 0, (hipStream_t)s, *d);
    } else if (total % 4 == 0 && aligned16(d->eps) && aligned16(d->out)) {
        hipLaunchKernelGGL(guidance_compose_kernel<4>, dim3(grid_for(total / 4, GUIDE_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, total / 4);
    } else {
        hipLaunchKernelGGL(guidance_compose_kernel<1>, dim3(grid_for(total, GUIDE_GRID_CAP)), dim3(256), 0, (hipStream_t)s, *d, total);
    }
    return frido_check_launch("guidance_compose");
}

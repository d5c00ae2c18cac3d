// Launcher toolkit of libfrido_hip: what the single-op launchers (`extern "C" int frido_x(const FridoX* d, frido_stream_t s)`) and the
// small element-wise kernels behind them share.  It defines NO status word: a file of plain f32 / f64 arithmetic (fold.hip, loss.hip,
// vqloss.hip) includes this header alone and registers nothing with the runtime; common.h includes it and adds the operand planes and
// the per-file status word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frido_hip.h"

// ---- host side ----
void frido_set_error(const char* fmt, ...);      // runtime.hip: the thread's frido_last_error() text
int frido_check_launch(const char* what);        // runtime.hip: hipGetLastError() as a FRIDO_* code, "<what>: launch failed: ..."

// rejects a descriptor before anything reaches the device: "<launcher>: <msg> (<condition>)"
#define FRIDO_REQUIRE(cond, msg)                                            \
    do {                                                                    \
        if (!(cond)) {                                                      \
            frido_set_error("%s: %s (%s)", __func__, msg, #cond);           \
            return FRIDO_EINVAL;                                            \
        }                                                                   \
    } while (0)

namespace {

// workgroups of 256 threads for a grid-stride loop over `work_items`, at most `cap` (the caller's choice: how many resident
// workgroups its kernel is worth)
inline int grid_for(int64_t work_items, int cap) {
    int64_t b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- device side ----
// V consecutive floats: one 16-byte access (V == 4, p 16-byte aligned) or one scalar (V == 1)
template <int V>
__device__ __forceinline__ void load_vec(const float* p, float v[V]) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void store_vec(float* p, const float v[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
// NaN or +-inf (what an update kernel reports as FRIDO_STATUS_NONFINITE)
__device__ __forceinline__ bool nonfinite(float v) { return !(fabsf(v) <= 3.0e38f); }
// classifier-free guidance, e_u + s * (e_c - e_u), every operation rounded on its own: the ONE expression of the DDIM / PLMS, DPM-Solver
// and inversion updates, so that a guided eps means the same bits in all of them
__device__ __forceinline__ float guided_eps(float e, float eu, float cfg) { return __fadd_rn(eu, __fmul_rn(cfg, __fsub_rn(e, eu))); }

}  // namespace

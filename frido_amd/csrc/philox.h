// The library's one noise generator: Philox4x32-10 + Box-Muller.  Every kernel that draws noise (frido_randn, the sampler updates in
// misc.hip, the objective in loss.hip) includes this file, so a noise key means the same bits everywhere.  Needs nothing but the HIP
// runtime header; include it inside the including file's anonymous namespace.
#pragma once

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// 4 standard normals for group `grp` of draw `draw` of global sample `sample`
__device__ __forceinline__ void randn4(uint64_t seed, int64_t sample, uint32_t draw, uint32_t stream, uint32_t grp, float out[4]) {
    uint32_t c[4] = {grp, draw, (uint32_t)sample, (uint32_t)((uint64_t)sample >> 32) ^ (stream << 20)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = ((float)c[0] + 1.0f) * 2.3283064365386963e-10f;
    const float u1 = (float)c[1] * 2.3283064365386963e-10f;
    const float u2 = ((float)c[2] + 1.0f) * 2.3283064365386963e-10f;
    const float u3 = (float)c[3] * 2.3283064365386963e-10f;
    const float r0 = sqrtf(-2.0f * logf(fminf(u0, 1.0f))), r1 = sqrtf(-2.0f * logf(fminf(u2, 1.0f)));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0);
    sincosf(6.283185307179586f * u3, &s1, &c1);
    out[0] = r0 * c0; out[1] = r0 * s0; out[2] = r1 * c1; out[3] = r1 * s1;
}

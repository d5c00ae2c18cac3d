// Multi-head flash attention for SMALL head dimensions (gfx950): per sample b and head h, O_h = softmax(alpha * Q_h K_h^T) V_h with
// an online softmax over 32-key groups -- the [Nq][Nk] score matrix is never formed.  The attention core of the reference's
// AttentionBlock (frido/modules/diffusionmodules/pyunet.py:303-358, QKVAttentionLegacy / QKVAttention 381-440): with
// num_head_channels = 32 the f8f4 denoiser has 12 heads over 1024 tokens, 18 over 256 and 30 over 64.  flash.hip tiles over d = C of
// ONE head (128 .. 576); here d is 32 or 64 and the grid runs over (sample, head, query block).
//
// The formulation is flash.hip's, TRANSPOSED so that one query lives in one MFMA column (= lane & 15) through the whole kernel:
//     S^T[key][q] = K_tile . Q^T      A = K fragment (LDS), B = Q fragment (registers, loaded once)
//     O^T[c][q]  += V^T_tile . P^T    A = V^T fragment (LDS), B = P fragment (registers)
//   * row max / row sum of a query are 8 in-register ops + two cross-lane steps (xor 16, 32); the running (max, sum) of a query sit in
//     the lanes that own its O^T column;
//   * the K rows of a 32-key group are stored PERMUTED in LDS (key 8a + 4t + b at row 16t + 4a + b) so that the two S^T fragments of a
//     lane hold keys 8g .. 8g+7 -- the 8 k-slots of the B operand of the PV MFMA: P goes from accumulator to operand registers by a pack;
//   * K / V^T use the [rows][64 B] sub-tile layout of igemm.hip / flash.hip (XOR slot swizzle, conflict-free 16-byte fragment reads): at
//     d = 32 a key row is exactly one 64-byte slot row per plane.
// What differs, because d is small:
//   * a wave owns QF = 2 query fragments (32 queries) where the plane has them: every K / V^T fragment read from LDS feeds two score /
//     output fragments (the accumulators are only d / 16 fragments per query fragment);
//   * a workgroup (4 waves) takes 64 keys per barrier: two 32-key groups, each with its own online-softmax step.  The next tile travels
//     global -> registers under the current tile's MFMAs and is written to the OTHER LDS buffer behind them: ONE barrier per tile, and
//     every load is an ordinary compiler-scheduled one (no LDS-DMA, no hand-counted waits: nothing here needs the ISA audit);
//   * heads and query blocks of one sample are adjacent workgroup ids on one XCD: they share the sample's K / V^T rows in L2.
// Two-plane mode (NS = 2): Q, K, V^T and P carry hi + lo planes, both products are hi*hi + hi*lo + lo*hi in f32.
#include "common.h"

namespace {

template <int NS>
__device__ __forceinline__ f32x4 mma3(const bf16x8 (&a)[NS], const bf16x8 (&b)[NS], f32x4 acc) {
    if constexpr (NS == 2) {
        acc = mfma_op<NS>(a[1], b[0], acc);
        acc = mfma_op<NS>(a[0], b[1], acc);
    }
    return mfma_op<NS>(a[0], b[0], acc);
}

__device__ __forceinline__ float xor_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float xor_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// physical 16-byte slot of logical slot `s` in row `row` of a [rows][64 B] sub-tile
__device__ __forceinline__ int swz(int row, int s) { return s ^ ((4 - ((row >> 2) & 3)) & 3); }

template <int D, int NS>
struct MGeo {
    static constexpr int NW = 4, NT = NW * 64;
    static constexpr int KT = 64, NG = KT / 32;          // keys per tile (one barrier), 32-key groups per tile
    static constexpr int KS = D / 32, CT = D / 16;       // QK^T k-steps; O^T row fragments
    static constexpr int KGRP = KS * 2048;               // bytes of one K group of a plane   ([KS][32 rows][64 B])
    static constexpr int VGRP = D * 64;                  // bytes of one V^T group of a plane ([D rows][64 B])
    static constexpr int KPL = NG * KGRP, VPL = NG * VGRP;
    static constexpr int V0 = NS * KPL;                  // V^T offset inside a buffer
    static constexpr int BUF = NS * (KPL + VPL);
    static constexpr int SMEM = 2 * BUF;                 // d = 64, two planes: exactly 64 KiB
    static constexpr int KU = KT * (D / 8) / NT;         // 16-byte units of a plane per thread: K ...
    static constexpr int VU = D * NG * 4 / NT;           // ... and V^T
    static_assert(KT * (D / 8) % NT == 0 && D * NG * 4 % NT == 0 && SMEM <= 65536, "tile geometry");
};

// FridoAttnMh descriptor (include/frido_hip.h); requirements checked by the launcher.
template <int D, int NS, int QF>
__global__ __launch_bounds__(256, 2) void flash_mh_kernel(const FridoAttnMh d) {
    using G = MGeo<D, NS>;
    constexpr int KS = G::KS, CT = G::CT, NG = G::NG;
    __shared__ __attribute__((aligned(16))) unsigned char smem[G::SMEM];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 15, g = lane >> 4;
    constexpr int BQ = G::NW * 16 * QF;

    // workgroup -> (sample, head, query block); consecutive logical ids (the heads and query blocks of one sample) land on one XCD
    const int qblocks = (d.Nq + BQ - 1) / BQ;
    const int per_b = qblocks * d.heads;
    const int nb = per_b * d.B;
    int bid = blockIdx.x;
    {
        const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    }
    const int z = bid / per_b, rem = bid - z * per_b;
    const int h = rem / qblocks, qb = rem - h * qblocks;
    const int q0 = qb * BQ + wave * (16 * QF);            // first query of this wave (within the sample)

    // ---- Q fragments: lane holds Q_h[q = r][32 ks + 8 g .. +8] of each of its QF query fragments (B operand of S^T = K Q^T) ----
    bf16x8 qf[QF][KS][NS];
    int64_t grow[QF];
    bool q_ok[QF];
#pragma unroll
    for (int f = 0; f < QF; ++f) {
        int qrow = q0 + f * 16 + r;
        q_ok[f] = qrow < d.Nq;
        qrow = q_ok[f] ? qrow : d.Nq - 1;
        grow[f] = (int64_t)z * d.Nq + qrow;                // global row of Q / output
        const frido_bf16* qp = d.Q + grow[f] * d.ldq + (int64_t)h * d.q_hs + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[f][ks][0] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
            if constexpr (NS == 2) qf[f][ks][1] = *reinterpret_cast<const bf16x8*>(qp + d.q_lo + ks * 32);
        }
    }

    // ---- tile staging.  A thread moves KU + VU 16-byte units per plane and tile.
    //      K unit u: key u / (D / 8) of the tile, 8 channels (u % (D / 8)) * 8 ..; V^T unit u: channel u / (4 NG), keys 8 (u % (4 NG)) .. ----
    const frido_bf16* Kb = d.K + (int64_t)z * d.k_bs + (int64_t)h * d.k_hs;
    const frido_bf16* Vb = d.VT + (int64_t)z * d.vt_bs + (int64_t)h * D * d.ldvt;
    int k_key[G::KU], k_col[G::KU], k_lds[G::KU];
#pragma unroll
    for (int i = 0; i < G::KU; ++i) {
        const int u = t + i * G::NT;
        const int key = u / (D / 8), sl = u % (D / 8);
        const int gk = key >> 5, kk = key & 31;
        const int row = 16 * ((kk >> 2) & 1) + 4 * (kk >> 3) + (kk & 3);       // key 8a + 4t + b -> row 16t + 4a + b
        k_key[i] = key;
        k_col[i] = sl * 8;
        k_lds[i] = gk * G::KGRP + (sl >> 2) * 2048 + row * 64 + (swz(row, sl & 3) << 4);
    }
    int v_off[G::VU], v_key[G::VU], v_lds[G::VU];
#pragma unroll
    for (int i = 0; i < G::VU; ++i) {
        const int u = t + i * G::NT;
        const int c = u / (4 * NG), w = u % (4 * NG);
        const int gk = w >> 2, ls = w & 3;
        v_key[i] = gk * 32;                                // first key (within the tile) of the unit's group
        v_off[i] = c * d.ldvt + gk * 32 + ls * 8;
        v_lds[i] = G::V0 + gk * G::VGRP + c * 64 + (swz(c & 15, ls) << 4);
    }
    const int ntiles = (d.Nk + G::KT - 1) / G::KT;
    u32x4 kreg[G::KU][NS], vreg[G::VU][NS];
    // Groups that start at or beyond Nk are not computed; their units are still moved (no divergent staging), from addresses clamped
    // into the operand: K rows past Nk read row Nk - 1, V^T groups past Nk re-read the tile's first group (a V^T row holds only
    // ldvt >= Nk rounded up to 32 columns).
#define MH_LOAD_TILE(j)                                                                                                   \
    {                                                                                                                     \
        const int key0 = (j) * G::KT;                                                                                     \
        _Pragma("unroll") for (int i = 0; i < G::KU; ++i) {                                                               \
            int key = key0 + k_key[i];                                                                                    \
            key = key < d.Nk ? key : d.Nk - 1;                                                                            \
            const frido_bf16* src = Kb + (int64_t)key * d.ldk + k_col[i];                                                 \
            _Pragma("unroll") for (int p = 0; p < NS; ++p) kreg[i][p] = *reinterpret_cast<const u32x4*>(src + (p ? d.k_lo : 0)); \
        }                                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < G::VU; ++i) {                                                               \
            const frido_bf16* src = Vb + key0 + v_off[i] - (key0 + v_key[i] < d.Nk ? 0 : v_key[i]);                       \
            _Pragma("unroll") for (int p = 0; p < NS; ++p) vreg[i][p] = *reinterpret_cast<const u32x4*>(src + (p ? d.vt_lo : 0)); \
        }                                                                                                                 \
    }
#define MH_STORE_TILE(j)                                                                                                  \
    {                                                                                                                     \
        unsigned char* sbuf = smem + ((j) & 1) * G::BUF;                                                                  \
        _Pragma("unroll") for (int i = 0; i < G::KU; ++i)                                                                 \
            _Pragma("unroll") for (int p = 0; p < NS; ++p) *reinterpret_cast<u32x4*>(sbuf + p * G::KPL + k_lds[i]) = kreg[i][p]; \
        _Pragma("unroll") for (int i = 0; i < G::VU; ++i)                                                                 \
            _Pragma("unroll") for (int p = 0; p < NS; ++p) *reinterpret_cast<u32x4*>(sbuf + p * G::VPL + v_lds[i]) = vreg[i][p]; \
    }
    // fragment read offset inside a [16 rows][64 B] chunk: row r, logical slot g
    const int frag = r * 64 + (swz(r, g) << 4);

    f32x4 o[QF][CT];
    float m_run[QF], l_run[QF];
#pragma unroll
    for (int f = 0; f < QF; ++f) {
        m_run[f] = -1.0e30f;
        l_run[f] = 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c) o[f][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float alpha = d.alpha;

    MH_LOAD_TILE(0)
    MH_STORE_TILE(0)
    __syncthreads();
    for (int j = 0; j < ntiles; ++j) {
        if (j + 1 < ntiles) MH_LOAD_TILE(j + 1)              // in flight under this tile's MFMAs
        const unsigned char* buf = smem + (j & 1) * G::BUF;
#pragma unroll
        for (int gk = 0; gk < NG; ++gk) {
            const int kg0 = j * G::KT + gk * 32;           // first key of the group
            if (kg0 < d.Nk) {                              // (uniform)
                // ================= S^T = K Q^T =================
                bf16x8 kf[KS][2][NS];                      // [k-step][half][plane]
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                        for (int p = 0; p < NS; ++p)
                            kf[ks][hf][p] = *reinterpret_cast<const bf16x8*>(buf + p * G::KPL + gk * G::KGRP + ks * 2048 + hf * 1024 + frag);
                bf16x8 pf[QF][NS];
#pragma unroll
                for (int f = 0; f < QF; ++f) {
                    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        s0 = mma3<NS>(kf[ks][0], qf[f][ks], s0);
                        s1 = mma3<NS>(kf[ks][1], qf[f][ks], s1);
                    }
                    // lane holds the scores of query r against keys kg0 + 8 g + {0..3} (s0) and + {4..7} (s1)
                    float sv[8] = {s0[0] * alpha, s0[1] * alpha, s0[2] * alpha, s0[3] * alpha, s1[0] * alpha, s1[1] * alpha, s1[2] * alpha, s1[3] * alpha};
                    if (kg0 + 32 > d.Nk) {                 // ragged last group (uniform branch)
                        const int k0 = kg0 + 8 * g;
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (k0 + i >= d.Nk) sv[i] = -1.0e30f;
                    }
                    float tmax = fmaxf(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])), fmaxf(fmaxf(sv[4], sv[5]), fmaxf(sv[6], sv[7])));
                    tmax = xor_max(tmax);
                    const float m_new = fmaxf(m_run[f], tmax);
                    const float corr = __expf(m_run[f] - m_new);
                    float pv[8], rs = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        pv[i] = __expf(sv[i] - m_new);
                        rs += pv[i];
                    }
                    rs = xor_sum(rs);
                    l_run[f] = l_run[f] * corr + rs;
                    m_run[f] = m_new;
                    // P fragment (B operand of O^T += V^T P^T): k-slot 8 g + i <-> key kg0 + 8 g + i
                    {
                        uint32_t hh[4], ll[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) split_op2(pv[2 * i], pv[2 * i + 1], NS, hh[i], ll[i]);
                        pf[f][0] = __builtin_bit_cast(bf16x8, u32x4{hh[0], hh[1], hh[2], hh[3]});
                        if constexpr (NS == 2) pf[f][1] = __builtin_bit_cast(bf16x8, u32x4{ll[0], ll[1], ll[2], ll[3]});
                    }
                    if (__any(corr != 1.0f)) {             // the running max moved for some query of this fragment: rescale O^T
#pragma unroll
                        for (int c = 0; c < CT; ++c) {
                            o[f][c][0] *= corr; o[f][c][1] *= corr; o[f][c][2] *= corr; o[f][c][3] *= corr;
                        }
                    }
                }
                // ================= O^T += V^T P^T =================
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    bf16x8 vf[NS];
#pragma unroll
                    for (int p = 0; p < NS; ++p)
                        vf[p] = *reinterpret_cast<const bf16x8*>(buf + G::V0 + p * G::VPL + gk * G::VGRP + c * 1024 + frag);
#pragma unroll
                    for (int f = 0; f < QF; ++f) o[f][c] = mma3<NS>(vf, pf[f], o[f][c]);
                }
            }
        }
        if (j + 1 < ntiles) MH_STORE_TILE(j + 1)             // the other buffer: every wave left it before the last barrier
        __syncthreads();
    }

    // ---- epilogue: lane holds O^T[c = 16 ct + 4 g + e][q = r]: four consecutive channels of its query per fragment ----
    bool sat = false, bad = false;
#pragma unroll
    for (int f = 0; f < QF; ++f) {
        if (!q_ok[f]) continue;
        const float inv = 1.0f / l_run[f];
        bad |= g == 0 && stat_bad(m_run[f], inv);          // softmax statistics of this query
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = h * D + c * 16 + g * 4;
            const float vv[4] = {o[f][c][0] * inv, o[f][c][1] * inv, o[f][c][2] * inv, o[f][c][3] * inv};
            store_op4(d.out_op, d.out_lo, NS, grow[f] * d.ldo + col, vv);
            if (NS == 2) sat |= op_sat4(vv);
        }
    }
    status_raise(sat, bad);
#undef MH_LOAD_TILE
#undef MH_STORE_TILE
}

template <int D, int NS, int QF>
int mh_launch(const FridoAttnMh& d, hipStream_t s) {
    const int bq = MGeo<D, NS>::NW * 16 * QF;
    const int64_t blocks = (int64_t)d.B * d.heads * ((d.Nq + bq - 1) / bq);
    if (blocks > 0x7fffffffll) {
        frido_set_error("frido_attn_mh: %lld workgroups exceed the grid limit", (long long)blocks);
        return FRIDO_EINVAL;
    }
    hipLaunchKernelGGL((flash_mh_kernel<D, NS, QF>), dim3((unsigned)blocks), dim3(256), 0, s, d);
    return frido_check_launch("attn_mh");
}

template <int D>
int mh_dispatch(const FridoAttnMh& d, hipStream_t s) {
    // two query fragments per wave (128 queries per workgroup) where the plane has them; the 8 x 8 plane (64 queries) and grids that
    // would leave compute units idle take one (64 queries per workgroup)
    const bool two = d.Nq > 64 && (int64_t)d.B * d.heads * ((d.Nq + 127) / 128) >= 512;
    if (d.nsplit == 2) return two ? mh_launch<D, 2, 2>(d, s) : mh_launch<D, 2, 1>(d, s);
    return two ? mh_launch<D, 1, 2>(d, s) : mh_launch<D, 1, 1>(d, s);
}

}  // namespace

extern "C" int frido_attn_mh_supported(int32_t dd) { return dd == 32 || dd == 64; }

extern "C" int frido_attn_mh(const FridoAttnMh* d, frido_stream_t s) {
    FRIDO_REQUIRE(d && d->Q && d->K && d->VT && d->out_op, "null pointer");
    FRIDO_REQUIRE(frido_attn_mh_supported(d->d), "head dimension must be 32 or 64");
    FRIDO_REQUIRE(d->B > 0 && d->heads > 0 && d->Nq > 0 && d->Nk > 0, "empty problem");
    FRIDO_REQUIRE(d->nsplit == 1 || d->nsplit == 2, "nsplit must be 1 or 2");
    FRIDO_REQUIRE(d->ldvt >= ((d->Nk + 31) & ~31) && (d->ldvt & 7) == 0, "V^T rows must be zero-padded to a multiple of 32 keys");
    FRIDO_REQUIRE(d->ldq >= d->d && d->ldk >= d->d && d->ldo >= d->heads * d->d && d->q_hs >= 0 && d->k_hs >= 0, "row strides shorter than the rows they hold");
    FRIDO_REQUIRE((d->ldq & 7) == 0 && (d->ldk & 7) == 0 && (d->q_hs & 7) == 0 && (d->k_hs & 7) == 0 && (d->ldo & 3) == 0 && (d->q_lo & 7) == 0 &&
                      (d->k_lo & 7) == 0 && (d->vt_lo & 7) == 0 && (d->out_lo & 3) == 0 && (d->k_bs & 7) == 0 && (d->vt_bs & 7) == 0,
                  "strides and plane offsets must keep 16-byte alignment");
    FRIDO_REQUIRE(((uintptr_t)d->Q & 15) == 0 && ((uintptr_t)d->K & 15) == 0 && ((uintptr_t)d->VT & 15) == 0 && ((uintptr_t)d->out_op & 7) == 0,
                  "operand pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)s;
    return d->d == 32 ? mh_dispatch<32>(*d, st) : mh_dispatch<64>(*d, st);
}

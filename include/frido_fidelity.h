/* The launches of the Inception Score and of the Kernel Inception Distance, the two metrics torch-fidelity computes beside FID from the
 * same Inception-v3 tower: row dot products in float64 (the tower's class logits, the polynomial-kernel Gram matrices of KID and their
 * sums), the finish of the MMD^2 estimate, and the four steps of the Inception Score.  SIX launchers beside the op table of frido_hip.h.
 *
 * A header of its own for the reason frido_fid.h has one: frido_hip.h is the op-kind ABI and these launches are no op kinds;
 * frido_amd/fidelity.py binds them from the same shared library, cross-checks each descriptor's size, and names a stale build if a
 * symbol is missing.  Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with
 * frido_last_error().  All sums are f64 in a written, fixed order; no atomics: a replay returns the same bits.  torch-fidelity is not
 * installed where this was written: the formulas below ARE the specification. */
#ifndef FRIDO_FIDELITY_H
#define FRIDO_FIDELITY_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups of one frido_rows_dot launch at the most; more tiles take further trips of the grid-stride loop */
#define FRIDO_ROWS_DOT_GRID_CAP 512

enum { FRIDO_ROWS_DOT_STORE_F32 = 0,        /* out f32: the dot rounded once */
       FRIDO_ROWS_DOT_STORE_F64 = 1,        /* out f64: the dot */
       FRIDO_ROWS_DOT_STORE_POLY_F64 = 2,   /* out f64: poly(dot) */
       FRIDO_ROWS_DOT_SUM_POLY = 3 };       /* nothing stored; partials[tile] = the sum of the tile's poly(dot) */

/* Row dot products.  Without index lists (ix == iy == NULL; S must be 1): pair (a, b), a < nx, b < ny, is X[a] . Y[b].  With lists
 * (both given): S subsets of m rows on either side, pair (a, b) of subset s, a, b < m, is X[ix[s * m + a]] . Y[iy[s * m + b]].  Below
 * RX, RY are the pair counts of one subset: (nx, ny) or (m, m).
 *   dot = fma((double)x[k], (double)y[k], dot) for k = 0 .. D - 1 in this order, from 0.0      (the product is exact in f64)
 *   poly(dot) = t^degree as ((t * t) * t) * t, t = dot * gamma + coef0; every multiply and add rounded on its own
 * STORE_*: out[(s * RX + a) * ldo + b].  SUM_POLY: the tiles of 64 x 64 pairs are numbered t = ti * ceil(RY / 64) + tj per subset
 * (symmetric: the tiles tj >= ti only, row by row of the upper triangle) and partials[s * T + t] is the tile's sum: per thread its
 * 4 x 4 pairs in (a, b) order from 0.0, the 64 lanes of a wave by the butterfly v += xor-shuffle(v, 32, 16, 8, 4, 2, 1), the four
 * waves as ((w0 + w1) + w2) + w3.  Pairs with a == b are left out with exclude_diag.  symmetric (SUM_POLY only; y == x, iy == ix):
 * the sums of the tiles tj > ti are doubled, which is exact.
 * The lists are read as they are: an index outside 0 .. nx - 1 (ny - 1) is taken as a row of zeros, never read. */
typedef struct FridoRowsDot {
    const float* x;          /* [nx][D] f32, 16-byte aligned */
    const float* y;          /* [ny][D] f32, 16-byte aligned */
    const int32_t* ix;       /* [S][m] or NULL */
    const int32_t* iy;       /* [S][m] or NULL */
    void* out;               /* STORE_*: [S * RX][ldo] f32 or f64 */
    double* partials;        /* SUM_POLY: [S * T] f64 */
    double gamma, coef0;     /* poly */
    int32_t nx, ny, D;       /* D % 4 == 0 */
    int32_t S, m;            /* with lists: S >= 1, m >= 1; without: S == 1, m == 0 */
    int32_t ldo;             /* STORE_*: >= RY */
    int32_t mode;            /* FRIDO_ROWS_DOT_* */
    int32_t degree;          /* poly: 1 .. 4 */
    int32_t exclude_diag;    /* SUM_POLY: 0 or 1 */
    int32_t symmetric;       /* SUM_POLY: 0 or 1 */
} FridoRowsDot;

/* Per subset s: sum_XX, sum_YY, sum_XY = the partials of the three Gram kinds added in tile order from 0.0, and
 *   mmd2 = (sum_XX + sum_YY) / ((double)m * (double)(m - 1)) - (2.0 * sum_XY) / ((double)m * (double)m)       every operation rounded on its own
 * out[s] = {sum_XX, sum_YY, sum_XY, mmd2}.  XX and YY are expected without their diagonals (exclude_diag). */
typedef struct FridoMmdFinish {
    const double* pxx;       /* [S][nxx] */
    const double* pyy;       /* [S][nyy] */
    const double* pxy;       /* [S][nxy] */
    double* out;             /* [S][4] f64 */
    int32_t S, m;            /* m >= 2 */
    int32_t nxx, nyy, nxy;   /* partials per subset of each kind */
} FridoMmdFinish;

/* Inception Score of logits [N][C].  Position p = 0 .. N - 1 stands for the row perm[p] (nothing is shuffled in memory; a value
 * outside 0 .. N - 1 is clamped into it); split i owns the positions i * N / splits .. (i + 1) * N / splits - 1 (integer division),
 * n_i of them.  With l = (double)logits[perm[p]][c]:
 *   frido_isc_rowstats   rowstats[p] = {m_p, ls_p}:  m_p = max_c l,  ls_p = log(sum_c exp(l - m_p))
 *   frido_isc_marginal   q[i][c] = (sum_p p_pc) / (double)n_i over the split's positions in order, from 0.0
 *   frido_isc_kl         kl[p] = sum_c p_pc * (logp_pc - log(q[i(p)][c]))
 *   frido_isc_finish     scores[i] = exp((sum_p kl[p]) / (double)n_i) over the split's positions in order, from 0.0
 * where logp_pc = (l - m_p) - ls_p and p_pc = exp(logp_pc) in both passes.  A sum over c is 64 lane partials (lane j adds c = j,
 * j + 64, ... ascending, from 0.0) joined by the butterfly v += xor-shuffle(v, 32, 16, 8, 4, 2, 1); one wave per position.
 * A term of kl whose p_pc is 0 (logp_pc below about -745, exp underflows) counts 0, its limit, so a q that underflows with it makes
 * no NaN.  The lane order above means 4-byte loads of the logits, a wave on 256 contiguous bytes per step: these kernels do not use the
 * 16-byte accesses of the other launches.  The four launchers take the same descriptor and run in the order above. */
typedef struct FridoIsc {
    const float* logits;     /* [N][C] f32 */
    const int32_t* perm;     /* [N] */
    double* rowstats;        /* [N][2] */
    double* q;               /* [splits][C] */
    double* kl;              /* [N] */
    double* scores;          /* [splits] */
    int32_t N, C, splits;    /* 1 <= splits <= N */
} FridoIsc;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_rows_dot(const FridoRowsDot* d, frido_stream_t s);
int frido_mmd_finish(const FridoMmdFinish* d, frido_stream_t s);
int frido_isc_rowstats(const FridoIsc* d, frido_stream_t s);
int frido_isc_marginal(const FridoIsc* d, frido_stream_t s);
int frido_isc_kl(const FridoIsc* d, frido_stream_t s);
int frido_isc_finish(const FridoIsc* d, frido_stream_t s);
int frido_sizeof_rows_dot(void);
int frido_sizeof_mmd_finish(void);
int frido_sizeof_isc(void);

#ifdef __cplusplus
}
#endif
#endif

/* The scans behind improved precision and recall (Kynkaanniemi et al. 2019; torch-fidelity's --prc) and density and coverage (Naeem et
 * al. 2020): row norms, the k-th nearest neighbour of every row and the ball-membership counts, all on SQUARED distances in float64,
 * formed on the fly from a slab of frido_rows_dot's float64 dot products (include/frido_fidelity.h, mode STORE_F64).  FOUR launchers
 * beside the op table of frido_hip.h.
 *
 * A header of its own for the reason frido_fidelity.h has one: frido_hip.h is the op-kind ABI and these launches are no op kinds;
 * frido_amd/manifold.py binds them from the same shared library, cross-checks each descriptor's size, and names a stale build if a
 * symbol is missing.  Same conventions as frido_hip.h: extern "C", DEVICE pointers, 0 on success or a negative FRIDO_E* code with
 * frido_last_error().  No atomics, every count an integer and every float64 value defined by value: a replay returns the same bits.
 * torch-fidelity, prdc and the ADM evaluator are not installed where this was written: the formulas below ARE the specification.
 *
 *   dot(x, y) = fma((double)x[j], (double)y[j], dot) for j = 0 .. D - 1 in this order, from 0.0      (frido_rows_dot's dot)
 *   n(x)      = dot(x, x), the same loop
 *   d2(x, y)  = fmax((n(x) + n(y)) - 2.0 * dot(x, y), 0.0)      every operation rounded on its own; 2.0 * dot is exact, so a contraction
 *               into an fma could not change a bit.  d2(x, x) == 0 exactly, d2 is bitwise symmetric, and the clamp is needed: rows that
 *               differ by an ulp in one coordinate give negative values before it.  No square root is taken anywhere.
 *   rad2_X[a] = the (k + 1)-th smallest value, counted WITH multiplicity, of { d2(X_a, X_b) : b = 0 .. n_X - 1 }: the row itself is in
 *               the set, so without duplicates this is the squared distance to the k-th nearest OTHER row (torch's kthvalue(k + 1)).
 *   With real rows R [N], generated rows G [M]:
 *   precision = #{ j : exists i, d2(G_j, R_i) <= rad2_R[i] } / M          recall   = #{ i : exists j, d2(G_j, R_i) <= rad2_G[j] } / N
 *   density   = (sum_j #{ i : d2(G_j, R_i) <= rad2_R[i] }) / (k M)        coverage = #{ i : min_j d2(G_j, R_i) <= rad2_R[i] } / N
 * The comparison is <=.
 *
 * A SLAB is [rows][ldo] float64: slab[a * ldo + b] = dot(row a of the slab's side, row b of the other side), b < ny; the columns
 * ny .. ldo - 1 are padding that no kernel here reads.  nrow[a] is n of slab row a, ncol[b] n of column b.  ldo is even and the slab
 * 16-byte aligned, so every slab row starts on 16 bytes. */
#ifndef FRIDO_MANIFOLD_H
#define FRIDO_MANIFOLD_H
#include "frido_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest neighbourhood k; frido_knn_select takes K = k + 1 <= FRIDO_MANIFOLD_MAX_K + 1 */
#define FRIDO_MANIFOLD_MAX_K 15
/* workgroups of one launch at the most; more work takes further trips of the grid-stride loop */
#define FRIDO_MANIFOLD_GRID_CAP 1024

/* out[a] = n(X_a): bit for bit the diagonal of frido_rows_dot(X, X, STORE_F64).  One thread per row, thread g = block * 256 + t takes
 * the rows g, g + grid * 256, ...; the row is read as D / 4 16-byte loads at x + a * D + 4 q, q ascending, and the four floats of a load
 * enter the one accumulator in their order. */
typedef struct FridoRowSqnorm {
    const float* x;          /* [n][D] f32, 16-byte aligned */
    double* out;             /* [n] f64 */
    int32_t n, D;            /* D % 4 == 0 */
} FridoRowSqnorm;

/* rad2[a] = the K-th smallest, with multiplicity, of { d2(a, b) : b < ny }, for every slab row a < rows.  One wave per row: wave
 * w = block * 4 + t / 64 takes the rows w, w + grid * 4, ...  K rounds; in each, lane l forms d2 for the column pairs
 * b = 2 l + 128 i, + 1 (one 16-byte load of the slab row and one of ncol per pair; the last column of an odd ny by 8-byte loads of
 * lane 0) and keeps the smallest pair (d2, b) that is lexicographically greater than the previous round's pair, the first round's
 * predecessor being (-1.0, -1); the 64 lanes' pairs are joined by a xor-shuffle butterfly of lexicographic minima.  The K-th round's
 * d2 is the result: ties are told apart by b, so equal values are counted as often as they occur.  The row is read K times. */
typedef struct FridoKnnSelect {
    const double* slab;      /* [rows][ldo] f64, 16-byte aligned */
    const double* nrow;      /* [rows] f64 */
    const double* ncol;      /* [ny] f64, 16-byte aligned */
    double* rad2;            /* [rows] f64 */
    int32_t rows, ny, ldo;   /* ldo >= ny, ldo % 2 == 0 */
    int32_t K;               /* 1 .. min(ny, FRIDO_MANIFOLD_MAX_K + 1) */
} FridoKnnSelect;

/* cnt[a] = #{ b < ny : d2(a, b) <= rad2_col[b] } for every slab row a.  One wave per row as above, the same column pairs per lane
 * (16-byte loads of the slab row, ncol and rad2_col), the lanes' int32 counts joined by v += xor-shuffle(v, 32, 16, 8, 4, 2, 1). */
typedef struct FridoBallRows {
    const double* slab;      /* [rows][ldo] f64, 16-byte aligned */
    const double* nrow;      /* [rows] f64 */
    const double* ncol;      /* [ny] f64, 16-byte aligned */
    const double* rad2_col;  /* [ny] f64, 16-byte aligned */
    int32_t* cnt;            /* [rows] i32 */
    int32_t rows, ny, ldo;   /* ldo >= ny, ldo % 2 == 0 */
} FridoBallRows;

/* cnt_col[b] += #{ a < rows : d2(a, b) <= rad2_row[a] } and dmin_col[b] = fmin(dmin_col[b], min_a d2(a, b)) for every column b < ny:
 * a plain read-modify-write, so the caller sets cnt_col = 0 and dmin_col = +inf before the first slab and launches the slabs in stream
 * order.  A workgroup takes the 32 columns b = 32 c + t % 32 of column tile c = block, block + grid, ...; its half-wave h = t / 32
 * walks the slab rows a = h, h + 8, ... (32 lanes on 256 contiguous bytes of a slab row), and the eight half-waves' counts and minima
 * of a column are joined through LDS by ONE thread, which alone touches cnt_col[b] and dmin_col[b] in the launch.  Sums of integers
 * and minima: the order does not matter. */
typedef struct FridoBallCols {
    const double* slab;      /* [rows][ldo] f64, 8-byte aligned */
    const double* nrow;      /* [rows] f64 */
    const double* ncol;      /* [ny] f64 */
    const double* rad2_row;  /* [rows] f64 */
    int32_t* cnt_col;        /* [ny] i32, read and written */
    double* dmin_col;        /* [ny] f64, read and written */
    int32_t rows, ny, ldo;   /* ldo >= ny */
} FridoBallCols;

/* bad arguments return FRIDO_EINVAL before any device is touched */
int frido_row_sqnorm(const FridoRowSqnorm* d, frido_stream_t s);
int frido_knn_select(const FridoKnnSelect* d, frido_stream_t s);
int frido_ball_rows(const FridoBallRows* d, frido_stream_t s);
int frido_ball_cols(const FridoBallCols* d, frido_stream_t s);
int frido_sizeof_row_sqnorm(void);
int frido_sizeof_knn_select(void);
int frido_sizeof_ball_rows(void);
int frido_sizeof_ball_cols(void);

#ifdef __cplusplus
}
#endif
#endif

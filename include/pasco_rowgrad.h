/*
 * pasco_rowgrad.h -- flat C ABI of the training kernels of the dense <-> rows operators and of local max pooling in
 * libpascohip.so (pasco_amd/csrc/rowgrad.hip).
 *
 * The forward operators are in include/pasco_hip.h: ph_to_dense (rows -> dense grid), ph_dense_gather (dense grid -> rows; the
 * second half of to_sparse) and ph_maxpool_fwd.  Each of them copies or selects values, so its adjoint copies gradients:
 *
 *   SparseTensor.dense():  d_feats[i]   = g[b_i, :, site(i)]                      pr_dense_rows
 *   to_sparse():           d_dense      = zeros, then d_dense[b_i, :, site_i] = g[i]   pr_rows_dense
 *   max pooling:           dx[i][c]     = sum_k [o = inv[k][i] >= 0] dy[o][c] [arg[o][c] == i]    pr_maxpool_arg, pr_maxpool_bwd
 *
 * The host restatement is pasco_amd/grad/host.py.  A separate surface from include/pasco_hip.h and include/pasco_grad.h: own
 * prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_grad.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pr_last_error().  Matrices are row-major fp32, a dense
 * grid is fp32 [B, C, X, Y, Z] (z fastest), coordinates are int32 [n, 4] = (b, x, y, z).
 *
 * Determinism: no floating-point atomics anywhere.  The dense <-> rows kernels are copies; the one sum (pr_maxpool_bwd) has one
 * fixed order, so a call repeated on the same inputs returns the same bits.
 */
#ifndef PASCO_ROWGRAD_H_
#define PASCO_ROWGRAD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PR_FN(name) pr_##name

#define PR_ABI_VERSION 1
#define PR_MAX_KVOL 64                       /* offsets of one pooling window */
#define PR_TILE 64                           /* pr_dense_rows / pr_rows_dense: rows and channels per workgroup */

int PR_FN(abi_version)(void);
const char *PR_FN(last_error)(void);

/* The adjoint of ph_to_dense: dense fp32 [B, c, X, Y, Z], coords int32 [n, 4] -> rows fp32 [n, c] (overwritten),
 *   rows[i] = dense[b_i, :, site(i)]
 * with site(i) by ph_to_dense's rule: per axis floor((coord - min) / ts); an index in [-dim, 0) wraps (+ dim); a row that is
 * still outside [0, dim) on an axis, or whose batch index is outside [0, B), is SKIPPED by the forward and gets a ZERO row here.
 * Several rows on one site (only a wrap produces them) EACH receive that site's values: the forward keeps one of them, in no
 * stated order, and this is the gradient torch's autograd gives for index_put_ (every writer is treated as the one that stayed).
 * ts >= 1; B, X, Y, Z >= 0; any c >= 1; n == 0 is a no-op. */
int PR_FN(dense_rows)(const float *dense, int32_t c, int32_t B, int32_t X, int32_t Y, int32_t Z, const int32_t *coords,
                      int64_t n, int32_t min_x, int32_t min_y, int32_t min_z, int32_t ts, float *rows, void *stream);

/* The adjoint of ph_dense_gather: rows fp32 [n, c], site_coords int32 [n, 4] (site units: no minimum, no stride, no wrap) ->
 * dense fp32 [B, c, X, Y, Z], OVERWRITTEN: one fill with zeros, then one launch that stores
 *   dense[b_i, :, x_i, y_i, z_i] = rows[i]
 * A row with any index outside its range is skipped (ph_dense_gather reads it as zeros).
 * PRECONDITION: the in-range sites are distinct (to_sparse lists every site once), so the plain stores do not race; a table
 * that breaks it leaves, per element, one of the candidate rows.  n == 0 writes zeros. */
int PR_FN(rows_dense)(const float *rows, int64_t n, int32_t c, const int32_t *site_coords, int32_t B, int32_t X, int32_t Y,
                      int32_t Z, float *dense, void *stream);

/* in fp32 [n_in, c], nbr int32 [K, n_out] (-1 = none), out fp32 [n_out, c] = ph_maxpool_fwd(in, nbr) -> arg int32 [n_out, c]:
 * the input row nbr[k][o] of the FIRST offset, in ascending k, whose value compares equal (==, so +0 and -0 tie) to out[o][ch];
 * -1 where the window is empty or nothing compares equal (a NaN maximum).  Entries of nbr outside [0, n_in) count as absent.
 * 1 <= K <= PR_MAX_KVOL; n_out == 0 is a no-op. */
int PR_FN(maxpool_arg)(const float *in, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out,
                       const float *out, int32_t *arg, void *stream);

/* dy fp32 [n_out, c], arg int32 [n_out, c] (pr_maxpool_arg), inv int32 [K, n_in] (pg_nbr_invert of the pooling table, with its
 * precondition) -> dx fp32 [n_in, c], OVERWRITTEN:
 *   dx[i][ch] = sum over k ascending with o = inv[k][i] in [0, n_out) of dy[o][ch] * [arg[o][ch] == i]
 * One thread per (i, ch); the terms are added in ascending k starting from +0.  kernel == stride: one term at the most;
 * stride-1 windows: up to K.  1 <= K <= PR_MAX_KVOL; n_in == 0 is a no-op; n_out == 0 writes zeros. */
int PR_FN(maxpool_bwd)(const float *dy, int64_t n_out, int32_t c, const int32_t *arg, const int32_t *inv, int32_t K,
                       int64_t n_in, float *dx, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_ROWGRAD_H_ */

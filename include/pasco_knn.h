/*
 * pasco_knn.h -- flat C ABI of the bipartite k-nearest-neighbour up-sampling of libpascohip.so (pasco_amd/csrc/knn.hip): what
 * a point-cloud segmenter's `knn_up` needs to carry the rows of a voxel map back to the points.
 *
 *   search:   idx[j][p], d2[j][p] = the j-th nearest candidate of query p, nearest first                          pk_knn
 *   weights:  w[j][p] = (1 / (d2[j][p] + 1e-8)) / the sum of those reciprocals over the present entries           pk_weights
 *   forward:  out[p] = sum_j w[j][p] * x[idx[j][p]]                                                               pk_interp_fwd
 *   backward: no kernel of its own.  The [k, m] index table flattened is a list of k * m entries keyed by candidate row:
 *             pq_group (include/pasco_field.h) with n_seg = n, then pq_seg_rows with w = the weights, src_mod = m, PQ_SUM; the
 *             terms of a candidate row are added in ascending (j, p).  That inherits pq_group's k * m < 2^24.
 *
 * Conventions (as pasco_field.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pk_last_error().  Feature matrices are row-major
 * fp32; tables are laid out [k, m] (entry j of query p at j * m + p), indices int32 with -1 = absent.  All fp32 arithmetic is
 * compiled with FP contraction off (a * b + c is two roundings) and there is no floating-point atomic: every sum has one fixed
 * order, so a call repeated on the same inputs returns the same bits.  The host restatement is pasco_amd/grad/host.py
 * (knn_search, knn_weights, knn_interp).  A separate surface from the other headers: own prefix, own version, no CPU oracle.
 *
 * Ordering rule of pk_knn (that of pasco_waffle.h): d2 = (dx*dx + dy*dy) + dz*dz in fp32 with d* = candidate - query in fp32; a
 * smaller d2 is nearer, equal d2 goes to the lower candidate index.  The result is exact under that rule (not approximate).
 *
 * The search structure is pasco_waffle.h's: a uniform grid of cubic cells of edge `h` with origin `lo` and `g` cells per axis
 * (fp64 geometry: cell of p = floor(((double)p - lo) / h) per axis, cell index (cz*gy + cy)*gx + cx), and the CSR of the
 * candidates by cell, `start` int32 [ncell + 1] and `order` int32 [n]: the candidates of cell c are order[start[c] ..
 * start[c + 1]) in ascending index - pw_grid_cells, then pq_group(cell, ncell), whose offsets / perm are start / order.  Every
 * candidate must be finite and lie in the grid; a query may lie anywhere, its home cell is clamped into the grid.  A search
 * visits the shells of cells at Chebyshev distance r = 0, 1, ... from the home cell.  Before shell r it stops when the list is
 * full and its worst d2 is below (1 - 2^-20) * L(r), where L(r) is a lower bound in fp64 of the squared distance of every
 * candidate in shell r or beyond: the minimum over the six directions that still have cells of (gap to that slab)^2 plus, for
 * the other axes, the squared distance of the query to the grid's extent.  (The fp32 d2 of a candidate is within 5 * 2^-24
 * relative of its exact squared distance, far inside the 2^-20 margin, so no candidate beyond the bound can order before the
 * list's worst.)  r never exceeds max(g): every loop is bounded by the grid's extent, none by "until found".
 *
 * A-priori error bounds, u = 2^-24, gamma(t) = t u / (1 - t u), all inputs taken as exact:
 *   d2           every term is non-negative: |d2 - exact| <= gamma(5) * exact.
 *   pk_weights   a_j = d2_j + e (e = the fp32 nearest 1e-8), r_j = 1 / a_j and the final quotient are one rounding each, the
 *                norm of q present entries is q - 1 additions of positive terms (2 roundings in r_j, q + 1 in the norm, one in
 *                the quotient):  |w_j - exact_j| <= gamma(q + 4) * exact_j  with exact_j formed from the given fp32 d2 and e.
 *   pk_interp_fwd  one rounded product per term and q - 1 additions (the first term is added to +0 exactly):
 *                |out[p][ch] - exact| <= gamma(q) * sum_j |w_j * x[idx_j][ch]|  for the given fp32 w and x.
 *   the backward   pq_seg_rows' bound (pasco_field.h) over the segment of a candidate row.
 */
#ifndef PASCO_KNN_H_
#define PASCO_KNN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_FN(name) pk_##name

#define PK_ABI_VERSION 1
#define PK_MAX_K 16                 /* neighbours per query */
#define PK_QUERY_BLOCK 64           /* queries of one workgroup of pk_knn: one wave, one query per lane */
#define PK_MAX_CELLS (1 << 24)      /* cells of the search grid (PW_MAX_CELLS) */

int PK_FN(abi_version)(void);
const char *PK_FN(last_error)(void);

/* cand fp32 [n, ldc] and q fp32 [m, ldq] (columns 0..2 = x, y, z; ldc, ldq >= 3; a base on any 4-byte boundary, such as column 1
 * of a [N, 4] batched-coordinate matrix), the CSR (start, order) of the candidates over the grid (lo, h, g) ->
 * idx int32 [k, m], d2 fp32 [k, m], OVERWRITTEN: the k nearest candidates of every query under the ordering rule, nearest first.
 * With fewer than k candidates the missing entries are idx = -1, d2 = +inf (ours).  A query with a non-finite coordinate has
 * all k entries absent (ours).  (A d2 that overflows to +inf belongs to a present candidate: its idx is >= 0.)
 * Served: 1 <= k <= PK_MAX_K, 0 <= n < 2^31, 0 <= m < 2^31 / k, h > 0, gx, gy, gz >= 1 with gx * gy * gz <= PK_MAX_CELLS;
 * m == 0 is a no-op, n == 0 writes all entries absent. */
int PK_FN(knn)(const float *cand, int32_t ldc, int64_t n, const int32_t *start, const int32_t *order, double lox, double loy,
               double loz, double h, int32_t gx, int32_t gy, int32_t gz, const float *q, int32_t ldq, int64_t m, int32_t k,
               int32_t *idx, float *d2, void *stream);

/* d2 fp32 [k, m], idx int32 [k, m] (pk_knn) -> w fp32 [k, m], OVERWRITTEN.  Over the present entries (idx >= 0) in ascending j:
 *   r_j = 1.0f / (d2_j + 1e-8f),  norm = ((r_0 + r_1) + ...),  w_j = r_j / norm
 * An absent entry has weight 0.  norm == 0 or a non-finite norm gives zero weights for the query (ours).
 * Served: 1 <= k <= PK_MAX_K, 0 <= m < 2^31 / k; m == 0 is a no-op. */
int PK_FN(weights)(const float *d2, const int32_t *idx, int32_t k, int64_t m, float *w, void *stream);

/* x fp32 [n, c], idx int32 [k, m], w fp32 [k, m] -> out fp32 [m, c], OVERWRITTEN:
 *   out[p] = the sum over the entries j with idx[j][p] in [0, n), in ascending j from +0, of w[j][p] * x[idx[j][p]]
 * each product rounded before it is added.  A query without a present entry gets a zero row.  Rows move in 16-byte pieces where
 * c % 4 == 0 and x and out are 16-byte aligned, one channel at a time otherwise; the operations per channel are the same.
 * Served: c >= 1, 1 <= k <= PK_MAX_K, 0 <= n < 2^31, 0 <= m < 2^31 / k; m == 0 is a no-op. */
int PK_FN(interp_fwd)(const float *x, int64_t n, int32_t c, const int32_t *idx, const float *w, int32_t k, int64_t m, float *out,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_KNN_H_ */

/*
 * pasco_waffle.h -- flat C ABI of the point-feature kernels in libpascohip.so (pasco_amd/csrc/waffle.hip).
 *
 * The WaffleIron point network (48 layers of a 2-D projection token mixer and a channel MLP over the 60-100 k tokens of a
 * voxelised scan) needs, around its tall [N, C] x [C, C] products - which run on the existing ph_conv_fwd route - the
 * neighbour searches, the point <-> 2-D grid projections, a depthwise 3 x 3 convolution and the neighbourhood embedding.
 * These entry points are those pieces.  The host restatement is pasco_amd/waffle/host.py: every integer equal, every float
 * the same sequence of fp32 operations.  A separate surface from include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_view.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pw_last_error().  Tokens are row-major [N, C] fp32.
 * `d_status` is one int32 the caller zeroes; kernels OR PW_STATUS_* bits into it instead of reading or writing out of bounds.
 * All fp32 arithmetic is compiled with FP contraction off: a * b + c is two roundings.
 *
 * A CSR of points by cell is `start` int32 [ncell + 1] and `order` int32 [N]: the points of cell c are
 * order[start[c] .. start[c + 1]), in ascending point index.
 *
 * Ordering rule of pw_knn and pw_nearest: d2 = (dx*dx + dy*dy) + dz*dz in fp32 with d* = point - query in fp32; a smaller d2
 * is nearer, equal d2 goes to the lower point index.  The result is exact under that rule (not approximate).
 *
 * The search structure is a uniform grid of cubic cells of edge `h` with origin `lo` and `G` cells per axis (fp64 geometry:
 * cell of p = floor(((double)p - lo) / h) per axis, cell index (cz*G[1] + cy)*G[0] + cx, x fastest).  Every point must lie
 * in the grid (pw_grid_cells refuses one that does not); a query may lie anywhere, its home cell is clamped into the grid.
 * A search visits the shells of cells at Chebyshev distance r = 0, 1, ... from the home cell.  Before shell r it stops when
 * the list is full and its worst d2 is below (1 - 2^-20) * L(r), where L(r) is a lower bound in fp64 of the squared distance
 * of every point in shell r or beyond: the minimum over the six directions that still have cells of (gap to that slab)^2
 * plus, for the other axes, the squared distance of the query to the grid's extent.  r never exceeds max(G): every loop is
 * bounded by the grid's extent, none by "until found".
 */
#ifndef PASCO_WAFFLE_H_
#define PASCO_WAFFLE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PW_FN(name) pw_##name

#define PW_ABI_VERSION 1
#define PW_MAX_K 32          /* pw_knn: neighbours per point */
#define PW_MAX_FEAT 8        /* pw_neigh_rows: input features per point */
#define PW_MAX_CELLS (1 << 24) /* cells of any CSR */

#define PW_STATUS_OFF_GRID 1     /* pw_cell_index / pw_grid_cells: a point outside the grid (its cell is written as 0) */
#define PW_STATUS_ORDER 2        /* pw_cells_build: `order` is no permutation sorted by (cell, index), or a cell out of range */
#define PW_STATUS_INDEX 4        /* pw_inflate / pw_neigh_rows / pw_flatten: an index out of range (that term is skipped) */
#define PW_STATUS_KEY_RANGE 8    /* pw_voxel_keys: a key outside [0, 2^21) (written as 0) */

int PW_FN(abi_version)(void);
const char *PW_FN(last_error)(void);

/* pc fp32 [n, ld] (columns 0..2 = x, y, z), mn fp32 [3] on the device (the per-column minimum), voxel > 0 ->
 * key int32 [n, 3] = (int)((pc - mn) / (float)voxel): one fp32 subtraction, one correctly rounded fp32 division, truncation.
 * The first point of every distinct key in lexicographic key order is the voxelised cloud. */
int PW_FN(voxel_keys)(const float *pc, int32_t ld, int64_t n, const float *mn, float voxel, int32_t *key, int32_t *d_status,
                      void *stream);

/* Cell of every point on one 2-D grid [H, W]: q_a = (int)(((double)pc[p, d_a] - lo_a) / res_a) (truncation), a = 0, 1;
 * cell = q_0 * W + q_1.  A q_a outside its range ORs PW_STATUS_OFF_GRID: the caller refuses the scan, nothing is clamped. */
int PW_FN(cell_index)(const float *pc, int32_t ld, int64_t n, int32_t d0, int32_t d1, double lo0, double lo1, double res0,
                      double res1, int32_t H, int32_t W, int32_t *cell, int32_t *d_status, void *stream);

/* Search cell of every point (see the top of this file); a point outside the grid ORs PW_STATUS_OFF_GRID. */
int PW_FN(grid_cells)(const float *xyz, int32_t ld, int64_t n, double lox, double loy, double loz, double h, int32_t gx,
                      int32_t gy, int32_t gz, int32_t *cell, int32_t *d_status, void *stream);

/* cell int32 [n] with values in [0, ncell), order int32 [n] = the permutation that sorts points by (cell, index) (a stable
 * sort of `cell`; the caller's plumbing) -> start int32 [ncell + 1] by one binary search per cell.  Every entry of `order`
 * is checked against its predecessor; a violation ORs PW_STATUS_ORDER.  n = 0 writes zeros. */
int PW_FN(cells_build)(const int32_t *cell, const int32_t *order, int64_t n, int32_t ncell, int32_t *start,
                       int32_t *d_status, void *stream);

/* out int32 [n, k]: the k nearest OTHER points of every point (index != the point's own), nearest first.  1 <= k <= PW_MAX_K,
 * k < n.  (start, order) is the CSR of the points by search cell. */
int PW_FN(knn)(const float *xyz, int32_t ld, int64_t n, const int32_t *start, const int32_t *order, double lox, double loy,
               double loz, double h, int32_t gx, int32_t gy, int32_t gz, int32_t k, int32_t *out, void *stream);

/* out int32 [m]: the nearest point of every query q fp32 [m, ldq] (anywhere in space).  n >= 1. */
int PW_FN(nearest)(const float *xyz, int32_t ld, int64_t n, const int32_t *start, const int32_t *order, double lox,
                   double loy, double loz, double h, int32_t gx, int32_t gy, int32_t gz, const float *q, int32_t ldq,
                   int64_t m, int32_t *out, void *stream);

/* tokens [n, C], scale / shift [C], CSR of one 2-D grid -> grid fp32 [ncell, C] (channels last):
 *   grid[c] = ((0 + t_0) + t_1 + ...) * (1.0f / ((float)count + 1e-6f)),  t_i = tokens[order[start[c] + i]] * scale + shift
 * and 0 for an empty cell.  One thread owns one (cell, channel) sum: no atomics, one fixed order. */
int PW_FN(flatten)(const float *tokens, int64_t n, int32_t C, const float *scale, const float *shift, const int32_t *start,
                   const int32_t *order, int32_t ncell, float *grid, int32_t *d_status, void *stream);

/* in fp32 [H, W, C] -> out fp32 [H, W, C] (may not alias in): depthwise 3 x 3, zero padding, w fp32 [9, C] with tap
 * t = (dy + 1) * 3 + (dx + 1) reading in[y + dy, x + dx], bias fp32 [C]:
 *   out = (((0 + w_0 * v_0) + w_1 * v_1) + ... + w_8 * v_8) + bias, taps outside the grid skipped, then max(out, 0) if relu. */
int PW_FN(dwconv3x3)(const float *in, int32_t H, int32_t W, int32_t C, const float *w, const float *bias, int32_t relu,
                     float *out, void *stream);

/* out[p, c] = tokens[p, c] + scale[c] * grid[cell[p], c]; out may be tokens.  A cell out of range ORs PW_STATUS_INDEX and
 * leaves out[p] = tokens[p]. */
int PW_FN(inflate)(const float *tokens, int64_t n, int32_t C, const float *scale, const float *grid, const int32_t *cell,
                   int32_t ncell, float *out, int32_t *d_status, void *stream);

/* Neighbourhood rows of the points p0 .. p0 + np - 1: feat fp32 [n, F] (F <= PW_MAX_FEAT), knn int32 [n, k], A fp32 [F, C],
 * b fp32 [C] -> rows fp32 [np * k, C]:
 *   rows[(p - p0) * k + j, c] = max(0, ((b[c] + A[0, c] * d_0) + A[1, c] * d_1) + ...),  d_f = feat[knn[p, j], f] - feat[p, f]
 * A neighbour index outside [0, n) ORs PW_STATUS_INDEX and counts as the point itself (d = 0). */
int PW_FN(neigh_rows)(const float *feat, int64_t n, int32_t F, const int32_t *knn, int32_t k, int64_t p0, int64_t np,
                      const float *A, const float *b, int32_t C, float *rows, int32_t *d_status, void *stream);

/* rows fp32 [np * k, C] -> out[p * ld_out + c] = max over j < k of rows[p * k + j, c] (ld_out >= C: a column slice of a wider
 * matrix can be the target).  Values must not be NaN. */
int PW_FN(group_max)(const float *rows, int64_t np, int32_t k, int32_t C, float *out, int32_t ld_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_WAFFLE_H_ */

/*
 * pasco_field.h -- flat C ABI of the point <-> voxel operators of libpascohip.so (pasco_amd/csrc/field.hip): what
 * MinkowskiEngine's TensorField, quantisation modes, SparseTensor.slice and MinkowskiInterpolation need.
 *
 *   grouping:        offsets, perm = the stable sort of the list entries by key (segment)                       pq_group
 *   segment rows:    out[s] = sum | average | maximum over the members j of segment s of (w_j *) x[j % src_mod]  pq_seg_rows
 *                    dx[arg[s][ch] % src_mod][ch] = dy[s][ch]                                                    pq_seg_max_bwd
 *   weighted gather: out[i] = x[idx[i]] * (1 / d[idx[i]])                                                        pq_gather_w
 *   interpolation:   rows[k][p], weights[k][p] of the eight corners of point p                                   pq_interp_map
 *                    out[p] = sum_k weights[k][p] * x[rows[k][p]]                                                pq_interp_fwd
 *
 * How the operators are composed (pasco_amd/me):
 *   TensorField.sparse()  sum / average / max:  pq_group over the point -> voxel map, then pq_seg_rows; the backward of the
 *                         average is pq_gather_w with the counts, of the sum the plain row gather (ph_gather_rows), of the
 *                         maximum pq_seg_max_bwd;
 *   SparseTensor.slice()  the plain row gather; its backward is pq_seg_rows (sum) over the same grouping;
 *   interpolation         pq_interp_map and pq_interp_fwd on every forward call; its backward is pq_group over the flattened
 *                         [8 * M] table with n_seg = n_in, then pq_seg_rows with w = weights and src_mod = M: the terms of an
 *                         input row are added in ascending (k, p).  Neither the map nor that grouping is cached: both are
 *                         recomputed on every call.
 *
 * The definitions are the ones MinkowskiEngine 0.5.4's documentation states; where it is silent the edge rule is this
 * library's and the entry says "(ours)".  The host restatement is pasco_amd/grad/host.py (field_*).  A separate surface from the
 * other headers: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_pool.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pq_last_error().  Matrices are row-major fp32, tables
 * are int32 with -1 = absent.
 *
 * Determinism: no floating-point atomics anywhere.  Every sum has one fixed order that depends on the shapes and the tables
 * alone, so a call repeated on the same inputs returns the same bits:
 *   - pq_seg_rows: one partial per PQ_SEG_ROWS consecutive members of a segment's list, added in list order from +0 inside the
 *     partial; then the partials in ascending order, starting from the first.  (The rule leaves room to spread one very long
 *     segment over several workgroups without changing a bit; today one thread walks a segment's partials.)
 *   - pq_interp_fwd: the present corners in ascending k, starting from +0.
 * Products are rounded before they are added (no fused multiply-add).  The grouping uses integer atomics only (digit counts,
 * whose result does not depend on their order).
 */
#ifndef PASCO_FIELD_H_
#define PASCO_FIELD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PQ_FN(name) pq_##name

#define PQ_ABI_VERSION 1
#define PQ_SEG_ROWS 64                       /* consecutive members of one partial sum */
#define PQ_CORNERS 8                         /* corners of one interpolation cell */

#define PQ_SUM 0                             /* pq_seg_rows */
#define PQ_AVG 1
#define PQ_MAX 2

int PQ_FN(abi_version)(void);
const char *PQ_FN(last_error)(void);

/* Bytes of workspace pq_group needs for n keys in n_seg segments, -1 outside the served range. */
int64_t PQ_FN(group_workspace_bytes)(int64_t n, int64_t n_seg);

/* keys int32 [n], each in [0, n_seg) or ABSENT (negative or >= n_seg) -> offsets int32 [n_seg + 1], perm int32 [n], both
 * OVERWRITTEN:
 *   perm[offsets[s] .. offsets[s + 1]) = the indices i with keys[i] == s, in ascending i   (a stable sort by key)
 *   offsets[n_seg] = the number of present keys; the tail of perm (the absent entries) is unspecified.
 * Served: 0 <= n < 2^24, 0 <= n_seg < 2^31; n == 0 writes zero offsets.  The workspace is 16-byte aligned. */
int PQ_FN(group)(const int32_t *keys, int64_t n, int64_t n_seg, int32_t *offsets, int32_t *perm, void *workspace,
                 int64_t workspace_bytes, void *stream);

/* x fp32 [n_src, c], offsets int32 [n_seg + 1] and perm int32 [n_list] (pq_group), w fp32 [n_list] or null, src_mod >= 1 ->
 * out fp32 [n_seg, c], cnt fp32 [n_seg] (may be null), and for PQ_MAX arg int32 [n_seg, c]; all OVERWRITTEN.
 * The members of segment s are the list entries j = perm[offsets[s]], ..., perm[offsets[s + 1] - 1] in this (list) order;
 * member j reads the source row j % src_mod and, where w is given, the weight w[j].  With src_mod >= n_list the row is j
 * itself; the backward of the interpolation passes src_mod = M for its [8, M] table.
 *   PQ_SUM: out[s] = the sum over the members of (w[j] *) x[j % src_mod], in the order stated at the top of this file
 *   PQ_AVG: that sum / cnt[s] where cnt[s] > 0 (the division is the last operation)
 *   PQ_MAX: out[s][ch] = the maximum of the members' values (w must be null); a NaN among them makes it NaN.  arg[s][ch] = the
 *           FIRST member j, in list order, whose value compares equal (==, so +0 and -0 tie and the first one's bits are the
 *           result) to the maximum; -1 for an empty segment or a NaN maximum (the rule of pp_seg_reduce).
 * cnt[s] = offsets[s + 1] - offsets[s].  An empty segment gives a zero row and count 0 (ours).  A member outside [0, n_list)
 * or whose row is outside [0, n_src) contributes nothing (ours; pq_group never produces one).
 * Served: c >= 1, 0 <= n_src, n_seg < 2^31, 0 <= n_list < 2^24 (the count is exact in fp32); n_seg == 0 is a no-op. */
int PQ_FN(seg_rows)(const float *x, int64_t n_src, int32_t c, const int32_t *offsets, const int32_t *perm, int64_t n_list,
                    int64_t n_seg, const float *w, int64_t src_mod, int32_t mode, float *out, float *cnt, int32_t *arg,
                    void *stream);

/* dy fp32 [n_seg, c], arg int32 [n_seg, c] (pq_seg_rows, PQ_MAX) -> dx fp32 [n_src, c], OVERWRITTEN: one fill with zeros, then
 *   dx[arg[s][ch] % src_mod][ch] = dy[s][ch]   for arg[s][ch] >= 0 with its row in [0, n_src)
 * The members of different segments are different list entries; with src_mod >= n_list every store goes to its own element.
 * n_src == 0 is a no-op. */
int PQ_FN(seg_max_bwd)(const float *dy, const int32_t *arg, int64_t n_seg, int32_t c, int64_t n_src, int64_t src_mod, float *dx,
                       void *stream);

/* x fp32 [n_src, c], idx int32 [n], d fp32 [n_src] -> out fp32 [n, c], OVERWRITTEN:
 *   out[i] = x[idx[i]] * (1 / d[idx[i]])      (the reciprocal is rounded, then the product)
 * d[idx[i]] == 0 or an index outside [0, n_src) gives a zero row.  The backward of the average:
 * dF_point[p] = dy[voxel(p)] / cnt[voxel(p)].
 * Served: c >= 1, 0 <= n, n_src < 2^31; n == 0 is a no-op. */
int PQ_FN(gather_w)(const float *x, int64_t n_src, int32_t c, const int32_t *idx, int64_t n, const float *d, float *out,
                    void *stream);

/* points fp32 [m, 4] = (b, x, y, z), the hash table of a coordinate map (tkeys uint64 [cap], tvals int32 [cap], cap a power of
 * two, as ph_map_find takes them), the map's tensor stride ts >= 1 -> rows int32 [8, m], weights fp32 [8, m], OVERWRITTEN.
 * Corner k = 4 * ox + 2 * oy + oz with o_d in {0, 1}; in fp32, per axis d:
 *   lower_d = floor(x_d / ts) * ts,  corner_d = lower_d + o_d * ts,  f_d = 1 - |x_d - corner_d| / ts
 *   (any ts >= 1: lower_d <= x_d < lower_d + ts holds whatever the stride, so every f_d lies in [0, 1]; a correctly rounded
 *   division never carries x_d / ts onto the next integer, a quotient formed with a reciprocal would, and lower_d is moved
 *   back by one stride where that is seen)
 *   evaluated as the distance to the opposite corner, (lower_d + ts - x_d) / ts for o_d = 0 and (x_d - lower_d) / ts for
 *   o_d = 1: one subtraction and one division, nothing cancels, so a small weight keeps its relative accuracy
 *   weights[k][p] = (f_x * f_y) * f_z
 *   rows[k][p]    = the map's row of (int(floor(b)), corner), or -1
 * The weights are NOT renormalised over the corners that exist (ME's rule).  A corner whose weight is exactly 0 is listed as
 * absent, row -1 (ours: an Inf feature on a corner the point does not touch must not make a NaN).  A point with a non-finite
 * coordinate or batch index, a batch index outside [0, 1024) or a coordinate with |x_d| >= 2^18 has all eight corners absent and
 * zero weights (ours); a corner the map's keys cannot hold (outside -2^17 .. 2^17 - 1) is absent.
 * Served: 0 <= m < 2^28, 1 <= ts <= 2^16; m == 0 is a no-op. */
int PQ_FN(interp_map)(const float *points, int64_t m, const uint64_t *tkeys, const int32_t *tvals, int64_t cap, int32_t ts,
                      int32_t *rows, float *weights, void *stream);

/* x fp32 [n_in, c], rows int32 [8, m], weights fp32 [8, m] (pq_interp_map) -> out fp32 [m, c], OVERWRITTEN:
 *   out[p] = the sum over the corners k with rows[k][p] in [0, n_in), in ascending k from +0, of weights[k][p] * x[rows[k][p]]
 * A point without a present corner gets a zero row.
 * Served: c >= 1, 0 <= m < 2^28, 0 <= n_in < 2^31; m == 0 is a no-op. */
int PQ_FN(interp_fwd)(const float *x, int64_t n_in, int32_t c, const int32_t *rows, const float *weights, int64_t m, float *out,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_FIELD_H_ */

/*
 * pasco_pool.h -- flat C ABI of the pooling, broadcast and channel-wise operators of libpascohip.so
 * (pasco_amd/csrc/pool.hip): MinkowskiEngine's global pooling, broadcast, local sum / average pooling, pooling transpose and
 * channel-wise convolution, each with its backward.
 *
 *   per-batch reductions:   sum[b] = sum_{i: b_i = b} x[i],  avg[b] = sum[b] / count[b],  max[b] with arg[b][ch]   pp_seg_reduce
 *                           dx[arg[b][ch]][ch] = dy[b][ch]                                                        pp_seg_max_bwd
 *   broadcast:              out[i] = x[i] + g[b_i] | x[i] * g[b_i] | cat(x[i], g[b_i]) | g[b_i]                   pp_broadcast
 *                           dx[i] = dy[i] * g[b_i],  dg[b] = sum_{i: b_i = b} dy[i] * x[i]                        pp_broadcast_mul_bwd
 *   local pooling:          sum[o] = sum_k x[nbr[k][o]],  avg[o] = sum[o] / cnt[o]                                pp_pool
 *                           dx[i] = sum_k dy[inv[k][i]] (/ cnt[inv[k][i]])                                        pp_pool_bwd
 *   channel-wise conv:      out[o][ch] = sum_k x[nbr[k][o]][ch] * W[k][ch] (+ b[ch])                              pp_chconv_fwd
 *                           dW[k][ch] = sum_o x[nbr[k][o]][ch] * dy[o][ch]                                        pp_chconv_wgrad
 *
 * The definitions are the ones MinkowskiEngine 0.5.4's documentation states; where it is silent the edge rule is this
 * library's and the entry says "(ours)".  The backward of the broadcast add / cat / copy is pp_seg_reduce (sum) on dy or on a
 * column slice of it (`ldx`); the input gradient of the channel-wise convolution is pp_chconv_fwd over pg_nbr_invert's table
 * with the same weights (a diagonal: nothing is transposed), its bias gradient is pg_colsum.
 *
 * Pooling transpose (MinkowskiPoolingTranspose, kernel 2 / stride 2 onto the expanded map) needs NO entry here: at
 * kernel == stride every child has exactly one parent, so ME's division by the number of contributors is a division by one and
 * out[child] = x[parent], the row gather of include/pasco_hip.h (ph_gather_rows); its backward is pp_pool (sum) over the
 * inverse of the same table.
 *
 * The host restatement is pasco_amd/grad/host.py (pool_*).  A separate surface from the other headers: own prefix, own version,
 * no CPU oracle.
 *
 * Conventions (as pasco_rowgrad.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pp_last_error().  Matrices are row-major fp32,
 * coordinates are int32 [n, 4] = (b, x, y, z), neighbour tables are int32 [K, n_out] with -1 = absent; entries outside
 * [0, n_in) count as absent.
 *
 * Determinism: no floating-point atomics anywhere.  Every sum has one fixed order that depends on the shapes alone, so a call
 * repeated on the same inputs returns the same bits:
 *   - sums over rows (pp_seg_reduce, pp_broadcast_mul_bwd, pp_chconv_wgrad): one partial per PP_SEG_ROWS consecutive rows,
 *     added in ascending row order from +0 inside the partial; then the partials in ascending order, starting from the first;
 *   - sums over offsets (pp_pool, pp_pool_bwd, pp_chconv_fwd): the present neighbours in ascending k, starting from +0
 *     (the bias, where there is one, is added last).
 * Products are rounded before they are added (no fused multiply-add).
 */
#ifndef PASCO_POOL_H_
#define PASCO_POOL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_FN(name) pp_##name

#define PP_ABI_VERSION 1
#define PP_MAX_KVOL 64                       /* offsets of one pooling window / channel-wise kernel */
#define PP_MAX_BATCH 64                      /* batch indices of one per-batch reduction or broadcast */
#define PP_SEG_ROWS 256                      /* consecutive rows of one partial sum */

#define PP_SUM 0                             /* pp_seg_reduce, pp_pool, pp_pool_bwd */
#define PP_AVG 1
#define PP_MAX 2                             /* pp_seg_reduce only */

#define PP_BC_ADD 0                          /* pp_broadcast */
#define PP_BC_MUL 1
#define PP_BC_CAT 2
#define PP_BC_COPY 3

int PP_FN(abi_version)(void);
const char *PP_FN(last_error)(void);

/* Bytes of workspace pp_seg_reduce and pp_broadcast_mul_bwd need for n rows of c channels in B segments (0 where none is
 * needed), -1 outside the served range. */
int64_t PP_FN(seg_workspace_bytes)(int64_t n, int32_t c, int32_t B);

/* x fp32 [n, c] with row stride ldx >= c elements (a column slice of a wider matrix), coords int32 [n, 4] (b_i = coords[i][0];
 * the rows of one batch index need NOT be contiguous or sorted) -> out fp32 [B, c], count fp32 [B] (may be null), and for
 * PP_MAX arg int32 [B, c]; all OVERWRITTEN.
 *   PP_SUM: out[b] = sum_{i: b_i = b} x[i]
 *   PP_AVG: out[b] = sum[b] / count[b] where count[b] > 0 (the division is the last operation)
 *   PP_MAX: out[b][ch] = the maximum of the segment's values; a NaN in the segment makes it NaN.  arg[b][ch] = the FIRST row, in
 *           ascending row order, whose value compares equal (==, so +0 and -0 tie and the first one's bits are the result) to
 *           the maximum; -1 for an empty segment or a NaN maximum (the rule of pr_maxpool_arg).
 * count[b] = the number of rows with b_i = b.  A batch index with no rows gives a zero row and count 0 (ours).  A row whose
 * batch index is outside [0, B) is ignored (ours).
 * Served: 1 <= B <= PP_MAX_BATCH, c >= 1, 0 <= n < 2^24 (the count is exact in fp32); n == 0 writes zeros (arg -1). */
int PP_FN(seg_reduce)(const float *x, int64_t n, int32_t c, int64_t ldx, const int32_t *coords, int32_t B, int32_t mode,
                      float *out, float *count, int32_t *arg, void *workspace, int64_t workspace_bytes, void *stream);

/* dy fp32 [B, c], arg int32 [B, c] (pp_seg_reduce, PP_MAX) -> dx fp32 [n, c], OVERWRITTEN: one fill with zeros, then
 *   dx[arg[b][ch]][ch] = dy[b][ch]   for arg[b][ch] in [0, n)
 * One store per (b, ch), all to different elements: no race.  n == 0 is a no-op. */
int PP_FN(seg_max_bwd)(const float *dy, const int32_t *arg, int32_t B, int32_t c, int64_t n, float *dx, void *stream);

/* x fp32 [n, c] (null for PP_BC_COPY), g fp32 [B, cg], coords int32 [n, 4], cnt fp32 [B] or null -> out, OVERWRITTEN:
 *   PP_BC_ADD:  out [n, c]      = x[i] + v(b_i)          (cg == c)
 *   PP_BC_MUL:  out [n, c]      = x[i] * v(b_i)          (cg == c)
 *   PP_BC_CAT:  out [n, c + cg] = cat(x[i], v(b_i))
 *   PP_BC_COPY: out [n, cg]     = v(b_i)                 (c is ignored)
 * with v(b) = g[b] where cnt is null, g[b] / cnt[b] otherwise (the backward of the per-batch average; 0 where cnt[b] == 0).
 * A row whose batch index is outside [0, B) gets a ZERO output row in every mode (ours; the Python level refuses such a tensor).
 * Served: 1 <= B <= PP_MAX_BATCH, c, cg >= 1, 0 <= n < 2^31; n == 0 is a no-op. */
int PP_FN(broadcast)(const float *x, int64_t n, int32_t c, const float *g, int32_t cg, const int32_t *coords, int32_t B,
                     const float *cnt, int32_t mode, float *out, void *stream);

/* The backward of PP_BC_MUL in one pass over the rows: dy, x fp32 [n, c], g fp32 [B, c], coords int32 [n, 4] ->
 *   dx fp32 [n, c] = dy[i] * g[b_i]                     (null: not wanted; a batch index outside [0, B) gives a zero row)
 *   dg fp32 [B, c] = sum_{i: b_i = b} dy[i] * x[i]      (null: not wanted; pp_seg_reduce's order, each product rounded first)
 * both OVERWRITTEN.  Workspace and served range of pp_seg_reduce. */
int PP_FN(broadcast_mul_bwd)(const float *dy, const float *x, const float *g, const int32_t *coords, int64_t n, int32_t c,
                             int32_t B, float *dx, float *dg, void *workspace, int64_t workspace_bytes, void *stream);

/* x fp32 [n_in, c], nbr int32 [K, n_out] -> out fp32 [n_out, c], cnt fp32 [n_out], both OVERWRITTEN:
 *   cnt[o] = the number of PRESENT neighbours of o;  sum[o] = sum over them, in ascending k from +0, of x[nbr[k][o]]
 *   PP_SUM: out[o] = sum[o];  PP_AVG: out[o] = sum[o] / cnt[o]  (ME's definition: the neighbours that exist, not the kernel
 *   volume);  cnt[o] == 0 gives a zero row (ours).
 * Served: 1 <= K <= PP_MAX_KVOL, c >= 1, 0 <= n_in, n_out < 2^31; n_out == 0 is a no-op. */
int PP_FN(pool)(const float *x, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out, int32_t mode,
                float *out, float *cnt, void *stream);

/* dy fp32 [n_out, c], cnt fp32 [n_out] (pp_pool; read for PP_AVG only), inv int32 [K, n_in] (pg_nbr_invert of the pooling
 * table, with its precondition) -> dx fp32 [n_in, c], OVERWRITTEN:
 *   dx[i] = sum over k ascending with o = inv[k][i] in [0, n_out) of  dy[o]               (PP_SUM)
 *                                                                     dy[o] * (1 / cnt[o]) (PP_AVG; cnt[o] == 0: no term)
 * from +0.  Served as pp_pool; n_in == 0 is a no-op, n_out == 0 writes zeros. */
int PP_FN(pool_bwd)(const float *dy, int64_t n_out, int32_t c, const float *cnt, const int32_t *inv, int32_t K, int64_t n_in,
                    int32_t mode, float *dx, void *stream);

/* x fp32 [n_in, c], nbr int32 [K, n_out], w fp32 [K, c], bias fp32 [c] or null -> out fp32 [n_out, c], OVERWRITTEN:
 *   out[o][ch] = (sum over the present neighbours, in ascending k from +0, of x[nbr[k][o]][ch] * w[k][ch]) (+ bias[ch])
 * An output row with no present neighbour is the bias, or zeros.  Served as pp_pool. */
int PP_FN(chconv_fwd)(const float *x, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out, const float *w,
                      const float *bias, float *out, void *stream);

/* Bytes of workspace pp_chconv_wgrad needs (0 where none is needed), -1 outside the served range. */
int64_t PP_FN(chconv_wgrad_workspace_bytes)(int32_t K, int32_t c, int64_t n_out);

/* x fp32 [n_in, c], dy fp32 [n_out, c], nbr int32 [K, n_out] -> dw fp32 [K, c], OVERWRITTEN:
 *   dw[k][ch] = sum over o with nbr[k][o] present of x[nbr[k][o]][ch] * dy[o][ch]
 * one partial per PP_SEG_ROWS consecutive OUTPUT rows (ascending o from +0), then the partials in ascending order.
 * Served as pp_pool with K * c < 2^31; n_out == 0 or n_in == 0 writes zeros. */
int PP_FN(chconv_wgrad)(const float *x, int64_t n_in, int32_t c, const float *dy, int64_t n_out, const int32_t *nbr, int32_t K,
                        float *dw, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_POOL_H_ */

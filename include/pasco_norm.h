/*
 * pasco_norm.h -- flat C ABI of training-mode batch normalisation over feature rows in libpascohip.so
 * (pasco_amd/csrc/norm.hip): the statistics as mergeable records, the normalisation with its activation folded in, and the
 * backward.  The autograd operator over it is pasco_amd/grad/norm.py (`batch_norm_rows`), the host restatement
 * pasco_amd/grad/host.py.  A separate surface from include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_rowgrad.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pn_last_error().
 *
 * Rows are fp32 [n, c], row-major and contiguous; 1 <= c <= PN_MAX_C, any c (16-byte accesses where c % 4 == 0 and the row
 * pointers are 16-byte aligned, 4-byte ones otherwise); 0 <= n with n * c < 2^62.
 *
 * Records (fp64, per channel, so that the record of another rank is one more partial to merge):
 *   moments record [3, c]:  count, mean, M2 = sum (x - mean)^2
 *   sums record    [2, c]:  sum g, sum g * xhat
 * Merge rule of moments records a, b (the pairwise update of Chan et al.), applied left to right from (0, 0, 0), a record of
 * count 0 skipped:
 *   n = n_a + n_b;  w = n_b / n;  d = mean_b - mean_a;  mean = mean_a + d * w;  M2 = (M2_a + M2_b) + (d * d) * (n_a * w)
 * in fp64 without contraction (the first record with rows comes out as it is: w = 1, n_a = 0).
 * A sums record is merged by plain addition, left to right.
 *
 * Determinism: no floating-point atomics, no in-launch ticket or fence.  A workgroup owns PN_TILE_ROWS consecutive rows and
 * writes one partial record; the partials are combined by a launch of their own, a channel's records by one thread, in ascending tile
 * order.  A call repeated on the same inputs returns the same bits.
 *
 * With z = (x - mean) * rstd * weight + bias (evaluated as ((x - mean) * rstd) * weight + bias in fp32, no contraction):
 *   act = PH_ACT_NONE:  y = z                          act'(z) = 1
 *   act = PH_ACT_RELU:  y = z > 0 ? z : 0              act'(z) = z > 0 ? 1 : 0        (z == 0 gets gradient 0)
 *   act = PH_ACT_LEAKY: y = z > 0 ? z : slope * z      act'(z) = z > 0 ? 1 : slope    (slope where z <= 0)
 * The backward recomputes z from x by the same expression; no pre-activation tensor is kept.
 */
#ifndef PASCO_NORM_H_
#define PASCO_NORM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_FN(name) pn_##name

#define PN_ABI_VERSION 1
#define PN_TILE_ROWS 128                     /* rows of one partial record */
#define PN_MAX_C (1 << 20)

int PN_FN(abi_version)(void);
const char *PN_FN(last_error)(void);

/* Bytes of scratch pn_moments and pn_bwd_sums need for the per-tile partials of n rows: ceil(n / PN_TILE_ROWS) * 3 * c * 8
 * (0 for n == 0); -1 for arguments outside the served range. */
int64_t PN_FN(ws_bytes)(int64_t n, int32_t c);

/* x fp32 [n, c] -> rec fp64 [3, c], the moments record of the n rows.  Launch 1: every tile's record into ws (fp64
 * [tiles, 3, c]): its count, its mean (the fp64 sum over the count) and M2 about THAT mean, from a second read of the tile -
 * never sum x^2 - n * mean^2.  Launch 2: pn_moments_merge's kernel over the tiles.  n == 0 writes (0, 0, 0) and reads no x. */
int PN_FN(moments)(const float *x, int64_t n, int32_t c, void *ws, int64_t ws_bytes, double *rec, void *stream);

/* recs fp64 [r, 3, c] -> out fp64 [3, c]: the merge rule above over the records in ascending order.  r == 0, or all counts
 * 0: (0, 0, 0).  out must not alias recs. */
int PN_FN(moments_merge)(const double *recs, int32_t r, int32_t c, double *out, void *stream);

/* rec fp64 [3, c] -> mean_rstd fp32 [2, c] = (mean, 1 / sqrt(M2 / count + eps)), formed in fp64 and rounded once; count 0
 * gives (0, 1 / sqrt(eps)).  Where running_mean / running_var (fp32 [c]) are not NULL and count > 0, in place:
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var  + momentum * M2 / max(count - 1, 1)
 * (fp64, rounded once); count 0 leaves them untouched. */
int PN_FN(finish)(const double *rec, int32_t c, double eps, double momentum, float *running_mean, float *running_var,
                  float *mean_rstd, void *stream);

/* y fp32 [n, c] = act(z); weight / bias fp32 [c] or NULL (1 / 0).  y may be x. */
int PN_FN(apply)(const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight, const float *bias,
                 int32_t act, float slope, float *y, void *stream);

/* dy, x fp32 [n, c] -> sums fp64 [2, c] = (sum g, sum g * xhat) over the n rows, g = dy * act'(z), xhat = (x - mean) * rstd.
 * Per-tile partials into ws (fp64 [tiles, 2, c]), then pn_sums_merge's kernel over them.  n == 0 writes zeros. */
int PN_FN(bwd_sums)(const float *dy, const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight,
                    const float *bias, int32_t act, float slope, void *ws, int64_t ws_bytes, double *sums, void *stream);

/* sums fp64 [r, 2, c] -> out fp64 [2, c]: added in ascending r starting from +0.  out must not alias sums. */
int PN_FN(sums_merge)(const double *sums, int32_t r, int32_t c, double *out, void *stream);

/* dx fp32 [n, c] = weight * rstd * (g - S0 / N - xhat * S1 / N), (S0, S1) = total_sums fp64 [2, c], N = the count of
 * total_rec fp64 [3, c], read on the device (S0 / N and S1 / N are formed in fp64 and rounded to fp32 once per channel).
 * dx may be dy. */
int PN_FN(bwd_dx)(const float *dy, const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight,
                  const float *bias, int32_t act, float slope, const double *total_sums, const double *total_rec, float *dx,
                  void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_NORM_H_ */

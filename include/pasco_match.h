/*
 * pasco_match.h -- flat C ABI of the panoptic matcher and mask losses in libpascohip.so (pasco_amd/csrc/match.hip).
 *
 * The reference's HungarianMatcher and SetCriterion.loss_masks both reduce N voxel rows of Q mask logits against T binary targets.
 * With p = sigmoid(x), fp = 0.25 (1-p)^2 softplus(-x), fn = 0.75 p^2 softplus(x) and tgt[n][t] in {0, 1}, over the rows that
 * count:
 *
 *   focal_sum[q][t] = sum_n (fp - fn)[n][q] tgt[n][t] + sum_n fn[n][q]
 *   inter[q][t]     = sum_n p[n][q] tgt[n][t]
 *   psum[q] = sum_n p[n][q],  tsum[t] = sum_n tgt[n][t],  count = the rows counted
 *   dice[q][t]      = 1 - (2 inter + 1) / (psum + tsum + 1)
 *
 * The matcher counts the "matchable" rows (known, at least one target), the loss the "known" rows.  The targets are 128-bit
 * words per row (bit t = the voxel lies in target t), the layout ph_attn_mask_pack uses; the [N, T] float matrix never exists.
 * The host restatement is pasco_amd/grad/host.py.  A separate surface from include/pasco_hip.h: own prefix, own version, no
 * CPU oracle.
 *
 * Conventions (as pasco_grad.h): device pointers only, EXCEPT pm_assign, which takes HOST pointers and touches no device; all
 * device work is enqueued on `stream`; no call synchronises, allocates or reads the environment; return 0 = ok, text of a
 * failure via pm_last_error().  A refused call launches nothing.
 * Served: 1 <= q <= 128, 1 <= t <= 128, n >= 0, finite logits.
 *
 * Determinism: no floating-point atomics.  Every row belongs to one row range; a range's partial sums are accumulated in
 * ascending row order and the ranges are added in ascending range order; the number of ranges is a function of (n, q, t) alone.
 * A call repeated on the same inputs returns the same bits.
 */
#ifndef PASCO_MATCH_H_
#define PASCO_MATCH_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_FN(name) pm_##name

#define PM_ABI_VERSION 1
#define PM_MAX_Q 128                         /* queries served */
#define PM_MAX_T 128                         /* targets served */
#define PM_FLAG_KNOWN 1                      /* flags bit 0: inside the grid and not unknown */
#define PM_FLAG_MATCHABLE 2                  /* flags bit 1: known and in at least one target */

int PM_FN(abi_version)(void);
const char *PM_FN(last_error)(void);

/* masks uint8 [T, X, Y, Z] (non-zero = inside), unknown uint8 [X, Y, Z] or NULL, coords int32 [N, 4] (column 0 ignored; the
 * voxel is coords[1..3] - origin) -> tbits uint32 [N, 4] (bits >= T are 0), flags uint8 [N], oob int32 [1] = the rows outside
 * [0, dims) (such rows get zero words and zero flags).  All three outputs are overwritten. */
int PM_FN(target_pack)(const uint8_t *masks, const uint8_t *unknown, const int32_t *coords, int64_t n, int32_t t, int32_t dx,
                       int32_t dy, int32_t dz, int32_t ox, int32_t oy, int32_t oz, uint32_t *tbits, uint8_t *flags,
                       int32_t *oob, void *stream);

/* Row ranges of pm_pair_sums for a shape (0 for n == 0 or a shape that is not served) and the bytes of scratch it needs. */
int64_t PM_FN(pair_sums_ranges)(int64_t n, int32_t q, int32_t t);
int64_t PM_FN(pair_sums_workspace_bytes)(int64_t n, int32_t q, int32_t t);

/* logits fp32 [N, Q] row-major, tbits uint32 [N, 4], flags uint8 [N]; a row counts when bit `flag_bit` (0 = known, 1 =
 * matchable) of its flag is set -> focal_sum fp32 [Q, T], dice fp32 [Q, T], stats fp32 [Q, T, 3] = (inter, psum, tsum),
 * count int32 [1], all overwritten.  Target bits at positions >= t are never looked at. */
int PM_FN(pair_sums)(const float *logits, const uint32_t *tbits, const uint8_t *flags, int32_t flag_bit, int64_t n, int32_t q,
                     int32_t t, float *focal_sum, float *dice, float *stats, int32_t *count, void *ws, int64_t ws_bytes,
                     void *stream);

/* dlogits fp32 [N, Q], overwritten in full.  tgt_of_query int32 [Q] (-1 = unmatched, else < t), coef fp32 [Q, 3] = (c, a, b).
 * For a known row and a matched query, with y the row's bit of the query's target:
 *   dx = c * d focal(x, y)/dx + p (1 - p) (a y + b)        (focal with alpha 0.25, gamma 2; the dice term through sigmoid)
 * every other element is exactly 0. */
int PM_FN(mask_loss_bwd)(const float *logits, const uint32_t *tbits, const uint8_t *flags, const int32_t *tgt_of_query,
                         const float *coef, int64_t n, int32_t q, int32_t t, float *dlogits, void *stream);

/* HOST pointers; no device work.  The rectangular linear sum assignment of cost fp64 [Q, T] row-major -> row[K], col[K],
 * K = min(Q, T), rows ascending (the result convention of scipy.optimize.linear_sum_assignment).  q, t >= 0.  A non-finite
 * cost is refused. */
int PM_FN(assign)(const double *cost, int32_t q, int32_t t, int32_t *row, int32_t *col);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_MATCH_H_ */

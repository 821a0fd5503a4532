/*
 * pasco_semloss.h -- flat C ABI of the semantic completion losses in libpascohip.so (pasco_amd/csrc/semloss.hip).
 *
 * The reference's compute_sem_compl_loss optimises, per scale and subnet, a class-weighted cross entropy and the Lovasz-softmax
 * loss of N rows of C logits against a dense uint8 label grid.  With p = softmax(F), y the row's label:
 *
 *   rows that count: min_C <= coords[1..3] <= max_C on all three axes;  y = target[(coords[1..3] - min_C) // scale]
 *   ce     = sum_n w[y_n] nll_n / sum_n w[y_n]                  over the counting rows with y != 255   (0/0 = NaN, as torch)
 *   err_c  = |[y == c] - p_c|   for EVERY counting row, the rows labelled 255 included (they are background for every class)
 *   loss_c = sum_i err_c[perm_c[i]] * inc_c[i],  perm_c = the rows in descending err_c, equal errors in ascending row order
 *   lovasz = mean of loss_c over the classes with at least one row y == c   (0 when there is none)
 *
 * The increment of the Jaccard index along the sorted order has a closed form in integers.  G = the rows with y == c, cf_i = the
 * foreground rows among sorted positions 0..i, I_i = G - cf_i, U_i = G + (i + 1) - cf_i, U_-1 = G:
 *   inc_i = 1 / U_i at a foreground position,  I_i / (U_i-1 U_i) at a background position.
 * The only global dependence is an int32 prefix sum over the sorted order.
 *
 * Labels as the kernels store them: 0..C-1, 255 = ignore, 254 = outside the box (the row counts for nothing).
 *
 * Conventions (as pasco_match.h): device pointers only, EXCEPT ps_geometry, whose `g` is a HOST pointer; all device work is
 * enqueued on `stream`; no call synchronises, allocates or reads the environment; return 0 = ok, text of a failure via
 * ps_last_error().  A refused call launches nothing and leaves its outputs untouched.
 * Served: 2 <= c <= 32 classes, 0 <= n <= 2^24 rows, scale >= 1, finite logits.
 *
 * Determinism: no floating-point atomics (integer atomics in LDS only).  Every float sum is a sum of per-thread partials in
 * ascending row order, a fixed tree within a workgroup, and the workgroups' partials in ascending order; the geometry is a
 * function of (n, c) alone.  A call repeated on the same inputs returns the same bits.
 */
#ifndef PASCO_SEMLOSS_H_
#define PASCO_SEMLOSS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_FN(name) ps_##name

#define PS_ABI_VERSION 1
#define PS_MIN_C 2
#define PS_MAX_C 32
#define PS_MAX_N (1 << 24)
#define PS_LABEL_IGNORE 255
#define PS_LABEL_OUTSIDE 254
#define PS_SORT_TILE 2048                    /* keys of one workgroup of the sort and of the Lovasz scan */
#define PS_GEOMETRY_WORDS 10

int PS_FN(abi_version)(void);
const char *PS_FN(last_error)(void);

/* g: HOST int64 [PS_GEOMETRY_WORDS] = (tile, tiles, range_rows, ranges, keys_bytes, perm_bytes, sort_bytes, rows_bytes,
 * lovasz_bytes, workspace_bytes).  tile = PS_SORT_TILE keys, tiles = ceil(n / tile); ranges of range_rows rows are what
 * ps_rows_fwd reduces over.  workspace_bytes = the five parts in this order, each padded to 256 bytes: what one forward needs
 * (the keys [C, N], the order [C, N] and the scratch of the three stages).  All zeros for a shape that is not served. */
int PS_FN(geometry)(int64_t n, int32_t c, int64_t *g);
int64_t PS_FN(workspace_bytes)(int64_t n, int32_t c);
/* The scratch of ps_sort_desc for s segments of m keys (0 for a shape that is not served). */
int64_t PS_FN(sort_workspace_bytes)(int64_t s, int64_t m);

/* logits fp32 [N, C], coords int32 [N, 4] (column 0 ignored), target uint8 [dx, dy, dz], box = int32 [6] on the DEVICE (min_C
 * then max_C, inclusive), weights fp32 [C] -> label uint8 [N]; ce fp32 [3] = (ce_num / ce_den, ce_num, ce_den); class_count
 * int32 [C]; info int32 [4] = (rows inside the box, rows inside the box whose label index falls outside the grid, labels in
 * C..253, 0); keys uint32 [C, N] = the bits of err_c per row, 0 for a row outside the box.  A row with a bad index or a bad
 * label is stored as 255.  ws of the geometry's rows_bytes.  All outputs are overwritten. */
int PS_FN(rows_fwd)(const float *logits, const int32_t *coords, const uint8_t *target, const int32_t *box, int32_t scale,
                    const float *weights, int64_t n, int32_t c, int32_t dx, int32_t dy, int32_t dz, uint8_t *label, float *ce,
                    int32_t *class_count, int32_t *info, uint32_t *keys, void *ws, int64_t ws_bytes, void *stream);

/* keys uint32 [S, M] (any values) -> perm int32 [S, M]: per segment the indices in descending key order, equal keys in
 * ascending index order.  1 <= s <= 65535, 0 <= m <= 2^24.  A least-significant-digit radix sort, four 8-bit passes; every
 * pass is one launch grid over all segments. */
int PS_FN(sort_desc)(const uint32_t *keys, int64_t s, int64_t m, int32_t *perm, void *ws, int64_t ws_bytes, void *stream);

/* perm int32 [C, N] (a permutation of 0..N-1 per class), label uint8 [N], keys uint32 [C, N], class_count int32 [C] ->
 * loss_c fp32 [C] (0 for an absent class), coef fp32 [N, C] (the increment of the row's sorted position, times -1 for a
 * foreground and +1 for a background row; 0 for an absent class and a row outside the box), lovasz fp32 [1] = the mean over
 * the present classes, present int32 [1].  ws of the geometry's lovasz_bytes.  All outputs are overwritten. */
int PS_FN(lovasz_fwd)(const int32_t *perm, const uint8_t *label, const uint32_t *keys, const int32_t *class_count, int64_t n,
                      int32_t c, float *loss_c, float *coef, float *lovasz, int32_t *present, void *ws, int64_t ws_bytes,
                      void *stream);

/* dlogits fp32 [N, C], overwritten in full:
 *   dlogits[n][k] = g[0] w[y] / ce[2] (p_k - [k == y]) [y < C] + g[1] / present p_k (coef[n][k] - sum_c coef[n][c] p_c)
 * g fp32 [2] on the DEVICE = the incoming gradients of (ce, lovasz); ce fp32 [3] and present int32 [1] as the forward wrote
 * them.  p is recomputed from the logits.  A row labelled 254 is exactly 0. */
int PS_FN(loss_bwd)(const float *logits, const uint8_t *label, const float *coef, const float *weights, const float *ce,
                    const int32_t *present, const float *g, int64_t n, int32_t c, float *dlogits, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_SEMLOSS_H_ */

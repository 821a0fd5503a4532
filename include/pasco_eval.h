/*
 * pasco_eval.h -- flat C ABI of the evaluation kernels in libpascohip.so (pasco_amd/csrc/eval.hip).
 *
 * The reference scores a step with numpy / Python passes over dense grids (pasco/models/net_panoptic_sparse.py:625-760,
 * pasco/models/metrics.py:74-691, pasco/loss/panoptic_quality.py:15-390).  These entry points make the per-site and
 * per-row passes of that scoring on the device; the bookkeeping on the small tables they return is host code
 * (pasco_amd/eval/).  They are a separate surface from include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_hip.h): device pointers unless named `h_*`; all work is enqueued on `stream`; no call
 * synchronises or allocates; return 0 = ok, text of a failure via pe_last_error().
 *
 * Layout: S = X*Y*Z sites, site = x*Y*Z + y*Z + z (C order of a dense [X, Y, Z] tensor).  GT semantic 255 = unknown.
 * Confidence bins: PE_BINS host-side fp32 edges (torch.linspace(0, 1, 16)); bin = (number of edges <= conf) - 1, i.e.
 * torch.bucketize(conf, edges, right=True) - 1, so conf = 1.0 has a 16th bin of its own.  A conf below the first edge
 * (not a probability) goes to bin 0; a NaN conf goes to bin PE_BINS - 1, as torch.bucketize puts it past every edge.
 * Every integer table is an exact count.  Floating sums are accumulated as fixed point and returned as fp64, so every
 * result is bitwise identical from run to run: a confidence adds rint(conf * 2^36), a -log term rint(term * 2^30), the
 * terms are summed exactly (in 128 bits across workgroups) and the total is rounded to fp64 once, then scaled back.
 * NaN and +-inf confidences and -log terms add nothing to a sum (they are still counted); finite confidences saturate at
 * +-512.  Within those rules no sum can overflow for up to PE_MAX_SITES sites or rows.
 */
#ifndef PASCO_EVAL_H_
#define PASCO_EVAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_FN(name) pe_##name

#define PE_ABI_VERSION 1
#define PE_BINS 16
#define PE_MAX_CLASSES 32  /* channels of one probability row */
#define PE_MAX_PRED 128    /* largest predicted segment id (the panop_* tables hold 128 segments) */
#define PE_MAX_GT 1023     /* largest ground-truth segment id */
#define PE_MAX_SITES (1LL << 27) /* sites of pe_ssc, rows of pe_mask_ece */

/* pe_ssc output: counts int64 [PE_SSC_COUNTS(c)], sums fp64 [PE_SSC_SUMS] */
#define PE_SSC_COUNTS(c) ((c) * (c) + 1 + 4 * PE_BINS)
#define PE_SSC_SUMS (2 * PE_BINS + 2)
/* pe_mask_ece output: counts int64 [2 * PE_BINS], sums fp64 [PE_BINS] */
#define PE_ECE_COUNTS (2 * PE_BINS)
#define PE_ECE_SUMS PE_BINS

int PE_FN(abi_version)(void);
const char *PE_FN(last_error)(void);

/* Scratch bytes of pe_ssc for `n_sites` sites of `c` classes, and of pe_mask_ece for `n_rows` rows. */
int64_t PE_FN(ssc_workspace_bytes)(int64_t n_sites, int32_t c);
int64_t PE_FN(ece_workspace_bytes)(int64_t n_rows);

/* One pass over the dense sites of one output (SSCMetrics.add_batch / add_batch_ece, metrics.py:566-622).
 *   probs  [S, c] fp32 channels-last class probabilities (c <= PE_MAX_CLASSES), conf [S] fp32, gt [S] uint8
 *   pred = first maximum of the row with a NaN as the maximum, -0.0 == +0.0 (torch.argmax).
 *   Sites with gt = 255 count as unknown only; sites with c <= gt < 255 are skipped (the host refuses such labels).
 *   counts: [c * c] confusion (gt, pred) over known sites | [1] unknown sites |
 *           [2][PE_BINS] sites per bin | [2][PE_BINS] correct (pred == gt) sites per bin; group 0 = pred == 0, 1 = pred != 0
 *   sums:   [2][PE_BINS] sum of conf per bin | [2] sum of -log(p[gt] + 1e-12) (fp32 log) per group */
int PE_FN(ssc)(const float *probs, const float *conf, const uint8_t *gt, int64_t n_sites, int32_t c,
               const float *h_edges, void *ws, int64_t ws_bytes, int64_t *counts, double *sums, void *stream);

/* One pass over the sparse rows of one panoptic output (pq_compute_single_core, panoptic_quality.py:198-236).
 *   site [n] int64, pred [n] int32 segment id (0 = none), gt_sem [S] uint8, gt_id [S] int32 GT panoptic id.
 *   area  [n_pred + 1] int64: rows of each pred id at known sites (the reference's area after unknown zeroing);
 *   inter [(n_gt + 1) * (n_pred + 1)] int64: rows at known sites per (gt id, pred id).
 *   Rows whose site or pred id is out of range are not counted.  A row whose gt id is out of range (< 0 or > n_gt)
 *   counts in `area` (the area is the prediction's) but in no `inter` cell.  n_pred <= PE_MAX_PRED, n_gt <= PE_MAX_GT. */
int PE_FN(panop_pairs)(const int64_t *site, const int32_t *pred, int64_t n, const uint8_t *gt_sem, const int32_t *gt_id,
                       int64_t n_sites, int32_t n_pred, int32_t n_gt, int64_t *area, int64_t *inter, void *stream);

/* map [n_pred + 1] int32: map[p] = g for the gt id with 2 * inter > area_p + gt_area_g - inter (IoU > 0.5, exact
 * integers; find_matched_segment at threshold 0.5, panoptic_quality.py:120-165), else 0.  One workgroup. */
int PE_FN(match)(const int64_t *area, const int64_t *gt_area, const int64_t *inter, int32_t n_pred, int32_t n_gt,
                 int32_t *map, void *stream);

/* The mask part of compute_ece_panop (metrics.py:140-158) over the rows with 0 <= site < n_sites, gt_id[site] != 0 and
 * conf != 0 (a NaN conf is kept); a pred id outside 0 .. n_pred maps to 0.  Bins and sums as pe_ssc's:
 *   counts: [PE_BINS] rows per bin | [PE_BINS] rows with map[pred] == gt_id;  sums: [PE_BINS] sum of conf per bin. */
int PE_FN(mask_ece)(const int64_t *site, const int32_t *pred, const float *conf, int64_t n, const int32_t *gt_id,
                    int64_t n_sites, const int32_t *map, int32_t n_pred, const float *h_edges, void *ws, int64_t ws_bytes,
                    int64_t *counts, double *sums, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_EVAL_H_ */

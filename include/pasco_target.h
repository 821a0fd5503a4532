/*
 * pasco_target.h -- flat C ABI of the training-target kernels in libpascohip.so (pasco_amd/csrc/target.hip).
 *
 * A frame's labelled completion grids become, per subnet, what the training step supervises against: the label grids
 * resampled under the subnet's transform (and the training crop), the multi-scale geometry / semantic labels and the mask
 * targets.  The host restatement is `build_train_item` (pasco_amd/data/semantic_kitti.py); these entry points reproduce it
 * bit for bit: every output is uint8, int32 or bool, there is no tolerance.  A separate surface like pasco_frame.h: own
 * prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_frame.h): device pointers unless named `h_*`; all work is enqueued on `stream`; no call
 * synchronises or allocates; return 0 = ok, text of a failure via pt_last_error().  Compiled with FP contraction off; no
 * environment reads.
 *
 * Host reads per batch, each covering all M subnets at once: the bounds after pt_resample; the bounds after
 * pt_crop_bounds when cropping; the presence tables after pt_labels.  Three at most, two without the crop.
 *
 * Numerics: the coordinate arithmetic is the `transform` chain of pasco_frame.h (fp32, fmaf over k = 0..3 from 0, rintf),
 * the same device function as pf_label_bounds (pasco_amd/csrc/transform_chain.h).  The crop compares double(c) against the
 * fp64 window the host computed: kept iff lo <= c < hi in x and in y.
 *
 * Box grids: `sem_box` / `ins_box` uint8 [M, box_stride], subnet m laid out row-major over its host-side upper bound
 * h_box_bound[m] = (lo xyz, hi xyz inclusive).  255 = no surviving sample.  A semantic sample survives iff it lies in the
 * box of the transformed known voxels and T^-1 lands it inside the grid on sem != 255; an instance sample iff the frame has
 * any non-zero instance id and it lands on ins != 255 (id 0 survives, and counts for the bounds).
 */
#ifndef PASCO_TARGET_H_
#define PASCO_TARGET_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_FN(name) pt_##name

#define PT_ABI_VERSION 1
#define PT_MAX_M 8           /* subnets per call (PF_MAX_M) */
#define PT_BOUNDS 18         /* int32 per subnet written by pt_resample: box, semantic-only, instance-only (lo xyz, hi xyz each) */
#define PT_CROP_BOUNDS 12    /* int32 per subnet written by pt_crop_bounds: semantic-only, instance-only */
#define PT_TABLE 768         /* int32 per presence table: 256 class flags, 256 first indices, 256 classes found there */
#define PT_MAX_T 128         /* targets pt_target_pack serves (PM_MAX_T) */

/* Where pt_labels writes one subnet.  Every grid is uint8, row-major [X, Y, Z] (z contiguous) with X, Y, Z = scene[] (each a
 * multiple of 4), the scale-s grids [X/s, Y/s, Z/s].  sem_labels["1_1"] is `semantic` itself. */
typedef struct {
  uint8_t *semantic;     /* filled with 255, then the surviving semantic samples */
  uint8_t *instance;     /* filled with 0, then the surviving instance samples */
  uint8_t *geo_1;        /* 255 where semantic == 255, 1 where semantic > 0, else 0 */
  uint8_t *geo_2;        /* per s^3 block: 255 if all voxels are 255, else 1 if any is in 1..254, else 0 */
  uint8_t *geo_4;
  uint8_t *sem_2;        /* per s^3 block: the most frequent class of 1..n_classes-1 (lowest index on a tie); without any: 0 if */
  uint8_t *sem_4;        /*   all voxels are 255, else 255 */
  int32_t min_C[3];      /* origin of the grids */
  int32_t scene[3];
} pt_subnet_out;

int PT_FN(abi_version)(void);
const char *PT_FN(last_error)(void);

/* Resampling of M <= PT_MAX_M subnets in one call.  sem / ins uint8 [X, Y, Z]; h_T, h_Tinv fp32 [M, 4, 4] (host, h_Tinv =
 * torch.inverse(T)); h_box_bound int32 [M, 6] must contain each subnet's exact box (the caller checks bounds[m][0..5] against
 * it after the read-back; samples outside it are not written).  Every byte of the first volume(h_box_bound[m]) bytes of
 * sem_box / ins_box row m is written.
 *   bounds int32 [M, PT_BOUNDS]; an empty set leaves lo = INT32_MAX, hi = INT32_MIN.
 * Reductions are integer min / max per block and one atomic per block and value: identical from run to run.
 * ws: pt_resample_workspace_bytes(M). */
int64_t PT_FN(resample_workspace_bytes)(int32_t M);
int PT_FN(resample)(const uint8_t *sem, const uint8_t *ins, int32_t X, int32_t Y, int32_t Z, const float *h_T,
                    const float *h_Tinv, int32_t M, const int32_t *h_box_bound, uint8_t *sem_box, uint8_t *ins_box,
                    int64_t box_stride, int32_t *bounds, void *ws, int64_t ws_bytes, void *stream);

/* Bounds of what the training crop keeps.  h_window fp64 [M, 4] = (lo x, hi x, lo y, hi y).
 *   out int32 [M, PT_CROP_BOUNDS]: semantic-only lo xyz, hi xyz; instance-only lo xyz, hi xyz. */
int PT_FN(crop_bounds)(const uint8_t *sem_box, const uint8_t *ins_box, int64_t box_stride, const int32_t *h_box_bound,
                       int32_t M, const double *h_window, int32_t *out, void *stream);

/* The label grids of M subnets from the box grids.  h_window fp64 [M, 4] or null (no crop); h_out [M] (host; its pointers
 * device).  table int32 [M, PT_TABLE] per subnet: [c] = 1 iff class c (1..254) occurs in `semantic`; [256 + i] = the smallest
 * row-major index of a voxel with instance id i (1..255), INT32_MAX if none (integer atomicMin: order independent);
 * [512 + i] = the semantic class at that voxel (0 if none).  One wave per 4^3 block; the class vote is wave ballots over the
 * classes present, no per-thread table. */
int PT_FN(labels)(const uint8_t *sem_box, const uint8_t *ins_box, int64_t box_stride, const int32_t *h_box_bound, int32_t M,
                  const double *h_window, const pt_subnet_out *h_out, int32_t n_classes, int32_t *table, void *stream);

/* The presence table (as above) of any pair of grids uint8 [n], n < 2^31: the frame's untransformed grids
 * (mask_label_origin). */
int PT_FN(presence)(const uint8_t *semantic, const uint8_t *instance, int64_t n, int32_t *table, void *stream);

/* masks bool [t, n] (one byte each, 0 / 1) from the two label grids uint8 [n] (n a multiple of 4) and two slot tables int32
 * [256]: cls_slot[c] = the target index of stuff class c, ins_slot[i] = that of instance id i, -1 = none.
 * masks[k][v] = cls_slot[semantic[v]] == k || ins_slot[instance[v]] == k. */
int PT_FN(masks)(const uint8_t *semantic, const uint8_t *instance, int64_t n, const int32_t *cls_slot, const int32_t *ins_slot,
                 int32_t t, uint8_t *masks, void *stream);

/* pm_target_pack (pasco_match.h) without the [t, X, Y, Z] tensor: per row of coords int32 [n, 4] (column 0 ignored, origin
 * subtracted), two bytes and two table entries are read.  tbits uint32 [n, 4] (16-byte aligned): bit k set iff target k
 * covers the voxel (a voxel can carry two bits: a stuff class with an instance id on it); flags uint8 [n]: bit 0 = known
 * (unknown null or 0 there), bit 1 = known and in at least one target; a row outside the grid gets zero words, flag 0 and
 * counts in oob int32 [1].  1 <= t <= PT_MAX_T. */
int PT_FN(target_pack)(const uint8_t *semantic, const uint8_t *instance, const int32_t *cls_slot, const int32_t *ins_slot,
                       const uint8_t *unknown, const int32_t *coords, int64_t n, int32_t t, int32_t dx, int32_t dy, int32_t dz,
                       int32_t ox, int32_t oy, int32_t oz, uint32_t *tbits, uint8_t *flags, int32_t *oob, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_TARGET_H_ */

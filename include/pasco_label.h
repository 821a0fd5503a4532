/*
 * pasco_label.h -- flat C ABI of the label-generation kernels in libpascohip.so (pasco_amd/csrc/label.hip).
 *
 * The ground-truth completion grid of a frame becomes the two grids every scoring path reads from
 * <preprocess_root>/instance_labels_v2/<seq>/<frame>_1_1.pkl: the panoptic "thing" instances (26-connected components
 * of each thing class) and the semantic grid with the voxels of tiny components turned into 255 (unknown).  The host
 * restatement is pasco_amd/data/instances.py (`instance_labels`, `semantic_grid`); these entry points reproduce it
 * exactly - every output is an integer.  A separate surface from include/pasco_hip.h: own prefix, own version, no CPU
 * oracle.
 *
 * Definition (site index of voxel (x, y, z) = x*Y*Z + y*Z + z; thing_ids in the caller's order):
 *   1. for each t in thing_ids the voxels with sem == t split into 26-connected components (neighbours differ by at
 *      most 1 on every axis, inside the grid); components of different classes never join;
 *   2. components are ordered by (position of their class in thing_ids, smallest site index of the component);
 *   3. a component of fewer than min_size voxels is dropped: instance 0 and semantic 255 on its voxels;
 *   4. the survivors are numbered 1..n in that order; every other voxel keeps its semantic value and has instance 0.
 * This is what a raster scan with a flood fill per class produces.  Two corners of that program are NOT reproduced:
 * it also applies the size rule to the background id 0 (a grid with fewer than min_size non-instance voxels), and it
 * numbers from 0 when the grid has no instance-0 voxel at all.  Neither occurs on a real frame.
 *
 * Conventions (as pasco_hip.h): device pointers unless named `h_*`; all work is enqueued on `stream`; no call
 * synchronises or allocates; return 0 = ok, text of a failure via pl_last_error().  Every result is identical from run
 * to run: the root of a component is its smallest site, whatever order the atomics land in.
 */
#ifndef PASCO_LABEL_H_
#define PASCO_LABEL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_FN(name) pl_##name

#define PL_ABI_VERSION 1
#define PL_MAX_THINGS 32      /* distinct thing ids per call, each in 1..254 */
#define PL_RECORD 4           /* int32 per record written by pl_instances */
#define PL_MAX_SITES (1 << 30)

/* record fields */
#define PL_REC_INSTANCES 0    /* surviving instances n */
#define PL_REC_DROPPED 1      /* components below min_size */
#define PL_REC_UNKNOWN 2      /* voxels turned 255 */
#define PL_REC_STATUS 3       /* 0 = clean, else PL_STATUS_* bits */

#define PL_STATUS_RAW_RANGE 1 /* pl_semantic_grid: a raw label >= n_lut (that voxel is written as 255) */
#define PL_STATUS_LOOP_CAP 2  /* pl_instances: a union loop hit its iteration cap (never expected; results invalid) */

int PL_FN(abi_version)(void);
const char *PL_FN(last_error)(void);

/* SemanticKITTI voxels/<frame>.label + .invalid -> the semantic grid.
 *   raw uint16 [S], invalid uint8 [S / 8] (bit-packed, most significant bit first; S % 8 == 0), lut uint8 [n_lut]
 *   sem uint8 [S] = 255 where the invalid bit is set, lut[raw] elsewhere.
 * A raw value >= n_lut writes 255 and ORs PL_STATUS_RAW_RANGE into d_status[0] (int32, zeroed by the caller). */
int PL_FN(semantic_grid)(const uint16_t *raw, const uint8_t *invalid, const uint8_t *lut, int32_t n_lut, int64_t S,
                         uint8_t *sem, int32_t *d_status, void *stream);

/* Scratch bytes of pl_instances for an [X, Y, Z] grid and n_things thing ids (< 0: unsupported shape). */
int64_t PL_FN(instances_workspace_bytes)(int32_t X, int32_t Y, int32_t Z, int32_t n_things);

/* sem uint8 [X, Y, Z]; h_thing_ids int32 [n_things] (host, distinct, 1..254, any order); min_size >= 0.
 *   instance     int32 [X, Y, Z]
 *   semantic_out uint8 [X, Y, Z] (may not alias sem)
 *   record       int32 [PL_RECORD]
 *   sizes        int32 [sizes_cap], nullable: voxel count of instance i at sizes[i - 1] for i <= sizes_cap; entries
 *                from n on are not written.
 * ws: pl_instances_workspace_bytes(X, Y, Z, n_things), 16-byte aligned. */
int PL_FN(instances)(const uint8_t *sem, int32_t X, int32_t Y, int32_t Z, const int32_t *h_thing_ids, int32_t n_things,
                     int32_t min_size, int32_t *instance, uint8_t *semantic_out, int32_t *record, int32_t *sizes,
                     int32_t sizes_cap, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_LABEL_H_ */

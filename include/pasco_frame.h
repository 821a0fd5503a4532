/*
 * pasco_frame.h -- flat C ABI of the frame-preparation kernels in libpascohip.so (pasco_amd/csrc/frame.hip).
 *
 * A frame (raw points + the labelled completion grids) becomes the input of one scene: point features, the voxel index
 * of every point under each subnet's rigid transform, and each subnet's completion bounds min_C / max_C.  The host
 * restatements are pasco_amd/data/semantic_kitti.py (`build_item`) and pasco_amd/data/kitti360.py
 * (`build_item_kitti360`); these entry points reproduce them bit for bit.  A separate surface from include/pasco_hip.h:
 * own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_hip.h): device pointers unless named `h_*`; all work is enqueued on `stream`; no call
 * synchronises or allocates; return 0 = ok, text of a failure via pf_last_error().
 *
 * Numerics (every kernel is compiled with FP contraction off):
 *   crop        lo <= v < hi per axis; each bound compares in fp32 (bound rounded to fp32) or in fp64 (pf_points_args).
 *   voxel       (double(v) - origin) floor-divided by the voxel size as numpy's npy_divmod does it in fp64.
 *   radius      sqrtf((x*x + y*y) + z*z) in fp32.
 *   centre      fp32 ((float(c) + 0.5f) * float(voxel)) + origin, or all fp64; dx = float(double(v) - centre).
 *   transform   metres: fp64 coordinates -> (c * 0.2 + 0.1) in fp64, + float(min_bound) in fp64, rounded to fp32;
 *               int64 coordinates -> float(c) * 0.2f + 0.1f + min_bound in fp32.  Then new_i = fmaf chain over
 *               k = 0..3 of T[i][k] * h[k] starting from 0, ((new_i - min_bound_i) - 0.1f) / 0.2f, rintf.
 */
#ifndef PASCO_FRAME_H_
#define PASCO_FRAME_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_FN(name) pf_##name

#define PF_ABI_VERSION 1
#define PF_MAX_SEGMENTS 4   /* pass-through column segments of pf_points */
#define PF_MAX_M 8          /* transforms per call */
#define PF_BOUNDS 12        /* int32 per subnet written by pf_label_bounds */

/* One run of pass-through feature columns: column j (0 <= j < width) of point p is ptr[p * row_stride + j * col_stride]
 * (fp32, device).  A transposed [width, P] array has row_stride 1 and col_stride P. */
typedef struct {
  const float *ptr;
  int64_t row_stride;
  int64_t col_stride;
  int32_t width;
} pf_segment;

typedef struct {
  double lo[3], hi[3];   /* crop extent */
  int32_t lo_fp64[3];    /* 1: compare against lo in fp64, 0: in fp32 */
  int32_t hi_fp64[3];
  double origin[3];      /* voxel grid origin (metres) */
  double voxel;          /* voxel size (metres) */
  int32_t centre_fp64;   /* 1: voxel centre in fp64, 0: in fp32 */
  int32_t n_pre;         /* segments [0, n_pre) go before the radius, [n_pre, n_seg) after it */
  int32_t n_seg;
  pf_segment seg[PF_MAX_SEGMENTS];
} pf_points_args;

int PF_FN(abi_version)(void);
const char *PF_FN(last_error)(void);

/* Feature row width: sum of segment widths + 1 (radius) + 6 (dx, dy, dz, x, y, z). */
int32_t PF_FN(points_channels)(const pf_points_args *h_args);
/* Scratch bytes of pf_points for P points. */
int64_t PF_FN(points_workspace_bytes)(int64_t n_points);

/* One pass over raw points pts fp32 [P, 4] (x, y, z, w; w is read only through a segment).
 * The points inside the crop extent are compacted in input order (stable; kept count K written to d_kept[0]):
 *   feat  fp32 [P, C] rows [pre segments..., radius, post segments..., dx, dy, dz, x, y, z], rows >= K untouched
 *   voxel fp64 [P, 3] the floor-divided voxel index (the host's `coords`), rows >= K untouched
 *   src   int32 [P] input row of each kept row (nullable)
 * ws: pf_points_workspace_bytes(P). */
int PF_FN(points)(const float *pts, int64_t n_points, const pf_points_args *h_args, float *feat, double *voxel,
                  int32_t *src, int64_t *d_kept, void *ws, int64_t ws_bytes, void *stream);

/* transform_coords (data/semantic_kitti.py) of n coordinates under M transforms (h_T fp32 [M, 4, 4], row major, host).
 * coords: fp64 [n, 3] (coords_int64 = 0) or int64 [n, 3] (coords_int64 = 1).  Rows i >= d_n[0] are skipped when d_n is
 * not null.  out int64 [M, n, 3].  Domain: results inside int32; the cast of a larger value is undefined. */
int PF_FN(transform_coords)(const void *coords, int32_t coords_int64, int64_t n, const int64_t *d_n, const float *h_T,
                            int32_t M, int64_t *out, void *stream);

/* Completion bounds of M subnets (build_item's min_C / max_C before the rounding to the completion scale) without the
 * resampled label grids.  sem / ins uint8 [X, Y, Z] (255 = unknown / no label).  h_T, h_Tinv fp32 [M, 4, 4] (host;
 * h_Tinv = torch.inverse(T)).  h_box_bound int32 [M, 6]: a host-side upper bound on each subnet's sample box
 * (lo xyz, hi xyz); it only sizes the launch of the second pass.
 *   out int32 [M, PF_BOUNDS]: box lo xyz, box hi xyz (transformed known voxels), lo xyz, hi xyz over the surviving
 *   samples.  An empty set leaves lo = INT32_MAX, hi = INT32_MIN.
 * ws: pf_bounds_workspace_bytes(M), no other requirement. */
int64_t PF_FN(bounds_workspace_bytes)(int32_t M);
int PF_FN(label_bounds)(const uint8_t *sem, const uint8_t *ins, int32_t X, int32_t Y, int32_t Z, const float *h_T,
                        const float *h_Tinv, int32_t M, const int32_t *h_box_bound, int32_t *out, void *ws,
                        int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_FRAME_H_ */

/*
 * pasco_view.h -- flat C ABI of the visualisation kernels in libpascohip.so (pasco_amd/csrc/view.hip).
 *
 * The outputs of a scored frame (panoptic grid, segment table, semantic arg-max, confidence grid) become images without
 * leaving the device: grid passes (majority pooling, a 3 x 3 x 3 window filter), one pass that turns the outputs into a grid
 * of colour indices per view, and a ray caster over that grid.  The host restatement is pasco_amd/viz/host.py; these entry
 * points reproduce it exactly - every integer, every byte and, for the filter, every fp32 bit.  A separate surface from
 * include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_label.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pv_last_error().  Grids are [X, Y, Z] with z
 * fastest: site of (x, y, z) = (x*Y + y)*Z + z, X*Y*Z < 2^31.  `d_status` is one int32 the caller zeroes; kernels OR
 * PV_STATUS_* bits into it instead of reading out of bounds.
 *
 * Three documented differences from the program these passes replace (a script that pickles a frame and one that draws it):
 *   1. that script pools the already pooled grid again (256 -> 128 -> 32) while it names the result "scale 4"; here every
 *      scale is pooled from the full grid (256 -> 64 for k = 4).
 *   2. its window filter is handed a 4-D array [1, X, Y, Z], so its three loops run over (1, X, Y) and each "window" is
 *      3 x 3 in (x, y) over the WHOLE z column, written to the whole column.  pv_window_filter is the 3-D filter the name
 *      says: 3 x 3 x 3 around the voxel, clipped at the borders.
 *   3. its mask view numbers every segment, stuff included; here `mask` shows things only, numbered as in `panoptic`.
 */
#ifndef PASCO_VIEW_H_
#define PASCO_VIEW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_FN(name) pv_##name

#define PV_ABI_VERSION 1
#define PV_MAX_LABEL 32       /* pv_majority_pool: labels are 0 .. 31 or 255 */
#define PV_MAX_SEGMENTS 128   /* pv_compose: entries of the segment table */
#define PV_SEG_ROWS 4         /* id, isthing, category, confidence (fp32 bits), each int32 [n_seg] */
#define PV_BRICK 8            /* pv_bricks / pv_render: a brick is 8 x 8 x 8 voxels, clipped at the grid's far faces */
#define PV_SENTINEL 255.0f    /* pv_window_filter: a voxel holding exactly this value is in no window */

#define PV_STATUS_LABEL_RANGE 1   /* pv_majority_pool: a label in 32 .. 254 (counted as 255) */
#define PV_STATUS_STEP_CAP 2      /* pv_render: a ray reached its step cap (that pixel is written as a miss) */
#define PV_STATUS_PALETTE 4       /* pv_render: a colour index >= n_palette (drawn with the last palette entry) */

/* pv_window_filter operations */
#define PV_OP_MEDIAN 0
#define PV_OP_MAX 1
#define PV_OP_AVG 2

/* pv_compose views and the layout of the colour indices they write (0 = empty) */
#define PV_VIEW_SEMANTIC 0
#define PV_VIEW_PANOPTIC 1
#define PV_VIEW_MASK 2
#define PV_VIEW_VOX_CONF 3
#define PV_VIEW_INS_CONF 4
#define PV_INSTANCE_BASE 32   /* the r-th thing of the segment table (r from 1) has index PV_INSTANCE_BASE + r - 1 */
#define PV_RAMP_BASE 1        /* confidence level q in 0 .. 255 has index PV_RAMP_BASE + q */
#define PV_STUFF_FIRST 9      /* panoptic view: semantic classes PV_STUFF_FIRST .. PV_STUFF_LAST are drawn as stuff */
#define PV_STUFF_LAST 19

/* pv_render faces: 2*axis for the face of smaller coordinate (entered moving in +axis), 2*axis + 1 for the other one;
 * PV_FACE_INSIDE when the ray starts inside the grid in an occupied voxel (no face was crossed); PV_FACE_NONE on a miss */
#define PV_FACE_INSIDE 6
#define PV_FACE_NONE 255

int PV_FN(abi_version)(void);
const char *PV_FN(last_error)(void);

/* grid uint8 [X, Y, Z], k in {2, 4, 8} -> out uint8 [X/k, Y/k, Z/k] (floor; a remainder at the far faces is ignored).
 * Per cell of k^3 voxels: among its labels that are neither 0 nor 255 the most frequent one, ties to the smallest label;
 * with no such label 0 if the cell holds a 0, else 255.  A label in 32 .. 254 counts as 255 and ORs PV_STATUS_LABEL_RANGE. */
int PV_FN(majority_pool)(const uint8_t *grid, int32_t X, int32_t Y, int32_t Z, int32_t k, uint8_t *out, int32_t *d_status,
                         void *stream);

/* in fp32 [X, Y, Z], mask uint8 [X, Y, Z] or NULL -> out fp32 [X, Y, Z] (may not alias in).  A voxel is valid when its
 * value != PV_SENTINEL and (mask == NULL or mask != 0).  out(x, y, z) over the valid voxels of the 3 x 3 x 3 window around
 * it, clipped at the borders, visited in raster order (x, then y, then z fastest):
 *   PV_OP_MEDIAN  the middle one of the sorted values; for an even count (a + b) * 0.5f of the two middle ones
 *   PV_OP_MAX     the largest
 *   PV_OP_AVG     ((0.0f + v0) + v1 + ...) / (float)count, every operation rounded to fp32
 * and PV_SENTINEL where the window holds no valid voxel.  Values must not be NaN. */
int PV_FN(window_filter)(const float *in, const uint8_t *mask, int32_t X, int32_t Y, int32_t Z, int32_t op, float *out,
                         void *stream);

/* One colour-index grid out uint32 [X, Y, Z] for `view`.  Inputs (those a view does not read may be NULL):
 *   panoptic int32 [X, Y, Z]; seg int32 [PV_SEG_ROWS, n_seg], 0 <= n_seg <= PV_MAX_SEGMENTS (NULL when 0);
 *   sem uint8 [X, Y, Z]; conf fp32 [X, Y, Z].
 * s(v) = the first segment whose id equals panoptic(v) when panoptic(v) != 0 (none: the voxel belongs to no segment);
 * rank(s) = the number of things among segments 0 .. s.  q(c) with fp32 operations, one rounding each:
 *   vmax > vmin:  t = (c - vmin) / (vmax - vmin); t = t > 0 ? t : 0; t = t < 1 ? t : 1; q = (int)(t * 255.0f + 0.5f)
 *   otherwise     q = 0                                                        (nothing is divided by zero)
 *   SEMANTIC  sem where sem is neither 0 nor 255                                               (reads sem)
 *   PANOPTIC  PV_INSTANCE_BASE + rank(s) - 1 where s is a thing; else sem where sem is in 9 .. 19  (panoptic, seg, sem)
 *   MASK      PV_INSTANCE_BASE + rank(s) - 1 where s is a thing                                (panoptic, seg)
 *   VOX_CONF  PV_RAMP_BASE + q(conf) where sem != 0                                            (sem, conf)
 *   INS_CONF  PV_RAMP_BASE + q(confidence of s) where s is a thing                             (panoptic, seg)
 * and 0 everywhere else. */
int PV_FN(compose)(const int32_t *panoptic, const int32_t *seg, int32_t n_seg, const uint8_t *sem, const float *conf,
                   int32_t X, int32_t Y, int32_t Z, int32_t view, float vmin, float vmax, uint32_t *out, void *stream);

/* Number of uint32 words pv_bricks writes for an [X, Y, Z] grid: ceil(NBX*NBY*NBZ / 32), NB* = ceil(* / PV_BRICK). */
int64_t PV_FN(brick_words)(int32_t X, int32_t Y, int32_t Z);

/* colour uint32 [X, Y, Z] -> bits uint32 [pv_brick_words]: bit (b & 31) of word (b >> 5) is set when brick
 * b = (bx*NBY + by)*NBZ + bz holds a non-zero voxel; every word is written whole, unused bits 0. */
int PV_FN(bricks)(const uint32_t *colour, int32_t X, int32_t Y, int32_t Z, uint32_t *bits, void *stream);

/* One ray per pixel of a W x H image through the colour grid (voxel (x, y, z) is the unit cube [x, x+1) x ..., so the
 * camera lives in voxel units).  cam fp32 [12] on the device: origin o, then d0, du, dv; the ray of pixel (i, j) (column i,
 * row j) is o + t*d, d = (d0 + (float)i*du) + (float)j*dv per component, not normalised.  Only + - * / in fp32, compiled
 * with FP contraction off; one reciprocal per axis and ray.
 *   hit  int32 [H, W]     site of the first non-zero voxel along the ray, -1 on a miss
 *   face uint8 [H, W]     the face through which that voxel was entered (see PV_FACE_*)
 *   rgb  uint8 [H, W, 3]  (palette[index] * factor[axis of the face]) >> 8 per channel, factor[2] for PV_FACE_INSIDE;
 *                         `background` on a miss
 * palette uint8 [n_palette, 3], n_palette >= 1; the face factors fx, fy, fz are 0 .. 256; background = r | g << 8 | b << 16.
 *
 * The walk (pasco_amd/viz/host.py `render` is the same sequence of operations):
 *   - an axis with d == 0 takes no step; the ray misses when o lies outside [0, extent) on that axis;
 *   - the ray enters at t0 = max(0, largest near-plane t) and misses unless t0 <= smallest far-plane t;
 *   - the start cell is floor(o + t0*d) clamped into the grid (on the entry axis: the first or last layer);
 *   - in a brick whose bit is set it walks voxels (Amanatides-Woo): the next plane on axis a is crossed at
 *     ((float)plane - o[a]) * inv[a], computed from the integer cell, never accumulated; the smallest wins, ties x, y, z;
 *   - in a brick whose bit is clear it crosses to the next brick the same way and re-derives the cell from o + t*d, clamped
 *     into that brick.
 * Steps are capped at X + Y + Z + 3 voxel steps and NBX + NBY + NBZ + 3 brick steps (a positive `step_cap` lowers both);
 * a ray that reaches a cap ORs PV_STATUS_STEP_CAP and is written as a miss.  No loop is unbounded. */
int PV_FN(render)(const uint32_t *colour, const uint32_t *bits, int32_t X, int32_t Y, int32_t Z, const float *cam,
                  int32_t W, int32_t H, const uint8_t *palette, int32_t n_palette, int32_t fx, int32_t fy, int32_t fz,
                  uint32_t background, int32_t step_cap, int32_t *hit, uint8_t *face, uint8_t *rgb, int32_t *d_status,
                  void *stream);

/* in uint8 [H*s, W*s, 3] -> out uint8 [H, W, 3]: (sum of the s x s block + s*s/2) / (s*s) in integers, 1 <= s <= 16. */
int PV_FN(downsample)(const uint8_t *in, int32_t W, int32_t H, int32_t s, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_VIEW_H_ */

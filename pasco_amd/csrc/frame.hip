// Frame preparation (include/pasco_frame.h): raw points -> cropped, compacted feature rows and voxel indices; voxel
// indices under M rigid transforms; the completion bounds of M subnets from the label grids.
//
// pf_points is two launches over the same split of the points into per-block chunks: k_count counts the kept points of
// each chunk, k_points takes its block's output offset from the counts of the blocks before it, compacts each tile of
// 256 points with a wave-ballot scan (input order is kept) and copies the rows, one wave per row.  pf_label_bounds is a
// fill, a pass over the grid (the box of the transformed known voxels) and a pass over that box (every sample mapped
// back with T^-1).  Both reduce in registers, then across the block through LDS, then one integer atomic per block and
// value: min / max are order independent, so results are identical from run to run.  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_frame.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = 2048;

#include "transform_chain.h"   // MINB, apply_T, metres_f64, metres_i64 (shared with target.hip)

struct Mats {
  float t[PF_MAX_M][16];
};

// ---- numerics -----------------------------------------------------------------------------------------------
// npy_divmod's floor division in fp64 (numpy/_core/src/npymath/npy_math_internal.h.src)
__device__ __forceinline__ double floor_div(double a, double b) {
  double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0) {
    if ((b < 0.0) != (mod < 0.0)) div -= 1.0;
  }
  double fl;
  if (div != 0.0) {
    fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
  } else {
    fl = copysign(0.0, a / b);
  }
  return fl;
}

__device__ __forceinline__ bool ge_bound(float v, double lo, int fp64) {
  return fp64 ? (static_cast<double>(v) >= lo) : (v >= static_cast<float>(lo));
}

__device__ __forceinline__ bool lt_bound(float v, double hi, int fp64) {
  return fp64 ? (static_cast<double>(v) < hi) : (v < static_cast<float>(hi));
}

__device__ __forceinline__ bool keep_point(const float *p, const pf_points_args &a) {
  bool k = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) k = k && ge_bound(p[d], a.lo[d], a.lo_fp64[d]) && lt_bound(p[d], a.hi[d], a.hi_fp64[d]);
  return k;
}

// ---- pf_points ----------------------------------------------------------------------------------------------
__device__ __forceinline__ void chunk_of(int64_t n, int nb, int b, int64_t &beg, int64_t &end) {
  int64_t tiles = (n + BLOCK - 1) / BLOCK;
  int64_t per = (tiles + nb - 1) / nb;
  beg = b * per * BLOCK;
  end = beg + per * BLOCK;
  if (beg > n) beg = n;
  if (end > n) end = n;
}

__device__ __forceinline__ int block_sum(int v, int *lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) lds[w] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) s += lds[i];
  return s;
}

__global__ __launch_bounds__(BLOCK) void k_count(const float *__restrict__ pts, int64_t n, pf_points_args a,
                                                 int *__restrict__ counts) {
  __shared__ int lds[WAVES];
  int64_t beg, end;
  chunk_of(n, gridDim.x, blockIdx.x, beg, end);
  int c = 0;
  for (int64_t i = beg + threadIdx.x; i < end; i += BLOCK) c += keep_point(pts + i * 4, a) ? 1 : 0;
  c = block_sum(c, lds);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// one feature value: column c of the row of input point p (radius / dxyz / xyz from the tile's LDS row `r`)
__device__ __forceinline__ float column(const pf_points_args &a, int64_t p, int c, const float *r) {
  int j = c;
  // unrolled: the segment table stays in kernel-argument registers (a dynamic index would copy it to scratch)
#pragma unroll
  for (int s = 0; s < PF_MAX_SEGMENTS; ++s) {
    if (s == a.n_pre) {
      if (j == 0) return r[0];
      j -= 1;
    }
    if (s < a.n_seg) {
      if (j < a.seg[s].width) return a.seg[s].ptr[p * a.seg[s].row_stride + j * a.seg[s].col_stride];
      j -= a.seg[s].width;
    }
  }
  if (a.n_pre == PF_MAX_SEGMENTS) {
    if (j == 0) return r[0];
    j -= 1;
  }
  return r[1 + j];
}

__global__ __launch_bounds__(BLOCK) void k_points(const float *__restrict__ pts, int64_t n, pf_points_args a, int C,
                                                  const int *__restrict__ counts, float *__restrict__ feat,
                                                  double *__restrict__ voxel, int32_t *__restrict__ src,
                                                  int64_t *__restrict__ d_kept) {
  __shared__ int lds[WAVES];
  __shared__ int wave_base[WAVES + 1];
  __shared__ int row_src[BLOCK];
  __shared__ float row_val[BLOCK][8];   // radius, dx, dy, dz, x, y, z (+ pad)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

  // offset of this block: the kept points of the blocks before it
  int pre = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += BLOCK) pre += counts[b];
  int64_t base = block_sum(pre, lds);

  int64_t beg, end;
  chunk_of(n, gridDim.x, blockIdx.x, beg, end);
  for (int64_t t0 = beg; t0 < end; t0 += BLOCK) {
    int64_t i = t0 + threadIdx.x;
    float p[3] = {0.f, 0.f, 0.f};
    bool k = false;
    if (i < end) {
      p[0] = pts[i * 4 + 0];
      p[1] = pts[i * 4 + 1];
      p[2] = pts[i * 4 + 2];
      k = keep_point(p, a);
    }
    unsigned long long m = __ballot(k);
    int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();   // the previous tile's rows are written out
    if (lane == 0) lds[w] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int q = 0; q < WAVES; ++q) {
        wave_base[q] = s;
        s += lds[q];
      }
      wave_base[WAVES] = s;
    }
    __syncthreads();
    const int tile_kept = wave_base[WAVES];
    if (k) {
      int r = wave_base[w] + in_wave;
      int64_t o = base + r;
      row_src[r] = static_cast<int>(i - t0);
      float *v = row_val[r];
      v[0] = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        double q = floor_div(static_cast<double>(p[d]) - a.origin[d], a.voxel);
        double centre = a.centre_fp64
                            ? (q + 0.5) * a.voxel + a.origin[d]
                            : static_cast<double>((static_cast<float>(q) + 0.5f) * static_cast<float>(a.voxel)) + a.origin[d];
        v[1 + d] = static_cast<float>(static_cast<double>(p[d]) - centre);
        v[4 + d] = p[d];
        voxel[o * 3 + d] = q;
      }
      if (src) src[o] = static_cast<int32_t>(i);
    }
    __syncthreads();
    for (int r = w; r < tile_kept; r += WAVES) {
      int64_t ip = t0 + row_src[r];
      float *dst = feat + (base + r) * C;
      for (int c = lane; c < C; c += 64) dst[c] = column(a, ip, c, row_val[r]);
    }
    base += tile_kept;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) d_kept[0] = base;
}

// ---- pf_transform_coords -----------------------------------------------------------------------------------
template <bool I64>
__global__ __launch_bounds__(BLOCK) void k_transform(const void *__restrict__ coords, int64_t n,
                                                     const int64_t *__restrict__ d_n, Mats T, int M,
                                                     int64_t *__restrict__ out) {
  int64_t lim = d_n ? d_n[0] : n;
  if (lim > n) lim = n;
  for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < lim; i += (int64_t)gridDim.x * BLOCK) {
    float h[3];
    if (I64) {
      const int64_t *c = static_cast<const int64_t *>(coords) + i * 3;
      int64_t v[3] = {c[0], c[1], c[2]};
      metres_i64(v, h);
    } else {
      const double *c = static_cast<const double *>(coords) + i * 3;
      double v[3] = {c[0], c[1], c[2]};
      metres_f64(v, h);
    }
    for (int m = 0; m < M; ++m) {
      int64_t o[3];
      apply_T(T.t[m], h, o);
      int64_t *dst = out + ((int64_t)m * n + i) * 3;
      dst[0] = o[0];
      dst[1] = o[1];
      dst[2] = o[2];
    }
  }
}

// ---- pf_label_bounds ----------------------------------------------------------------------------------------
__global__ void k_bounds_init(int32_t *out, int M, int32_t *flag) {
  int t = threadIdx.x;
  if (t < M * PF_BOUNDS) {
    int j = t % PF_BOUNDS;
    out[t] = ((j / 3) % 2 == 0) ? INT32_MAX : INT32_MIN;
  }
  if (t == 0) flag[0] = 0;
}

// min over the block of v[0..5] as (min, min, min, max, max, max); thread 0 adds them to dst with integer atomics
__device__ __forceinline__ void block_minmax6(int v[6], int (*lds)[6], int32_t *dst) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    for (int o = 32; o > 0; o >>= 1) {
      int u = __shfl_down(v[j], o, 64);
      v[j] = j < 3 ? min(v[j], u) : max(v[j], u);
    }
  }
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) lds[w][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    int j = threadIdx.x;
    int r = lds[0][j];
    for (int q = 1; q < WAVES; ++q) r = j < 3 ? min(r, lds[q][j]) : max(r, lds[q][j]);
    if (j < 3) {
      if (r != INT32_MAX) atomicMin(dst + j, r);
    } else {
      if (r != INT32_MIN) atomicMax(dst + j, r);
    }
  }
}

// pass 1: box of transform_coords(known voxel, T_m); any non-zero instance id
__global__ __launch_bounds__(BLOCK) void k_bounds_box(const uint8_t *__restrict__ sem, const uint8_t *__restrict__ ins,
                                                      int X, int Y, int Z, Mats T, int M, int32_t *__restrict__ out,
                                                      int32_t *__restrict__ flag) {
  __shared__ int lds[WAVES][6];
  const int64_t S = (int64_t)X * Y * Z;
  const int m = blockIdx.y;
  int v[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
  bool any_ins = false;
  for (int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x; s < S; s += (int64_t)gridDim.x * BLOCK) {
    if (m == 0) any_ins = any_ins || ins[s] != 0;
    if (sem[s] == 255) continue;
    int64_t c[3] = {s / ((int64_t)Y * Z), (s / Z) % Y, s % Z};
    float h[3];
    metres_i64(c, h);
    int64_t o[3];
    apply_T(T.t[m], h, o);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = min(v[d], (int)o[d]);
      v[3 + d] = max(v[3 + d], (int)o[d]);
    }
  }
  if (m == 0 && __any(any_ins) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
  block_minmax6(v, lds, out + m * PF_BOUNDS);
}

// pass 2: every sample of the box mapped back with T_m^-1; it counts where it lands inside the grid on sem != 255, or
// (frames with an instance) on ins != 255
__global__ __launch_bounds__(BLOCK) void k_bounds_samples(const uint8_t *__restrict__ sem, const uint8_t *__restrict__ ins,
                                                          int X, int Y, int Z, Mats Tinv, int M,
                                                          int32_t *__restrict__ out, const int32_t *__restrict__ flag) {
  __shared__ int lds[WAVES][6];
  const int m = blockIdx.y;
  const int32_t *box = out + m * PF_BOUNDS;
  int v[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
  const bool has_ins = flag[0] != 0;
  const int64_t lo[3] = {box[0], box[1], box[2]};
  const int64_t ext[3] = {(int64_t)box[3] - box[0] + 1, (int64_t)box[4] - box[1] + 1, (int64_t)box[5] - box[2] + 1};
  const bool empty = box[0] == INT32_MAX;
  const int64_t V = empty ? 0 : ext[0] * ext[1] * ext[2];
  for (int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x; s < V; s += (int64_t)gridDim.x * BLOCK) {
    int64_t c[3] = {lo[0] + s / (ext[1] * ext[2]), lo[1] + (s / ext[2]) % ext[1], lo[2] + s % ext[2]};
    float h[3];
    metres_i64(c, h);
    int64_t b[3];
    apply_T(Tinv.t[m], h, b);
    if (b[0] < 0 || b[0] >= X || b[1] < 0 || b[1] >= Y || b[2] < 0 || b[2] >= Z) continue;
    int64_t site = (b[0] * Y + b[1]) * Z + b[2];
    bool hit = sem[site] != 255 || (has_ins && ins[site] != 255);
    if (!hit) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = min(v[d], (int)c[d]);
      v[3 + d] = max(v[3 + d], (int)c[d]);
    }
  }
  block_minmax6(v, lds, out + m * PF_BOUNDS + 6);
}

int grid_for(int64_t work) {
  int64_t b = (work + BLOCK - 1) / BLOCK;
  if (b < 1) b = 1;
  return static_cast<int>(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" {

SIDE_EXPORTS(PF_FN, PF_ABI_VERSION)

int32_t PF_FN(points_channels)(const pf_points_args *a) {
  int32_t c = 7;
  for (int s = 0; s < a->n_seg; ++s) c += a->seg[s].width;
  return c;
}

int64_t PF_FN(points_workspace_bytes)(int64_t n) { return (int64_t)grid_for(n) * (int64_t)sizeof(int); }

int PF_FN(points)(const float *pts, int64_t n, const pf_points_args *h_args, float *feat, double *voxel, int32_t *src,
                  int64_t *d_kept, void *ws, int64_t ws_bytes, void *stream) {
  if (!h_args || !d_kept) return fail("pf_points: null argument");
  const pf_points_args &a = *h_args;
  if (n < 0 || n > INT32_MAX) return fail("pf_points: n_points %lld out of range", (long long)n);
  if (a.n_seg < 0 || a.n_seg > PF_MAX_SEGMENTS || a.n_pre < 0 || a.n_pre > a.n_seg)
    return fail("pf_points: %d segments (%d before the radius)", a.n_seg, a.n_pre);
  for (int s = 0; s < a.n_seg; ++s)
    if ((n > 0 && !a.seg[s].ptr) || a.seg[s].width <= 0) return fail("pf_points: segment %d is empty", s);
  if (!(a.voxel > 0.0)) return fail("pf_points: voxel size must be > 0");
  if (n > 0 && (!pts || !feat || !voxel)) return fail("pf_points: null array");
  int nb = grid_for(n);
  if (ws_bytes < (int64_t)nb * (int64_t)sizeof(int)) return fail("pf_points: workspace of %lld bytes < %lld", (long long)ws_bytes,
                                                                 (long long)nb * (long long)sizeof(int));
  hipStream_t st = static_cast<hipStream_t>(stream);
  int *counts = static_cast<int *>(ws);
  const int C = PF_FN(points_channels)(h_args);
  hipLaunchKernelGGL(k_count, dim3(nb), dim3(BLOCK), 0, st, pts, n, a, counts);
  SIDE_CHECK_LAUNCH("k_count");
  hipLaunchKernelGGL(k_points, dim3(nb), dim3(BLOCK), 0, st, pts, n, a, C, counts, feat, voxel, src, d_kept);
  SIDE_CHECK_LAUNCH("k_points");
  return 0;
}

int PF_FN(transform_coords)(const void *coords, int32_t coords_int64, int64_t n, const int64_t *d_n, const float *h_T,
                            int32_t M, int64_t *out, void *stream) {
  if (M < 1 || M > PF_MAX_M) return fail("pf_transform_coords: M = %d outside 1..%d", M, PF_MAX_M);
  if (n < 0) return fail("pf_transform_coords: n < 0");
  if (!h_T) return fail("pf_transform_coords: null transform");
  if (n == 0) return 0;
  if (!coords || !out) return fail("pf_transform_coords: null array");
  Mats T;
  for (int m = 0; m < M; ++m)
    for (int j = 0; j < 16; ++j) T.t[m][j] = h_T[m * 16 + j];
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (coords_int64)
    hipLaunchKernelGGL(k_transform<true>, dim3(grid_for(n)), dim3(BLOCK), 0, st, coords, n, d_n, T, M, out);
  else
    hipLaunchKernelGGL(k_transform<false>, dim3(grid_for(n)), dim3(BLOCK), 0, st, coords, n, d_n, T, M, out);
  SIDE_CHECK_LAUNCH("k_transform");
  return 0;
}

int64_t PF_FN(bounds_workspace_bytes)(int32_t) { return 64; }

int PF_FN(label_bounds)(const uint8_t *sem, const uint8_t *ins, int32_t X, int32_t Y, int32_t Z, const float *h_T,
                        const float *h_Tinv, int32_t M, const int32_t *h_box_bound, int32_t *out, void *ws,
                        int64_t ws_bytes, void *stream) {
  if (M < 1 || M > PF_MAX_M) return fail("pf_label_bounds: M = %d outside 1..%d", M, PF_MAX_M);
  if (X <= 0 || Y <= 0 || Z <= 0) return fail("pf_label_bounds: empty grid %d x %d x %d", X, Y, Z);
  if (!sem || !ins || !out || !ws || !h_T || !h_Tinv || !h_box_bound) return fail("pf_label_bounds: null argument");
  if (ws_bytes < PF_FN(bounds_workspace_bytes)(M)) return fail("pf_label_bounds: workspace too small");
  Mats T, Ti;
  int64_t vmax = 1;
  for (int m = 0; m < M; ++m) {
    for (int j = 0; j < 16; ++j) {
      T.t[m][j] = h_T[m * 16 + j];
      Ti.t[m][j] = h_Tinv[m * 16 + j];
    }
    int64_t v = 1;
    for (int d = 0; d < 3; ++d) {
      int64_t e = (int64_t)h_box_bound[m * 6 + 3 + d] - h_box_bound[m * 6 + d] + 1;
      if (e <= 0) return fail("pf_label_bounds: box bound of subnet %d is empty on axis %d", m, d);
      v *= e;
    }
    if (v > vmax) vmax = v;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t *flag = static_cast<int32_t *>(ws);
  hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(BLOCK), 0, st, out, M, flag);
  SIDE_CHECK_LAUNCH("k_bounds_init");
  const int64_t S = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_bounds_box, dim3(grid_for(S), M), dim3(BLOCK), 0, st, sem, ins, X, Y, Z, T, M, out, flag);
  SIDE_CHECK_LAUNCH("k_bounds_box");
  hipLaunchKernelGGL(k_bounds_samples, dim3(grid_for(vmax), M), dim3(BLOCK), 0, st, sem, ins, X, Y, Z, Ti, M, out, flag);
  SIDE_CHECK_LAUNCH("k_bounds_samples");
  return 0;
}

}  // extern "C"

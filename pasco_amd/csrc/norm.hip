// Training-mode batch normalisation over feature rows for gfx950 (include/pasco_norm.h).
//
// Every row kernel has one geometry.  A workgroup of 256 threads owns PN_TILE_ROWS consecutive rows and one chunk of channels.
// Lanes run along the channels: with V = 4 floats per access where c % 4 == 0 and the row pointers are 16-byte aligned (V = 1
// otherwise) a row has cu = c / V units, L = min(64, next power of two >= cu) neighbouring threads take the units of one row and
// the 256 / L thread rows step through the tile.  For c >= 256 a wave reads 1 KiB of one row per instruction; for c = 32 it
// reads eight whole rows, which are contiguous too.  A thread keeps its channels for the whole tile, so the per-channel
// constants are loaded once and the per-channel sums stay in registers.
//
// Reductions: thread -> LDS -> the thread row 0 adds the 256 / L partials of its channels in ascending thread-row order ->
// one fp64 record per tile in the workspace.  The combine over the tiles is a launch of its own (a channel's records folded by
// one thread in ascending tile order): no atomics, no ticket, no fence; the launch boundary orders the partials.  The statistics are fp64
// throughout: the kernels are memory bound (4 - 6 fp64 operations per loaded float).
//
// k_tile_moments reads its tile twice: the sum first, then M2 about the tile's own mean.  The second read is served by the L2
// (a tile chunk is at most 128 KiB), so the rows cross the HBM interface once here and once in k_apply.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_hip.h"
#include "../../include/pasco_norm.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int TILE = PN_TILE_ROWS;

// How the threads of a workgroup lie over (row, channel unit).
struct Geo {
  int L;        // threads along the channel units of a row: a power of two, 1 .. 64
  int R;        // thread rows: BLOCK / L
  int cu;       // units per row: c / V
};

template <int V>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float *p) { v[0] = *p; }
  __device__ __forceinline__ void store(float *p) const { *p = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float *p) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// The channels and rows of one thread.
struct Mine {
  int lx, ry;
  int64_t ch;           // first channel (only meaningful where `on`)
  bool on;              // the thread has channels
  int64_t r0, r1;       // the tile's rows [r0, r1)
};

template <int V>
__device__ __forceinline__ Mine mine(Geo g, int64_t n) {
  Mine m;
  m.lx = threadIdx.x & (g.L - 1);
  m.ry = threadIdx.x / g.L;
  const int64_t u = (int64_t)blockIdx.y * g.L + m.lx;
  m.on = u < g.cu;
  m.ch = u * V;
  m.r0 = (int64_t)blockIdx.x * TILE;
  m.r1 = m.r0 + TILE < n ? m.r0 + TILE : n;
  return m;
}

// Per-channel constants of the normalisation.
template <int V>
struct Chan {
  float mean[V], rstd[V], w[V], b[V];
  __device__ __forceinline__ void load(const float *mean_rstd, const float *weight, const float *bias, int64_t ch, int c) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      mean[j] = mean_rstd[ch + j];
      rstd[j] = mean_rstd[c + ch + j];
      w[j] = weight != nullptr ? weight[ch + j] : 1.f;
      b[j] = bias != nullptr ? bias[ch + j] : 0.f;
    }
  }
};

// The one expression of xhat and z: forward and backward evaluate exactly this (no contraction in this file).
__device__ __forceinline__ float xhat_of(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float z_of(float xh, float w, float b) { return xh * w + b; }

__device__ __forceinline__ float act_fwd(float z, int act, float slope) {
  if (act == PH_ACT_RELU) return z > 0.f ? z : 0.f;
  if (act == PH_ACT_LEAKY) return z > 0.f ? z : slope * z;
  return z;
}
__device__ __forceinline__ float act_bwd(float z, int act, float slope) {
  if (act == PH_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == PH_ACT_LEAKY) return z > 0.f ? 1.f : slope;
  return 1.f;
}

// Adds the V values of every thread over the thread rows, in ascending thread-row order; the result is valid in thread row 0.
// `red` is BLOCK * V doubles.  Ends with no barrier: a caller that reuses `red` synchronises first.
template <int V>
__device__ __forceinline__ void reduce_rows(double *red, Geo g, const Mine &m, double (&acc)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j) red[(m.ry * g.L + m.lx) * V + j] = acc[j];
  __syncthreads();
  if (m.ry == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      double s = red[m.lx * V + j];
      for (int r = 1; r < g.R; ++r) s += red[(r * g.L + m.lx) * V + j];
      acc[j] = s;
    }
  }
}

template <int V>
__global__ void __launch_bounds__(BLOCK) k_tile_moments(const float *__restrict__ x, int64_t n, int c, Geo g, double *__restrict__ part) {
  __shared__ double red[BLOCK * V];
  __shared__ double mean_s[64 * V];
  const Mine m = mine<V>(g, n);
  const double cnt = (double)(m.r1 - m.r0);      // >= 1: the grid has no empty tile

  double acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.0;
  if (m.on)
    for (int64_t r = m.r0 + m.ry; r < m.r1; r += g.R) {
      Vec<V> t;
      t.load(x + r * c + m.ch);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += (double)t.v[j];
    }
  reduce_rows<V>(red, g, m, acc);
  if (m.ry == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) mean_s[m.lx * V + j] = acc[j] / cnt;
  }
  __syncthreads();

  double mu[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mu[j] = mean_s[m.lx * V + j], acc[j] = 0.0;
  if (m.on)
    for (int64_t r = m.r0 + m.ry; r < m.r1; r += g.R) {
      Vec<V> t;
      t.load(x + r * c + m.ch);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double d = (double)t.v[j] - mu[j];
        acc[j] += d * d;
      }
    }
  reduce_rows<V>(red, g, m, acc);
  if (m.ry == 0 && m.on) {
    double *p = part + (int64_t)blockIdx.x * 3 * c + m.ch;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      p[j] = cnt;
      p[c + j] = mu[j];
      p[2 * (int64_t)c + j] = acc[j];
    }
  }
}

// The combine kernels fold the records of a channel in ascending order - a chain of dependent fp64 operations that nothing can
// shorten - so everything that is NOT on the chain is taken off it.  A workgroup owns MERGE_CH channels and stages MERGE_K
// records per pass: thread (k, channel) loads record k of the pass (the loads of the next pass are issued before this pass is
// worked on), and for the moments forms the running count in front of its record (a scan; counts are integers in fp64: exact
// in any order) and the record's two weights, one division per thread, side by side.  Thread row 0 then folds the pass from
// LDS: per record a subtraction, a product and a sum on the mean's chain.
constexpr int MERGE_CH = 8;
constexpr int MERGE_K = BLOCK / MERGE_CH;

// THE merge rule of moments records (include/pasco_norm.h): pn_moments runs it over its tiles, pn_moments_merge over records.
// A record without rows is staged as (w, mean, M2, n_a * w) = (0, 0, 0, 0): d * 0 and (d * d) * 0 are zeros and adding them
// changes nothing, so the fold needs no branch and no select.
__global__ void __launch_bounds__(BLOCK) k_moments_merge(const double *__restrict__ recs, int r, int c, double *__restrict__ out) {
  __shared__ double s_m[BLOCK], s_q[BLOCK], s_w[BLOCK], s_nw[BLOCK];
  __shared__ double s_tot[(BLOCK / 64) * MERGE_CH];
  const int tid = threadIdx.x;
  const int k = tid / MERGE_CH, cl = tid % MERGE_CH;
  const int lane = tid & 63, wave = tid >> 6;
  const int ch = blockIdx.x * MERGE_CH + cl;
  const bool on = ch < c;
  double base = 0.0, mean = 0.0, m2 = 0.0;
  double nn = 0.0, nm = 0.0, nq = 0.0;      // the record of the NEXT pass
  if (on && k < r) {
    const double *p = recs + (int64_t)k * 3 * c + ch;
    nn = p[0], nm = p[c], nq = p[2 * (int64_t)c];
  }
  for (int i0 = 0; i0 < r; i0 += MERGE_K) {
    const bool has = nn > 0.0;
    const double cn = has ? nn : 0.0;
    s_m[tid] = has ? nm : 0.0;
    s_q[tid] = has ? nq : 0.0;
    nn = 0.0, nm = 0.0, nq = 0.0;
    if (on && i0 + MERGE_K + k < r) {
      const double *p = recs + (int64_t)(i0 + MERGE_K + k) * 3 * c + ch;
      nn = p[0], nm = p[c], nq = p[2 * (int64_t)c];
    }
    // the count in front of every record: a scan over the records of the pass, per channel.  Counts are integers held in
    // fp64, so these sums are exact whatever their order.
    double incl = cn;
#pragma unroll
    for (int off = MERGE_CH; off < 64; off <<= 1) {
      const double t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane >= 64 - MERGE_CH) s_tot[wave * MERGE_CH + cl] = incl;
    __syncthreads();
    double before = base + (incl - cn);
#pragma unroll
    for (int v = 0; v < BLOCK / 64; ++v) {
      const double t = s_tot[v * MERGE_CH + cl];
      if (v < wave) before += t;
      base += t;
    }
    const double w = has ? cn / (before + cn) : 0.0;
    s_w[tid] = w;
    s_nw[tid] = before * w;
    __syncthreads();
    if (k == 0) {
      // eight records at a time from LDS into registers, then their part of the chain: a subtraction, a product and a sum
      // per record on the mean's side, two sums on M2's
      for (int j0 = 0; j0 < MERGE_K; j0 += 8) {
        double wj[8], mj[8], qj[8], nwj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int e = (j0 + j) * MERGE_CH + cl;
          wj[j] = s_w[e], mj[j] = s_m[e], qj[j] = s_q[e], nwj[j] = s_nw[e];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const double d = mj[j] - mean;
          mean = mean + d * wj[j];
          m2 = (m2 + qj[j]) + (d * d) * nwj[j];
        }
      }
    }
    __syncthreads();
  }
  if (k == 0 && on) {
    out[ch] = base;
    out[c + ch] = mean;
    out[2 * (int64_t)c + ch] = m2;
  }
}

__global__ void __launch_bounds__(BLOCK) k_sums_merge(const double *__restrict__ sums, int r, int c, double *__restrict__ out) {
  __shared__ double s_0[BLOCK], s_1[BLOCK];
  const int tid = threadIdx.x;
  const int k = tid / MERGE_CH, cl = tid % MERGE_CH;
  const int ch = blockIdx.x * MERGE_CH + cl;
  const bool on = ch < c;
  double a0 = 0.0, a1 = 0.0;
  double n0 = 0.0, n1 = 0.0;      // the record of the NEXT pass; +0 where the pass has none (a + 0 == a)
  if (on && k < r) {
    const double *p = sums + (int64_t)k * 2 * c + ch;
    n0 = p[0], n1 = p[c];
  }
  for (int i0 = 0; i0 < r; i0 += MERGE_K) {
    s_0[tid] = n0;
    s_1[tid] = n1;
    n0 = 0.0, n1 = 0.0;
    if (on && i0 + MERGE_K + k < r) {
      const double *p = sums + (int64_t)(i0 + MERGE_K + k) * 2 * c + ch;
      n0 = p[0], n1 = p[c];
    }
    __syncthreads();
    if (k == 0) {
      for (int j0 = 0; j0 < MERGE_K; j0 += 8) {
        double u[8], v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = s_0[(j0 + j) * MERGE_CH + cl], v[j] = s_1[(j0 + j) * MERGE_CH + cl];
#pragma unroll
        for (int j = 0; j < 8; ++j) a0 += u[j], a1 += v[j];
      }
    }
    __syncthreads();
  }
  if (k == 0 && on) {
    out[ch] = a0;
    out[c + ch] = a1;
  }
}

__global__ void __launch_bounds__(BLOCK) k_finish(const double *__restrict__ rec, int c, double eps, double momentum,
                                                  float *running_mean, float *running_var, float *__restrict__ mean_rstd) {
  const int ch = blockIdx.x * BLOCK + threadIdx.x;
  if (ch >= c) return;
  const double n = rec[ch], mean = rec[c + ch], m2 = rec[2 * (int64_t)c + ch];
  const bool any = n > 0.0;
  const double var = any ? m2 / n : 0.0;
  mean_rstd[ch] = (float)(any ? mean : 0.0);
  mean_rstd[c + ch] = (float)(1.0 / sqrt(var + eps));
  if (!any) return;
  if (running_mean != nullptr) running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mean);
  if (running_var != nullptr) {
    const double unb = m2 / (n > 1.0 ? n - 1.0 : 1.0);
    running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unb);
  }
}

template <int V>
__global__ void __launch_bounds__(BLOCK) k_apply(const float *x, int64_t n, int c, Geo g, const float *__restrict__ mean_rstd,
                                                 const float *__restrict__ weight, const float *__restrict__ bias, int act,
                                                 float slope, float *y) {
  const Mine m = mine<V>(g, n);
  if (!m.on) return;
  Chan<V> k;
  k.load(mean_rstd, weight, bias, m.ch, c);
  for (int64_t r = m.r0 + m.ry; r < m.r1; r += g.R) {
    Vec<V> t;
    t.load(x + r * c + m.ch);
#pragma unroll
    for (int j = 0; j < V; ++j) t.v[j] = act_fwd(z_of(xhat_of(t.v[j], k.mean[j], k.rstd[j]), k.w[j], k.b[j]), act, slope);
    t.store(y + r * c + m.ch);
  }
}

template <int V>
__global__ void __launch_bounds__(BLOCK) k_tile_bwd_sums(const float *__restrict__ dy, const float *__restrict__ x, int64_t n, int c,
                                                         Geo g, const float *__restrict__ mean_rstd,
                                                         const float *__restrict__ weight, const float *__restrict__ bias, int act,
                                                         float slope, double *__restrict__ part) {
  __shared__ double red[BLOCK * V];
  const Mine m = mine<V>(g, n);
  double s0[V], s1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s0[j] = 0.0, s1[j] = 0.0;
  if (m.on) {
    Chan<V> k;
    k.load(mean_rstd, weight, bias, m.ch, c);
    for (int64_t r = m.r0 + m.ry; r < m.r1; r += g.R) {
      Vec<V> t, d;
      t.load(x + r * c + m.ch);
      d.load(dy + r * c + m.ch);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float xh = xhat_of(t.v[j], k.mean[j], k.rstd[j]);
        const float gj = d.v[j] * act_bwd(z_of(xh, k.w[j], k.b[j]), act, slope);
        s0[j] += (double)gj;
        s1[j] += (double)gj * (double)xh;
      }
    }
  }
  reduce_rows<V>(red, g, m, s0);
  __syncthreads();
  reduce_rows<V>(red, g, m, s1);
  if (m.ry == 0 && m.on) {
    double *p = part + (int64_t)blockIdx.x * 2 * c + m.ch;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      p[j] = s0[j];
      p[c + j] = s1[j];
    }
  }
}

template <int V>
__global__ void __launch_bounds__(BLOCK) k_bwd_dx(const float *dy, const float *__restrict__ x, int64_t n, int c, Geo g,
                                                  const float *__restrict__ mean_rstd, const float *__restrict__ weight,
                                                  const float *__restrict__ bias, int act, float slope,
                                                  const double *__restrict__ total_sums, const double *__restrict__ total_rec,
                                                  float *dx) {
  const Mine m = mine<V>(g, n);
  if (!m.on) return;
  Chan<V> k;
  k.load(mean_rstd, weight, bias, m.ch, c);
  float a0[V], a1[V], ws[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const double cnt = total_rec[m.ch + j];
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    a0[j] = (float)(total_sums[m.ch + j] * inv);
    a1[j] = (float)(total_sums[c + m.ch + j] * inv);
    ws[j] = k.w[j] * k.rstd[j];
  }
  for (int64_t r = m.r0 + m.ry; r < m.r1; r += g.R) {
    Vec<V> t, d;
    t.load(x + r * c + m.ch);
    d.load(dy + r * c + m.ch);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xh = xhat_of(t.v[j], k.mean[j], k.rstd[j]);
      const float gj = d.v[j] * act_bwd(z_of(xh, k.w[j], k.b[j]), act, slope);
      d.v[j] = ws[j] * ((gj - a0[j]) - xh * a1[j]);
    }
    d.store(dx + r * c + m.ch);
  }
}

inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

// nullptr = fine, else what is wrong
const char *range_error(int64_t n, int32_t c) {
  if (c < 1 || c > PN_MAX_C) return "c outside [1, PN_MAX_C]";
  if (n < 0 || (double)n * c >= 0x1p62) return "n outside [0, 2^62 / c)";
  if (tiles_of(n) >= (1ll << 31)) return "too many row tiles";
  return nullptr;
}

Geo geo_of(int32_t c, int V) {
  Geo g;
  g.cu = c / V;
  g.L = 1;
  while (g.L < g.cu && g.L < 64) g.L *= 2;
  g.R = BLOCK / g.L;
  return g;
}

dim3 grid_of(int64_t n, Geo g) { return dim3((unsigned)tiles_of(n), (unsigned)((g.cu + g.L - 1) / g.L)); }

int act_ok(int32_t act) { return act == PH_ACT_NONE || act == PH_ACT_RELU || act == PH_ACT_LEAKY; }

unsigned chan_blocks(int32_t c) { return (unsigned)((c + BLOCK - 1) / BLOCK); }

unsigned merge_blocks(int32_t c) { return (unsigned)((c + MERGE_CH - 1) / MERGE_CH); }

}  // namespace

SIDE_EXPORTS(PN_FN, PN_ABI_VERSION)

extern "C" int64_t PN_FN(ws_bytes)(int64_t n, int32_t c) {
  if (range_error(n, c) != nullptr) return -1;
  return tiles_of(n) * 3 * (int64_t)c * (int64_t)sizeof(double);
}

extern "C" int PN_FN(moments_merge)(const double *recs, int32_t r, int32_t c, double *out, void *stream) {
  if (c < 1 || c > PN_MAX_C || r < 0) return fail("moments_merge: r = %d, c = %d outside the served range", r, c);
  if (out == nullptr || (recs == nullptr && r > 0)) return fail("moments_merge: null pointer");
  hipLaunchKernelGGL(k_moments_merge, dim3(merge_blocks(c)), dim3(BLOCK), 0, st_of(stream), recs, r, c, out);
  SIDE_CHECK_LAUNCH("k_moments_merge");
  return 0;
}

extern "C" int PN_FN(sums_merge)(const double *sums, int32_t r, int32_t c, double *out, void *stream) {
  if (c < 1 || c > PN_MAX_C || r < 0) return fail("sums_merge: r = %d, c = %d outside the served range", r, c);
  if (out == nullptr || (sums == nullptr && r > 0)) return fail("sums_merge: null pointer");
  hipLaunchKernelGGL(k_sums_merge, dim3(merge_blocks(c)), dim3(BLOCK), 0, st_of(stream), sums, r, c, out);
  SIDE_CHECK_LAUNCH("k_sums_merge");
  return 0;
}

extern "C" int PN_FN(moments)(const float *x, int64_t n, int32_t c, void *ws, int64_t ws_bytes, double *rec, void *stream) {
  if (const char *e = range_error(n, c)) return fail("moments: n = %lld, c = %d: %s", (long long)n, c, e);
  if (rec == nullptr) return fail("moments: null rec");
  if (n == 0) return PN_FN(moments_merge)(nullptr, 0, c, rec, stream);
  if (x == nullptr || ws == nullptr) return fail("moments: null pointer");
  if (ws_bytes < PN_FN(ws_bytes)(n, c) || !aligned16(ws))
    return fail("moments: the workspace has %lld bytes, %lld needed (16-byte aligned)", (long long)ws_bytes,
                (long long)PN_FN(ws_bytes)(n, c));
  double *part = static_cast<double *>(ws);
  if (c % 4 == 0 && aligned16(x)) {
    const Geo g = geo_of(c, 4);
    hipLaunchKernelGGL(k_tile_moments<4>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), x, n, c, g, part);
  } else {
    const Geo g = geo_of(c, 1);
    hipLaunchKernelGGL(k_tile_moments<1>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), x, n, c, g, part);
  }
  SIDE_CHECK_LAUNCH("k_tile_moments");
  return PN_FN(moments_merge)(part, (int32_t)tiles_of(n), c, rec, stream);
}

extern "C" int PN_FN(finish)(const double *rec, int32_t c, double eps, double momentum, float *running_mean, float *running_var,
                             float *mean_rstd, void *stream) {
  if (c < 1 || c > PN_MAX_C) return fail("finish: c = %d outside [1, %d]", c, PN_MAX_C);
  if (!(eps >= 0.0)) return fail("finish: eps = %g, must be >= 0", eps);
  if (rec == nullptr || mean_rstd == nullptr) return fail("finish: null pointer");
  hipLaunchKernelGGL(k_finish, dim3(chan_blocks(c)), dim3(BLOCK), 0, st_of(stream), rec, c, eps, momentum, running_mean,
                     running_var, mean_rstd);
  SIDE_CHECK_LAUNCH("k_finish");
  return 0;
}

extern "C" int PN_FN(apply)(const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight, const float *bias,
                            int32_t act, float slope, float *y, void *stream) {
  if (const char *e = range_error(n, c)) return fail("apply: n = %lld, c = %d: %s", (long long)n, c, e);
  if (!act_ok(act)) return fail("apply: act = %d", act);
  if (n == 0) return 0;
  if (x == nullptr || y == nullptr || mean_rstd == nullptr) return fail("apply: null pointer");
  if (c % 4 == 0 && aligned16(x) && aligned16(y)) {
    const Geo g = geo_of(c, 4);
    hipLaunchKernelGGL(k_apply<4>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), x, n, c, g, mean_rstd, weight, bias, act, slope, y);
  } else {
    const Geo g = geo_of(c, 1);
    hipLaunchKernelGGL(k_apply<1>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), x, n, c, g, mean_rstd, weight, bias, act, slope, y);
  }
  SIDE_CHECK_LAUNCH("k_apply");
  return 0;
}

extern "C" int PN_FN(bwd_sums)(const float *dy, const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight,
                               const float *bias, int32_t act, float slope, void *ws, int64_t ws_bytes, double *sums,
                               void *stream) {
  if (const char *e = range_error(n, c)) return fail("bwd_sums: n = %lld, c = %d: %s", (long long)n, c, e);
  if (!act_ok(act)) return fail("bwd_sums: act = %d", act);
  if (sums == nullptr) return fail("bwd_sums: null sums");
  if (n == 0) return PN_FN(sums_merge)(nullptr, 0, c, sums, stream);
  if (dy == nullptr || x == nullptr || mean_rstd == nullptr || ws == nullptr) return fail("bwd_sums: null pointer");
  if (ws_bytes < PN_FN(ws_bytes)(n, c) || !aligned16(ws))
    return fail("bwd_sums: the workspace has %lld bytes, %lld needed (16-byte aligned)", (long long)ws_bytes,
                (long long)PN_FN(ws_bytes)(n, c));
  double *part = static_cast<double *>(ws);
  if (c % 4 == 0 && aligned16(x) && aligned16(dy)) {
    const Geo g = geo_of(c, 4);
    hipLaunchKernelGGL(k_tile_bwd_sums<4>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), dy, x, n, c, g, mean_rstd, weight, bias,
                       act, slope, part);
  } else {
    const Geo g = geo_of(c, 1);
    hipLaunchKernelGGL(k_tile_bwd_sums<1>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), dy, x, n, c, g, mean_rstd, weight, bias,
                       act, slope, part);
  }
  SIDE_CHECK_LAUNCH("k_tile_bwd_sums");
  return PN_FN(sums_merge)(part, (int32_t)tiles_of(n), c, sums, stream);
}

extern "C" int PN_FN(bwd_dx)(const float *dy, const float *x, int64_t n, int32_t c, const float *mean_rstd, const float *weight,
                             const float *bias, int32_t act, float slope, const double *total_sums, const double *total_rec,
                             float *dx, void *stream) {
  if (const char *e = range_error(n, c)) return fail("bwd_dx: n = %lld, c = %d: %s", (long long)n, c, e);
  if (!act_ok(act)) return fail("bwd_dx: act = %d", act);
  if (n == 0) return 0;
  if (dy == nullptr || x == nullptr || mean_rstd == nullptr || total_sums == nullptr || total_rec == nullptr || dx == nullptr)
    return fail("bwd_dx: null pointer");
  if (c % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx)) {
    const Geo g = geo_of(c, 4);
    hipLaunchKernelGGL(k_bwd_dx<4>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), dy, x, n, c, g, mean_rstd, weight, bias, act,
                       slope, total_sums, total_rec, dx);
  } else {
    const Geo g = geo_of(c, 1);
    hipLaunchKernelGGL(k_bwd_dx<1>, grid_of(n, g), dim3(BLOCK), 0, st_of(stream), dy, x, n, c, g, mean_rstd, weight, bias, act,
                       slope, total_sums, total_rec, dx);
  }
  SIDE_CHECK_LAUNCH("k_bwd_dx");
  return 0;
}

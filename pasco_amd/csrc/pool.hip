// Pooling, broadcast and channel-wise kernels for gfx950 (include/pasco_pool.h).  All of them move rows and do one or two
// flops per element: the roof is bytes over the HBM rate, there is no MFMA and no inline assembly.
//
// Lane order: lanes run along the channels of a row.  A kernel is instantiated for V = 4 (a thread owns four consecutive
// channels and moves them as one 16-byte piece) and V = 1 (scalar); V = 4 needs every row to start on a 16-byte boundary:
// widths and row strides that are multiples of four and 16-byte aligned base pointers (`wide` in each entry), as k_wgrad's vec_x / vec_y.
//
// Row kernels (k_broadcast, k_window = pooling and the channel-wise convolution, k_pool_bwd): one thread per (row, channel group), the offsets of a window are
// visited in ascending k.
//
// Sums over rows (k_seg_part, k_seg_max_part, k_chconv_wgrad_part): a workgroup is ONE wave; it owns PP_SEG_ROWS consecutive
// rows and 64 * V channels, every thread walks the rows in ascending order and keeps one running sum per batch index in LDS
// (B * 64 * V floats, at most 64 KiB, touched by that thread alone: no race, no atomics on floats).  The partials go to the workspace and a
// second kernel adds them in ascending order.  The wide instantiation is taken only above 64 channels: below, V = 1 keeps
// more lanes of the wave busy.  The row counts are integers: LDS integer atomics, whose result does not depend on the order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_pool.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int SEG = PP_SEG_ROWS;
constexpr int UNROLL = 8;                  // rows whose loads a thread of a row-sum kernel has in flight

template <int V>
struct Pack {
  float v[V];
};

template <int V>
__device__ __forceinline__ Pack<V> ld(const float *p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void st(float *p, const Pack<V> &r) {
  if constexpr (V == 4)
    *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else
    *p = r.v[0];
}

template <int V>
__device__ __forceinline__ Pack<V> zero() {
  Pack<V> r;
#pragma unroll
  for (int j = 0; j < V; ++j) r.v[j] = 0.f;
  return r;
}

// ---- broadcast ---------------------------------------------------------------------------------------------------------------
// One thread per (row, V columns of the OUTPUT row).  cx = the width taken from x (0 for COPY), cg = the width of g.
template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_broadcast(const float *__restrict__ x, int64_t n, int cx, const float *__restrict__ g, int cg, const int4 *__restrict__ coords,
                int B, const float *__restrict__ cnt, int mode, float *__restrict__ out) {
  const int cout = (mode == PP_BC_CAT) ? cx + cg : (mode == PP_BC_COPY ? cg : cx);
  const int groups = cout / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * groups) return;
  const int64_t i = t / groups;
  const int col = (int)(t - i * groups) * V;
  const bool from_x = (mode == PP_BC_CAT) && col < cx;
  const int b = coords[i].x;
  Pack<V> r = zero<V>();
  if (b < 0 || b >= B) {                           // a zero row, whatever the mode
  } else if (from_x) {
    r = ld<V>(x + i * cx + col);
  } else {
    const int gc = (mode == PP_BC_CAT) ? col - cx : col;
    Pack<V> v = ld<V>(g + (int64_t)b * cg + gc);
    if (cnt != nullptr) {
      const float cn = cnt[b];
#pragma unroll
      for (int j = 0; j < V; ++j) v.v[j] = cn > 0.f ? v.v[j] / cn : 0.f;
    }
    if (mode == PP_BC_ADD || mode == PP_BC_MUL) {
      const Pack<V> a = ld<V>(x + i * cx + col);
#pragma unroll
      for (int j = 0; j < V; ++j) r.v[j] = (mode == PP_BC_ADD) ? a.v[j] + v.v[j] : a.v[j] * v.v[j];
    } else {
      r = v;
    }
  }
  st<V>(out + i * cout + col, r);
}

// ---- local pooling and the channel-wise convolution ------------------------------------------------------------------------------
// w == nullptr: pooling (mode PP_SUM / PP_AVG, cnt written by the thread of channel group 0); otherwise the channel-wise
// convolution (products with w[k], bias added last).
template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_window(const float *__restrict__ x, int64_t n_in, int c, const int32_t *__restrict__ nbr, int kvol, int64_t n_out, int mode,
             const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ out, float *__restrict__ cnt) {
  const int groups = c / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_out * groups) return;
  const int64_t o = t / groups;
  const int col = (int)(t - o * groups) * V;
  Pack<V> s = zero<V>();
  int present = 0;
  for (int k = 0; k < kvol; ++k) {
    const int32_t r = nbr[(int64_t)k * n_out + o];
    if (r < 0 || r >= n_in) continue;
    ++present;
    const Pack<V> a = ld<V>(x + (int64_t)r * c + col);
    if (w != nullptr) {
      const Pack<V> ww = ld<V>(w + (int64_t)k * c + col);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += a.v[j] * ww.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += a.v[j];
    }
  }
  if (w != nullptr) {
    if (bias != nullptr) {
      const Pack<V> bb = ld<V>(bias + col);
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += bb.v[j];
    }
  } else {
    if (mode == PP_AVG && present > 0) {
      const float cn = (float)present;
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] = s.v[j] / cn;
    }
    if (col == 0) cnt[o] = (float)present;
  }
  st<V>(out + o * c + col, s);
}

template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_pool_bwd(const float *__restrict__ dy, int64_t n_out, int c, const float *__restrict__ cnt, const int32_t *__restrict__ inv,
               int kvol, int64_t n_in, int mode, float *__restrict__ dx) {
  const int groups = c / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_in * groups) return;
  const int64_t i = t / groups;
  const int col = (int)(t - i * groups) * V;
  Pack<V> s = zero<V>();
  for (int k = 0; k < kvol; ++k) {
    const int32_t o = inv[(int64_t)k * n_in + i];
    if (o < 0 || o >= n_out) continue;
    float scale = 1.f;
    if (mode == PP_AVG) {
      const float cn = cnt[o];
      if (!(cn > 0.f)) continue;
      scale = 1.f / cn;
    }
    const Pack<V> a = ld<V>(dy + (int64_t)o * c + col);
    if (mode == PP_AVG) {
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += a.v[j] * scale;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += a.v[j];
    }
  }
  st<V>(dx + i * c + col, s);
}

// ---- sums over rows ----------------------------------------------------------------------------------------------------------
// grid (partials, column blocks), one wave.  part [P, B, c]; cnt_part int32 [P, B] (written by column block 0; may be null).
// y != nullptr: the addend is x[i] * y[i] (ldx == c then) and, where dx != nullptr, dx[i] = x[i] * g[b_i] is stored on the way
// (x = dy, y = the forward's rows: pp_broadcast_mul_bwd).
template <int V>
__global__ void __launch_bounds__(WAVE)
    k_seg_part(const float *__restrict__ x, int64_t n, int c, int64_t ldx, const int4 *__restrict__ coords, int B,
               const float *__restrict__ y, const float *__restrict__ g, float *__restrict__ dx, float *__restrict__ part,
               int32_t *__restrict__ cnt_part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];                  // [B][WAVE * V]; first, the counts: int32 [B]
  int32_t *cs = reinterpret_cast<int32_t *>(sm);
  const int lane = threadIdx.x;
  const int64_t p = blockIdx.x;
  const int col = (blockIdx.y * WAVE + lane) * V;
  const int64_t r0 = p * SEG;
  const int64_t r1 = (r0 + SEG < n) ? r0 + SEG : n;
  if (cnt_part != nullptr && blockIdx.y == 0) {
    if (lane < B) cs[lane] = 0;
    __syncthreads();
    for (int64_t r = r0 + lane; r < r1; r += WAVE) {
      const int b = coords[r].x;
      if (b >= 0 && b < B) atomicAdd(&cs[b], 1);
    }
    __syncthreads();
    if (lane < B) cnt_part[p * B + lane] = cs[lane];
    __syncthreads();                               // the counts are out before their words become running sums
  }
  for (int b = 0; b < B; ++b) st<V>(sm + ((size_t)b * WAVE + lane) * V, zero<V>());
  if (col < c) {
    // UNROLL rows at a time: their loads are issued together, then the rows are added one after the other in ascending order
    for (int64_t rb = r0; rb < r1; rb += UNROLL) {
      int bs[UNROLL];
      Pack<V> as[UNROLL], ys[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t r = rb + u;
        const bool have = r < r1;
        bs[u] = have ? coords[r].x : -1;
        as[u] = have ? ld<V>(x + r * ldx + col) : zero<V>();
        ys[u] = (have && y != nullptr) ? ld<V>(y + r * c + col) : zero<V>();
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t r = rb + u;
        if (r >= r1) break;
        const int b = bs[u];
        const bool in = b >= 0 && b < B;
        Pack<V> a = as[u];
        if (dx != nullptr) {
          Pack<V> d = zero<V>();
          if (in) {
            const Pack<V> gg = ld<V>(g + (int64_t)b * c + col);
#pragma unroll
            for (int j = 0; j < V; ++j) d.v[j] = a.v[j] * gg.v[j];
          }
          st<V>(dx + r * c + col, d);
        }
        if (!in) continue;
        if (y != nullptr) {
#pragma unroll
          for (int j = 0; j < V; ++j) a.v[j] = a.v[j] * ys[u].v[j];
        }
        float *acc = sm + ((size_t)b * WAVE + lane) * V;
        Pack<V> t = ld<V>(acc);
#pragma unroll
        for (int j = 0; j < V; ++j) t.v[j] += a.v[j];
        st<V>(acc, t);
      }
    }
    for (int b = 0; b < B; ++b) st<V>(part + (p * B + b) * c + col, ld<V>(sm + ((size_t)b * WAVE + lane) * V));
  }
}

// count fp32 [B] = sum_p cnt_part[p][b]
__global__ void k_seg_count(const int32_t *__restrict__ cnt_part, int64_t P, int B, float *__restrict__ count) {
  const int b = threadIdx.x;
  if (b >= B) return;
  int32_t s = 0;
  for (int64_t p = 0; p < P; ++p) s += cnt_part[p * B + b];
  count[b] = (float)s;
}

// out[e] = part[0][e] + part[1][e] + ...  over E = rows * c elements; avg: / count[row] where count > 0.
__global__ void __launch_bounds__(BLOCK)
    k_part_sum(const float *__restrict__ part, int64_t P, int64_t E, int c, const float *__restrict__ count, float *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  if (P > 0) {
    s = part[e];
    for (int64_t pb = 1; pb < P; pb += UNROLL) {             // UNROLL loads in flight, added in ascending order
      float v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = pb + u < P ? part[(pb + u) * E + e] : 0.f;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        if (pb + u < P) s += v[u];
    }
  }
  if (count != nullptr) {
    const float cn = count[e / c];
    if (cn > 0.f) s = s / cn;
  }
  out[e] = s;
}

// The running maximum of one segment: a == -2 empty, a == -1 a NaN maximum (sticky), otherwise the first row that holds m.
struct MaxState {
  float m;
  int32_t a;
};

__device__ __forceinline__ void max_merge(MaxState &s, float v, int32_t row) {
  if (row == -2) return;                          // an empty partial
  if (s.a == -2) {
    s.m = v;
    s.a = (v != v) ? -1 : row;
  } else if (s.m != s.m) {
  } else if (v != v) {
    s.m = v;
    s.a = -1;
  } else if (v > s.m) {
    s.m = v;
    s.a = row;
  }
}

__global__ void __launch_bounds__(WAVE)
    k_seg_max_part(const float *__restrict__ x, int64_t n, int c, int64_t ldx, const int4 *__restrict__ coords, int B,
                   float *__restrict__ pm, int32_t *__restrict__ pa, int32_t *__restrict__ cnt_part) {
  extern __shared__ __attribute__((aligned(16))) float sm[];                  // float [B][WAVE], int32 [B][WAVE]; first, the counts
  int32_t *sa = reinterpret_cast<int32_t *>(sm + (size_t)B * WAVE);
  int32_t *cs = reinterpret_cast<int32_t *>(sm);
  const int lane = threadIdx.x;
  const int64_t p = blockIdx.x;
  const int col = blockIdx.y * WAVE + lane;
  const int64_t r0 = p * SEG;
  const int64_t r1 = (r0 + SEG < n) ? r0 + SEG : n;
  if (cnt_part != nullptr && blockIdx.y == 0) {
    if (lane < B) cs[lane] = 0;
    __syncthreads();
    for (int64_t r = r0 + lane; r < r1; r += WAVE) {
      const int b = coords[r].x;
      if (b >= 0 && b < B) atomicAdd(&cs[b], 1);
    }
    __syncthreads();
    if (lane < B) cnt_part[p * B + lane] = cs[lane];
    __syncthreads();
  }
  for (int b = 0; b < B; ++b) {
    sm[b * WAVE + lane] = 0.f;
    sa[b * WAVE + lane] = -2;
  }
  if (col >= c) return;
  for (int64_t r = r0; r < r1; ++r) {
    const int b = coords[r].x;
    if (b < 0 || b >= B) continue;
    MaxState s{sm[b * WAVE + lane], sa[b * WAVE + lane]};
    max_merge(s, x[r * ldx + col], (int32_t)r);
    sm[b * WAVE + lane] = s.m;
    sa[b * WAVE + lane] = s.a;
  }
  for (int b = 0; b < B; ++b) {
    pm[(p * B + b) * c + col] = sm[b * WAVE + lane];
    pa[(p * B + b) * c + col] = sa[b * WAVE + lane];
  }
}

__global__ void __launch_bounds__(BLOCK)
    k_seg_max_finish(const float *__restrict__ pm, const int32_t *__restrict__ pa, int64_t P, int64_t E, float *__restrict__ out,
                     int32_t *__restrict__ arg) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= E) return;
  MaxState s{0.f, -2};
  for (int64_t p = 0; p < P; ++p) max_merge(s, pm[p * E + e], pa[p * E + e]);
  out[e] = s.a == -2 ? 0.f : s.m;
  arg[e] = s.a < 0 ? -1 : s.a;
}

__global__ void __launch_bounds__(BLOCK)
    k_seg_max_bwd(const float *__restrict__ dy, const int32_t *__restrict__ arg, int64_t E, int c, int64_t n, float *__restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= E) return;
  const int32_t a = arg[e];
  if (a >= 0 && a < n) dx[(int64_t)a * c + e % c] = dy[e];
}

// grid (partials, column blocks, K), one wave: part [P, K, c]
template <int V>
__global__ void __launch_bounds__(WAVE)
    k_chconv_wgrad_part(const float *__restrict__ x, int64_t n_in, int c, const float *__restrict__ dy, int64_t n_out,
                        const int32_t *__restrict__ nbr, int kvol, float *__restrict__ part) {
  const int col = (blockIdx.y * WAVE + threadIdx.x) * V;
  if (col >= c) return;
  const int64_t p = blockIdx.x;
  const int k = blockIdx.z;
  const int64_t o0 = p * SEG;
  const int64_t o1 = (o0 + SEG < n_out) ? o0 + SEG : n_out;
  Pack<V> s = zero<V>();
  for (int64_t ob = o0; ob < o1; ob += UNROLL) {           // the loads of UNROLL rows together, the sums in ascending order
    bool on[UNROLL];
    Pack<V> as[UNROLL], ds[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t o = ob + u;
      const int32_t r = o < o1 ? nbr[(int64_t)k * n_out + o] : -1;
      on[u] = r >= 0 && r < n_in;
      as[u] = on[u] ? ld<V>(x + (int64_t)r * c + col) : zero<V>();
      ds[u] = on[u] ? ld<V>(dy + o * c + col) : zero<V>();
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (!on[u]) continue;
#pragma unroll
      for (int j = 0; j < V; ++j) s.v[j] += as[u].v[j] * ds[u].v[j];
    }
  }
  st<V>(part + (p * kvol + k) * c + col, s);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// flat grid of BLOCK threads over `threads`, or -1
int64_t flat_grid(int64_t threads) {
  const int64_t g = (threads + BLOCK - 1) / BLOCK;
  return g < (1ll << 31) ? g : -1;
}

bool seg_shape_ok(int64_t n, int32_t c, int32_t B) {
  return n >= 0 && n < (1ll << 24) && c >= 1 && B >= 1 && B <= PP_MAX_BATCH && (c + WAVE - 1) / WAVE <= 65535;
}

inline int64_t partials_of(int64_t n) { return (n + SEG - 1) / SEG; }

// workspace: part fp32 [P, B, c] | second array of the same size (the max's rows) | cnt_part int32 [P, B] | count fp32 [B]
int64_t seg_bytes(int64_t n, int32_t c, int32_t B) {
  const int64_t P = partials_of(n);
  return (2 * P * B * c + P * B + B) * 4;
}

bool window_shape_ok(int32_t K, int32_t c, int64_t n_in, int64_t n_out) {
  return K >= 1 && K <= PP_MAX_KVOL && c >= 1 && n_in >= 0 && n_out >= 0 && n_in < (1ll << 31) && n_out < (1ll << 31);
}

}  // namespace

SIDE_EXPORTS(PP_FN, PP_ABI_VERSION)

extern "C" int64_t PP_FN(seg_workspace_bytes)(int64_t n, int32_t c, int32_t B) {
  return seg_shape_ok(n, c, B) ? seg_bytes(n, c, B) : -1;
}

extern "C" int PP_FN(seg_reduce)(const float *x, int64_t n, int32_t c, int64_t ldx, const int32_t *coords, int32_t B, int32_t mode,
                                 float *out, float *count, int32_t *arg, void *workspace, int64_t workspace_bytes, void *stream) {
  if (B < 1 || B > PP_MAX_BATCH) return fail("seg_reduce: B = %d outside [1, %d] (PP_MAX_BATCH)", B, PP_MAX_BATCH);
  if (!seg_shape_ok(n, c, B)) return fail("seg_reduce: n = %lld, c = %d outside the served range (n < 2^24)", (long long)n, c);
  if (mode != PP_SUM && mode != PP_AVG && mode != PP_MAX) return fail("seg_reduce: mode = %d", mode);
  if (ldx < c) return fail("seg_reduce: ldx = %lld below c = %d", (long long)ldx, c);
  if (out == nullptr || (mode == PP_MAX && arg == nullptr)) return fail("seg_reduce: null output");
  if (n > 0 && (x == nullptr || coords == nullptr)) return fail("seg_reduce: null pointer");
  const int64_t need = seg_bytes(n, c, B);
  if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return fail("seg_reduce: workspace of %lld bytes, %lld needed (16-byte aligned)", (long long)workspace_bytes, (long long)need);
  const int64_t P = partials_of(n);
  const int64_t E = (int64_t)B * c;
  float *part = static_cast<float *>(workspace);
  int32_t *part2 = reinterpret_cast<int32_t *>(part + P * E);
  int32_t *cnt_part = part2 + P * E;
  float *countf = reinterpret_cast<float *>(cnt_part + P * B);
  const bool want_count = count != nullptr || mode == PP_AVG;
  float *cdst = count != nullptr ? count : countf;
  hipStream_t s = st_of(stream);
  if (P > 0) {
    if (mode == PP_MAX) {
      const dim3 grid((unsigned)P, (unsigned)((c + WAVE - 1) / WAVE));
      const size_t lds = (size_t)2 * B * WAVE * 4;
      hipLaunchKernelGGL(k_seg_max_part, grid, dim3(WAVE), lds, s, x, n, c, ldx, (const int4 *)coords, B, part, part2,
                         want_count ? cnt_part : nullptr);
      SIDE_CHECK_LAUNCH("k_seg_max_part");
    } else {
      const bool wide = c > WAVE && c % 4 == 0 && ldx % 4 == 0 && aligned16(x);
      const int V = wide ? 4 : 1;
      const dim3 grid((unsigned)P, (unsigned)((c + WAVE * V - 1) / (WAVE * V)));
      const size_t lds = (size_t)B * WAVE * V * 4;                  // at most 64 KiB (B = PP_MAX_BATCH, V = 4)
      if (wide)
        hipLaunchKernelGGL(k_seg_part<4>, grid, dim3(WAVE), lds, s, x, n, c, ldx, (const int4 *)coords, B, (const float *)nullptr,
                           (const float *)nullptr, (float *)nullptr, part, want_count ? cnt_part : nullptr);
      else
        hipLaunchKernelGGL(k_seg_part<1>, grid, dim3(WAVE), lds, s, x, n, c, ldx, (const int4 *)coords, B, (const float *)nullptr,
                           (const float *)nullptr, (float *)nullptr, part, want_count ? cnt_part : nullptr);
      SIDE_CHECK_LAUNCH("k_seg_part");
    }
  }
  if (want_count) {
    hipLaunchKernelGGL(k_seg_count, dim3(1), dim3(WAVE), 0, s, cnt_part, P, B, cdst);
    SIDE_CHECK_LAUNCH("k_seg_count");
  }
  const int64_t grid = flat_grid(E);
  if (mode == PP_MAX)
    hipLaunchKernelGGL(k_seg_max_finish, dim3((unsigned)grid), dim3(BLOCK), 0, s, part, part2, P, E, out, arg);
  else
    hipLaunchKernelGGL(k_part_sum, dim3((unsigned)grid), dim3(BLOCK), 0, s, part, P, E, c, mode == PP_AVG ? cdst : (const float *)nullptr,
                       out);
  SIDE_CHECK_LAUNCH("seg_reduce finish");
  return 0;
}

extern "C" int PP_FN(seg_max_bwd)(const float *dy, const int32_t *arg, int32_t B, int32_t c, int64_t n, float *dx, void *stream) {
  if (B < 1 || B > PP_MAX_BATCH) return fail("seg_max_bwd: B = %d outside [1, %d] (PP_MAX_BATCH)", B, PP_MAX_BATCH);
  if (c < 1 || n < 0 || n >= (1ll << 31)) return fail("seg_max_bwd: c = %d, n = %lld outside the served range", c, (long long)n);
  if (n == 0) return 0;
  if (dy == nullptr || arg == nullptr || dx == nullptr) return fail("seg_max_bwd: null pointer");
  SIDE_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)n * c * sizeof(float), st_of(stream)));
  const int64_t E = (int64_t)B * c;
  hipLaunchKernelGGL(k_seg_max_bwd, dim3((unsigned)flat_grid(E)), dim3(BLOCK), 0, st_of(stream), dy, arg, E, c, n, dx);
  SIDE_CHECK_LAUNCH("k_seg_max_bwd");
  return 0;
}

extern "C" int PP_FN(broadcast)(const float *x, int64_t n, int32_t c, const float *g, int32_t cg, const int32_t *coords, int32_t B,
                                const float *cnt, int32_t mode, float *out, void *stream) {
  if (B < 1 || B > PP_MAX_BATCH) return fail("broadcast: B = %d outside [1, %d] (PP_MAX_BATCH)", B, PP_MAX_BATCH);
  if (mode < PP_BC_ADD || mode > PP_BC_COPY) return fail("broadcast: mode = %d", mode);
  if (mode == PP_BC_COPY) c = 0;
  if (cg < 1 || (mode != PP_BC_COPY && c < 1) || n < 0 || n >= (1ll << 31))
    return fail("broadcast: c = %d, cg = %d, n = %lld outside the served range", c, cg, (long long)n);
  if ((mode == PP_BC_ADD || mode == PP_BC_MUL) && cg != c) return fail("broadcast: cg = %d, must equal c = %d", cg, c);
  if (n == 0) return 0;
  if (g == nullptr || coords == nullptr || out == nullptr || (x == nullptr && mode != PP_BC_COPY)) return fail("broadcast: null pointer");
  const int cout = (mode == PP_BC_CAT) ? c + cg : (mode == PP_BC_COPY ? cg : c);
  const bool wide = c % 4 == 0 && cg % 4 == 0 && aligned16(g) && aligned16(out) && (mode == PP_BC_COPY || aligned16(x));
  const int64_t grid = flat_grid(n * (cout / (wide ? 4 : 1)));
  if (grid < 0) return fail("broadcast: too many workgroups for n = %lld, %d columns", (long long)n, cout);
  if (wide)
    hipLaunchKernelGGL(k_broadcast<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n, c, g, cg, (const int4 *)coords, B, cnt,
                       mode, out);
  else
    hipLaunchKernelGGL(k_broadcast<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n, c, g, cg, (const int4 *)coords, B, cnt,
                       mode, out);
  SIDE_CHECK_LAUNCH("k_broadcast");
  return 0;
}

extern "C" int PP_FN(broadcast_mul_bwd)(const float *dy, const float *x, const float *g, const int32_t *coords, int64_t n, int32_t c,
                                        int32_t B, float *dx, float *dg, void *workspace, int64_t workspace_bytes, void *stream) {
  if (B < 1 || B > PP_MAX_BATCH) return fail("broadcast_mul_bwd: B = %d outside [1, %d] (PP_MAX_BATCH)", B, PP_MAX_BATCH);
  if (!seg_shape_ok(n, c, B)) return fail("broadcast_mul_bwd: n = %lld, c = %d outside the served range (n < 2^24)", (long long)n, c);
  if (dx == nullptr && dg == nullptr) return 0;
  if (n > 0 && (dy == nullptr || coords == nullptr || (dx != nullptr && g == nullptr) || (dg != nullptr && x == nullptr)))
    return fail("broadcast_mul_bwd: null pointer");
  const int64_t need = seg_bytes(n, c, B);
  if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return fail("broadcast_mul_bwd: workspace of %lld bytes, %lld needed (16-byte aligned)", (long long)workspace_bytes, (long long)need);
  const int64_t P = partials_of(n);
  const int64_t E = (int64_t)B * c;
  float *part = static_cast<float *>(workspace);
  hipStream_t s = st_of(stream);
  if (P > 0) {
    // without dg the products with x are not formed: the rows are added as they are and the partials are not read
    const float *y = dg != nullptr ? x : nullptr;
    const bool wide = c > WAVE && c % 4 == 0 && aligned16(dy) && (y == nullptr || aligned16(y)) &&
                      (dx == nullptr || (aligned16(dx) && aligned16(g)));
    const int V = wide ? 4 : 1;
    const dim3 grid((unsigned)P, (unsigned)((c + WAVE * V - 1) / (WAVE * V)));
    const size_t lds = (size_t)B * WAVE * V * 4;                  // at most 64 KiB (B = PP_MAX_BATCH, V = 4)
    if (wide)
      hipLaunchKernelGGL(k_seg_part<4>, grid, dim3(WAVE), lds, s, dy, n, c, (int64_t)c, (const int4 *)coords, B, y, g, dx, part,
                         (int32_t *)nullptr);
    else
      hipLaunchKernelGGL(k_seg_part<1>, grid, dim3(WAVE), lds, s, dy, n, c, (int64_t)c, (const int4 *)coords, B, y, g, dx, part,
                         (int32_t *)nullptr);
    SIDE_CHECK_LAUNCH("k_seg_part");
  }
  if (dg != nullptr) {
    hipLaunchKernelGGL(k_part_sum, dim3((unsigned)flat_grid(E)), dim3(BLOCK), 0, s, part, P, E, c, (const float *)nullptr, dg);
    SIDE_CHECK_LAUNCH("k_part_sum");
  }
  return 0;
}

namespace {

int window_launch(const char *what, const float *x, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out, int32_t mode,
                  const float *w, const float *bias, float *out, float *cnt, void *stream) {
  const bool wide = c % 4 == 0 && aligned16(x) && aligned16(out) && (w == nullptr || aligned16(w)) && (bias == nullptr || aligned16(bias));
  const int64_t grid = flat_grid(n_out * (c / (wide ? 4 : 1)));
  if (grid < 0) return fail("%s: too many workgroups for n_out = %lld, c = %d", what, (long long)n_out, c);
  if (wide)
    hipLaunchKernelGGL(k_window<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_in, c, nbr, K, n_out, mode, w, bias, out, cnt);
  else
    hipLaunchKernelGGL(k_window<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_in, c, nbr, K, n_out, mode, w, bias, out, cnt);
  SIDE_CHECK_LAUNCH(what);
  return 0;
}

}  // namespace

extern "C" int PP_FN(pool)(const float *x, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out, int32_t mode,
                           float *out, float *cnt, void *stream) {
  if (K < 1 || K > PP_MAX_KVOL) return fail("pool: K = %d outside [1, %d] (PP_MAX_KVOL)", K, PP_MAX_KVOL);
  if (!window_shape_ok(K, c, n_in, n_out))
    return fail("pool: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (mode != PP_SUM && mode != PP_AVG) return fail("pool: mode = %d", mode);
  if (n_out == 0) return 0;
  if (nbr == nullptr || out == nullptr || cnt == nullptr || (x == nullptr && n_in > 0)) return fail("pool: null pointer");
  return window_launch("pool", x, n_in, c, nbr, K, n_out, mode, nullptr, nullptr, out, cnt, stream);
}

extern "C" int PP_FN(pool_bwd)(const float *dy, int64_t n_out, int32_t c, const float *cnt, const int32_t *inv, int32_t K, int64_t n_in,
                               int32_t mode, float *dx, void *stream) {
  if (K < 1 || K > PP_MAX_KVOL) return fail("pool_bwd: K = %d outside [1, %d] (PP_MAX_KVOL)", K, PP_MAX_KVOL);
  if (!window_shape_ok(K, c, n_in, n_out))
    return fail("pool_bwd: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (mode != PP_SUM && mode != PP_AVG) return fail("pool_bwd: mode = %d", mode);
  if (n_in == 0) return 0;
  if (dx == nullptr) return fail("pool_bwd: null dx");
  if (n_out == 0) {
    SIDE_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)n_in * c * sizeof(float), st_of(stream)));
    return 0;
  }
  if (dy == nullptr || inv == nullptr || (mode == PP_AVG && cnt == nullptr)) return fail("pool_bwd: null pointer");
  const bool wide = c % 4 == 0 && aligned16(dy) && aligned16(dx);
  const int64_t grid = flat_grid(n_in * (c / (wide ? 4 : 1)));
  if (grid < 0) return fail("pool_bwd: too many workgroups for n_in = %lld, c = %d", (long long)n_in, c);
  if (wide)
    hipLaunchKernelGGL(k_pool_bwd<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), dy, n_out, c, cnt, inv, K, n_in, mode, dx);
  else
    hipLaunchKernelGGL(k_pool_bwd<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), dy, n_out, c, cnt, inv, K, n_in, mode, dx);
  SIDE_CHECK_LAUNCH("k_pool_bwd");
  return 0;
}

extern "C" int PP_FN(chconv_fwd)(const float *x, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out, const float *w,
                                 const float *bias, float *out, void *stream) {
  if (K < 1 || K > PP_MAX_KVOL) return fail("chconv_fwd: K = %d outside [1, %d] (PP_MAX_KVOL)", K, PP_MAX_KVOL);
  if (!window_shape_ok(K, c, n_in, n_out))
    return fail("chconv_fwd: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (n_out == 0) return 0;
  if (nbr == nullptr || out == nullptr || w == nullptr || (x == nullptr && n_in > 0)) return fail("chconv_fwd: null pointer");
  return window_launch("chconv_fwd", x, n_in, c, nbr, K, n_out, PP_SUM, w, bias, out, nullptr, stream);
}

extern "C" int64_t PP_FN(chconv_wgrad_workspace_bytes)(int32_t K, int32_t c, int64_t n_out) {
  if (!window_shape_ok(K, c, 0, n_out) || (int64_t)K * c >= (1ll << 31) || (c + WAVE - 1) / WAVE > 65535) return -1;
  return partials_of(n_out) * K * c * 4;
}

extern "C" int PP_FN(chconv_wgrad)(const float *x, int64_t n_in, int32_t c, const float *dy, int64_t n_out, const int32_t *nbr, int32_t K,
                                   float *dw, void *workspace, int64_t workspace_bytes, void *stream) {
  if (K < 1 || K > PP_MAX_KVOL) return fail("chconv_wgrad: K = %d outside [1, %d] (PP_MAX_KVOL)", K, PP_MAX_KVOL);
  const int64_t need = PP_FN(chconv_wgrad_workspace_bytes)(K, c, n_out);
  if (need < 0 || n_in < 0 || n_in >= (1ll << 31))
    return fail("chconv_wgrad: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (dw == nullptr) return fail("chconv_wgrad: null dw");
  const int64_t E = (int64_t)K * c;
  hipStream_t s = st_of(stream);
  if (n_out == 0 || n_in == 0) {
    SIDE_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)E * sizeof(float), s));
    return 0;
  }
  if (x == nullptr || dy == nullptr || nbr == nullptr) return fail("chconv_wgrad: null pointer");
  if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return fail("chconv_wgrad: workspace of %lld bytes, %lld needed (16-byte aligned)", (long long)workspace_bytes, (long long)need);
  const int64_t P = partials_of(n_out);
  float *part = static_cast<float *>(workspace);
  const bool wide = c > WAVE && c % 4 == 0 && aligned16(x) && aligned16(dy);
  const int V = wide ? 4 : 1;
  const dim3 grid((unsigned)P, (unsigned)((c + WAVE * V - 1) / (WAVE * V)), (unsigned)K);
  if (wide)
    hipLaunchKernelGGL(k_chconv_wgrad_part<4>, grid, dim3(WAVE), 0, s, x, n_in, c, dy, n_out, nbr, K, part);
  else
    hipLaunchKernelGGL(k_chconv_wgrad_part<1>, grid, dim3(WAVE), 0, s, x, n_in, c, dy, n_out, nbr, K, part);
  SIDE_CHECK_LAUNCH("k_chconv_wgrad_part");
  hipLaunchKernelGGL(k_part_sum, dim3((unsigned)flat_grid(E)), dim3(BLOCK), 0, s, part, P, E, c, (const float *)nullptr, dw);
  SIDE_CHECK_LAUNCH("k_part_sum");
  return 0;
}

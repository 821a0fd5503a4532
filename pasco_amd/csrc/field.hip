// Point <-> voxel kernels for gfx950 (include/pasco_field.h): the grouping of list entries by segment, sums / averages / maxima
// of a segment's rows, the weighted gather, and the eight-corner interpolation.  All of them move rows and do one or two flops
// per element: the roof is bytes over the HBM rate, there is no MFMA and no inline assembly.
//
// Lane order (as pool.hip): lanes run along the channels of a row.  A row kernel is instantiated for V = 4 (a thread owns four
// consecutive channels and moves them as one 16-byte piece) and V = 1 (scalar); V = 4 needs every row to start on a 16-byte
// boundary: a width that is a multiple of four and 16-byte aligned base pointers (`wide` in each entry).
//
// pq_group: a least-significant-digit radix sort of (key, index) pairs over 8-bit digits, ascending, as many passes as the
// segment count has bytes (semloss.hip's ps_sort_desc is the same construction on ~key).  Absent keys become the key n_seg and
// sort behind every segment.  Per pass k_sort_hist counts the digits of every tile of TILE keys (LDS integer atomics),
// k_sort_scan turns the [tiles, 256] counts into the first output position of every (tile, digit), and k_sort_scatter ranks
// stably inside the tile (ballots inside a wave, the waves stacked in order) - so equal keys keep their ascending index.
// offsets[s] is then the lower bound of s in the sorted keys, one binary search per segment.
//
// pq_seg_rows: one thread per (segment, channel group) walks the segment's list: UNROLL members' loads are issued together,
// then added one after the other; a partial closes every PQ_SEG_ROWS members and joins the running total.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_field.h"
#include "ph_common.h"                     // ph_pack / ph_packable / ph_find: the coordinate maps' key and probe (nothing else)
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int SEG = PQ_SEG_ROWS;
constexpr int UNROLL = 8;                  // members whose loads a thread of pq_seg_rows has in flight
constexpr int KPT = 8;                     // keys per thread of a sort tile
constexpr int TILE = BLOCK * KPT;          // 2048 keys
constexpr int WAVE_KEYS = TILE / 4;        // consecutive keys of one wave of a tile

static_assert(SEG % UNROLL == 0, "a partial is a whole number of load groups");

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

// ---- grouping ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_keys(const int32_t *__restrict__ keys, int64_t n, uint32_t n_seg, uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t k = keys[i];
  out[i] = (k < 0 || (uint32_t)k >= n_seg) ? n_seg : (uint32_t)k;
}

__device__ __forceinline__ uint32_t digit_of(uint32_t key, int shift) { return (key >> shift) & 255u; }

__global__ void __launch_bounds__(BLOCK) k_sort_hist(const uint32_t *__restrict__ kin, int64_t n, int shift, uint32_t *__restrict__ counts) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.x;
  hist[tid] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int64_t pos = t0 + r * BLOCK + tid;
    if (pos < n) atomicAdd(&hist[digit_of(kin[pos], shift)], 1u);
  }
  __syncthreads();
  counts[(int64_t)blockIdx.x * 256 + tid] = hist[tid];
}

// One workgroup, thread d = digit d: counts[tile][d] becomes the first output position of the tile's keys with digit d =
// (all keys with a smaller digit) + (the keys with digit d in earlier tiles).
__global__ void __launch_bounds__(BLOCK) k_sort_scan(uint32_t *__restrict__ counts, int64_t tiles) {
  __shared__ uint32_t tot[256];
  const int d = threadIdx.x;
  constexpr int AHEAD = 8;                       // tiles whose counts are loaded together: the walk is latency-bound otherwise
  uint32_t run = 0u;
  for (int64_t t = 0; t < tiles; t += AHEAD) {
    uint32_t v[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) v[u] = t + u < tiles ? counts[(t + u) * 256 + d] : 0u;
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      if (t + u < tiles) counts[(t + u) * 256 + d] = run;
      run += v[u];
    }
  }
  tot[d] = run;
  __syncthreads();
  uint32_t base = 0u;
  for (int j = 0; j < d; ++j) base += tot[j];
  for (int64_t t = 0; t < tiles; t += AHEAD) {
    uint32_t v[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) v[u] = t + u < tiles ? counts[(t + u) * 256 + d] : 0u;
#pragma unroll
    for (int u = 0; u < AHEAD; ++u)
      if (t + u < tiles) counts[(t + u) * 256 + d] = v[u] + base;
  }
}

// iin == nullptr: the indices are the positions (the first pass).
__global__ void __launch_bounds__(BLOCK) k_sort_scatter(const uint32_t *__restrict__ kin, const int32_t *__restrict__ iin, int64_t n,
                                                        int shift, const uint32_t *__restrict__ counts, uint32_t *__restrict__ kout,
                                                        int32_t *__restrict__ iout) {
  __shared__ uint32_t cnt[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < 4 * 256; j += BLOCK) (&cnt[0][0])[j] = 0u;
  __syncthreads();
  const int64_t start = (int64_t)blockIdx.x * TILE + (int64_t)wave * WAVE_KEYS;
  uint32_t key[KPT], rank[KPT];
  int32_t idx[KPT];
  int dig[KPT];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int64_t pos = start + r * 64 + lane;
    const bool valid = pos < n;
    key[r] = valid ? kin[pos] : 0u;
    idx[r] = valid ? (iin == nullptr ? (int32_t)pos : iin[pos]) : 0;
    const uint32_t d = digit_of(key[r], shift);
    dig[r] = valid ? (int)d : -1;
    uint64_t peers = __ballot(valid);              // the lanes of this round with the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint64_t bal = __ballot(valid && ((d >> b) & 1u) != 0u);
      peers &= ((d >> b) & 1u) != 0u ? bal : ~bal;
    }
    rank[r] = 0u;
    if (valid) {
      const uint32_t before = cnt[wave][d];
      const uint32_t lower = (uint32_t)__popcll(peers & below);
      rank[r] = before + lower;
      __builtin_amdgcn_wave_barrier();
      if (lower == 0u) cnt[wave][d] = before + (uint32_t)__popcll(peers);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    // thread d stacks the four waves' counts of digit d on the tile's first position for that digit
    uint32_t run = counts[(int64_t)blockIdx.x * 256 + tid];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t v = cnt[w][tid];
      cnt[w][tid] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    if (dig[r] < 0) continue;
    const int64_t dst = (int64_t)cnt[wave][dig[r]] + rank[r];
    if (dst >= n) continue;      // cannot happen while the counts come from k_sort_hist on the same keys
    kout[dst] = key[r];
    iout[dst] = idx[r];
  }
}

// offsets[s] = the number of sorted keys below s, s = 0 .. n_seg
__global__ void __launch_bounds__(BLOCK) k_offsets(const uint32_t *__restrict__ sorted, int64_t n, int64_t n_seg, int32_t *__restrict__ offsets) {
  const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (s > n_seg) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)sorted[mid] < s)
      lo = mid + 1;
    else
      hi = mid;
  }
  offsets[s] = (int32_t)lo;
}

// ---- segment rows ------------------------------------------------------------------------------------------------------------
struct SegRange {
  int64_t o0, o1;
};

__device__ __forceinline__ SegRange seg_range(const int32_t *__restrict__ offsets, int64_t s, int64_t n_list) {
  int64_t o0 = offsets[s], o1 = offsets[s + 1];
  o0 = o0 < 0 ? 0 : o0;
  o1 = o1 > n_list ? n_list : o1;
  if (o1 < o0) o1 = o0;
  return {o0, o1};
}

// the source row of list entry j, or -1
__device__ __forceinline__ int64_t member_row(int32_t j, int64_t n_list, int64_t n_src, int64_t src_mod) {
  if (j < 0 || j >= n_list) return -1;
  const int64_t row = src_mod >= n_list ? (int64_t)j : (int64_t)((uint32_t)j % (uint32_t)src_mod);
  return row < n_src ? row : -1;
}

template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_seg_rows(const float *__restrict__ x, int64_t n_src, int c, const int32_t *__restrict__ offsets, const int32_t *__restrict__ perm,
               int64_t n_list, int64_t n_seg, const float *__restrict__ w, int64_t src_mod, int mode, float *__restrict__ out,
               float *__restrict__ cnt) {
  const int groups = c / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_seg * groups) return;
  const int64_t s = t / groups;
  const int col = (int)(t - s * groups) * V;
  const SegRange g = seg_range(offsets, s, n_list);
  Pack<V> total = zero<V>();
  for (int64_t cb = g.o0; cb < g.o1; cb += SEG) {                  // one partial
    const int64_t ce = cb + SEG < g.o1 ? cb + SEG : g.o1;
    Pack<V> part = zero<V>();
    for (int64_t jb = cb; jb < ce; jb += UNROLL) {
      bool on[UNROLL];
      float ws[UNROLL];
      Pack<V> as[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int32_t j = jb + u < ce ? perm[jb + u] : -1;
        const int64_t row = member_row(j, n_list, n_src, src_mod);
        on[u] = row >= 0;
        as[u] = on[u] ? ld<V>(x + row * c + col) : zero<V>();
        ws[u] = (on[u] && w != nullptr) ? w[j] : 1.f;
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        if (!on[u]) continue;
        if (w != nullptr) {
#pragma unroll
          for (int q = 0; q < V; ++q) part.v[q] += ws[u] * as[u].v[q];
        } else {
#pragma unroll
          for (int q = 0; q < V; ++q) part.v[q] += as[u].v[q];
        }
      }
    }
    if (cb == g.o0) {
      total = part;
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q) total.v[q] += part.v[q];
    }
  }
  const float cn = (float)(g.o1 - g.o0);
  if (mode == PQ_AVG && cn > 0.f) {
#pragma unroll
    for (int q = 0; q < V; ++q) total.v[q] = total.v[q] / cn;
  }
  if (col == 0 && cnt != nullptr) cnt[s] = cn;
  st<V>(out + s * c + col, total);
}

// One thread per (segment, channel).  a == -2 empty so far, a == -1 a NaN maximum (sticky), otherwise the first member that holds m.
__global__ void __launch_bounds__(BLOCK)
    k_seg_max(const float *__restrict__ x, int64_t n_src, int c, const int32_t *__restrict__ offsets, const int32_t *__restrict__ perm,
              int64_t n_list, int64_t n_seg, int64_t src_mod, float *__restrict__ out, float *__restrict__ cnt, int32_t *__restrict__ arg) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_seg * c) return;
  const int64_t s = t / c;
  const int col = (int)(t - s * c);
  const SegRange g = seg_range(offsets, s, n_list);
  float m = 0.f;
  int32_t a = -2;
  for (int64_t p = g.o0; p < g.o1; ++p) {
    const int32_t j = perm[p];
    const int64_t row = member_row(j, n_list, n_src, src_mod);
    if (row < 0) continue;
    const float v = x[row * c + col];
    if (a == -2) {
      m = v;
      a = (v != v) ? -1 : j;
    } else if (m != m) {
    } else if (v != v) {
      m = v;
      a = -1;
    } else if (v > m) {
      m = v;
      a = j;
    }
  }
  out[t] = a == -2 ? 0.f : m;
  arg[t] = a < 0 ? -1 : a;
  if (col == 0 && cnt != nullptr) cnt[s] = (float)(g.o1 - g.o0);
}

__global__ void __launch_bounds__(BLOCK)
    k_seg_max_bwd(const float *__restrict__ dy, const int32_t *__restrict__ arg, int64_t E, int c, int64_t n_src, int64_t src_mod,
                  float *__restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= E) return;
  const int32_t a = arg[e];
  if (a < 0) return;
  const int64_t row = (int64_t)a % src_mod;
  if (row < n_src) dx[row * c + e % c] = dy[e];
}

// ---- weighted gather ---------------------------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_gather_w(const float *__restrict__ x, int64_t n_src, int c, const int32_t *__restrict__ idx, int64_t n, const float *__restrict__ d,
               float *__restrict__ out) {
  const int groups = c / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n * groups) return;
  const int64_t i = t / groups;
  const int col = (int)(t - i * groups) * V;
  const int32_t r = idx[i];
  Pack<V> o = zero<V>();
  if (r >= 0 && r < n_src) {
    const float dv = d[r];
    if (dv != 0.f) {
      const float scale = 1.f / dv;
      const Pack<V> a = ld<V>(x + (int64_t)r * c + col);
#pragma unroll
      for (int q = 0; q < V; ++q) o.v[q] = a.v[q] * scale;
    }
  }
  st<V>(out + i * c + col, o);
}

// ---- interpolation -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK)
    k_interp_map(const float *__restrict__ pts, int64_t m, const uint64_t *__restrict__ tkeys, const int32_t *__restrict__ tvals,
                 uint64_t mask, int ts, int32_t *__restrict__ rows, float *__restrict__ weights) {
  const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= m) return;
  const float b = pts[4 * p];
  const float tsf = (float)ts;
  bool ok = isfinite(b) && b >= 0.f && b < 1024.f;
  float f[3][2];
  int lower[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float xd = pts[4 * p + 1 + d];
    // a coordinate is convertible to the keys' integers only inside +-2^18; beyond, no corner can be in the map
    const bool fine = isfinite(xd) && fabsf(xd) < 262144.f;
    ok = ok && fine;
    float lo = fine ? floorf(xd / tsf) * tsf : 0.f;
    // lower <= x < lower + ts, whatever the stride (a quotient formed with a reciprocal can land on the next integer)
    if (lo > xd) lo -= tsf;
    if (lo + tsf <= xd) lo += tsf;               // (lo + ts is exact; x - lo would round)
    lower[d] = (int)lo;
    // 1 - |x - corner| / ts is the distance to the OTHER corner over ts: formed directly, nothing cancels
    f[d][0] = fine ? ((lo + tsf) - xd) / tsf : 0.f;
    f[d][1] = fine ? (xd - lo) / tsf : 0.f;
  }
  const int bi = ok ? (int)floorf(b) : 0;
#pragma unroll
  for (int k = 0; k < PQ_CORNERS; ++k) {
    const int ox = (k >> 2) & 1, oy = (k >> 1) & 1, oz = k & 1;
    const float wk = ok ? (f[0][ox] * f[1][oy]) * f[2][oz] : 0.f;
    int32_t row = -1;
    if (ok && wk != 0.f) {
      const int cx = lower[0] + ox * ts, cy = lower[1] + oy * ts, cz = lower[2] + oz * ts;
      if (ph_packable(bi, cx, cy, cz)) row = ph_find(tkeys, tvals, mask, ph_pack(bi, cx, cy, cz));
    }
    rows[(int64_t)k * m + p] = row;
    weights[(int64_t)k * m + p] = wk;
  }
}

template <int V>
__global__ void __launch_bounds__(BLOCK)
    k_interp_fwd(const float *__restrict__ x, int64_t n_in, int c, const int32_t *__restrict__ rows, const float *__restrict__ weights,
                 int64_t m, float *__restrict__ out) {
  const int groups = c / V;
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= m * groups) return;
  const int64_t p = t / groups;
  const int col = (int)(t - p * groups) * V;
  int32_t r[PQ_CORNERS];
  float wk[PQ_CORNERS];
  Pack<V> a[PQ_CORNERS];
#pragma unroll
  for (int k = 0; k < PQ_CORNERS; ++k) {
    r[k] = rows[(int64_t)k * m + p];
    const bool on = r[k] >= 0 && r[k] < n_in;
    if (!on) r[k] = -1;
    wk[k] = on ? weights[(int64_t)k * m + p] : 0.f;
    a[k] = on ? ld<V>(x + (int64_t)r[k] * c + col) : zero<V>();
  }
  Pack<V> s = zero<V>();
#pragma unroll
  for (int k = 0; k < PQ_CORNERS; ++k) {
    if (r[k] < 0) continue;
#pragma unroll
    for (int q = 0; q < V; ++q) s.v[q] += wk[k] * a[k].v[q];
  }
  st<V>(out + p * c + col, s);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// flat grid of BLOCK threads over `threads`, or -1
int64_t flat_grid(int64_t threads) {
  const int64_t g = (threads + BLOCK - 1) / BLOCK;
  return g < (1ll << 31) ? g : -1;
}

inline int64_t pad256(int64_t b) { return (b + 255) / 256 * 256; }

inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

bool group_shape_ok(int64_t n, int64_t n_seg) { return n >= 0 && n < (1ll << 24) && n_seg >= 0 && n_seg < (1ll << 31); }

// workspace: keys A uint32 [n] | keys B uint32 [n] | indices B int32 [n] | counts uint32 [tiles, 256]
int64_t group_bytes(int64_t n) { return 3 * pad256(4 * n) + tiles_of(n) * 256 * 4; }

int sort_passes(int64_t n_seg) {
  int bits = 0;
  while ((n_seg >> bits) != 0) ++bits;             // the key n_seg (an absent entry) is the largest
  const int p = (bits + 7) / 8;
  return p < 1 ? 1 : p;
}

}  // namespace

SIDE_EXPORTS(PQ_FN, PQ_ABI_VERSION)

extern "C" int64_t PQ_FN(group_workspace_bytes)(int64_t n, int64_t n_seg) { return group_shape_ok(n, n_seg) ? group_bytes(n) : -1; }

extern "C" int PQ_FN(group)(const int32_t *keys, int64_t n, int64_t n_seg, int32_t *offsets, int32_t *perm, void *workspace,
                            int64_t workspace_bytes, void *stream) {
  if (n < 0 || n >= (1ll << 24)) return fail("group: n = %lld outside the served range (n < 2^24)", (long long)n);
  if (n_seg < 0 || n_seg >= (1ll << 31)) return fail("group: n_seg = %lld outside the served range [0, 2^31)", (long long)n_seg);
  if (offsets == nullptr) return fail("group: null offsets");
  hipStream_t s = st_of(stream);
  if (n == 0 || n_seg == 0) {                      // nothing present
    SIDE_CHECK_HIP(hipMemsetAsync(offsets, 0, (size_t)(n_seg + 1) * sizeof(int32_t), s));
    return 0;
  }
  if (keys == nullptr || perm == nullptr) return fail("group: null pointer");
  const int64_t need = group_bytes(n);
  if (workspace == nullptr || workspace_bytes < need || !aligned16(workspace))
    return fail("group: workspace of %lld bytes, %lld needed (16-byte aligned)", (long long)workspace_bytes, (long long)need);
  const int64_t part = pad256(4 * n), tiles = tiles_of(n);
  char *base = static_cast<char *>(workspace);
  uint32_t *kbuf[2] = {reinterpret_cast<uint32_t *>(base), reinterpret_cast<uint32_t *>(base + part)};
  int32_t *idx_b = reinterpret_cast<int32_t *>(base + 2 * part);
  uint32_t *counts = reinterpret_cast<uint32_t *>(base + 3 * part);
  hipLaunchKernelGGL(k_keys, dim3((unsigned)flat_grid(n)), dim3(BLOCK), 0, s, keys, n, (uint32_t)n_seg, kbuf[0]);
  SIDE_CHECK_LAUNCH("k_keys");
  const int passes = sort_passes(n_seg);
  const int32_t *iin = nullptr;
  for (int p = 0; p < passes; ++p) {
    int32_t *iout = (passes - 1 - p) % 2 == 0 ? perm : idx_b;          // the last pass writes perm
    hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)tiles), dim3(BLOCK), 0, s, kbuf[p & 1], n, 8 * p, counts);
    SIDE_CHECK_LAUNCH("k_sort_hist");
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(BLOCK), 0, s, counts, tiles);
    SIDE_CHECK_LAUNCH("k_sort_scan");
    hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)tiles), dim3(BLOCK), 0, s, kbuf[p & 1], iin, n, 8 * p, counts, kbuf[(p + 1) & 1], iout);
    SIDE_CHECK_LAUNCH("k_sort_scatter");
    iin = iout;
  }
  hipLaunchKernelGGL(k_offsets, dim3((unsigned)flat_grid(n_seg + 1)), dim3(BLOCK), 0, s, kbuf[passes & 1], n, n_seg, offsets);
  SIDE_CHECK_LAUNCH("k_offsets");
  return 0;
}

extern "C" int PQ_FN(seg_rows)(const float *x, int64_t n_src, int32_t c, const int32_t *offsets, const int32_t *perm, int64_t n_list,
                               int64_t n_seg, const float *w, int64_t src_mod, int32_t mode, float *out, float *cnt, int32_t *arg,
                               void *stream) {
  if (n_list < 0 || n_list >= (1ll << 24)) return fail("seg_rows: n_list = %lld outside the served range (n < 2^24)", (long long)n_list);
  if (c < 1) return fail("seg_rows: c = %d outside the served range (c >= 1)", c);
  if (n_seg < 0 || n_seg >= (1ll << 31)) return fail("seg_rows: n_seg = %lld outside the served range [0, 2^31)", (long long)n_seg);
  if (n_src < 0 || n_src >= (1ll << 31)) return fail("seg_rows: n_src = %lld outside the served range [0, 2^31)", (long long)n_src);
  if (mode != PQ_SUM && mode != PQ_AVG && mode != PQ_MAX) return fail("seg_rows: mode = %d", mode);
  if (src_mod < 1) return fail("seg_rows: src_mod = %lld, must be >= 1", (long long)src_mod);
  if (mode == PQ_MAX && w != nullptr) return fail("seg_rows: the maximum takes no weights");
  if (n_seg == 0) return 0;
  if (out == nullptr || offsets == nullptr || (mode == PQ_MAX && arg == nullptr)) return fail("seg_rows: null pointer");
  if (n_list > 0 && (perm == nullptr || (x == nullptr && n_src > 0))) return fail("seg_rows: null pointer");
  hipStream_t s = st_of(stream);
  if (mode == PQ_MAX) {
    const int64_t grid = flat_grid(n_seg * c);
    if (grid < 0) return fail("seg_rows: too many workgroups for n_seg = %lld, c = %d", (long long)n_seg, c);
    hipLaunchKernelGGL(k_seg_max, dim3((unsigned)grid), dim3(BLOCK), 0, s, x, n_src, c, offsets, perm, n_list, n_seg, src_mod, out, cnt, arg);
    SIDE_CHECK_LAUNCH("k_seg_max");
    return 0;
  }
  const bool wide = c % 4 == 0 && aligned16(x) && aligned16(out);
  const int64_t grid = flat_grid(n_seg * (c / (wide ? 4 : 1)));
  if (grid < 0) return fail("seg_rows: too many workgroups for n_seg = %lld, c = %d", (long long)n_seg, c);
  if (wide)
    hipLaunchKernelGGL(k_seg_rows<4>, dim3((unsigned)grid), dim3(BLOCK), 0, s, x, n_src, c, offsets, perm, n_list, n_seg, w, src_mod, mode, out, cnt);
  else
    hipLaunchKernelGGL(k_seg_rows<1>, dim3((unsigned)grid), dim3(BLOCK), 0, s, x, n_src, c, offsets, perm, n_list, n_seg, w, src_mod, mode, out, cnt);
  SIDE_CHECK_LAUNCH("k_seg_rows");
  return 0;
}

extern "C" int PQ_FN(seg_max_bwd)(const float *dy, const int32_t *arg, int64_t n_seg, int32_t c, int64_t n_src, int64_t src_mod,
                                  float *dx, void *stream) {
  if (c < 1) return fail("seg_max_bwd: c = %d outside the served range (c >= 1)", c);
  if (n_seg < 0 || n_seg >= (1ll << 31) || n_src < 0 || n_src >= (1ll << 31))
    return fail("seg_max_bwd: n_seg = %lld, n_src = %lld outside the served range [0, 2^31)", (long long)n_seg, (long long)n_src);
  if (src_mod < 1) return fail("seg_max_bwd: src_mod = %lld, must be >= 1", (long long)src_mod);
  if (n_src == 0) return 0;
  if (dx == nullptr) return fail("seg_max_bwd: null dx");
  SIDE_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)n_src * c * sizeof(float), st_of(stream)));
  if (n_seg == 0) return 0;
  if (dy == nullptr || arg == nullptr) return fail("seg_max_bwd: null pointer");
  const int64_t E = n_seg * c;
  const int64_t grid = flat_grid(E);
  if (grid < 0) return fail("seg_max_bwd: too many workgroups for n_seg = %lld, c = %d", (long long)n_seg, c);
  hipLaunchKernelGGL(k_seg_max_bwd, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), dy, arg, E, c, n_src, src_mod, dx);
  SIDE_CHECK_LAUNCH("k_seg_max_bwd");
  return 0;
}

extern "C" int PQ_FN(gather_w)(const float *x, int64_t n_src, int32_t c, const int32_t *idx, int64_t n, const float *d, float *out,
                               void *stream) {
  if (c < 1) return fail("gather_w: c = %d outside the served range (c >= 1)", c);
  if (n < 0 || n >= (1ll << 31) || n_src < 0 || n_src >= (1ll << 31))
    return fail("gather_w: n = %lld, n_src = %lld outside the served range [0, 2^31)", (long long)n, (long long)n_src);
  if (n == 0) return 0;
  if (idx == nullptr || out == nullptr || (n_src > 0 && (x == nullptr || d == nullptr))) return fail("gather_w: null pointer");
  const bool wide = c % 4 == 0 && aligned16(x) && aligned16(out);
  const int64_t grid = flat_grid(n * (c / (wide ? 4 : 1)));
  if (grid < 0) return fail("gather_w: too many workgroups for n = %lld, c = %d", (long long)n, c);
  if (wide)
    hipLaunchKernelGGL(k_gather_w<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_src, c, idx, n, d, out);
  else
    hipLaunchKernelGGL(k_gather_w<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_src, c, idx, n, d, out);
  SIDE_CHECK_LAUNCH("k_gather_w");
  return 0;
}

extern "C" int PQ_FN(interp_map)(const float *points, int64_t m, const uint64_t *tkeys, const int32_t *tvals, int64_t cap, int32_t ts,
                                 int32_t *rows, float *weights, void *stream) {
  if (m < 0 || m >= (1ll << 28)) return fail("interp_map: m = %lld outside the served range (m < 2^28)", (long long)m);
  if (ts < 1 || ts > 65536) return fail("interp_map: tensor stride %d outside [1, 65536]", ts);
  if (cap < 1 || (cap & (cap - 1)) != 0) return fail("interp_map: cap = %lld must be a power of two", (long long)cap);
  if (m == 0) return 0;
  if (points == nullptr || tkeys == nullptr || tvals == nullptr || rows == nullptr || weights == nullptr)
    return fail("interp_map: null pointer");
  hipLaunchKernelGGL(k_interp_map, dim3((unsigned)flat_grid(m)), dim3(BLOCK), 0, st_of(stream), points, m, tkeys, tvals,
                     (uint64_t)cap - 1, ts, rows, weights);
  SIDE_CHECK_LAUNCH("k_interp_map");
  return 0;
}

extern "C" int PQ_FN(interp_fwd)(const float *x, int64_t n_in, int32_t c, const int32_t *rows, const float *weights, int64_t m,
                                 float *out, void *stream) {
  if (c < 1) return fail("interp_fwd: c = %d outside the served range (c >= 1)", c);
  if (m < 0 || m >= (1ll << 28)) return fail("interp_fwd: m = %lld outside the served range (m < 2^28)", (long long)m);
  if (n_in < 0 || n_in >= (1ll << 31)) return fail("interp_fwd: n_in = %lld outside the served range [0, 2^31)", (long long)n_in);
  if (m == 0) return 0;
  if (rows == nullptr || weights == nullptr || out == nullptr || (x == nullptr && n_in > 0)) return fail("interp_fwd: null pointer");
  const bool wide = c % 4 == 0 && aligned16(x) && aligned16(out);
  const int64_t grid = flat_grid(m * (c / (wide ? 4 : 1)));
  if (grid < 0) return fail("interp_fwd: too many workgroups for m = %lld, c = %d", (long long)m, c);
  if (wide)
    hipLaunchKernelGGL(k_interp_fwd<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_in, c, rows, weights, m, out);
  else
    hipLaunchKernelGGL(k_interp_fwd<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n_in, c, rows, weights, m, out);
  SIDE_CHECK_LAUNCH("k_interp_fwd");
  return 0;
}

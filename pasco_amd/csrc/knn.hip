// Bipartite k-nearest-neighbour up-sampling for gfx950 (include/pasco_knn.h): the exact search of every query's k nearest
// candidates over a uniform grid, the inverse-squared-distance weights and the weighted row gather.  The backward is pq_group +
// pq_seg_rows (field.hip) over the flattened [k, m] table and has no kernel here.
//
// Layout choices:
//   k_knn       one query per lane, one wave (PK_QUERY_BLOCK = 64 lanes) per workgroup: the lanes of a wave walk different
//               numbers of shells, so a workgroup of one wave keeps the slowest query from holding three other waves' slots.
//               The candidate list lives in REGISTERS: the kernel is instantiated for every K = 1 .. PK_MAX_K and every access to
//               the list is a compile-time index of a fully unrolled loop - a runtime-indexed per-thread array would go to
//               scratch, and a runtime k inside a longer list costs a mask per slot in scalar registers, which spilled.  A
//               candidate that orders before the list's last slot is carried down the list by K compare-and-swap steps (an
//               insertion network over 64-bit (d2, index) keys: slot j keeps the smaller of itself and what is carried).  Empty
//               slots hold (+inf, INT_MAX), which orders behind every candidate, so "not full yet" needs no counter: the k-th
//               index is INT_MAX.
//               Candidates are read through `order` a run of cells at a time: a row of cells along x is one contiguous range of
//               the CSR (k_search of waffle.hip, whose shells and stopping bound these are).
//   k_weights   one thread per query, two passes over its k entries (the norm, then the quotients); the [k, m] layout makes
//               every pass a coalesced read.
//   k_interp    one thread per (query, 4 channels) where rows are 16-byte aligned, per (query, channel) otherwise; the k entries
//               are taken four at a time so that four row loads are in flight, and added in ascending j.
//
// Why every loop ends: shells run r = 0 .. max(g) - 1, a shell's loops run over the clipped cube, a cell run's loop over its CSR
// range clipped to [0, n), the list steps over K entries.  Every index read from a table is checked against its range before it
// is used as an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_knn.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int QB = PK_QUERY_BLOCK;
constexpr float INF = __builtin_huge_valf();
constexpr double DINF = __builtin_huge_val();
constexpr int NONE = 0x7fffffff;             // the index of an empty list slot: behind every candidate

struct Cells {
  double lo[3];
  double h;
  int g[3];
};

__device__ __forceinline__ int home_cell(float v, double lo, double h, int g) {
  const double t = floor((static_cast<double>(v) - lo) / h);
  return t >= 0.0 ? (t < static_cast<double>(g) ? static_cast<int>(t) : g - 1) : 0;
}

// The list of one query, ascending.  An entry is ONE 64-bit key, (the bits of d2) << 32 | index: d2 is a sum of squares, so it
// is +0 or positive (or +inf), where the order of the floats is the order of their bits as unsigned integers - one unsigned
// comparison of two keys is the ordering rule, ties by index included.  The last slot is the k-th entry, what a candidate has to
// beat; an empty slot is EMPTY = (+inf, INT_MAX), behind every candidate.
template <int K>
struct List {
  uint64_t key[K];
};

constexpr uint64_t EMPTY = (static_cast<uint64_t>(0x7f800000u) << 32) | static_cast<uint32_t>(NONE);

template <int K>
__device__ __forceinline__ void list_offer(List<K> &l, float d2, int i) {
  if (!(d2 <= INF)) return;                                       // a NaN never enters (finite inputs make none)
  uint64_t ck = (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | static_cast<uint32_t>(i);
  if (!(ck < l.key[K - 1])) return;
#pragma unroll
  for (int j = 0; j < K; ++j) {        // slot j keeps the smaller of itself and what is carried
    const uint64_t t = l.key[j];
    const bool before = ck < t;
    l.key[j] = before ? ck : t;
    ck = before ? t : ck;
  }
}

template <int K>
__device__ __forceinline__ void scan_range(List<K> &l, const float *__restrict__ cand, int ldc, int n,
                                           const int *__restrict__ order, int a, int b, float qx, float qy, float qz) {
  a = a < 0 ? 0 : a;
  b = b > n ? n : b;
  for (int s = a; s < b; ++s) {
    const int i = order[s];
    if (i < 0 || i >= n) continue;
    const float dx = cand[static_cast<int64_t>(i) * ldc + 0] - qx;
    const float dy = cand[static_cast<int64_t>(i) * ldc + 1] - qy;
    const float dz = cand[static_cast<int64_t>(i) * ldc + 2] - qz;
    list_offer<K>(l, (dx * dx + dy * dy) + dz * dz, i);
  }
}

template <int K>
__global__ __launch_bounds__(QB) void k_knn(const float *__restrict__ cand, int ldc, int n, const int *__restrict__ start,
                                            const int *__restrict__ order, Cells c, const float *__restrict__ q, int ldq, int m,
                                            int *__restrict__ idx, float *__restrict__ d2) {
  const int t = blockIdx.x * QB + threadIdx.x;
  if (t >= m) return;                 // no barrier below
  const float qx = q[static_cast<int64_t>(t) * ldq + 0], qy = q[static_cast<int64_t>(t) * ldq + 1],
              qz = q[static_cast<int64_t>(t) * ldq + 2];
  List<K> l;
#pragma unroll
  for (int j = 0; j < K; ++j) l.key[j] = EMPTY;
  const bool finite = fabsf(qx) < INF && fabsf(qy) < INF && fabsf(qz) < INF;      // false for a NaN as well
  if (finite && n > 0) {
    const float qv[3] = {qx, qy, qz};
    int hc[3];
    double outside2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      hc[a] = home_cell(qv[a], c.lo[a], c.h, c.g[a]);
      const double below = c.lo[a] - static_cast<double>(qv[a]);
      const double above = static_cast<double>(qv[a]) - (c.lo[a] + static_cast<double>(c.g[a]) * c.h);
      double o = below > above ? below : above;
      o = o > 0.0 ? o : 0.0;
      outside2[a] = o * o;
    }
    const int gx = c.g[0], gy = c.g[1], gz = c.g[2];
    const int rmax = (gx > gy ? (gx > gz ? gx : gz) : (gy > gz ? gy : gz));
    for (int r = 0; r < rmax; ++r) {
      if (r > 0) {
        double L = DINF;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double rest = outside2[(a + 1) % 3] + outside2[(a + 2) % 3];
          if (hc[a] + r <= c.g[a] - 1) {
            double gap = (c.lo[a] + static_cast<double>(hc[a] + r) * c.h) - static_cast<double>(qv[a]);
            gap = gap > 0.0 ? gap : 0.0;
            const double v = gap * gap + rest;
            L = v < L ? v : L;
          }
          if (hc[a] - r >= 0) {
            double gap = static_cast<double>(qv[a]) - (c.lo[a] + static_cast<double>(hc[a] - r + 1) * c.h);
            gap = gap > 0.0 ? gap : 0.0;
            const double v = gap * gap + rest;
            L = v < L ? v : L;
          }
        }
        if (L == DINF) break;           // no cell is left in any direction
        const float kd = __uint_as_float(static_cast<uint32_t>(l.key[K - 1] >> 32));
        if (static_cast<int>(static_cast<uint32_t>(l.key[K - 1])) != NONE && static_cast<double>(kd) < (1.0 - 0x1p-20) * L) break;
      }
      const int z0 = hc[2] - r > 0 ? hc[2] - r : 0, z1 = hc[2] + r < gz - 1 ? hc[2] + r : gz - 1;
      const int y0 = hc[1] - r > 0 ? hc[1] - r : 0, y1 = hc[1] + r < gy - 1 ? hc[1] + r : gy - 1;
      const int x0 = hc[0] - r > 0 ? hc[0] - r : 0, x1 = hc[0] + r < gx - 1 ? hc[0] + r : gx - 1;
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * gy + y) * gx;
          const bool face = z - hc[2] == r || hc[2] - z == r || y - hc[1] == r || hc[1] - y == r;
          // a face row is the whole clipped run along x; any other row only its two end cells (r > 0 there).  ONE call site
          // of the scan: the insertion network is inlined once, not three times
          for (int part = 0; part < (face ? 1 : 2); ++part) {
            int ca = row + x0, cb = row + x1 + 1;
            if (!face) {
              const int x = part == 0 ? hc[0] - r : hc[0] + r;
              if (x < 0 || x > gx - 1) continue;
              ca = row + x;
              cb = ca + 1;
            }
            scan_range<K>(l, cand, ldc, n, order, start[ca], start[cb], qx, qy, qz);
          }
        }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int i = static_cast<int>(static_cast<uint32_t>(l.key[j]));
    idx[static_cast<int64_t>(j) * m + t] = i != NONE ? i : -1;
    d2[static_cast<int64_t>(j) * m + t] = __uint_as_float(static_cast<uint32_t>(l.key[j] >> 32));      // +inf in an empty slot
  }
}

__global__ __launch_bounds__(BLOCK) void k_weights(const float *__restrict__ d2, const int *__restrict__ idx, int k, int64_t m,
                                                   float *__restrict__ w) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (p >= m) return;
  float norm = 0.0f;
  bool any = false;
  for (int j = 0; j < k; ++j) {
    if (idx[j * m + p] < 0) continue;
    const float r = 1.0f / (d2[j * m + p] + 1e-8f);
    norm = any ? norm + r : r;
    any = true;
  }
  const bool ok = any && norm != 0.0f && fabsf(norm) < INF;       // (a NaN norm fails the last test)
  for (int j = 0; j < k; ++j) {
    float v = 0.0f;
    if (ok && idx[j * m + p] >= 0) v = (1.0f / (d2[j * m + p] + 1e-8f)) / norm;
    w[j * m + p] = v;
  }
}

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

constexpr int AHEAD = 4;                     // entries of a query whose row loads are in flight together

template <int V>
__global__ __launch_bounds__(BLOCK) void k_interp(const float *__restrict__ x, int64_t n, int c, const int *__restrict__ idx,
                                                  const float *__restrict__ w, int k, int64_t m, float *__restrict__ out) {
  const int groups = c / V;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (t >= m * groups) return;
  const int64_t p = t / groups;
  const int col = static_cast<int>(t - p * groups) * V;
  Pack<V> s;
#pragma unroll
  for (int e = 0; e < V; ++e) s.v[e] = 0.0f;
  for (int j0 = 0; j0 < k; j0 += AHEAD) {
    int r[AHEAD];
    float wk[AHEAD];
    Pack<V> a[AHEAD];
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      const int j = j0 + u;
      int row = j < k ? idx[j * m + p] : -1;
      if (row < 0 || row >= n) row = -1;
      r[u] = row;
      wk[u] = row >= 0 ? w[j * m + p] : 0.0f;
      if (row >= 0) {
        a[u] = ld<V>(x + static_cast<int64_t>(row) * c + col);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) a[u].v[e] = 0.0f;
      }
    }
#pragma unroll
    for (int u = 0; u < AHEAD; ++u) {
      if (r[u] < 0) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) s.v[e] += wk[u] * a[u].v[e];
    }
  }
  st<V>(out + p * c + col, s);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static_assert(PK_MAX_K == 16, "pk_knn dispatches k = 1 .. 16");

bool bad_k(int k) { return k < 1 || k > PK_MAX_K; }

// m queries of k entries each: the [k, m] tables are indexed below 2^31
bool bad_table(int k, int64_t m) { return m < 0 || m * k >= (int64_t{1} << 31); }

template <int K>
void launch_knn(const float *cand, int ldc, int n, const int *start, const int *order, const Cells &c, const float *q, int ldq,
                int m, int *idx, float *d2, hipStream_t s) {
  hipLaunchKernelGGL(k_knn<K>, dim3((unsigned)((m + QB - 1) / QB)), dim3(QB), 0, s, cand, ldc, n, start, order, c, q, ldq, m, idx,
                     d2);
}

}  // namespace

SIDE_EXPORTS(PK_FN, PK_ABI_VERSION)

extern "C" int PK_FN(knn)(const float *cand, int32_t ldc, int64_t n, const int32_t *start, const int32_t *order, double lox,
                          double loy, double loz, double h, int32_t gx, int32_t gy, int32_t gz, const float *q, int32_t ldq,
                          int64_t m, int32_t k, int32_t *idx, float *d2, void *stream) {
  if (bad_k(k)) return fail("knn: k = %d outside the served range [1, %d]", k, PK_MAX_K);
  if (ldc < 3 || ldq < 3) return fail("knn: ldc = %d, ldq = %d: rows of at least three columns (x, y, z)", ldc, ldq);
  if (n < 0 || n >= (int64_t{1} << 31)) return fail("knn: n = %lld outside the served range [0, 2^31)", (long long)n);
  if (bad_table(k, m)) return fail("knn: m = %lld, k = %d outside the served range (0 <= m, m * k < 2^31)", (long long)m, k);
  if (!(h > 0.0) || gx < 1 || gy < 1 || gz < 1 || static_cast<int64_t>(gx) * gy * gz > PK_MAX_CELLS)
    return fail("knn: h = %g, grid %d x %d x %d (h > 0, at least one and at most %d cells)", h, gx, gy, gz, PK_MAX_CELLS);
  if (m == 0) return 0;
  if (!q || !idx || !d2 || !start || (n > 0 && (!cand || !order))) return fail("knn: null pointer");
  const Cells c{{lox, loy, loz}, h, {gx, gy, gz}};
  hipStream_t s = st_of(stream);
  const int ni = static_cast<int>(n), mi = static_cast<int>(m);
  switch (k) {
#define PK_CASE(K)                                                           \
  case K:                                                                    \
    launch_knn<K>(cand, ldc, ni, start, order, c, q, ldq, mi, idx, d2, s);   \
    break;
    PK_CASE(1) PK_CASE(2) PK_CASE(3) PK_CASE(4) PK_CASE(5) PK_CASE(6) PK_CASE(7) PK_CASE(8)
    PK_CASE(9) PK_CASE(10) PK_CASE(11) PK_CASE(12) PK_CASE(13) PK_CASE(14) PK_CASE(15) PK_CASE(16)
#undef PK_CASE
  }
  SIDE_CHECK_LAUNCH("k_knn");
  return 0;
}

extern "C" int PK_FN(weights)(const float *d2, const int32_t *idx, int32_t k, int64_t m, float *w, void *stream) {
  if (bad_k(k)) return fail("weights: k = %d outside the served range [1, %d]", k, PK_MAX_K);
  if (bad_table(k, m)) return fail("weights: m = %lld, k = %d outside the served range (0 <= m, m * k < 2^31)", (long long)m, k);
  if (m == 0) return 0;
  if (!d2 || !idx || !w) return fail("weights: null pointer");
  hipLaunchKernelGGL(k_weights, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), d2, idx, k, m, w);
  SIDE_CHECK_LAUNCH("k_weights");
  return 0;
}

extern "C" int PK_FN(interp_fwd)(const float *x, int64_t n, int32_t c, const int32_t *idx, const float *w, int32_t k, int64_t m,
                                 float *out, void *stream) {
  if (c < 1) return fail("interp_fwd: c = %d outside the served range (c >= 1)", c);
  if (bad_k(k)) return fail("interp_fwd: k = %d outside the served range [1, %d]", k, PK_MAX_K);
  if (n < 0 || n >= (int64_t{1} << 31)) return fail("interp_fwd: n = %lld outside the served range [0, 2^31)", (long long)n);
  if (bad_table(k, m)) return fail("interp_fwd: m = %lld, k = %d outside the served range (0 <= m, m * k < 2^31)", (long long)m, k);
  if (m == 0) return 0;
  if (!idx || !w || !out || (!x && n > 0)) return fail("interp_fwd: null pointer");
  const bool wide = c % 4 == 0 && aligned16(x) && aligned16(out);
  const int64_t grid = (m * (c / (wide ? 4 : 1)) + BLOCK - 1) / BLOCK;
  if (grid >= (int64_t{1} << 31)) return fail("interp_fwd: too many workgroups for m = %lld, c = %d", (long long)m, c);
  if (wide)
    hipLaunchKernelGGL(k_interp<4>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n, c, idx, w, k, m, out);
  else
    hipLaunchKernelGGL(k_interp<1>, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), x, n, c, idx, w, k, m, out);
  SIDE_CHECK_LAUNCH("k_interp");
  return 0;
}

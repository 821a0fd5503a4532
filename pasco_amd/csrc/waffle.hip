// WaffleIron point features (include/pasco_waffle.h): voxel keys, 2-D cell indices, the CSR of points by cell, exact k-nearest
// and nearest searches on a uniform grid, the flatten / depthwise 3 x 3 / inflate token mixer and the neighbourhood rows of
// the embedding.  pasco_amd/waffle/host.py restates every kernel with the same operations in the same order; the tall
// [N, C] x [C, C] products between these kernels run on the ph_conv_fwd route and are not here.
//
// Layout choices:
//   k_search    one thread per query.  Its candidate list (k <= 32 pairs) lives in LDS, entry-major, so the lanes of a wave hit
//               different banks and no runtime-indexed register array goes to scratch.  A row of cells along x is one
//               contiguous range of the CSR, so a full shell face is read as a few long runs.
//   k_flatten   one thread per (cell, 4 channels): the points of a cell are summed in CSR order by that one thread, the lanes of
//               a wave read 256 consecutive channels of the same token row in 16-byte pieces.
//   k_dwconv    one thread per (y, x, 4 channels), channels fastest: every tap is a coalesced row read, weights are [9, C].
//   k_inflate   one thread per (point, 4 channels).  All three fall back to one channel per thread where C % 4 != 0 or a
//               pointer is not 16-byte aligned; the operations per channel are the same.
//   k_neigh     one thread per (point, neighbour, channel); the <= 8 feature differences are recomputed per thread from rows
//               that the whole wave shares.
//
// Why every loop ends: shells run r = 0 .. max(G) - 1, a shell's loops run over the clipped cube, a cell's loop over its CSR
// range clipped to [0, n), the list insertion over k entries, the binary search over 32 halvings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_waffle.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int SEARCH_BLOCK = 128;
constexpr float INF = __builtin_huge_valf();
constexpr double DINF = __builtin_huge_val();
constexpr int64_t MAX_ELEMS = int64_t{1} << 40;

unsigned blocks_for(int64_t n, int block = BLOCK) { return static_cast<unsigned>((n + block - 1) / block); }

bool bad_rows(int64_t n, int64_t width) { return n < 0 || n >= (int64_t{1} << 31) || width <= 0 || n * width >= MAX_ELEMS; }

struct Cells {
  double lo[3];
  double h;
  int g[3];
};

bool bad_cells(const Cells &c) {
  if (!(c.h > 0.0) || c.g[0] <= 0 || c.g[1] <= 0 || c.g[2] <= 0) return true;
  return static_cast<int64_t>(c.g[0]) * c.g[1] * c.g[2] > PW_MAX_CELLS;
}

// ---- pw_voxel_keys ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_voxel_keys(const float *__restrict__ pc, int ld, int64_t n,
                                                      const float *__restrict__ mn, float voxel, int *__restrict__ key,
                                                      int *__restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= n * 3) return;
  const int64_t p = i / 3;
  const int a = static_cast<int>(i - p * 3);
  const float s = pc[p * ld + a] - mn[a];
  const float qf = s / voxel;
  int q = 0;
  if (qf >= 0.0f && qf < 2097152.0f) q = static_cast<int>(qf);
  else atomicOr(status, PW_STATUS_KEY_RANGE);
  key[i] = q;
}

// ---- pw_cell_index ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_cell_index(const float *__restrict__ pc, int ld, int64_t n, int d0, int d1,
                                                      double lo0, double lo1, double res0, double res1, int H, int W,
                                                      int *__restrict__ cell, int *__restrict__ status) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (p >= n) return;
  const double t0 = (static_cast<double>(pc[p * ld + d0]) - lo0) / res0;
  const double t1 = (static_cast<double>(pc[p * ld + d1]) - lo1) / res1;
  // truncation toward zero, as an integer cast: (-1, 0] maps to 0
  const bool ok = t0 > -1.0 && t0 < static_cast<double>(H) && t1 > -1.0 && t1 < static_cast<double>(W);
  int c = 0;
  if (ok) c = static_cast<int>(t0) * W + static_cast<int>(t1);
  else atomicOr(status, PW_STATUS_OFF_GRID);
  cell[p] = c;
}

// ---- pw_grid_cells ----------------------------------------------------------------------------------------------
__device__ __forceinline__ int home_cell(float v, double lo, double h, int g, bool *inside) {
  const double t = floor((static_cast<double>(v) - lo) / h);
  *inside = t >= 0.0 && t < static_cast<double>(g);
  return t >= 0.0 ? (t < static_cast<double>(g) ? static_cast<int>(t) : g - 1) : 0;     // a NaN lands in cell 0
}

__global__ __launch_bounds__(BLOCK) void k_grid_cells(const float *__restrict__ xyz, int ld, int64_t n, Cells c,
                                                      int *__restrict__ cell, int *__restrict__ status) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (p >= n) return;
  bool ix, iy, iz;
  const int cx = home_cell(xyz[p * ld + 0], c.lo[0], c.h, c.g[0], &ix);
  const int cy = home_cell(xyz[p * ld + 1], c.lo[1], c.h, c.g[1], &iy);
  const int cz = home_cell(xyz[p * ld + 2], c.lo[2], c.h, c.g[2], &iz);
  int out = 0;
  if (ix && iy && iz) out = (cz * c.g[1] + cy) * c.g[0] + cx;
  else atomicOr(status, PW_STATUS_OFF_GRID);
  cell[p] = out;
}

// ---- pw_cells_build ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_cells_build(const int *__restrict__ cell, const int *__restrict__ order, int n,
                                                       int ncell, int *__restrict__ start, int *__restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i < n) {                        // order[i] against order[i - 1]
    const int p = order[i];
    bool bad = p < 0 || p >= n;
    if (!bad) {
      const int c = cell[p];
      bad = c < 0 || c >= ncell;
      if (!bad && i > 0) {
        const int pp = order[i - 1];
        if (pp < 0 || pp >= n) bad = true;
        else {
          const int cp = cell[pp];
          bad = cp > c || (cp == c && pp >= p);
        }
      }
    }
    if (bad) atomicOr(status, PW_STATUS_ORDER);
  }
  if (i <= ncell) {                   // start[i] = the first position whose cell is >= i
    int lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = lo + (hi - lo) / 2;
      const int p = order[mid];
      const int c = (p >= 0 && p < n) ? cell[p] : ncell;
      if (c < static_cast<int>(i)) lo = mid + 1;
      else hi = mid;
    }
    start[i] = lo;
  }
}

// ---- pw_knn / pw_nearest ----------------------------------------------------------------------------------------
struct List {
  float *d;      // entry e of this thread at d[e * SEARCH_BLOCK]
  int *idx;
  int k, cnt;
  float worst_d;
  int worst_i;
};

__device__ __forceinline__ void list_offer(List &l, float d2, int i) {
  if (l.cnt == l.k && !(d2 < l.worst_d || (d2 == l.worst_d && i < l.worst_i))) return;
  int e = l.cnt < l.k ? l.cnt : l.k - 1;          // the slot that is free, or the worst one, which leaves
  for (int it = 0; it < PW_MAX_K && e > 0; ++it) {
    const float pd = l.d[(e - 1) * SEARCH_BLOCK];
    const int pi = l.idx[(e - 1) * SEARCH_BLOCK];
    if (pd < d2 || (pd == d2 && pi < i)) break;
    l.d[e * SEARCH_BLOCK] = pd;
    l.idx[e * SEARCH_BLOCK] = pi;
    --e;
  }
  l.d[e * SEARCH_BLOCK] = d2;
  l.idx[e * SEARCH_BLOCK] = i;
  if (l.cnt < l.k) ++l.cnt;
  if (l.cnt == l.k) {
    l.worst_d = l.d[(l.k - 1) * SEARCH_BLOCK];
    l.worst_i = l.idx[(l.k - 1) * SEARCH_BLOCK];
  }
}

__device__ __forceinline__ void scan_range(List &l, const float *__restrict__ xyz, int ld, int n,
                                           const int *__restrict__ order, int a, int b, float qx, float qy, float qz,
                                           int self) {
  a = a < 0 ? 0 : a;
  b = b > n ? n : b;
  for (int s = a; s < b; ++s) {
    const int i = order[s];
    if (i < 0 || i >= n || i == self) continue;
    const float dx = xyz[static_cast<int64_t>(i) * ld + 0] - qx;
    const float dy = xyz[static_cast<int64_t>(i) * ld + 1] - qy;
    const float dz = xyz[static_cast<int64_t>(i) * ld + 2] - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    list_offer(l, d2, i);
  }
}

// SELF: the queries are the points themselves and a point is no neighbour of itself.
template <bool SELF>
__global__ __launch_bounds__(SEARCH_BLOCK) void k_search(const float *__restrict__ xyz, int ld, int n,
                                                         const int *__restrict__ start, const int *__restrict__ order,
                                                         Cells c, const float *__restrict__ q, int ldq, int m, int k,
                                                         int *__restrict__ out) {
  __shared__ float s_d[PW_MAX_K * SEARCH_BLOCK];
  __shared__ int s_i[PW_MAX_K * SEARCH_BLOCK];
  const int t = blockIdx.x * SEARCH_BLOCK + threadIdx.x;
  if (t >= m) return;                 // no barrier below
  const float qx = q[static_cast<int64_t>(t) * ldq + 0], qy = q[static_cast<int64_t>(t) * ldq + 1],
              qz = q[static_cast<int64_t>(t) * ldq + 2];
  const float qv[3] = {qx, qy, qz};
  int hc[3];
  double outside2[3];
  for (int a = 0; a < 3; ++a) {
    bool in;
    hc[a] = home_cell(qv[a], c.lo[a], c.h, c.g[a], &in);
    const double below = c.lo[a] - static_cast<double>(qv[a]);
    const double above = static_cast<double>(qv[a]) - (c.lo[a] + static_cast<double>(c.g[a]) * c.h);
    double o = below > above ? below : above;
    o = o > 0.0 ? o : 0.0;
    outside2[a] = o * o;
  }
  List l;
  l.d = s_d + threadIdx.x;
  l.idx = s_i + threadIdx.x;
  l.k = k;
  l.cnt = 0;
  l.worst_d = INF;
  l.worst_i = 0x7fffffff;
  const int self = SELF ? t : -1;
  const int gx = c.g[0], gy = c.g[1], gz = c.g[2];
  const int rmax = (gx > gy ? (gx > gz ? gx : gz) : (gy > gz ? gy : gz));
  const int ncell = gx * gy * gz;
  for (int r = 0; r < rmax; ++r) {
    if (r > 0) {
      double L = DINF;
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
      if (l.cnt == l.k && static_cast<double>(l.worst_d) < (1.0 - 0x1p-20) * L) break;
    }
    const int z0 = hc[2] - r > 0 ? hc[2] - r : 0, z1 = hc[2] + r < gz - 1 ? hc[2] + r : gz - 1;
    const int y0 = hc[1] - r > 0 ? hc[1] - r : 0, y1 = hc[1] + r < gy - 1 ? hc[1] + r : gy - 1;
    const int x0 = hc[0] - r > 0 ? hc[0] - r : 0, x1 = hc[0] + r < gx - 1 ? hc[0] + r : gx - 1;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int row = (z * gy + y) * gx;
        const bool face = z - hc[2] == r || hc[2] - z == r || y - hc[1] == r || hc[1] - y == r;
        if (face) {                   // the whole clipped run along x
          const int ca = row + x0, cb = row + x1 + 1;
          if (ca >= 0 && cb <= ncell) scan_range(l, xyz, ld, n, order, start[ca], start[cb], qx, qy, qz, self);
        } else {                      // only the two end cells (r > 0 here)
          const int xa = hc[0] - r, xb = hc[0] + r;
          if (xa >= 0) scan_range(l, xyz, ld, n, order, start[row + xa], start[row + xa + 1], qx, qy, qz, self);
          if (xb <= gx - 1) scan_range(l, xyz, ld, n, order, start[row + xb], start[row + xb + 1], qx, qy, qz, self);
        }
      }
  }
  for (int e = 0; e < k; ++e)
    out[static_cast<int64_t>(t) * k + e] = e < l.cnt ? l.idx[e * SEARCH_BLOCK] : -1;
}

// V consecutive channels per thread: 4 (one 16-byte access) where C % 4 == 0 and every pointer is 16-byte aligned, else 1.
// The operations per channel are the same either way, so the results are the same bits.
template <int V>
__device__ __forceinline__ void ld(const float *p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p);
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
    v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void st(float *p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- pw_flatten -------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BLOCK) void k_flatten(const float *__restrict__ tokens, int n, int C,
                                                   const float *__restrict__ scale, const float *__restrict__ shift,
                                                   const int *__restrict__ start, const int *__restrict__ order, int ncell,
                                                   float *__restrict__ grid, int *__restrict__ status) {
  const int cv = C / V;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= static_cast<int64_t>(ncell) * cv) return;
  const int cell = static_cast<int>(i / cv), ch = static_cast<int>(i - static_cast<int64_t>(cell) * cv) * V;
  int a = start[cell], b = start[cell + 1];
  bool bad = a < 0 || b > n || a > b;
  a = a < 0 ? 0 : a;
  b = b > n ? n : b;
  float sc[V], sh[V], sum[V];
  ld<V>(scale + ch, sc);
  ld<V>(shift + ch, sh);
#pragma unroll
  for (int v = 0; v < V; ++v) sum[v] = 0.0f;
  int cnt = 0;
  for (int s = a; s < b; ++s) {
    const int p = order[s];
    if (p < 0 || p >= n) {
      bad = true;
      continue;
    }
    float x[V];
    ld<V>(tokens + static_cast<int64_t>(p) * C + ch, x);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float t = x[v] * sc[v] + sh[v];
      sum[v] = sum[v] + t;
    }
    ++cnt;
  }
  float r[V];
  const float w = cnt > 0 ? 1.0f / (static_cast<float>(cnt) + 1e-6f) : 0.0f;
#pragma unroll
  for (int v = 0; v < V; ++v) r[v] = cnt > 0 ? sum[v] * w : 0.0f;
  st<V>(grid + static_cast<int64_t>(cell) * C + ch, r);
  if (bad) atomicOr(status, PW_STATUS_INDEX);
}

// ---- pw_dwconv3x3 -----------------------------------------------------------------------------------------------
template <bool RELU, int V>
__global__ __launch_bounds__(BLOCK) void k_dwconv(const float *__restrict__ in, int H, int W, int C,
                                                  const float *__restrict__ w, const float *__restrict__ bias,
                                                  float *__restrict__ out) {
  const int cv = C / V;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= static_cast<int64_t>(H) * W * cv) return;
  const int ch = static_cast<int>(i % cv) * V;
  const int64_t site = i / cv;
  const int x = static_cast<int>(site % W), y = static_cast<int>(site / W);
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      float val[V], wt[V];
      ld<V>(in + (static_cast<int64_t>(yy) * W + xx) * C + ch, val);
      ld<V>(w + ((dy + 1) * 3 + (dx + 1)) * C + ch, wt);
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = acc[v] + wt[v] * val[v];
    }
  float b[V];
  ld<V>(bias + ch, b);
#pragma unroll
  for (int v = 0; v < V; ++v) {
    acc[v] = acc[v] + b[v];
    if (RELU) acc[v] = acc[v] > 0.0f ? acc[v] : 0.0f;
  }
  st<V>(out + site * C + ch, acc);
}

// ---- pw_inflate -------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BLOCK) void k_inflate(const float *tokens, int64_t n, int C, const float *__restrict__ scale,
                                                   const float *__restrict__ grid, const int *__restrict__ cell, int ncell,
                                                   float *out, int *__restrict__ status) {
  const int cv = C / V;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= n * cv) return;
  const int64_t p = i / cv;
  const int ch = static_cast<int>(i - p * cv) * V;
  const int c = cell[p];
  float r[V];
  ld<V>(tokens + p * C + ch, r);
  if (c >= 0 && c < ncell) {
    float sc[V], g[V];
    ld<V>(scale + ch, sc);
    ld<V>(grid + static_cast<int64_t>(c) * C + ch, g);
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = r[v] + sc[v] * g[v];
  } else {
    atomicOr(status, PW_STATUS_INDEX);
  }
  st<V>(out + p * C + ch, r);
}

// ---- pw_neigh_rows ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_neigh(const float *__restrict__ feat, int64_t n, int F,
                                                 const int *__restrict__ knn, int k, int64_t p0, int64_t rows_total,
                                                 const float *__restrict__ A, const float *__restrict__ b, int C,
                                                 float *__restrict__ rows, int *__restrict__ status) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= rows_total * C) return;
  const int64_t row = i / C;
  const int ch = static_cast<int>(i - row * C);
  const int64_t p = p0 + row / k;
  const int j = static_cast<int>(row % k);
  int64_t nb = knn[p * k + j];
  if (nb < 0 || nb >= n) {
    nb = p;
    atomicOr(status, PW_STATUS_INDEX);
  }
  float acc = b[ch];
  for (int f = 0; f < F; ++f) {
    const float d = feat[nb * F + f] - feat[p * F + f];
    acc = acc + A[f * C + ch] * d;
  }
  rows[i] = acc > 0.0f ? acc : 0.0f;
}

// ---- pw_group_max -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_group_max(const float *__restrict__ rows, int64_t np, int k, int C,
                                                     float *__restrict__ out, int ld_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (i >= np * C) return;
  const int64_t p = i / C;
  const int ch = static_cast<int>(i - p * C);
  float m = rows[(p * k) * C + ch];
  for (int j = 1; j < k; ++j) {
    const float v = rows[(p * k + j) * C + ch];
    m = v > m ? v : m;
  }
  out[p * ld_out + ch] = m;
}

Cells make_cells(double lox, double loy, double loz, double h, int32_t gx, int32_t gy, int32_t gz) {
  Cells c;
  c.lo[0] = lox;
  c.lo[1] = loy;
  c.lo[2] = loz;
  c.h = h;
  c.g[0] = gx;
  c.g[1] = gy;
  c.g[2] = gz;
  return c;
}

}  // namespace

extern "C" {

SIDE_EXPORTS(PW_FN, PW_ABI_VERSION)

int PW_FN(voxel_keys)(const float *pc, int32_t ld, int64_t n, const float *mn, float voxel, int32_t *key, int32_t *d_status,
                      void *stream) {
  if (bad_rows(n, ld) || ld < 3 || !(voxel > 0.0f)) return fail("pw_voxel_keys: n = %lld, ld = %d, voxel = %g", (long long)n, ld, voxel);
  if (!d_status || (n > 0 && (!pc || !mn || !key))) return fail("pw_voxel_keys: a NULL argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_voxel_keys, dim3(blocks_for(n * 3)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), pc, ld, n, mn,
                     voxel, key, d_status);
  SIDE_CHECK_LAUNCH("k_voxel_keys");
  return 0;
}

int PW_FN(cell_index)(const float *pc, int32_t ld, int64_t n, int32_t d0, int32_t d1, double lo0, double lo1, double res0,
                      double res1, int32_t H, int32_t W, int32_t *cell, int32_t *d_status, void *stream) {
  if (bad_rows(n, ld) || d0 < 0 || d0 >= ld || d1 < 0 || d1 >= ld || !(res0 > 0.0) || !(res1 > 0.0) || H <= 0 || W <= 0 ||
      static_cast<int64_t>(H) * W > PW_MAX_CELLS)
    return fail("pw_cell_index: n = %lld, ld = %d, dims (%d, %d), res (%g, %g), grid %d x %d", (long long)n, ld, d0, d1, res0,
                res1, H, W);
  if (!d_status || (n > 0 && (!pc || !cell))) return fail("pw_cell_index: a NULL argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_cell_index, dim3(blocks_for(n)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), pc, ld, n, d0, d1,
                     lo0, lo1, res0, res1, H, W, cell, d_status);
  SIDE_CHECK_LAUNCH("k_cell_index");
  return 0;
}

int PW_FN(grid_cells)(const float *xyz, int32_t ld, int64_t n, double lox, double loy, double loz, double h, int32_t gx,
                      int32_t gy, int32_t gz, int32_t *cell, int32_t *d_status, void *stream) {
  const Cells c = make_cells(lox, loy, loz, h, gx, gy, gz);
  if (bad_rows(n, ld) || ld < 3 || bad_cells(c)) return fail("pw_grid_cells: n = %lld, ld = %d, h = %g, grid %d x %d x %d", (long long)n, ld, h, gx, gy, gz);
  if (!d_status || (n > 0 && (!xyz || !cell))) return fail("pw_grid_cells: a NULL argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_grid_cells, dim3(blocks_for(n)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), xyz, ld, n, c, cell,
                     d_status);
  SIDE_CHECK_LAUNCH("k_grid_cells");
  return 0;
}

int PW_FN(cells_build)(const int32_t *cell, const int32_t *order, int64_t n, int32_t ncell, int32_t *start,
                       int32_t *d_status, void *stream) {
  if (n < 0 || n >= (int64_t{1} << 31) - BLOCK || ncell <= 0 || ncell > PW_MAX_CELLS)
    return fail("pw_cells_build: n = %lld, ncell = %d", (long long)n, ncell);
  if (!start || !d_status || (n > 0 && (!cell || !order))) return fail("pw_cells_build: a NULL argument");
  const int64_t threads = n > ncell + 1 ? n : ncell + 1;
  hipLaunchKernelGGL(k_cells_build, dim3(blocks_for(threads)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), cell, order,
                     static_cast<int>(n), ncell, start, d_status);
  SIDE_CHECK_LAUNCH("k_cells_build");
  return 0;
}

int PW_FN(knn)(const float *xyz, int32_t ld, int64_t n, const int32_t *start, const int32_t *order, double lox, double loy,
               double loz, double h, int32_t gx, int32_t gy, int32_t gz, int32_t k, int32_t *out, void *stream) {
  const Cells c = make_cells(lox, loy, loz, h, gx, gy, gz);
  if (bad_rows(n, ld) || ld < 3 || bad_cells(c) || k < 1 || k > PW_MAX_K || k >= n)
    return fail("pw_knn: n = %lld, ld = %d, k = %d (1 .. %d, < n), h = %g, grid %d x %d x %d", (long long)n, ld, k, PW_MAX_K,
                h, gx, gy, gz);
  if (!xyz || !start || !order || !out) return fail("pw_knn: a NULL argument");
  hipLaunchKernelGGL(k_search<true>, dim3(blocks_for(n, SEARCH_BLOCK)), dim3(SEARCH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), xyz, ld, static_cast<int>(n), start, order, c, xyz, ld,
                     static_cast<int>(n), k, out);
  SIDE_CHECK_LAUNCH("k_search<knn>");
  return 0;
}

int PW_FN(nearest)(const float *xyz, int32_t ld, int64_t n, const int32_t *start, const int32_t *order, double lox,
                   double loy, double loz, double h, int32_t gx, int32_t gy, int32_t gz, const float *q, int32_t ldq,
                   int64_t m, int32_t *out, void *stream) {
  const Cells c = make_cells(lox, loy, loz, h, gx, gy, gz);
  if (bad_rows(n, ld) || n < 1 || ld < 3 || bad_cells(c) || bad_rows(m, ldq) || ldq < 3)
    return fail("pw_nearest: n = %lld, ld = %d, m = %lld, ldq = %d, h = %g, grid %d x %d x %d", (long long)n, ld, (long long)m,
                ldq, h, gx, gy, gz);
  if (!xyz || !start || !order || (m > 0 && (!q || !out))) return fail("pw_nearest: a NULL argument");
  if (m == 0) return 0;
  hipLaunchKernelGGL(k_search<false>, dim3(blocks_for(m, SEARCH_BLOCK)), dim3(SEARCH_BLOCK), 0,
                     static_cast<hipStream_t>(stream), xyz, ld, static_cast<int>(n), start, order, c, q, ldq,
                     static_cast<int>(m), 1, out);
  SIDE_CHECK_LAUNCH("k_search<nearest>");
  return 0;
}

int PW_FN(flatten)(const float *tokens, int64_t n, int32_t C, const float *scale, const float *shift, const int32_t *start,
                   const int32_t *order, int32_t ncell, float *grid, int32_t *d_status, void *stream) {
  if (bad_rows(n, C) || ncell <= 0 || ncell > PW_MAX_CELLS) return fail("pw_flatten: n = %lld, C = %d, ncell = %d", (long long)n, C, ncell);
  if (!scale || !shift || !start || !grid || !d_status || (n > 0 && (!tokens || !order))) return fail("pw_flatten: a NULL argument");
  const bool wide = C % 4 == 0 && aligned16(tokens) && aligned16(scale) && aligned16(shift) && aligned16(grid);
  const hipStream_t st_ = static_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL(k_flatten<4>, dim3(blocks_for(static_cast<int64_t>(ncell) * (C / 4))), dim3(BLOCK), 0, st_, tokens,
                       static_cast<int>(n), C, scale, shift, start, order, ncell, grid, d_status);
  else
    hipLaunchKernelGGL(k_flatten<1>, dim3(blocks_for(static_cast<int64_t>(ncell) * C)), dim3(BLOCK), 0, st_, tokens,
                       static_cast<int>(n), C, scale, shift, start, order, ncell, grid, d_status);
  SIDE_CHECK_LAUNCH("k_flatten");
  return 0;
}

int PW_FN(dwconv3x3)(const float *in, int32_t H, int32_t W, int32_t C, const float *w, const float *bias, int32_t relu,
                     float *out, void *stream) {
  if (H <= 0 || W <= 0 || C <= 0 || static_cast<int64_t>(H) * W > PW_MAX_CELLS || static_cast<int64_t>(H) * W * C >= MAX_ELEMS)
    return fail("pw_dwconv3x3: grid %d x %d x %d", H, W, C);
  if (!in || !w || !bias || !out) return fail("pw_dwconv3x3: a NULL argument");
  if (in == out) return fail("pw_dwconv3x3: out may not alias in");
  const bool wide = C % 4 == 0 && aligned16(in) && aligned16(w) && aligned16(bias) && aligned16(out);
  const dim3 g(blocks_for(static_cast<int64_t>(H) * W * (wide ? C / 4 : C)));
  const hipStream_t st_ = static_cast<hipStream_t>(stream);
  if (relu && wide) hipLaunchKernelGGL((k_dwconv<true, 4>), g, dim3(BLOCK), 0, st_, in, H, W, C, w, bias, out);
  else if (relu) hipLaunchKernelGGL((k_dwconv<true, 1>), g, dim3(BLOCK), 0, st_, in, H, W, C, w, bias, out);
  else if (wide) hipLaunchKernelGGL((k_dwconv<false, 4>), g, dim3(BLOCK), 0, st_, in, H, W, C, w, bias, out);
  else hipLaunchKernelGGL((k_dwconv<false, 1>), g, dim3(BLOCK), 0, st_, in, H, W, C, w, bias, out);
  SIDE_CHECK_LAUNCH("k_dwconv");
  return 0;
}

int PW_FN(inflate)(const float *tokens, int64_t n, int32_t C, const float *scale, const float *grid, const int32_t *cell,
                   int32_t ncell, float *out, int32_t *d_status, void *stream) {
  if (bad_rows(n, C) || ncell <= 0 || ncell > PW_MAX_CELLS) return fail("pw_inflate: n = %lld, C = %d, ncell = %d", (long long)n, C, ncell);
  if (!d_status || (n > 0 && (!tokens || !scale || !grid || !cell || !out))) return fail("pw_inflate: a NULL argument");
  if (n == 0) return 0;
  const bool wide = C % 4 == 0 && aligned16(tokens) && aligned16(scale) && aligned16(grid) && aligned16(out);
  const hipStream_t st_ = static_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL(k_inflate<4>, dim3(blocks_for(n * (C / 4))), dim3(BLOCK), 0, st_, tokens, n, C, scale, grid, cell, ncell,
                       out, d_status);
  else
    hipLaunchKernelGGL(k_inflate<1>, dim3(blocks_for(n * C)), dim3(BLOCK), 0, st_, tokens, n, C, scale, grid, cell, ncell, out,
                       d_status);
  SIDE_CHECK_LAUNCH("k_inflate");
  return 0;
}

int PW_FN(neigh_rows)(const float *feat, int64_t n, int32_t F, const int32_t *knn, int32_t k, int64_t p0, int64_t np,
                      const float *A, const float *b, int32_t C, float *rows, int32_t *d_status, void *stream) {
  if (bad_rows(n, C) || F < 1 || F > PW_MAX_FEAT || k < 1 || k > PW_MAX_K || p0 < 0 || np < 0 || p0 + np > n ||
      np * k * C >= MAX_ELEMS)
    return fail("pw_neigh_rows: n = %lld, F = %d, k = %d, points %lld + %lld, C = %d", (long long)n, F, k, (long long)p0,
                (long long)np, C);
  if (!d_status || (np > 0 && (!feat || !knn || !A || !b || !rows))) return fail("pw_neigh_rows: a NULL argument");
  if (np == 0) return 0;
  hipLaunchKernelGGL(k_neigh, dim3(blocks_for(np * k * C)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), feat, n, F, knn,
                     k, p0, np * k, A, b, C, rows, d_status);
  SIDE_CHECK_LAUNCH("k_neigh");
  return 0;
}

int PW_FN(group_max)(const float *rows, int64_t np, int32_t k, int32_t C, float *out, int32_t ld_out, void *stream) {
  if (np < 0 || k < 1 || C <= 0 || ld_out < C || np * k * C >= MAX_ELEMS || np * ld_out >= MAX_ELEMS)
    return fail("pw_group_max: np = %lld, k = %d, C = %d, ld_out = %d", (long long)np, k, C, ld_out);
  if (np > 0 && (!rows || !out)) return fail("pw_group_max: a NULL argument");
  if (np == 0) return 0;
  hipLaunchKernelGGL(k_group_max, dim3(blocks_for(np * C)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), rows, np, k, C,
                     out, ld_out);
  SIDE_CHECK_LAUNCH("k_group_max");
  return 0;
}

}  // extern "C"

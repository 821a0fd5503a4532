// Training kernels of the dense <-> rows operators and of local max pooling for gfx950 (include/pasco_rowgrad.h).
//
// k_dense_rows / k_rows_dense move a [n, c] row matrix from / to the sites of a [B, c, X, Y, Z] grid.  The two sides want
// opposite lane orders: a row's channels are contiguous on the row side (c * 4 bytes), while on the dense side one channel of
// neighbouring sites is contiguous and a row's channels lie X * Y * Z elements apart.  A thread per (row, channel) therefore
// strides one of the two sides by a whole channel plane per lane.  Here a workgroup of 256 threads owns PR_TILE = 64 consecutive
// rows x 64 channels and transposes them through LDS:
//   dense side: lane = row, wave w takes channels w, w + 4, ... of the tile.  Rows in to_sparse order are runs of consecutive
//               sites along z, so the 64 lanes of one access touch a few contiguous runs of one channel plane;
//   row side:   lane = channel, wave w takes rows w, w + 4, ...: 256 contiguous bytes per row.
// The tile is 64 x 65 dwords: with the one-dword pad the column accesses of the dense side (address lane * 65 + channel) and the
// row accesses of the row side (address row * 65 + lane) both put the 32 lanes of a ds_read_b32 / ds_write_b32 lane group on 32
// different banks.  Tails (n % 64, c % 64) are masked: nothing outside the arrays is read or written, the site of a row is
// range-checked before it is used, and a skipped row moves zeros (k_dense_rows) or nothing (k_rows_dense).
//
// k_maxpool_arg / k_maxpool_bwd: one thread per output element, offsets visited in ascending order.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_rowgrad.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int TILE = PR_TILE;
constexpr int PAD = TILE + 1;
constexpr int PER_WAVE = TILE / (BLOCK / 64);     // channels (dense side) or rows (row side) of the tile per wave

struct Grid {
  int b, x, y, z;
};

// floor(v / ts), ts >= 1
__device__ __forceinline__ int64_t floor_div(int64_t v, int64_t ts) {
  int64_t q = v / ts;
  if (v % ts != 0 && v < 0) --q;
  return q;
}

// Element offset of channel 0 of the site of coordinate p (channel ch lies ch * per_b further), or -1 for a skipped row.
// wrap: ph_to_dense's rule (an index in [-dim, 0) wraps); otherwise ph_dense_gather's (no wrap).
__device__ __forceinline__ int64_t site_base(int4 p, int64_t x, int64_t y, int64_t z, bool wrap, Grid d, int c, int64_t per_b) {
  if (wrap) {
    if (x < 0) x += d.x;
    if (y < 0) y += d.y;
    if (z < 0) z += d.z;
  }
  if (p.x < 0 || p.x >= d.b || x < 0 || x >= d.x || y < 0 || y >= d.y || z < 0 || z >= d.z) return -1;
  return (int64_t)p.x * c * per_b + (x * d.y + y) * d.z + z;
}

__global__ void __launch_bounds__(BLOCK)
    k_dense_rows(const float *__restrict__ dense, const int4 *__restrict__ coords, int64_t n, int c, int mx, int my, int mz,
                 int ts, Grid d, int ctiles, float *__restrict__ rows) {
  __shared__ float tile[TILE * PAD];
  const int64_t bid = blockIdx.x;
  const int c0 = (int)(bid % ctiles) * TILE;
  const int64_t r0 = (bid / ctiles) * TILE;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t per_b = (int64_t)d.x * d.y * d.z;

  // dense side: lane = row
  int64_t base = -1;
  if (r0 + lane < n) {
    const int4 p = coords[r0 + lane];
    base = site_base(p, floor_div((int64_t)p.y - mx, ts), floor_div((int64_t)p.z - my, ts), floor_div((int64_t)p.w - mz, ts),
                     true, d, c, per_b);
  }
  float v[PER_WAVE];
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int ch = c0 + wave + 4 * j;
    v[j] = (base >= 0 && ch < c) ? dense[base + (int64_t)ch * per_b] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) tile[lane * PAD + wave + 4 * j] = v[j];
  __syncthreads();

  // row side: lane = channel
  const int ch = c0 + lane;
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int r = wave + 4 * j;
    if (r0 + r < n && ch < c) rows[(r0 + r) * c + ch] = tile[r * PAD + lane];
  }
}

__global__ void __launch_bounds__(BLOCK)
    k_rows_dense(const float *__restrict__ rows, const int4 *__restrict__ sc, int64_t n, int c, Grid d, int ctiles,
                 float *__restrict__ dense) {
  __shared__ float tile[TILE * PAD];
  const int64_t bid = blockIdx.x;
  const int c0 = (int)(bid % ctiles) * TILE;
  const int64_t r0 = (bid / ctiles) * TILE;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t per_b = (int64_t)d.x * d.y * d.z;

  // the site of this lane's row (dense side), read early: its latency overlaps the row loads
  int64_t base = -1;
  if (r0 + lane < n) {
    const int4 p = sc[r0 + lane];
    base = site_base(p, p.y, p.z, p.w, false, d, c, per_b);
  }

  // row side: lane = channel
  const int ch_row = c0 + lane;
  float v[PER_WAVE];
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int r = wave + 4 * j;
    v[j] = (r0 + r < n && ch_row < c) ? rows[(r0 + r) * c + ch_row] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) tile[(wave + 4 * j) * PAD + lane] = v[j];
  __syncthreads();

  // dense side: lane = row
  if (base < 0) return;
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int ch = c0 + wave + 4 * j;
    if (ch < c) dense[base + (int64_t)ch * per_b] = tile[lane * PAD + wave + 4 * j];
  }
}

__global__ void __launch_bounds__(BLOCK)
    k_maxpool_arg(const float *__restrict__ in, int64_t n_in, int c, const int32_t *__restrict__ nbr, int kvol, int64_t n_out,
                  const float *__restrict__ out, int32_t *__restrict__ arg) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_out * c) return;
  const int64_t o = t / c;
  const int ch = (int)(t - o * c);
  const float m = out[t];
  int32_t a = -1;
  for (int k = 0; k < kvol; ++k) {
    const int32_t r = nbr[(int64_t)k * n_out + o];
    if (r >= 0 && r < n_in && in[(int64_t)r * c + ch] == m) {
      a = r;
      break;
    }
  }
  arg[t] = a;
}

__global__ void __launch_bounds__(BLOCK)
    k_maxpool_bwd(const float *__restrict__ dy, int64_t n_out, int c, const int32_t *__restrict__ arg,
                  const int32_t *__restrict__ inv, int kvol, int64_t n_in, float *__restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= n_in * c) return;
  const int64_t i = t / c;
  const int ch = (int)(t - i * c);
  float s = 0.f;
  for (int k = 0; k < kvol; ++k) {
    const int32_t o = inv[(int64_t)k * n_in + i];
    if (o >= 0 && o < n_out && arg[(int64_t)o * c + ch] == i) s += dy[(int64_t)o * c + ch];
  }
  dx[t] = s;
}

inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

// grid of the tile kernels, or -1
int64_t tile_grid(int64_t n, int32_t c, int *ctiles) {
  *ctiles = (c + TILE - 1) / TILE;
  const int64_t g = ((n + TILE - 1) / TILE) * *ctiles;
  return g < (1ll << 31) ? g : -1;
}

bool grid_ok(int32_t c, int32_t B, int32_t X, int32_t Y, int32_t Z) {
  if (c < 1 || B < 0 || X < 0 || Y < 0 || Z < 0) return false;
  return (double)B * c * X * Y * Z < 0x1p60;      // the element offsets are int64
}

}  // namespace

SIDE_EXPORTS(PR_FN, PR_ABI_VERSION)

extern "C" int PR_FN(dense_rows)(const float *dense, int32_t c, int32_t B, int32_t X, int32_t Y, int32_t Z,
                                 const int32_t *coords, int64_t n, int32_t min_x, int32_t min_y, int32_t min_z, int32_t ts,
                                 float *rows, void *stream) {
  if (!grid_ok(c, B, X, Y, Z)) return fail("dense_rows: c = %d, grid (%d, %d, %d, %d) outside the served range", c, B, X, Y, Z);
  if (ts < 1) return fail("dense_rows: ts = %d, must be >= 1", ts);
  if (n < 0 || n >= (1ll << 31)) return fail("dense_rows: n = %lld outside [0, 2^31)", (long long)n);
  if (n == 0) return 0;
  if (coords == nullptr || rows == nullptr || (dense == nullptr && (int64_t)B * X * Y * Z > 0))
    return fail("dense_rows: null pointer");
  int ctiles;
  const int64_t grid = tile_grid(n, c, &ctiles);
  if (grid < 0) return fail("dense_rows: too many workgroups for n = %lld, c = %d", (long long)n, c);
  const Grid d{B, X, Y, Z};
  hipLaunchKernelGGL(k_dense_rows, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), dense, (const int4 *)coords, n, c, min_x,
                     min_y, min_z, ts, d, ctiles, rows);
  SIDE_CHECK_LAUNCH("k_dense_rows");
  return 0;
}

extern "C" int PR_FN(rows_dense)(const float *rows, int64_t n, int32_t c, const int32_t *site_coords, int32_t B, int32_t X,
                                 int32_t Y, int32_t Z, float *dense, void *stream) {
  if (!grid_ok(c, B, X, Y, Z)) return fail("rows_dense: c = %d, grid (%d, %d, %d, %d) outside the served range", c, B, X, Y, Z);
  if (n < 0 || n >= (1ll << 31)) return fail("rows_dense: n = %lld outside [0, 2^31)", (long long)n);
  const int64_t elems = (int64_t)B * c * X * Y * Z;
  if (elems == 0) return 0;
  if (dense == nullptr) return fail("rows_dense: null dense");
  SIDE_CHECK_HIP(hipMemsetAsync(dense, 0, (size_t)elems * sizeof(float), st_of(stream)));
  if (n == 0) return 0;
  if (rows == nullptr || site_coords == nullptr) return fail("rows_dense: null pointer");
  int ctiles;
  const int64_t grid = tile_grid(n, c, &ctiles);
  if (grid < 0) return fail("rows_dense: too many workgroups for n = %lld, c = %d", (long long)n, c);
  const Grid d{B, X, Y, Z};
  hipLaunchKernelGGL(k_rows_dense, dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), rows, (const int4 *)site_coords, n, c, d,
                     ctiles, dense);
  SIDE_CHECK_LAUNCH("k_rows_dense");
  return 0;
}

extern "C" int PR_FN(maxpool_arg)(const float *in, int64_t n_in, int32_t c, const int32_t *nbr, int32_t K, int64_t n_out,
                                  const float *out, int32_t *arg, void *stream) {
  if (K < 1 || K > PR_MAX_KVOL) return fail("maxpool_arg: K = %d outside [1, %d]", K, PR_MAX_KVOL);
  if (c < 1 || n_in < 0 || n_out < 0 || n_in >= (1ll << 31) || n_out >= (1ll << 31))
    return fail("maxpool_arg: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (n_out == 0) return 0;
  if (nbr == nullptr || out == nullptr || arg == nullptr || (in == nullptr && n_in > 0)) return fail("maxpool_arg: null pointer");
  const int64_t blocks = (n_out * c + BLOCK - 1) / BLOCK;
  if (blocks >= (1ll << 31)) return fail("maxpool_arg: %lld workgroups", (long long)blocks);
  hipLaunchKernelGGL(k_maxpool_arg, dim3((unsigned)blocks), dim3(BLOCK), 0, st_of(stream), in, n_in, c, nbr, K, n_out, out, arg);
  SIDE_CHECK_LAUNCH("k_maxpool_arg");
  return 0;
}

extern "C" int PR_FN(maxpool_bwd)(const float *dy, int64_t n_out, int32_t c, const int32_t *arg, const int32_t *inv, int32_t K,
                                  int64_t n_in, float *dx, void *stream) {
  if (K < 1 || K > PR_MAX_KVOL) return fail("maxpool_bwd: K = %d outside [1, %d]", K, PR_MAX_KVOL);
  if (c < 1 || n_in < 0 || n_out < 0 || n_in >= (1ll << 31) || n_out >= (1ll << 31))
    return fail("maxpool_bwd: c = %d, n_in = %lld, n_out = %lld outside the served range", c, (long long)n_in, (long long)n_out);
  if (n_in == 0) return 0;
  if (dx == nullptr) return fail("maxpool_bwd: null dx");
  if (n_out == 0) {
    SIDE_CHECK_HIP(hipMemsetAsync(dx, 0, (size_t)n_in * c * sizeof(float), st_of(stream)));
    return 0;
  }
  if (dy == nullptr || arg == nullptr || inv == nullptr) return fail("maxpool_bwd: null pointer");
  const int64_t blocks = (n_in * c + BLOCK - 1) / BLOCK;
  if (blocks >= (1ll << 31)) return fail("maxpool_bwd: %lld workgroups", (long long)blocks);
  hipLaunchKernelGGL(k_maxpool_bwd, dim3((unsigned)blocks), dim3(BLOCK), 0, st_of(stream), dy, n_out, c, arg, inv, K, n_in, dx);
  SIDE_CHECK_LAUNCH("k_maxpool_bwd");
  return 0;
}

// Training kernels of the sparse convolution family for gfx950 (include/pasco_grad.h): the inverse of a neighbour table, the
// weight gradient and the bias gradient.  The input gradient needs no kernel of its own: it is the forward convolution over the
// inverse table with the transposed kernel (pasco_amd/me/autograd.py).
//
// k_wgrad: dw[k] = sum_o x[nbr[k][o]]^T dy[o].  The rows are the contraction, so they are the K dimension of
// v_mfma_f32_32x32x2_f32 (exact fp32): one MFMA takes two rows, operand A = x[row h][32 cin], operand B = dy[row h][32 cout]
// (lane l holds column l & 31 of row h = l >> 5 for both), and accumulates the 32 x 32 (cin, cout) tile.  A workgroup (256
// threads = 2 x 2 waves, each TM x TN MFMA tiles) owns one kernel offset, one slab of consecutive output rows and one
// (64 TM cin) x (64 TN cout) tile.  It walks the slab in chunks of 32 rows: the gathered x rows and the dy rows go through
// registers into two ROW-MAJOR LDS tiles (an absent neighbour is a zero row in both), and the waves read them back with
// ds_read_b32: the 32 lanes of a lane group read 32 consecutive dwords of one row, so the read is conflict free whatever the row
// stride and the "transposed" operand needs no transpose at all (MI355X_MICROARCH.md "LDS": ds_read_b32 groups {0-31}, {32-63},
// bank = dword mod 32).  The stores are ds_write_b128 of 8 lanes x 16 bytes = 32 consecutive dwords per group.
// The next chunk's rows are loaded into registers while the current one is multiplied.
//
// Determinism: a workgroup adds its rows in ascending order; the slabs' partial tiles are added in ascending slab order by
// k_wgrad_reduce; the slab length is a function of the shapes (pg_wgrad_slab_rows).  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_grad.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BLOCK = 256;
constexpr int WG_CHUNK = 32;     // rows per LDS stage

struct WgradArgs {
  const float *x;
  const float *dy;
  const int32_t *nbr;
  float *part;            // [slabs, K, cin, cout] (the workspace), or dw itself when there is one slab
  int64_t n_in, n_out, slab_rows;
  int cin, cout, kvol;
  int ci_tiles, co_tiles;
  int vec_x, vec_y;       // rows may be read as float4 (channels % 4 == 0 and a 16-byte aligned base)
};

__global__ void k_nbr_scatter(const int32_t *__restrict__ nbr, int64_t total, int64_t n_out, int64_t n_in,
                              int32_t *__restrict__ inv) {
  const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (t >= total) return;
  const int64_t k = t / n_out;
  const int64_t o = t - k * n_out;
  const int32_t i = nbr[t];
  if (i >= 0 && i < n_in) inv[k * n_in + i] = (int32_t)o;
}

template <int TM, int TN>
__global__ void __launch_bounds__(BLOCK) k_wgrad(WgradArgs a) {
  constexpr int BCI = 64 * TM, BCO = 64 * TN;
  constexpr int X_TPR = BCI / 4, Y_TPR = BCO / 4;          // float4 slots per row
  constexpr int X_SLOTS = WG_CHUNK * X_TPR / BLOCK;        // float4 slots per thread and chunk
  constexpr int Y_SLOTS = WG_CHUNK * Y_TPR / BLOCK;
  static_assert(X_SLOTS >= 1 && Y_SLOTS >= 1, "loader shape");

  __shared__ __attribute__((aligned(16))) float Xs[WG_CHUNK * BCI];
  __shared__ __attribute__((aligned(16))) float Ys[WG_CHUNK * BCO];

  // tile fastest: the workgroups that gather the same rows for other column tiles run next to each other
  const int tiles = a.ci_tiles * a.co_tiles;
  const int64_t bid = blockIdx.x;
  const int tile = (int)(bid % tiles);
  const int64_t rest = bid / tiles;
  const int k = (int)(rest % a.kvol);
  const int64_t slab = rest / a.kvol;
  const int ci0 = (tile / a.co_tiles) * BCI;
  const int co0 = (tile % a.co_tiles) * BCO;
  const int64_t o_begin = slab * a.slab_rows;
  const int64_t o_end = (o_begin + a.slab_rows < a.n_out) ? o_begin + a.slab_rows : a.n_out;
  const int nchunks = (int)((o_end - o_begin + WG_CHUNK - 1) / WG_CHUNK);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5;
  const int l31 = lane & 31;
  const int cin = a.cin, cout = a.cout;
  const int32_t *nbr_k = a.nbr + (int64_t)k * a.n_out;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 rx[X_SLOTS], ry[Y_SLOTS];
  int idx_x[X_SLOTS], idx_y[Y_SLOTS];      // input row of each slot's output row in the chunk being loaded, -1 = zero row

  // neighbour of output row `o` (absent, past the slab, or out of the input's range -> -1)
  auto nbr_of = [&](int64_t o) {
    int idx = -1;
    if (o < o_end) {
      idx = nbr_k[o];
      if (idx >= a.n_in) idx = -1;
    }
    return idx;
  };
  auto load_idx = [&](int chunk) {
    const int64_t o0 = o_begin + (int64_t)chunk * WG_CHUNK;
#pragma unroll
    for (int p = 0; p < X_SLOTS; ++p) idx_x[p] = nbr_of(o0 + (tid + p * BLOCK) / X_TPR);
#pragma unroll
    for (int p = 0; p < Y_SLOTS; ++p) idx_y[p] = nbr_of(o0 + (tid + p * BLOCK) / Y_TPR);
  };
  auto load_row4 = [&](const float *row, int c, int cols, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
      if (c < cols) v = *reinterpret_cast<const float4 *>(row + c);
    } else {
      if (c + 0 < cols) v.x = row[c + 0];
      if (c + 1 < cols) v.y = row[c + 1];
      if (c + 2 < cols) v.z = row[c + 2];
      if (c + 3 < cols) v.w = row[c + 3];
    }
    return v;
  };
  auto load_rows = [&](int chunk) {
    const int64_t o0 = o_begin + (int64_t)chunk * WG_CHUNK;
#pragma unroll
    for (int p = 0; p < X_SLOTS; ++p) {
      const int slot = tid + p * BLOCK;
      const int c = ci0 + (slot % X_TPR) * 4;
      rx[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx_x[p] >= 0) rx[p] = load_row4(a.x + (int64_t)idx_x[p] * cin, c, cin, a.vec_x);
    }
#pragma unroll
    for (int p = 0; p < Y_SLOTS; ++p) {
      const int slot = tid + p * BLOCK;
      const int c = co0 + (slot % Y_TPR) * 4;
      ry[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx_y[p] >= 0) ry[p] = load_row4(a.dy + (o0 + slot / Y_TPR) * cout, c, cout, a.vec_y);
    }
  };
  auto store_rows = [&]() {
#pragma unroll
    for (int p = 0; p < X_SLOTS; ++p) *reinterpret_cast<float4 *>(&Xs[(tid + p * BLOCK) * 4]) = rx[p];
#pragma unroll
    for (int p = 0; p < Y_SLOTS; ++p) *reinterpret_cast<float4 *>(&Ys[(tid + p * BLOCK) * 4]) = ry[p];
  };
  // a wave whose 32 TM x 32 TN tile lies beyond the channels (cin or cout <= 32 in a 64-wide tile) has only zeros to add
  const bool live = ci0 + wm * TM * 32 < cin && co0 + wn * TN * 32 < cout;
  auto compute = [&]() {
    if (!live) return;
#pragma unroll 4
    for (int r2 = 0; r2 < WG_CHUNK / 2; ++r2) {
      const int row = 2 * r2 + h;
      float av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = Xs[row * BCI + (wm * TM + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < TN; ++j) bv[j] = Ys[row * BCO + (wn * TN + j) * 32 + l31];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  };

  if (nchunks > 0) {
    load_idx(0);
    load_rows(0);
    if (nchunks > 1) load_idx(1);
  }
  for (int c = 0; c < nchunks; ++c) {
    store_rows();
    __syncthreads();
    if (c + 1 < nchunks) {
      load_rows(c + 1);
      if (c + 2 < nchunks) load_idx(c + 2);
    }
    compute();
    __syncthreads();
  }

  // C/D layout of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); row = cin, column = cout
  float *dst = a.part + ((int64_t)slab * a.kvol + k) * cin * cout;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = co0 + (wn * TN + j) * 32 + l31;
    if (co >= cout) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (ci < cin) dst[(int64_t)ci * cout + co] = acc[i][j][r];
      }
    }
  }
}

// dw[e] = ((part[0][e] + part[1][e]) + part[2][e]) + ...: ascending slab order
__global__ void k_wgrad_reduce(const float *__restrict__ part, int64_t elems, int64_t slabs, float *__restrict__ dw) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= elems) return;
  float s = part[e];
  for (int64_t q = 1; q < slabs; ++q) s += part[q * elems + e];
  dw[e] = s;
}

// One block: 64 columns x PG_COLSUM_ROWS rows; thread (col, chain) adds rows chain, chain + 4, ... of its block, the four
// chains are added 0 + 1 + 2 + 3.
__global__ void __launch_bounds__(BLOCK) k_colsum_part(const float *__restrict__ dy, int64_t n, int c, float *__restrict__ part) {
  __shared__ float sm[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int chain = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * PG_COLSUM_ROWS;
  const int64_t r1 = (r0 + PG_COLSUM_ROWS < n) ? r0 + PG_COLSUM_ROWS : n;
  float s = 0.f;
  if (col < c)
    for (int64_t r = r0 + chain; r < r1; r += 4) s += dy[r * c + col];
  sm[chain][threadIdx.x & 63] = s;
  __syncthreads();
  if (chain == 0 && col < c) {
    const int l = threadIdx.x;
    part[(int64_t)blockIdx.y * c + col] = ((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l];
  }
}

__global__ void k_colsum_finish(const float *__restrict__ part, int64_t blocks, int c, float *__restrict__ out) {
  const int col = blockIdx.x * BLOCK + threadIdx.x;
  if (col >= c) return;
  float s = part[col];
  for (int64_t b = 1; b < blocks; ++b) s += part[b * c + col];
  out[col] = s;
}

inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

bool wgrad_shape_ok(int32_t K, int32_t cin, int32_t cout, int64_t n_out) {
  return K >= 1 && K <= PG_MAX_KVOL && cin >= 1 && cout >= 1 && n_out >= 0 && n_out < (1ll << 31) &&
         (int64_t)K * cin * cout < (1ll << 31);
}

int64_t slab_rows_of(int32_t K, int32_t cin, int32_t cout, int64_t n_out) {
  int64_t rows = PG_SLAB_ROWS;
  const int64_t tile_bytes = (int64_t)K * cin * cout * 4;
  while (rows < n_out && ((n_out + rows - 1) / rows) * tile_bytes > PG_WGRAD_WORKSPACE_CAP) rows *= 2;
  return rows;
}

}  // namespace

SIDE_EXPORTS(PG_FN, PG_ABI_VERSION)

extern "C" int PG_FN(nbr_invert)(const int32_t *nbr, int32_t K, int64_t n_out, int64_t n_in, int32_t *inv, void *stream) {
  if (K < 1 || K > PG_MAX_KVOL) return fail("nbr_invert: K = %d outside [1, %d]", K, PG_MAX_KVOL);
  if (n_out < 0 || n_in < 0 || n_out >= (1ll << 31) || n_in >= (1ll << 31))
    return fail("nbr_invert: n_out = %lld / n_in = %lld outside [0, 2^31)", (long long)n_out, (long long)n_in);
  if (n_in == 0) return 0;
  if (inv == nullptr || (n_out > 0 && nbr == nullptr)) return fail("nbr_invert: null pointer");
  SIDE_CHECK_HIP(hipMemsetAsync(inv, 0xff, (size_t)K * n_in * sizeof(int32_t), st_of(stream)));     // every byte 0xff = -1
  if (n_out == 0) return 0;
  const int64_t total = (int64_t)K * n_out;
  const int64_t blocks = (total + BLOCK - 1) / BLOCK;
  if (blocks >= (1ll << 31)) return fail("nbr_invert: table too large");
  hipLaunchKernelGGL(k_nbr_scatter, dim3((unsigned)blocks), dim3(BLOCK), 0, st_of(stream), nbr, total, n_out, n_in, inv);
  SIDE_CHECK_LAUNCH("k_nbr_scatter");
  return 0;
}

extern "C" int64_t PG_FN(wgrad_slab_rows)(int32_t K, int32_t cin, int32_t cout, int64_t n_out) {
  if (!wgrad_shape_ok(K, cin, cout, n_out)) return -1;
  return slab_rows_of(K, cin, cout, n_out);
}

extern "C" int64_t PG_FN(wgrad_workspace_bytes)(int32_t K, int32_t cin, int32_t cout, int64_t n_out) {
  if (!wgrad_shape_ok(K, cin, cout, n_out)) return -1;
  const int64_t rows = slab_rows_of(K, cin, cout, n_out);
  const int64_t slabs = (n_out + rows - 1) / rows;
  return slabs <= 1 ? 0 : slabs * K * cin * cout * 4;
}

extern "C" int PG_FN(conv_wgrad)(const float *x, int64_t n_in, int32_t cin, const float *dy, int64_t n_out, int32_t cout,
                                 const int32_t *nbr, int32_t K, float *dw, void *workspace, int64_t workspace_bytes,
                                 void *stream) {
  if (!wgrad_shape_ok(K, cin, cout, n_out) || n_in < 0 || n_in >= (1ll << 31))
    return fail("conv_wgrad: K = %d, cin = %d, cout = %d, n_in = %lld, n_out = %lld outside the served range", K, cin, cout,
                (long long)n_in, (long long)n_out);
  if (dw == nullptr) return fail("conv_wgrad: null dw");
  const int64_t elems = (int64_t)K * cin * cout;
  if (n_out == 0 || n_in == 0) {
    SIDE_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)elems * sizeof(float), st_of(stream)));
    return 0;
  }
  if (x == nullptr || dy == nullptr || nbr == nullptr) return fail("conv_wgrad: null pointer");
  const int64_t rows = slab_rows_of(K, cin, cout, n_out);
  const int64_t slabs = (n_out + rows - 1) / rows;
  const int64_t need = slabs <= 1 ? 0 : slabs * elems * 4;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 3) != 0))
    return fail("conv_wgrad: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)workspace_bytes, (long long)need);
  WgradArgs a;
  a.x = x;
  a.dy = dy;
  a.nbr = nbr;
  a.part = slabs <= 1 ? dw : static_cast<float *>(workspace);
  a.n_in = n_in;
  a.n_out = n_out;
  a.slab_rows = rows;
  a.cin = cin;
  a.cout = cout;
  a.kvol = K;
  a.vec_x = (cin % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
  a.vec_y = (cout % 4 == 0 && ((uintptr_t)dy & 15) == 0) ? 1 : 0;
  const bool wide = cin > 64 && cout > 64;
  const int bc = wide ? 128 : 64;
  a.ci_tiles = (cin + bc - 1) / bc;
  a.co_tiles = (cout + bc - 1) / bc;
  const int64_t grid = slabs * K * a.ci_tiles * a.co_tiles;
  if (grid >= (1ll << 31)) return fail("conv_wgrad: %lld workgroups", (long long)grid);
  if (wide)
    hipLaunchKernelGGL((k_wgrad<2, 2>), dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), a);
  else
    hipLaunchKernelGGL((k_wgrad<1, 1>), dim3((unsigned)grid), dim3(BLOCK), 0, st_of(stream), a);
  SIDE_CHECK_LAUNCH("k_wgrad");
  if (slabs > 1) {
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((elems + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), a.part,
                       elems, slabs, dw);
    SIDE_CHECK_LAUNCH("k_wgrad_reduce");
  }
  return 0;
}

extern "C" int64_t PG_FN(colsum_workspace_bytes)(int64_t n, int32_t c) {
  if (n < 0 || c < 1) return -1;
  const int64_t blocks = (n + PG_COLSUM_ROWS - 1) / PG_COLSUM_ROWS;
  return blocks <= 1 ? 0 : blocks * c * 4;
}

extern "C" int PG_FN(colsum)(const float *dy, int64_t n, int32_t c, float *out, void *workspace, int64_t workspace_bytes,
                             void *stream) {
  if (n < 0 || c < 1 || n >= (1ll << 31)) return fail("colsum: n = %lld, c = %d outside the served range", (long long)n, c);
  if (out == nullptr) return fail("colsum: null out");
  if (n == 0) {
    SIDE_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)c * sizeof(float), st_of(stream)));
    return 0;
  }
  if (dy == nullptr) return fail("colsum: null dy");
  const int64_t blocks = (n + PG_COLSUM_ROWS - 1) / PG_COLSUM_ROWS;
  const int64_t need = blocks <= 1 ? 0 : blocks * c * 4;
  if (need > 0 && (workspace == nullptr || workspace_bytes < need || ((uintptr_t)workspace & 3) != 0))
    return fail("colsum: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)workspace_bytes, (long long)need);
  if (blocks > 65535) return fail("colsum: %lld row blocks", (long long)blocks);
  float *part = blocks <= 1 ? out : static_cast<float *>(workspace);
  hipLaunchKernelGGL(k_colsum_part, dim3((unsigned)((c + 63) / 64), (unsigned)blocks), dim3(BLOCK), 0, st_of(stream), dy, n, c,
                     part);
  SIDE_CHECK_LAUNCH("k_colsum_part");
  if (blocks > 1) {
    hipLaunchKernelGGL(k_colsum_finish, dim3((unsigned)((c + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), part, blocks, c,
                       out);
    SIDE_CHECK_LAUNCH("k_colsum_finish");
  }
  return 0;
}

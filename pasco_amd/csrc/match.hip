// The panoptic matcher and mask losses for gfx950 (include/pasco_match.h): the targets as 128-bit words per voxel, the per-pair
// sums both the matcher's cost and the losses are made of, the gradient of the losses with respect to the logits, and the
// assignment itself on the host (pm_assign.h).
//
// k_pair_part: focal_diff[q][t] = sum_n (fp - fn)[n][q] tgt[n][t] and inter[q][t] = sum_n p[n][q] tgt[n][t] are sums over rows of
// outer products, the shape of k_wgrad (grad.hip): the rows are the K dimension of v_mfma_f32_32x32x2_f32 (exact fp32), one MFMA
// takes two rows, operand A = a left operand's [row h][32 queries], operand B = tgt[row h][32 targets] (lane l holds column l & 31
// of row h = l >> 5 for both).  A workgroup (256 threads = 4 waves) owns one range of consecutive rows and ALL of [Q, T]: wave w
// owns queries 32 w .. 32 w + 31 and every 32-target tile, for both left operands (2 TT accumulator tiles).  It walks the range in
// chunks of 32 rows.  Thread (column c = tid & 127, half = tid >> 7) owns column c of rows half, half + 2, ... of every chunk: it
// forms fp - fn and p of its logits in registers (a row that does not count, or a column >= Q, gives zeros), expands bit c of the
// row's target word to 0.0 / 1.0 (0 for c >= T, so bits beyond T are never looked at) and writes the three ROW-MAJOR LDS tiles
// (128 consecutive dwords per row and half: conflict free); the waves read them back with ds_read_b32, 32 consecutive dwords of
// one row per lane group (MI355X_MICROARCH.md "LDS": conflict free).  The same thread keeps sum fn, sum p (its query column) and
// the target count (its target column) in registers: a fixed column per thread, so they never pass through the MFMA.  The next
// chunk's logits, words and flags are loaded into registers while the current one is multiplied.  LDS: 2 x 16 KB + 4 TT KB.
//
// k_pair_final adds the ranges' partials in ascending range order and finalises focal_sum, dice, stats and count.
// Determinism: a workgroup adds its rows in ascending order; the range length is a function of (n, q, t) alone; no atomics on
// floats (the only atomic is the integer count of out-of-grid rows in k_target_pack).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_match.h"
#include "side_common.h"
#include "pm_assign.h"

#pragma clang fp contract(off)

SIDE_EXPORTS(PM_FN, PM_ABI_VERSION)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BLOCK = 256;
constexpr int CHUNK = 32;            // rows per LDS stage
constexpr int COLS = 128;            // columns of a left-operand LDS tile (PM_MAX_Q)
constexpr int PER = CHUNK / 2;       // rows per thread and chunk
constexpr int MIN_RANGE = 128;       // rows of a range at least
constexpr int MAX_RANGES = 256;      // ranges at most (one per CU)

hipStream_t st_of(void *s) { return reinterpret_cast<hipStream_t>(s); }

int64_t range_rows_of(int64_t n) {
  int64_t r = (n + MAX_RANGES - 1) / MAX_RANGES;
  r = (r + CHUNK - 1) / CHUNK * CHUNK;
  return r < MIN_RANGE ? MIN_RANGE : r;
}

bool served(int64_t n, int32_t q, int32_t t) { return n >= 0 && n <= INT32_MAX && q >= 1 && q <= PM_MAX_Q && t >= 1 && t <= PM_MAX_T; }

int pad32(int v) { return (v + 31) / 32 * 32; }

// floats of one range's partials: focal_diff [QP, TP], inter [QP, TP], fn sum [QP], p sum [QP], target count [TP] (int bits),
// rows counted (int bits) padded to 4
int64_t part_floats(int32_t q, int32_t t) {
  const int64_t qp = pad32(q), tp = pad32(t);
  return 2 * qp * tp + 2 * qp + tp + 4;
}

// p = sigmoid(x), omp = 1 - p without cancellation, sp = softplus(x), sn = softplus(-x); no overflow for any finite x
struct Terms {
  float p, omp, sp, sn;
};

__device__ __forceinline__ Terms terms_of(float x) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float big = inv, small = e * inv;
  const float l = log1pf(e);
  Terms r;
  r.p = x >= 0.f ? big : small;
  r.omp = x >= 0.f ? small : big;
  r.sp = fmaxf(x, 0.f) + l;
  r.sn = fmaxf(-x, 0.f) + l;
  return r;
}

__global__ void k_target_pack(const uint8_t *__restrict__ masks, const uint8_t *__restrict__ unknown,
                              const int32_t *__restrict__ coords, int64_t n, int t, int dx, int dy, int dz, int ox, int oy, int oz,
                              uint32_t *__restrict__ tbits, uint8_t *__restrict__ flags, int32_t *__restrict__ oob) {
  const int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  const int64_t x = (int64_t)coords[row * 4 + 1] - ox, y = (int64_t)coords[row * 4 + 2] - oy, z = (int64_t)coords[row * 4 + 3] - oz;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  uint8_t f = 0;
  if (x < 0 || x >= dx || y < 0 || y >= dy || z < 0 || z >= dz) {
    atomicAdd(oob, 1);
  } else {
    const int64_t vol = (int64_t)dx * dy * dz;
    const int64_t idx = (x * dy + y) * dz + z;
    for (int k = 0; k < t; ++k)
      if (masks[k * vol + idx] != 0) w[k >> 5] |= 1u << (k & 31);
    const bool known = unknown == nullptr || unknown[idx] == 0;
    if (known) f = (uint8_t)(PM_FLAG_KNOWN | ((w[0] | w[1] | w[2] | w[3]) != 0u ? PM_FLAG_MATCHABLE : 0));
  }
  *reinterpret_cast<uint4 *>(tbits + row * 4) = make_uint4(w[0], w[1], w[2], w[3]);
  flags[row] = f;
}

struct PairArgs {
  const float *logits;
  const uint32_t *tbits;
  const uint8_t *flags;
  float *part;
  int64_t n, range_rows, pfloats;
  int q, t, qp, tp, fmask;
};

template <int TT>
__global__ void __launch_bounds__(BLOCK) k_pair_part(PairArgs a) {
  constexpr int TCOLS = TT * 32;
  __shared__ float As[CHUNK * COLS];      // fp - fn
  __shared__ float Ps[CHUNK * COLS];      // p
  __shared__ float Ts[CHUNK * TCOLS];     // the targets as 0.0 / 1.0
  __shared__ int redi[2 * BLOCK];

  const int64_t r_begin = (int64_t)blockIdx.x * a.range_rows;
  const int64_t r_end = (r_begin + a.range_rows < a.n) ? r_begin + a.range_rows : a.n;
  const int nchunks = (int)((r_end - r_begin + CHUNK - 1) / CHUNK);

  const int tid = threadIdx.x;
  const int col = tid & (COLS - 1), half = tid >> 7;
  const int lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int q = a.q, t = a.t;
  const bool qcol = col < q, tcol = col < t;

  f32x16 acc[2][TT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float rx[PER];          // the logits of the chunk being loaded
  uint32_t rb[PER];       // bit `col` of the row's word, 0 for a row that does not count or col >= T
  int ron[PER];           // the row counts
  float fn_acc = 0.f, p_acc = 0.f;
  int t_acc = 0, n_acc = 0;

  auto load = [&](int chunk) {
    const int64_t r0 = r_begin + (int64_t)chunk * CHUNK;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t row = r0 + half + 2 * i;
      rx[i] = 0.f;
      rb[i] = 0u;
      ron[i] = 0;
      if (row < r_end) {
        ron[i] = (a.flags[row] & a.fmask) != 0;
        if (ron[i] && qcol) rx[i] = a.logits[row * q + col];
        if (ron[i] && tcol) rb[i] = (a.tbits[row * 4 + (col >> 5)] >> (col & 31)) & 1u;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int lr = half + 2 * i;
      float d = 0.f, p = 0.f;
      if (ron[i] && qcol) {
        const Terms m = terms_of(rx[i]);
        const float fp = 0.25f * (m.omp * m.omp) * m.sn;
        const float fn = 0.75f * (m.p * m.p) * m.sp;
        d = fp - fn;
        p = m.p;
        fn_acc += fn;
        p_acc += p;
      }
      As[lr * COLS + col] = d;
      Ps[lr * COLS + col] = p;
      if (col < TCOLS) Ts[lr * TCOLS + col] = rb[i] ? 1.f : 0.f;
      t_acc += (int)rb[i];
      n_acc += ron[i];
    }
  };
  // a wave whose 32 queries lie beyond Q has only zeros to add
  const bool live = wave * 32 < q;
  auto compute = [&]() {
    if (!live) return;
#pragma unroll 4
    for (int r2 = 0; r2 < CHUNK / 2; ++r2) {
      const int row = 2 * r2 + h;
      const float a0 = As[row * COLS + wave * 32 + l31];
      const float a1 = Ps[row * COLS + wave * 32 + l31];
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        const float b = Ts[row * TCOLS + j * 32 + l31];
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][j], 0, 0, 0);
      }
    }
  };

  if (nchunks > 0) load(0);
  for (int c = 0; c < nchunks; ++c) {
    stage();
    __syncthreads();
    if (c + 1 < nchunks) load(c + 1);
    compute();
    __syncthreads();
  }

  // C/D layout of the 32 x 32 MFMA: column = lane & 31 (target), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (query).  The
  // partial tiles are padded to [QP, TP], so a live wave's rows and every column are inside.
  float *dst = a.part + (int64_t)blockIdx.x * a.pfloats;
  const int64_t tile = (int64_t)a.qp * a.tp;
  if (live) {
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const int tc = j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[(int64_t)qr * a.tp + tc] = acc[0][j][r];
        dst[tile + (int64_t)qr * a.tp + tc] = acc[1][j][r];
      }
    }
  }
  // the per-column sums of the two halves, half 0 first
  As[tid] = fn_acc;
  Ps[tid] = p_acc;
  redi[tid] = t_acc;
  redi[BLOCK + tid] = n_acc;
  __syncthreads();
  if (tid < COLS) {
    float *tail = dst + 2 * tile;
    if (tid < a.qp) {
      tail[tid] = As[tid] + As[tid + COLS];
      tail[a.qp + tid] = Ps[tid] + Ps[tid + COLS];
    }
    if (tid < a.tp) tail[2 * a.qp + tid] = __int_as_float(redi[tid] + redi[tid + COLS]);
    if (tid == 0) tail[2 * a.qp + a.tp] = __int_as_float(redi[BLOCK] + redi[BLOCK + COLS]);
  }
}

// One block per query, one thread per target: the ranges in ascending order.
__global__ void __launch_bounds__(128) k_pair_final(const float *__restrict__ part, int64_t ranges, int64_t pfloats, int q, int t,
                                                    int qp, int tp, float *__restrict__ focal_sum, float *__restrict__ dice,
                                                    float *__restrict__ stats, int32_t *__restrict__ count) {
  const int qi = blockIdx.x, ti = threadIdx.x;
  const int64_t tile = (int64_t)qp * tp;
  if (qi == 0 && ti == 0) {
    int c = 0;
    for (int64_t r = 0; r < ranges; ++r) c += __float_as_int(part[r * pfloats + 2 * tile + 2 * qp + tp]);
    *count = c;
  }
  if (ti >= t) return;
  float fd = 0.f, in = 0.f, fn = 0.f, ps = 0.f;
  int ts = 0;
  for (int64_t r = 0; r < ranges; ++r) {
    const float *p = part + r * pfloats;
    fd += p[(int64_t)qi * tp + ti];
    in += p[tile + (int64_t)qi * tp + ti];
    fn += p[2 * tile + qi];
    ps += p[2 * tile + qp + qi];
    ts += __float_as_int(p[2 * tile + 2 * qp + ti]);
  }
  const float tsf = (float)ts;
  const int64_t o = (int64_t)qi * t + ti;
  focal_sum[o] = fd + fn;
  dice[o] = 1.f - (2.f * in + 1.f) / (ps + tsf + 1.f);
  stats[o * 3 + 0] = in;
  stats[o * 3 + 1] = ps;
  stats[o * 3 + 2] = tsf;
}

__global__ void __launch_bounds__(BLOCK) k_mask_loss_bwd(const float *__restrict__ logits, const uint32_t *__restrict__ tbits,
                                                         const uint8_t *__restrict__ flags, const int32_t *__restrict__ tgt_of_query,
                                                         const float *__restrict__ coef, int64_t total, int q, int t,
                                                         float *__restrict__ dlogits) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / q;
  const int c = (int)(i - row * q);
  const int k = tgt_of_query[c];
  float g = 0.f;
  if (k >= 0 && k < t && (flags[row] & PM_FLAG_KNOWN) != 0) {
    const bool y = ((tbits[row * 4 + (k >> 5)] >> (k & 31)) & 1u) != 0u;
    const Terms m = terms_of(logits[i]);
    // d fp/dx = -0.25 (1-p)^2 (2 p softplus(-x) + (1-p));  d fn/dx = 0.75 p^2 (2 (1-p) softplus(x) + p)
    const float dfp = -0.25f * (m.omp * m.omp) * (2.f * m.p * m.sn + m.omp);
    const float dfn = 0.75f * (m.p * m.p) * (2.f * m.omp * m.sp + m.p);
    const float cc = coef[c * 3 + 0], ca = coef[c * 3 + 1], cb = coef[c * 3 + 2];
    g = cc * (y ? dfp : dfn) + (m.p * m.omp) * (y ? ca + cb : cb);
  }
  dlogits[i] = g;
}

}  // namespace

extern "C" int PM_FN(target_pack)(const uint8_t *masks, const uint8_t *unknown, const int32_t *coords, int64_t n, int32_t t,
                                  int32_t dx, int32_t dy, int32_t dz, int32_t ox, int32_t oy, int32_t oz, uint32_t *tbits,
                                  uint8_t *flags, int32_t *oob, void *stream) {
  if (n < 0 || n > INT32_MAX) return fail("pm_target_pack: n = %lld rows not served", (long long)n);
  if (t < 1 || t > PM_MAX_T) return fail("pm_target_pack: %d targets not served (1..%d)", t, PM_MAX_T);
  if (dx < 1 || dy < 1 || dz < 1) return fail("pm_target_pack: grid %d x %d x %d", dx, dy, dz);
  if (masks == nullptr || oob == nullptr || (n > 0 && (coords == nullptr || tbits == nullptr || flags == nullptr)))
    return fail("pm_target_pack: null pointer (masks %p coords %p tbits %p flags %p oob %p)", (const void *)masks,
                (const void *)coords, (void *)tbits, (void *)flags, (void *)oob);
  if (((uintptr_t)tbits & 15) != 0) return fail("pm_target_pack: tbits not 16-byte aligned");
  SIDE_CHECK_HIP(hipMemsetAsync(oob, 0, sizeof(int32_t), st_of(stream)));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_target_pack, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), masks, unknown,
                     coords, n, t, dx, dy, dz, ox, oy, oz, tbits, flags, oob);
  SIDE_CHECK_LAUNCH("k_target_pack");
  return 0;
}

extern "C" int64_t PM_FN(pair_sums_ranges)(int64_t n, int32_t q, int32_t t) {
  if (!served(n, q, t) || n == 0) return 0;
  const int64_t rr = range_rows_of(n);
  return (n + rr - 1) / rr;
}

extern "C" int64_t PM_FN(pair_sums_workspace_bytes)(int64_t n, int32_t q, int32_t t) {
  return PM_FN(pair_sums_ranges)(n, q, t) * part_floats(q, t) * (int64_t)sizeof(float);
}

extern "C" int PM_FN(pair_sums)(const float *logits, const uint32_t *tbits, const uint8_t *flags, int32_t flag_bit, int64_t n,
                                int32_t q, int32_t t, float *focal_sum, float *dice, float *stats, int32_t *count, void *ws,
                                int64_t ws_bytes, void *stream) {
  if (q < 1 || q > PM_MAX_Q) return fail("pm_pair_sums: %d queries not served (1..%d)", q, PM_MAX_Q);
  if (t < 1 || t > PM_MAX_T) return fail("pm_pair_sums: %d targets not served (1..%d)", t, PM_MAX_T);
  if (n < 0 || n > INT32_MAX) return fail("pm_pair_sums: n = %lld rows not served", (long long)n);
  if (flag_bit != 0 && flag_bit != 1) return fail("pm_pair_sums: flag_bit %d (0 = known, 1 = matchable)", flag_bit);
  if (focal_sum == nullptr || dice == nullptr || stats == nullptr || count == nullptr ||
      (n > 0 && (logits == nullptr || tbits == nullptr || flags == nullptr)))
    return fail("pm_pair_sums: null pointer (logits %p tbits %p flags %p focal_sum %p dice %p stats %p count %p)",
                (const void *)logits, (const void *)tbits, (const void *)flags, (void *)focal_sum, (void *)dice, (void *)stats,
                (void *)count);
  const int64_t need = PM_FN(pair_sums_workspace_bytes)(n, q, t);
  if (need > 0 && (ws == nullptr || ws_bytes < need || ((uintptr_t)ws & 3) != 0))
    return fail("pm_pair_sums: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)ws_bytes, (long long)need);
  PairArgs a;
  a.logits = logits;
  a.tbits = tbits;
  a.flags = flags;
  a.part = static_cast<float *>(ws);
  a.n = n;
  a.range_rows = range_rows_of(n);
  a.pfloats = part_floats(q, t);
  a.q = q;
  a.t = t;
  a.qp = pad32(q);
  a.tp = pad32(t);
  a.fmask = 1 << flag_bit;
  const int64_t ranges = PM_FN(pair_sums_ranges)(n, q, t);
  if (ranges > 0) {
    const dim3 grid((unsigned)ranges), block(BLOCK);
    switch (a.tp / 32) {
      case 1: hipLaunchKernelGGL(k_pair_part<1>, grid, block, 0, st_of(stream), a); break;
      case 2: hipLaunchKernelGGL(k_pair_part<2>, grid, block, 0, st_of(stream), a); break;
      case 3: hipLaunchKernelGGL(k_pair_part<3>, grid, block, 0, st_of(stream), a); break;
      default: hipLaunchKernelGGL(k_pair_part<4>, grid, block, 0, st_of(stream), a); break;
    }
    SIDE_CHECK_LAUNCH("k_pair_part");
  }
  hipLaunchKernelGGL(k_pair_final, dim3((unsigned)q), dim3(128), 0, st_of(stream), a.part, ranges, a.pfloats, q, t, a.qp, a.tp,
                     focal_sum, dice, stats, count);
  SIDE_CHECK_LAUNCH("k_pair_final");
  return 0;
}

extern "C" int PM_FN(mask_loss_bwd)(const float *logits, const uint32_t *tbits, const uint8_t *flags, const int32_t *tgt_of_query,
                                    const float *coef, int64_t n, int32_t q, int32_t t, float *dlogits, void *stream) {
  if (q < 1 || q > PM_MAX_Q) return fail("pm_mask_loss_bwd: %d queries not served (1..%d)", q, PM_MAX_Q);
  if (t < 1 || t > PM_MAX_T) return fail("pm_mask_loss_bwd: %d targets not served (1..%d)", t, PM_MAX_T);
  if (n < 0 || n > INT32_MAX) return fail("pm_mask_loss_bwd: n = %lld rows not served", (long long)n);
  if (n == 0) return 0;
  if (logits == nullptr || tbits == nullptr || flags == nullptr || tgt_of_query == nullptr || coef == nullptr || dlogits == nullptr)
    return fail("pm_mask_loss_bwd: null pointer (logits %p tbits %p flags %p tgt_of_query %p coef %p dlogits %p)",
                (const void *)logits, (const void *)tbits, (const void *)flags, (const void *)tgt_of_query, (const void *)coef,
                (void *)dlogits);
  const int64_t total = n * q;
  hipLaunchKernelGGL(k_mask_loss_bwd, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), logits, tbits,
                     flags, tgt_of_query, coef, total, q, t, dlogits);
  SIDE_CHECK_LAUNCH("k_mask_loss_bwd");
  return 0;
}

extern "C" int PM_FN(assign)(const double *cost, int32_t q, int32_t t, int32_t *row, int32_t *col) {
  if (q < 0 || t < 0) return fail("pm_assign: a %d x %d cost matrix", q, t);
  if (q == 0 || t == 0) return 0;
  if (cost == nullptr || row == nullptr || col == nullptr)
    return fail("pm_assign: null pointer (cost %p row %p col %p)", (const void *)cost, (void *)row, (void *)col);
  if (pm_lsa::solve(cost, q, t, row, col) != 0) return fail("pm_assign: the %d x %d cost matrix has a non-finite entry", q, t);
  return 0;
}

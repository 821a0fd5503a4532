// Backward of the masked cross-attention (include/pasco_attngrad.h) for gfx950: fp32, no score tensor, no float atomics.
//
// The forward (csrc/attn.hip k_attn_cross) streams 16-key tiles per wave with an online softmax.  The backward keeps its split
// of the keys into contiguous ranges of 16-key tiles, one wave64 per range, and runs in three steps:
//
//   k_pa_stats + k_pa_stats_merge   the row statistics are recomputed, not saved: per range the partial (m, l) of every query,
//                                   merged in ascending range order into lse[q] = m + log l (+inf: nothing allowed, every P of
//                                   the row is 0) and delta[q] = sum_d dout[q][d] out[q][d]
//   k_pa_main                       keys stationary: a wave visits, for each of its key tiles, all query tiles; dK and dV of the
//                                   16 keys accumulate in registers over the query tiles and are written once with plain
//                                   stores (a key has one owner); the wave's partial dQ^T accumulates over its tiles
//   k_pa_dq_reduce                  dQ = the partials added in ascending range order
//
// Every product is v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate).  Per (key tile, query tile) pair, with the
// fragments kf / vr (lane = key, 4 dims per step) and qf / dof (lane = query, 4 dims per step) - the forward's operand layout:
//
//   S^T [key][q] = mfma(kf, qf)     C/D layout: lane = query, registers = keys 4g + r   (g = lane >> 4)
//   dP^T[key][q] = mfma(vr, dof)    same layout; P^T = exp(S^T - lse[q]), dS^T = P^T (dP^T - delta[q]) per lane
//   dQ^T[d][q]  += mfma(K^T, dS^T)  dS^T registers are the B operand as they are (as P is in the forward)
//   S   [q][key] = mfma(qf, kf)     THE SAME FRAGMENTS WITH A AND B SWAPPED: lane = key, registers = queries 4g + r
//   dP  [q][key] = mfma(dof, vr)
//   dV^T[d][key] += mfma(dout^T, P)   dK^T[d][key] += mfma(Q^T, dS)
//
// 7 x 12 = 84 MFMAs per pair; no transpose, no barrier in the loop, no cross-lane traffic (LDS only holds the query side, staged
// once per workgroup).  (The alternative - transposing P and dS through LDS, 60 MFMAs - is discussed in DESIGN.md 4m.)  The D layout of dK^T / dV^T has lane = key and 4 consecutive dims per lane: one
// 16-byte store per lane and 16-dim block.  Keys >= n have zero fragments, P = 0, and no store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_attngrad.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DH = PA_DH;
constexpr int DT = DH / 16;
constexpr int PA_WAVE_TARGET = 2048;      // key ranges aimed at over all (b, h): 256 CUs x 4 SIMDs x 2 waves

struct PaArgs {
  const float *q, *k, *v, *out, *dout;
  const uint32_t *bits, *any;
  float *dq, *dk, *dv;
  float *lse, *delta;      // [B*H][qrows]
  float *ml;               // [B*H*splits][qrows][2]   partial (m, l) of the statistics pass
  float *dqp;              // [B*H*splits][qrows][DH]  partial dQ
  int64_t n;
  int B, H, Qn;
  int qrows;               // Qn rounded up to whole 16-query tiles
  int splits, tpw;         // key ranges per (b, h), 16-key tiles per range
};

// The key ranges of a shape: a function of (n, b * h) alone (never of the device).  The forward's arithmetic with one
// difference: 2048 / (b h) is rounded DOWN to whole workgroups of 4 ranges, so that the grid never exceeds 512 workgroups.  At
// two workgroups per CU (the 8-tile instantiation) that is one round: with the forward's rounding up the decoder's shape
// (b h = 24) has 528 workgroups, and the 16 left over run alone after the others (measured at N = 210 542: 6.5 ms against 4.2 ms).
void pa_ranges(int64_t n, int64_t bh, int64_t *splits_out, int64_t *tpw_out) {
  const int64_t ntile = (n + 15) / 16;
  int64_t splits = PA_WAVE_TARGET / bh;
  if (splits >= 4) splits -= splits % 4;
  if (splits < 1) splits = 1;
  if (splits > ntile) splits = ntile;
  int64_t tpw = (ntile + splits - 1) / splits;
  if (tpw < 1) tpw = 1;
  *splits_out = (ntile + tpw - 1) / tpw;
  *tpw_out = tpw;
}

struct PaLayout {
  int64_t qrows, splits, tpw, off_lse, off_delta, off_ml, off_dqp, bytes;
};

int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

PaLayout pa_layout(int64_t n, int64_t b, int64_t h, int64_t qn) {
  PaLayout L;
  L.qrows = (qn + 15) / 16 * 16;
  pa_ranges(n, b * h, &L.splits, &L.tpw);
  const int64_t bh = b * h;
  L.off_lse = 0;
  L.off_delta = align256(L.off_lse + bh * L.qrows * 4);
  L.off_ml = align256(L.off_delta + bh * L.qrows * 4);
  L.off_dqp = align256(L.off_ml + bh * L.splits * L.qrows * 2 * 4);
  L.bytes = align256(L.off_dqp + bh * L.splits * L.qrows * DH * 4);
  return L;
}

// Which (b, h, key range) a wave owns.
struct Owner {
  int64_t w, t0, t1;
  int bh, b, h;
};

__device__ __forceinline__ bool pa_owner(const PaArgs &a, Owner &o) {
  // grid = (ranges / 4 rounded up, B * H): the four waves of a workgroup own consecutive ranges of ONE (b, h)
  const int split = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  o.bh = (int)blockIdx.y;
  o.w = (int64_t)o.bh * a.splits + split;
  o.b = o.bh / a.H;
  o.h = o.bh - o.b * a.H;
  const int64_t ntile = (a.n + 15) / 16;
  o.t0 = (int64_t)split * a.tpw;
  o.t1 = o.t0 + a.tpw;
  if (o.t1 > ntile) o.t1 = ntile;
  return split < a.splits;      // false: a wave of the last workgroup beyond the last range
}

// The forward's two mask rules as one word: a query attends to a key when its bit is set in (key's word | force word).
// No mask: all ones.  Mask without `any`: zero.  Mask with `any`: the queries allowed nowhere.
__device__ __forceinline__ uint4 pa_force_words(const PaArgs &a, int b) {
  if (a.bits == nullptr) return make_uint4(~0u, ~0u, ~0u, ~0u);
  if (a.any == nullptr) return make_uint4(0u, 0u, 0u, 0u);
  const uint4 y = *reinterpret_cast<const uint4 *>(a.any + b * 4);
  return make_uint4(~y.x, ~y.y, ~y.z, ~y.w);
}

__device__ __forceinline__ unsigned pa_word(const uint4 &m, int sel) {      // sel is a compile-time constant where it is used
  return sel == 0 ? m.x : (sel == 1 ? m.y : (sel == 2 ? m.z : m.w));
}

__device__ __forceinline__ f32x4 pa_ld4(const float *p, bool ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (ok) v = *reinterpret_cast<const f32x4 *>(p);
  return v;
}

// S^T tile [16 keys x 16 queries] (or S with the operands swapped): 12 MFMAs over the 48 dims.
__device__ __forceinline__ f32x4 pa_dot48(const f32x4 (&x)[DT], const f32x4 (&y)[DT]) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < DT; ++j) {
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][0], y[j][0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][1], y[j][1], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][2], y[j][2], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j][3], y[j][3], s, 0, 0, 0);
  }
  return s;
}

// ---- statistics pass --------------------------------------------------------------------------------------------------------
// One wave = one key range x all QT query tiles: the forward's loop without the V product.
template <int QT>
__global__ void __launch_bounds__(256) k_pa_stats(PaArgs a) {
  Owner o;
  if (!pa_owner(a, o)) return;
  const int lane = threadIdx.x & 63;
  const int qi = lane & 15, g = lane >> 4;
  const int D = a.H * DH;
  const uint4 fw = pa_force_words(a, o.b);

  f32x4 qf[QT][DT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int qq = qt * 16 + qi;
#pragma unroll
    for (int j = 0; j < DT; ++j) qf[qt][j] = pa_ld4(a.q + ((int64_t)o.bh * a.Qn + qq) * DH + 16 * j + 4 * g, qq < a.Qn);
  }
  float m[QT], l[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m[qt] = -INFINITY;
    l[qt] = 0.f;
  }
  const float *kb = a.k + (int64_t)o.b * a.n * D + o.h * DH;
  for (int64_t t = o.t0; t < o.t1; ++t) {
    const int64_t nb = t * 16;
    f32x4 kf[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) kf[j] = pa_ld4(kb + (nb + qi) * D + 16 * j + 4 * g, nb + qi < a.n);
    uint4 mb[4];
    bool kin[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t key = nb + 4 * g + r;
      kin[r] = key < a.n;
      mb[r] = fw;
      if (a.bits != nullptr && kin[r]) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a.bits + ((int64_t)o.b * a.n + key) * 4);
        mb[r] = make_uint4(x.x | fw.x, x.y | fw.y, x.z | fw.z, x.w | fw.w);
      }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt * 16 >= a.Qn) continue;      // uniform
      const f32x4 s = pa_dot48(kf, qf[qt]);
      const int bsel = (qt & 1) * 16 + qi;
      float sv[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = kin[r] && ((pa_word(mb[r], qt >> 1) >> bsel) & 1u);
        sv[r] = ok ? s[r] : -INFINITY;
        tmax = fmaxf(tmax, sv[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m[qt], tmax);
      const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = __expf(m[qt] - m_safe);      // m = -inf -> 0 (nothing accumulated yet)
      m[qt] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) psum += __expf(sv[r] - m_safe);
      l[qt] = l[qt] * alpha + psum;
    }
  }
  float *pw = a.ml + o.w * (int64_t)a.qrows * 2;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    if (qt * 16 >= a.Qn) continue;
    float lt = l[qt];
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    if (g == 0) {
      pw[(qt * 16 + qi) * 2] = m[qt];
      pw[(qt * 16 + qi) * 2 + 1] = lt;
    }
  }
}

// One thread per (b, h, row of the padded query tiles): the ranges in ascending order.  Rows >= Qn get lse = +inf, delta = 0,
// so that the main pass needs no test for them.
__global__ void __launch_bounds__(256) k_pa_stats_merge(PaArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.B * a.H * a.qrows) return;
  const int bh = (int)(idx / a.qrows), qq = (int)(idx - (int64_t)bh * a.qrows);
  if (qq >= a.Qn) {
    a.lse[idx] = INFINITY;
    a.delta[idx] = 0.f;
    return;
  }
  const float *base = a.ml + ((int64_t)bh * a.splits * a.qrows + qq) * 2;
  const int64_t step = (int64_t)a.qrows * 2;
  float M = -INFINITY;
  for (int s = 0; s < a.splits; ++s) M = fmaxf(M, base[s * step]);
  const float Msafe = (M == -INFINITY) ? 0.f : M;
  float L = 0.f;
  for (int s = 0; s < a.splits; ++s) L += base[s * step + 1] * expf(base[s * step] - Msafe);
  a.lse[idx] = L > 0.f ? Msafe + logf(L) : INFINITY;
  const int b = bh / a.H, h = bh - b * a.H;
  const int64_t row = ((int64_t)b * a.Qn + qq) * (a.H * DH) + h * DH;
  // delta in the order the MFMAs of the main pass form dP = dout . v (per 16-dim block j and step c, the four dims
  // 16j + 4k + c in ascending k, one fused multiply-add each): where out == v bit for bit (a query with one allowed key),
  // dP - delta is then an exact zero, as it is in exact arithmetic
  float d = 0.f;
  for (int j = 0; j < DT; ++j)
    for (int c = 0; c < 4; ++c)
      for (int kk = 0; kk < 4; ++kk) {
        const int e = 16 * j + 4 * kk + c;
        d = fmaf(a.dout[row + e], a.out[row + e], d);
      }
  a.delta[idx] = d;
}

// lse / delta [B*H][qrows] -> [B*H][Qn] (pa_attn_bwd_stats)
__global__ void __launch_bounds__(256) k_pa_stats_copy(PaArgs a, float *lse, float *delta) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)a.B * a.H * a.Qn) return;
  const int64_t bh = idx / a.Qn, qq = idx - bh * a.Qn;
  lse[idx] = a.lse[bh * a.qrows + qq];
  delta[idx] = a.delta[bh * a.qrows + qq];
}

// ---- main pass --------------------------------------------------------------------------------------------------------------
// One wave = one key range; QT = query tiles the instantiation has registers for (tiles at or beyond Qn are skipped).
//
// The query side of a (b, h) - Q, dout, lse, delta: 2 x 19 KB at 100 queries - is staged in LDS once per workgroup and read from
// there for every key tile, in both orientations.  Rows are padded to LDS_ROW = 52 dwords: the row reads (ds_read_b128, lane =
// (row qi, dims 4g ..): 52 qi mod 64 are 16 distinct multiples of 4) and the transposed reads (ds_read_b32, lane = (dim qi, row
// 4g + c): 208 g mod 64 = 16 g) both put the lanes of a group on distinct banks.  Rows >= Qn are zeros with lse = +inf.
constexpr int LDS_ROW = 52;

// Two waves per SIMD (at most 256 registers): the second wave covers the first one's global loads of the next key tile and the
// 40-cycle dependent latency inside the 12-MFMA chains; two workgroups' LDS (2 x 53 KB at QT = 8) fit a CU.
template <int QT>
__global__ void __launch_bounds__(256, 2) k_pa_main(PaArgs a) {
  __shared__ __attribute__((aligned(16))) float Qs[QT * 16 * LDS_ROW];
  __shared__ __attribute__((aligned(16))) float Ds[QT * 16 * LDS_ROW];
  __shared__ __attribute__((aligned(16))) float lse[QT * 16];
  __shared__ __attribute__((aligned(16))) float delta[QT * 16];
  Owner o;
  const bool live = pa_owner(a, o);
  const int D = a.H * DH;
  {
    const float *qb = a.q + (int64_t)o.bh * a.Qn * DH;                         // row stride DH
    const float *dob = a.dout + (int64_t)o.b * a.Qn * D + o.h * DH;            // row stride D
    for (int e = threadIdx.x; e < QT * 16 * (DH / 4); e += 256) {
      const int row = e / (DH / 4), c4 = e - row * (DH / 4);
      *reinterpret_cast<f32x4 *>(Qs + row * LDS_ROW + 4 * c4) = pa_ld4(qb + (int64_t)row * DH + 4 * c4, row < a.Qn);
      *reinterpret_cast<f32x4 *>(Ds + row * LDS_ROW + 4 * c4) = pa_ld4(dob + (int64_t)row * D + 4 * c4, row < a.Qn);
    }
    for (int e = threadIdx.x; e < QT * 16; e += 256) {
      const bool in = e < a.qrows;      // the statistics exist for the rows of the live tiles: +inf / 0 at and beyond Qn
      lse[e] = in ? a.lse[(int64_t)o.bh * a.qrows + e] : INFINITY;
      delta[e] = in ? a.delta[(int64_t)o.bh * a.qrows + e] : 0.f;
    }
  }
  __syncthreads();
  if (!live) return;
  const int lane = threadIdx.x & 63;
  const int qi = lane & 15, g = lane >> 4;
  const bool want_q = a.dq != nullptr, want_k = a.dk != nullptr, want_v = a.dv != nullptr;
  const uint4 fw = pa_force_words(a, o.b);
  const float *kb = a.k + (int64_t)o.b * a.n * D + o.h * DH;
  const float *vb = a.v + (int64_t)o.b * a.n * D + o.h * DH;
  const float *q_row = Qs + qi * LDS_ROW + 4 * g, *d_row = Ds + qi * LDS_ROW + 4 * g;       // + 16 qt rows, + 16 j
  const float *q_tr = Qs + 4 * g * LDS_ROW + qi, *d_tr = Ds + 4 * g * LDS_ROW + qi;         // + (16 qt + c) rows, + 16 dt

  f32x4 dqa[QT][DT];      // dQ^T[d = 16 dt + 4g + r][q = 16 qt + qi] of this range
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dqa[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = (int)o.t0; t < (int)o.t1; ++t) {      // 32-bit counter (n < 2^34): the 8-tile instantiation fits 256 registers with it
    const int64_t nb = (int64_t)t * 16;
    // ---- key side: row fragments (lane = key qi, dims 16j + 4g ..), the mask word of the lane's key --------------------------
    const int64_t key_l = nb + qi;
    const bool kvl = key_l < a.n;
    f32x4 kf[DT], vr[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
      kf[j] = pa_ld4(kb + key_l * D + 16 * j + 4 * g, kvl);
      vr[j] = pa_ld4(vb + key_l * D + 16 * j + 4 * g, kvl);
    }
    uint4 mk = fw;          // lane = key orientation
    if (a.bits != nullptr && kvl) {
      const uint4 x = *reinterpret_cast<const uint4 *>(a.bits + ((int64_t)o.b * a.n + key_l) * 4);
      mk = make_uint4(x.x | fw.x, x.y | fw.y, x.z | fw.z, x.w | fw.w);
    }
    // lane = query orientation: the 4 keys 4g + r of the lane's S^T registers, and K^T[d = 16 dt + qi][key = 4g + r]
    uint4 mb[4];
    bool kin[4];
    float kT[DT][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t key = nb + 4 * g + r;
      kin[r] = key < a.n;
      mb[r] = fw;
      if (want_q) {
        if (a.bits != nullptr && kin[r]) {
          const uint4 x = *reinterpret_cast<const uint4 *>(a.bits + ((int64_t)o.b * a.n + key) * 4);
          mb[r] = make_uint4(x.x | fw.x, x.y | fw.y, x.z | fw.z, x.w | fw.w);
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) kT[dt][r] = kin[r] ? kb[key * D + 16 * dt + qi] : 0.f;
      } else {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) kT[dt][r] = 0.f;
      }
    }
    f32x4 dka[DT], dva[DT];      // dK^T / dV^T[d = 16 dt + 4g + r][key = qi]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dka[dt] = dva[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt * 16 >= a.Qn) continue;      // uniform
      const int qq = qt * 16 + qi;
      f32x4 qf[DT], dof[DT];
#pragma unroll
      for (int j = 0; j < DT; ++j) {
        qf[j] = *reinterpret_cast<const f32x4 *>(q_row + qt * 16 * LDS_ROW + 16 * j);
        dof[j] = *reinterpret_cast<const f32x4 *>(d_row + qt * 16 * LDS_ROW + 16 * j);
      }
      if (want_q) {
        // lane = query qq, register r = key 4g + r
        const f32x4 s = pa_dot48(kf, qf);
        const f32x4 dp = pa_dot48(vr, dof);
        const float lq = lse[qq], dq_ = delta[qq];      // +inf / 0 at and beyond Qn
        const int bsel = (qt & 1) * 16 + qi;
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = kin[r] && ((pa_word(mb[r], qt >> 1) >> bsel) & 1u);
          const float p = ok ? __expf(s[r] - lq) : 0.f;
          ds[r] = p * (dp[r] - dq_);
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) dqa[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kT[dt][r], ds[r], dqa[qt][dt], 0, 0, 0);
      }
      if (want_k || want_v) {
        // lane = key qi, register r = query 16 qt + 4g + r
        const f32x4 s = pa_dot48(qf, kf);
        const f32x4 l4 = *reinterpret_cast<const f32x4 *>(lse + qt * 16 + 4 * g);
        const unsigned word = pa_word(mk, qt >> 1) >> ((qt & 1) * 16 + 4 * g);
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = kvl && ((word >> r) & 1u);
          p[r] = ok ? __expf(s[r] - l4[r]) : 0.f;
        }
        if (want_v) {
          // A = dout^T: lane (d = qi, g), step c -> dout[q = 16 qt + 4g + c][16 dt + qi]
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float x = d_tr[(qt * 16 + c) * LDS_ROW + 16 * dt];
              dva[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, p[c], dva[dt], 0, 0, 0);
            }
        }
        if (want_k) {
          const f32x4 dp = pa_dot48(dof, vr);
          const f32x4 d4 = *reinterpret_cast<const f32x4 *>(delta + qt * 16 + 4 * g);
          float ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[r] = p[r] * (dp[r] - d4[r]);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float x = q_tr[(qt * 16 + c) * LDS_ROW + 16 * dt];
              dka[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, ds[c], dka[dt], 0, 0, 0);
            }
        }
      }
    }
    // ---- this tile's keys: written once, by their one owner ------------------------------------------------------------------
    if (kvl) {
      const int64_t row = ((int64_t)o.b * a.n + key_l) * D + o.h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        if (want_k) *reinterpret_cast<f32x4 *>(a.dk + row + 16 * dt) = dka[dt];
        if (want_v) *reinterpret_cast<f32x4 *>(a.dv + row + 16 * dt) = dva[dt];
      }
    }
  }

  if (want_q) {
    float *pw = a.dqp + o.w * (int64_t)a.qrows * DH;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      if (qt * 16 >= a.Qn) continue;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        *reinterpret_cast<f32x4 *>(pw + (qt * 16 + qi) * DH + 16 * dt + 4 * g) = dqa[qt][dt];
    }
  }
}

// One thread per element of dq: the ranges in ascending order.
__global__ void __launch_bounds__(256) k_pa_dq_reduce(PaArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_bh = (int64_t)a.Qn * DH;
  if (idx >= (int64_t)a.B * a.H * per_bh) return;
  const int64_t bh = idx / per_bh, e = idx - bh * per_bh;      // e = q * DH + d
  const float *base = a.dqp + bh * a.splits * a.qrows * DH + e;
  const int64_t step = (int64_t)a.qrows * DH;
  float x = 0.f;
  for (int s = 0; s < a.splits; ++s) x += base[s * step];
  a.dq[idx] = x;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool pa_served(int64_t n, int32_t b, int32_t h, int32_t qn, int32_t dh) {
  return dh == DH && qn >= 1 && qn <= PA_MAX_Q && b >= 1 && h >= 1 && n >= 1 && (int64_t)b * h <= 65535 && n < (1ll << 34);
}

int pa_check(const char *what, int64_t n, int32_t b, int32_t h, int32_t qn, int32_t dh, const void *ws, int64_t ws_bytes) {
  if (dh != DH) return fail("%s: head dim %d not served (%d)", what, dh, DH);
  if (qn < 1 || qn > PA_MAX_Q) return fail("%s: %d queries not served (1..%d)", what, qn, PA_MAX_Q);
  if (!pa_served(n, b, h, qn, dh)) return fail("%s: shape n = %lld, b = %d, h = %d outside the served range", what, (long long)n, b, h);
  const int64_t need = pa_layout(n, b, h, qn).bytes;
  if (ws == nullptr || ws_bytes < need)
    return fail("%s: workspace of %lld bytes, %lld needed", what, (long long)(ws == nullptr ? 0 : ws_bytes), (long long)need);
  return 0;
}

void pa_fill(PaArgs &a, const PaLayout &L, void *ws, int64_t n, int32_t b, int32_t h, int32_t qn) {
  char *w = (char *)ws;
  a.lse = (float *)(w + L.off_lse);
  a.delta = (float *)(w + L.off_delta);
  a.ml = (float *)(w + L.off_ml);
  a.dqp = (float *)(w + L.off_dqp);
  a.n = n; a.B = b; a.H = h; a.Qn = qn;
  a.qrows = (int)L.qrows; a.splits = (int)L.splits; a.tpw = (int)L.tpw;
}

int pa_launch_stats(const PaArgs &a, hipStream_t st) {
  const dim3 grid((unsigned)((a.splits + 3) / 4), (unsigned)(a.B * a.H)), block(256);
  const int qt = a.qrows / 16;
  if (qt <= 1) hipLaunchKernelGGL(k_pa_stats<1>, grid, block, 0, st, a);
  else if (qt <= 2) hipLaunchKernelGGL(k_pa_stats<2>, grid, block, 0, st, a);
  else if (qt <= 4) hipLaunchKernelGGL(k_pa_stats<4>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_pa_stats<8>, grid, block, 0, st, a);
  SIDE_CHECK_LAUNCH("k_pa_stats");
  const int64_t rows = (int64_t)a.B * a.H * a.qrows;
  hipLaunchKernelGGL(k_pa_stats_merge, dim3((unsigned)((rows + 255) / 256)), block, 0, st, a);
  SIDE_CHECK_LAUNCH("k_pa_stats_merge");
  return 0;
}

}  // namespace

SIDE_EXPORTS(PA_FN, PA_ABI_VERSION)

extern "C" int64_t PA_FN(attn_bwd_workspace_bytes)(int64_t n, int32_t b, int32_t h, int32_t qn, int32_t dh) {
  if (!pa_served(n, b, h, qn, dh)) return 0;
  return pa_layout(n, b, h, qn).bytes;
}

extern "C" int PA_FN(attn_bwd_stats)(const float *q, const float *k, const uint32_t *bits, const uint32_t *any,
                                     const float *out, const float *dout, float *lse, float *delta, int64_t n, int32_t b,
                                     int32_t h, int32_t qn, int32_t dh, void *ws, int64_t ws_bytes, void *stream) {
  if (pa_check("attn_bwd_stats", n, b, h, qn, dh, ws, ws_bytes)) return 1;
  if (!q || !k || !out || !dout || !lse || !delta) return fail("attn_bwd_stats: null tensor");
  PaArgs a = {};
  a.q = q; a.k = k; a.out = out; a.dout = dout; a.bits = bits; a.any = any;
  pa_fill(a, pa_layout(n, b, h, qn), ws, n, b, h, qn);
  hipStream_t st = (hipStream_t)stream;
  if (pa_launch_stats(a, st)) return 1;
  const int64_t rows = (int64_t)b * h * qn;
  hipLaunchKernelGGL(k_pa_stats_copy, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, a, lse, delta);
  SIDE_CHECK_LAUNCH("k_pa_stats_copy");
  return 0;
}

extern "C" int PA_FN(attn_cross_bwd)(const float *q, const float *k, const float *v, const uint32_t *bits, const uint32_t *any,
                                     const float *out, const float *dout, float *dq, float *dk, float *dv, int64_t n,
                                     int32_t b, int32_t h, int32_t qn, int32_t dh, void *ws, int64_t ws_bytes, void *stream) {
  if (pa_check("attn_cross_bwd", n, b, h, qn, dh, ws, ws_bytes)) return 1;
  if (!q || !k || !v || !out || !dout) return fail("attn_cross_bwd: null tensor");
  if (!dq && !dk && !dv) return fail("attn_cross_bwd: no output wanted (dq, dk and dv are all null)");
  PaArgs a = {};
  a.q = q; a.k = k; a.v = v; a.out = out; a.dout = dout; a.bits = bits; a.any = any;
  a.dq = dq; a.dk = dk; a.dv = dv;
  pa_fill(a, pa_layout(n, b, h, qn), ws, n, b, h, qn);
  hipStream_t st = (hipStream_t)stream;
  if (pa_launch_stats(a, st)) return 1;
  const dim3 grid((unsigned)((a.splits + 3) / 4), (unsigned)(a.B * a.H)), block(256);
  const int qt = a.qrows / 16;
  if (qt <= 1) hipLaunchKernelGGL(k_pa_main<1>, grid, block, 0, st, a);
  else if (qt <= 2) hipLaunchKernelGGL(k_pa_main<2>, grid, block, 0, st, a);
  else if (qt <= 4) hipLaunchKernelGGL(k_pa_main<4>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_pa_main<8>, grid, block, 0, st, a);
  SIDE_CHECK_LAUNCH("k_pa_main");
  if (dq != nullptr) {
    const int64_t elems = (int64_t)b * h * qn * DH;
    hipLaunchKernelGGL(k_pa_dq_reduce, dim3((unsigned)((elems + 255) / 256)), block, 0, st, a);
    SIDE_CHECK_LAUNCH("k_pa_dq_reduce");
  }
  return 0;
}

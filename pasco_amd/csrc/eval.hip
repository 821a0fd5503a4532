// Evaluation passes (include/pasco_eval.h): SSC confusion + calibration bins over the dense sites of one output, panoptic
// (gt id, pred id) intersections over its sparse rows, the IoU > 0.5 match and the mask calibration bins.
//
// Accumulation: every thread keeps a run of equal keys in registers (neighbouring sites of one thread mostly share the
// (gt, pred) cell and the confidence bin: empty space) and flushes a run with one LDS integer atomic; a workgroup writes its
// LDS histogram to its own slab, and k_reduce adds the slabs in block order.  Floating sums are 64-bit fixed point, so
// there is no float atomic anywhere and every result is bitwise reproducible.  A slab entry holds at most 2^17 sites
// (PE_MAX_SITES / MAX_BLOCKS) of |term| <= 2^45, so it fits int64; the sum over slabs does not (2^27 confidences of 1.0
// are 2^63) and k_reduce adds in 128 bits.  The (gt, pred) intersection table is up to
// 1024 x 129 cells - larger than LDS - and takes global integer atomics after the same run caching; integer sums do not
// depend on their order either.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_eval.h"
#include "side_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NB = PE_BINS;
constexpr int MAX_BLOCKS = 1024;
constexpr int SITES_PER_THREAD = 8;
constexpr double CONF_SCALE = 68719476736.0;   // 2^36
constexpr double NLL_SCALE = 1073741824.0;     // 2^30
constexpr float CONF_LIMIT = 512.0f;           // finite confidences saturate here (pasco_eval.h)

struct Edges {
  float e[NB];
};

__device__ __forceinline__ int bin_of(float c, const Edges &E) {
  if (c != c) return NB - 1;  // NaN: torch.bucketize puts it past the last edge
  int n = 0;
#pragma unroll
  for (int i = 0; i < NB; ++i) n += (E.e[i] <= c) ? 1 : 0;
  return n > 0 ? n - 1 : 0;  // below the first edge (not a probability): bin 0 instead of torch's index -1
}

// Confidence term: NaN and +-inf add nothing, finite values saturate at +-CONF_LIMIT.
__device__ __forceinline__ long long conf_fixed(float v) {
  if (!isfinite(v)) return 0;
  return llrint(static_cast<double>(fminf(fmaxf(v, -CONF_LIMIT), CONF_LIMIT)) * CONF_SCALE);
}

// -log term: |t| <= 104 for every finite t (-log of the smallest subnormal); NaN and +-inf add nothing.
__device__ __forceinline__ long long nll_fixed(float t) { return isfinite(t) ? llrint(static_cast<double>(t) * NLL_SCALE) : 0; }

// First maximum of a row, a NaN being the maximum (torch.argmax); -0.0 == +0.0.
__device__ __forceinline__ int argmax_row(const float *row, int C) {
  float best = row[0];
  int pred = 0;
  for (int c = 1; c < C && best == best; ++c) {
    const float v = row[c];
    if (v > best || v != v) {
      best = v;
      pred = c;
    }
  }
  return pred;
}

__device__ __forceinline__ void lds_add(unsigned long long *p, long long v) {
  if (v != 0) atomicAdd(p, static_cast<unsigned long long>(v));
}

int blocks_for(int64_t n) {
  int64_t b = (n + (int64_t)BLOCK * SITES_PER_THREAD - 1) / ((int64_t)BLOCK * SITES_PER_THREAD);
  if (b < 1) b = 1;
  return b > MAX_BLOCKS ? MAX_BLOCKS : (int)b;
}

int ssc_slab(int c) { return PE_SSC_COUNTS(c) + PE_SSC_SUMS; }
constexpr int ECE_SLAB = PE_ECE_COUNTS + PE_ECE_SUMS;

// slab: [c*c confusion | 1 unknown | 2*NB count | 2*NB correct] ints, then [2*NB conf | 2 nll] fixed point
__global__ __launch_bounds__(BLOCK) void k_ssc(const float *__restrict__ probs, const float *__restrict__ conf,
                                               const uint8_t *__restrict__ gt, int64_t S, int C, Edges E,
                                               long long *__restrict__ slabs) {
  __shared__ unsigned long long s_h[PE_MAX_CLASSES * PE_MAX_CLASSES + 1 + 4 * NB + PE_SSC_SUMS];
  const int n_int = C * C + 1 + 4 * NB;
  const int slab = n_int + PE_SSC_SUMS;
  for (int i = threadIdx.x; i < slab; i += BLOCK) s_h[i] = 0;
  __syncthreads();
  unsigned long long *cm = s_h, *unk = s_h + C * C, *cnt = unk + 1, *cor = cnt + 2 * NB, *csum = cor + 2 * NB,
                     *nll = csum + 2 * NB;

  int cm_key = -1, b_key = -1;
  long long cm_n = 0, b_n = 0, b_cor = 0, b_fx = 0, n_unk = 0, nll0 = 0, nll1 = 0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < S; s += stride) {
    const int g = gt[s];
    if (g == 255) {
      ++n_unk;
      continue;
    }
    if (g >= C) continue;  // not a class of this output (the host refuses such labels)
    const float *row = probs + s * C;
    const int pred = argmax_row(row, C);
    const int key = g * C + pred;
    if (key != cm_key) {
      if (cm_key >= 0) lds_add(&cm[cm_key], cm_n);
      cm_key = key;
      cm_n = 0;
    }
    ++cm_n;
    const float cf = conf[s];
    const int grp = pred != 0;
    const int bk = grp * NB + bin_of(cf, E);
    if (bk != b_key) {
      if (b_key >= 0) {
        lds_add(&cnt[b_key], b_n);
        lds_add(&cor[b_key], b_cor);
        lds_add(&csum[b_key], b_fx);
      }
      b_key = bk;
      b_n = b_cor = b_fx = 0;
    }
    ++b_n;
    b_cor += (pred == g);
    b_fx += conf_fixed(cf);
    const long long l = nll_fixed(-logf(row[g] + 1e-12f));
    if (grp) nll1 += l; else nll0 += l;
  }
  if (cm_key >= 0) lds_add(&cm[cm_key], cm_n);
  if (b_key >= 0) {
    lds_add(&cnt[b_key], b_n);
    lds_add(&cor[b_key], b_cor);
    lds_add(&csum[b_key], b_fx);
  }
  lds_add(unk, n_unk);
  lds_add(&nll[0], nll0);
  lds_add(&nll[1], nll1);
  __syncthreads();
  long long *out = slabs + (int64_t)blockIdx.x * slab;
  for (int i = threadIdx.x; i < slab; i += BLOCK) out[i] = static_cast<long long>(s_h[i]);
}

// slab: [NB count | NB correct] ints, then [NB conf] fixed point
__global__ __launch_bounds__(BLOCK) void k_mask_ece(const int64_t *__restrict__ site, const int32_t *__restrict__ pred,
                                                    const float *__restrict__ conf, int64_t n,
                                                    const int32_t *__restrict__ gt_id, int64_t S,
                                                    const int32_t *__restrict__ map, int P, Edges E,
                                                    long long *__restrict__ slabs) {
  __shared__ unsigned long long s_h[ECE_SLAB];
  for (int i = threadIdx.x; i < ECE_SLAB; i += BLOCK) s_h[i] = 0;
  __syncthreads();
  int b_key = -1;
  long long b_n = 0, b_cor = 0, b_fx = 0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += stride) {
    const int64_t s = site[r];
    if (s < 0 || s >= S) continue;
    const int g = gt_id[s];
    const float cf = conf[r];
    if (g == 0 || cf == 0.0f) continue;
    const int p = pred[r];
    const int mp = (p >= 0 && p <= P) ? map[p] : 0;
    const int bk = bin_of(cf, E);
    if (bk != b_key) {
      if (b_key >= 0) {
        lds_add(&s_h[b_key], b_n);
        lds_add(&s_h[NB + b_key], b_cor);
        lds_add(&s_h[2 * NB + b_key], b_fx);
      }
      b_key = bk;
      b_n = b_cor = b_fx = 0;
    }
    ++b_n;
    b_cor += (mp == g);
    b_fx += conf_fixed(cf);
  }
  if (b_key >= 0) {
    lds_add(&s_h[b_key], b_n);
    lds_add(&s_h[NB + b_key], b_cor);
    lds_add(&s_h[2 * NB + b_key], b_fx);
  }
  __syncthreads();
  long long *out = slabs + (int64_t)blockIdx.x * ECE_SLAB;
  for (int i = threadIdx.x; i < ECE_SLAB; i += BLOCK) out[i] = static_cast<long long>(s_h[i]);
}

// Entry i of the slabs summed in block order; entries >= n_int are fixed point: scale_a below n_int + n_a, scale_b above.
// Counts stay below 2^27; the fixed-point sums are added in 128 bits and rounded to fp64 once.
__global__ __launch_bounds__(BLOCK) void k_reduce(const long long *__restrict__ slabs, int n_blocks, int slab, int n_int,
                                                  int n_a, double inv_a, double inv_b, int64_t *__restrict__ counts,
                                                  double *__restrict__ sums) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= slab) return;
  __int128 acc = 0;
  for (int b = 0; b < n_blocks; ++b) acc += slabs[(int64_t)b * slab + i];
  if (i < n_int)
    counts[i] = static_cast<int64_t>(acc);
  else
    sums[i - n_int] = static_cast<double>(acc) * (i - n_int < n_a ? inv_a : inv_b);
}

__global__ __launch_bounds__(BLOCK) void k_panop_pairs(const int64_t *__restrict__ site, const int32_t *__restrict__ pred,
                                                       int64_t n, const uint8_t *__restrict__ gt_sem,
                                                       const int32_t *__restrict__ gt_id, int64_t S, int P, int G,
                                                       unsigned long long *__restrict__ area,
                                                       unsigned long long *__restrict__ inter) {
  __shared__ unsigned long long s_area[PE_MAX_PRED + 1];
  for (int i = threadIdx.x; i <= P; i += BLOCK) s_area[i] = 0;
  __syncthreads();
  int a_key = -1, i_key = -1;
  long long a_n = 0, i_n = 0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n; r += stride) {
    const int64_t s = site[r];
    if (s < 0 || s >= S || gt_sem[s] == 255) continue;
    const int p = pred[r];
    if (p < 0 || p > P) continue;
    if (p != a_key) {
      if (a_key >= 0) lds_add(&s_area[a_key], a_n);
      a_key = p;
      a_n = 0;
    }
    ++a_n;
    const int g = gt_id[s];
    if (g < 0 || g > G) continue;
    const int key = g * (P + 1) + p;
    if (key != i_key) {
      if (i_key >= 0) atomicAdd(&inter[i_key], static_cast<unsigned long long>(i_n));
      i_key = key;
      i_n = 0;
    }
    ++i_n;
  }
  if (a_key >= 0) lds_add(&s_area[a_key], a_n);
  if (i_key >= 0) atomicAdd(&inter[i_key], static_cast<unsigned long long>(i_n));
  __syncthreads();
  for (int i = threadIdx.x; i <= P; i += BLOCK)
    if (s_area[i]) atomicAdd(&area[i], s_area[i]);
}

__global__ __launch_bounds__(BLOCK) void k_match(const int64_t *__restrict__ area, const int64_t *__restrict__ gt_area,
                                                 const int64_t *__restrict__ inter, int P, int G, int32_t *__restrict__ map) {
  for (int p = threadIdx.x; p <= P; p += BLOCK) {
    int m = 0;
    const int64_t ap = area[p];
    if (p > 0 && ap > 0) {
      for (int g = 1; g <= G; ++g) {
        const int64_t it = inter[(int64_t)g * (P + 1) + p];
        if (it > 0 && 2 * it > ap + gt_area[g] - it) {
          m = g;
          break;
        }
      }
    }
    map[p] = m;
  }
}

Edges edges_from(const float *h) {
  Edges e;
  for (int i = 0; i < NB; ++i) e.e[i] = h[i];
  return e;
}

}  // namespace

extern "C" {

SIDE_EXPORTS(PE_FN, PE_ABI_VERSION)

int64_t pe_ssc_workspace_bytes(int64_t n_sites, int32_t c) {
  return (int64_t)blocks_for(n_sites) * ssc_slab(c) * (int64_t)sizeof(long long);
}

int64_t pe_ece_workspace_bytes(int64_t n_rows) { return (int64_t)blocks_for(n_rows) * ECE_SLAB * (int64_t)sizeof(long long); }

int pe_ssc(const float *probs, const float *conf, const uint8_t *gt, int64_t n_sites, int32_t c, const float *h_edges,
           void *ws, int64_t ws_bytes, int64_t *counts, double *sums, void *stream) {
  if (c < 1 || c > PE_MAX_CLASSES) return fail("pe_ssc: %d classes, 1 .. %d supported", c, PE_MAX_CLASSES);
  if (n_sites < 0 || n_sites > PE_MAX_SITES) return fail("pe_ssc: %lld sites, at most %lld", (long long)n_sites, PE_MAX_SITES);
  if (ws_bytes < pe_ssc_workspace_bytes(n_sites, c)) return fail("pe_ssc: workspace of %lld bytes too small", (long long)ws_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = blocks_for(n_sites), slab = ssc_slab(c);
  hipLaunchKernelGGL(k_ssc, dim3(nb), dim3(BLOCK), 0, st, probs, conf, gt, n_sites, c, edges_from(h_edges),
                     static_cast<long long *>(ws));
  SIDE_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_reduce, dim3((slab + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, static_cast<const long long *>(ws), nb,
                     slab, PE_SSC_COUNTS(c), 2 * NB, 1.0 / CONF_SCALE, 1.0 / NLL_SCALE, counts, sums);
  SIDE_CHECK_HIP(hipGetLastError());
  return 0;
}

int pe_panop_pairs(const int64_t *site, const int32_t *pred, int64_t n, const uint8_t *gt_sem, const int32_t *gt_id,
                   int64_t n_sites, int32_t n_pred, int32_t n_gt, int64_t *area, int64_t *inter, void *stream) {
  if (n_pred < 0 || n_pred > PE_MAX_PRED) return fail("pe_panop_pairs: pred id %d beyond %d", n_pred, PE_MAX_PRED);
  if (n_gt < 0 || n_gt > PE_MAX_GT) return fail("pe_panop_pairs: gt id %d beyond %d", n_gt, PE_MAX_GT);
  if (n < 0) return fail("pe_panop_pairs: %lld rows", (long long)n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SIDE_CHECK_HIP(hipMemsetAsync(area, 0, sizeof(int64_t) * (n_pred + 1), st));
  SIDE_CHECK_HIP(hipMemsetAsync(inter, 0, sizeof(int64_t) * (int64_t)(n_gt + 1) * (n_pred + 1), st));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_panop_pairs, dim3(blocks_for(n)), dim3(BLOCK), 0, st, site, pred, n, gt_sem, gt_id, n_sites, n_pred,
                     n_gt, reinterpret_cast<unsigned long long *>(area), reinterpret_cast<unsigned long long *>(inter));
  SIDE_CHECK_HIP(hipGetLastError());
  return 0;
}

int pe_match(const int64_t *area, const int64_t *gt_area, const int64_t *inter, int32_t n_pred, int32_t n_gt, int32_t *map,
             void *stream) {
  if (n_pred < 0 || n_pred > PE_MAX_PRED) return fail("pe_match: pred id %d beyond %d", n_pred, PE_MAX_PRED);
  if (n_gt < 0 || n_gt > PE_MAX_GT) return fail("pe_match: gt id %d beyond %d", n_gt, PE_MAX_GT);
  hipLaunchKernelGGL(k_match, dim3(1), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), area, gt_area, inter, n_pred, n_gt,
                     map);
  SIDE_CHECK_HIP(hipGetLastError());
  return 0;
}

int pe_mask_ece(const int64_t *site, const int32_t *pred, const float *conf, int64_t n, const int32_t *gt_id,
                int64_t n_sites, const int32_t *map, int32_t n_pred, const float *h_edges, void *ws, int64_t ws_bytes,
                int64_t *counts, double *sums, void *stream) {
  if (n_pred < 0 || n_pred > PE_MAX_PRED) return fail("pe_mask_ece: pred id %d beyond %d", n_pred, PE_MAX_PRED);
  if (n < 0 || n > PE_MAX_SITES) return fail("pe_mask_ece: %lld rows, at most %lld", (long long)n, PE_MAX_SITES);
  if (ws_bytes < pe_ece_workspace_bytes(n)) return fail("pe_mask_ece: workspace of %lld bytes too small", (long long)ws_bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nb = blocks_for(n);
  hipLaunchKernelGGL(k_mask_ece, dim3(nb), dim3(BLOCK), 0, st, site, pred, conf, n, gt_id, n_sites, map, n_pred,
                     edges_from(h_edges), static_cast<long long *>(ws));
  SIDE_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(BLOCK), 0, st, static_cast<const long long *>(ws), nb, ECE_SLAB, PE_ECE_COUNTS,
                     NB, 1.0 / CONF_SCALE, 1.0 / CONF_SCALE, counts, sums);
  SIDE_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"

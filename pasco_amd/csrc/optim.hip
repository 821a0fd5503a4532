// AdamW with the global-norm clip folded in, over a table of tensors, for gfx950 (include/pasco_optim.h).
//
// Three launches per step, ordered by the stream alone: k_sqnorm (one fp64 partial per chunk), k_prepare (one workgroup: the
// partials in a fixed order, the clip scale, the per-tensor state records and fp32 scalars, the apply flag) and k_adamw (the
// update, 28 bytes per element).  The two table kernels have one geometry: a workgroup of 256 threads takes one chunk of
// PO_CHUNK = 4096 consecutive elements of ONE tensor at a time and strides over the chunk table with a capped grid; thread t
// owns the quads t, t + 256, t + 512, t + 768 of the chunk, so a wave's 16-byte accesses cover 1 KiB contiguous.  A tensor under
// 4 K elements (the BatchNorm weights and biases: most tensors of the net) is one chunk with a ragged end, a 256 x 256 x 27
// kernel 432 full ones: the same launch serves both, and the tensor count has no limit.
//
// k_adamw issues the 16 loads of a full chunk (4 quads of p, g, m, v) before the first store: the pointers come from a table
// in memory, so the compiler cannot prove that a store to p leaves the next quad of g alone and would otherwise serialise them.
//
// Every fp32 operation of the update is rounded on its own (contraction is off in this file; `/` and sqrt are the correctly
// rounded ones, hipcc's default for HIP), so the result is the one the torch restatement of pasco_amd/grad/host.py computes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_optim.h"
#include "side_common.h"

#pragma clang fp contract(off)

static_assert(sizeof(po_tensor) == 48 && sizeof(po_chunk) == 8 && sizeof(po_state) == 24 && sizeof(po_result) == 24 &&
                  sizeof(po_step) == 8 && sizeof(po_scalars) == 32 && sizeof(po_group) == 40,
              "the records of include/pasco_optim.h, as pasco_amd/grad/optimlib.py lays them out");

namespace {

constexpr int BLOCK = 256;
constexpr int QUADS = PO_CHUNK / 4;
constexpr int ITER = QUADS / BLOCK;
constexpr int MAX_GRID = 2048;                       // 256 CUs x 8 workgroups: the cap for memory-bound kernels
constexpr int64_t MAX_TOTAL = (int64_t)1 << 40;
constexpr int64_t MAX_CHUNKS = MAX_TOTAL / PO_CHUNK + ((int64_t)1 << 31);      // every tensor may end in a ragged chunk
static_assert(PO_CHUNK % (4 * BLOCK) == 0, "a chunk is a whole number of quads per thread");

__device__ __forceinline__ bool aligned16(const void *a, const void *b, const void *c, const void *d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// The chunk `c` of the table: its tensor and its length; false for an entry that points outside the table (never written by
// pasco_amd/grad/optim.py; an entry that did would otherwise address memory that is not the tensor's).
__device__ __forceinline__ bool chunk_of(const po_tensor *tensors, int32_t T, const po_chunk *chunks, int64_t c, po_tensor &t,
                                         int32_t &start, int &len) {
  const po_chunk ch = chunks[c];
  if (ch.tensor < 0 || ch.tensor >= T || ch.start < 0) return false;
  t = tensors[ch.tensor];
  if ((int64_t)ch.start >= t.n) return false;
  const int64_t left = t.n - ch.start;
  start = ch.start;
  len = left < PO_CHUNK ? (int)left : PO_CHUNK;
  return true;
}

// Sum over the 256 threads in a fixed tree: inside a wave by halving distances, the four waves in ascending order.  Valid in
// every thread.  `red` is BLOCK / 64 + 1 doubles.
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) s += red[w];
    red[BLOCK / 64] = s;
  }
  __syncthreads();
  const double s = red[BLOCK / 64];
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(BLOCK) k_sqnorm(const po_tensor *__restrict__ tensors, int32_t T, const po_chunk *__restrict__ chunks,
                                                  int64_t C, double *__restrict__ partials) {
  __shared__ double red[BLOCK / 64 + 1];
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    po_tensor t;
    int32_t start;
    int len;
    double acc = 0.0;
    if (chunk_of(tensors, T, chunks, c, t, start, len)) {
      const float *g = t.g + start;
      const bool vec = aligned16(t.p, t.g, t.m, t.v);
#pragma unroll
      for (int i = 0; i < ITER; ++i) {
        const int e = 4 * ((int)threadIdx.x + i * BLOCK);
        if (e >= len) break;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && e + 4 <= len) {
          const float4 q = *reinterpret_cast<const float4 *>(g + e);
          x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
        } else {
          for (int j = 0; j < 4 && e + j < len; ++j) x[j] = g[e + j];
        }
        // a lane past the end adds +0 * +0: the sum does not see it
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
      }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[c] = s;
  }
}

__global__ void __launch_bounds__(BLOCK) k_prepare(const po_tensor *__restrict__ tensors, int32_t T, const double *__restrict__ partials,
                                                   int64_t C, po_groups groups, int32_t n_groups, double max_norm, double grad_scale,
                                                   int32_t policy, po_state *__restrict__ states, po_scalars *__restrict__ scalars,
                                                   po_result *result, po_step *step) {
  __shared__ double red[BLOCK / 64 + 1];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < C; i += BLOCK) acc += partials[i];
  const double sumsq = block_sum(acc, red);
  const bool apply = __builtin_isfinite(sumsq) || policy != PO_POLICY_SKIP;
  if (threadIdx.x == 0) {
    const double norm = grad_scale * sqrt(sumsq);
    double c = 1.0;
    if (max_norm > 0.0) {
      c = max_norm / (norm + 1e-6);
      if (c >= 1.0) c = 1.0;      // a NaN fails the comparison and stays
    }
    result->sumsq = sumsq;
    result->norm = norm;
    if (!apply) result->skipped = result->skipped + 1;
    step->clip = (float)(c * grad_scale);
    step->apply = apply ? 1 : 0;
  }
  if (!apply) return;
  for (int32_t i = threadIdx.x; i < T; i += BLOCK) {
    const po_tensor t = tensors[i];
    if (t.group < 0 || t.group >= n_groups || t.state < 0) continue;
    const po_group h = groups.g[t.group];
    po_state st = states[t.state];
    st.step += 1;
    st.beta1_pow = st.beta1_pow * h.beta1;
    st.beta2_pow = st.beta2_pow * h.beta2;
    states[t.state] = st;
    po_scalars k;
    k.decay = (float)(1.0 - h.lr * h.weight_decay);
    k.omb1 = (float)(1.0 - h.beta1);
    k.b2 = (float)h.beta2;
    k.omb2 = (float)(1.0 - h.beta2);
    k.bc2sqrt = (float)sqrt(1.0 - st.beta2_pow);
    k.eps = (float)h.eps;
    k.neg_step = (float)(-h.lr / (1.0 - st.beta1_pow));
    k.unused = 0.f;
    scalars[t.state] = k;
  }
}

// THE update of one element (include/pasco_optim.h); pasco_amd/grad/host.py optim_adamw_ is the same line by line.
__device__ __forceinline__ void update(float &p, float g, float &m, float &v, float s, const po_scalars &k) {
  const float gs = g * s;
  p = p * k.decay;
  m = m + (gs - m) * k.omb1;
  v = v * k.b2 + (gs * gs) * k.omb2;
  const float d = __builtin_sqrtf(v) / k.bc2sqrt + k.eps;
  p = p + (m / d) * k.neg_step;
}

__device__ __forceinline__ void update4(float4 &p, const float4 &g, float4 &m, float4 &v, float s, const po_scalars &k) {
  update(p.x, g.x, m.x, v.x, s, k);
  update(p.y, g.y, m.y, v.y, s, k);
  update(p.z, g.z, m.z, v.z, s, k);
  update(p.w, g.w, m.w, v.w, s, k);
}

__global__ void __launch_bounds__(BLOCK) k_adamw(const po_tensor *__restrict__ tensors, int32_t T, const po_chunk *__restrict__ chunks,
                                                 int64_t C, const po_scalars *__restrict__ scalars, const po_step *__restrict__ step) {
  if (step->apply == 0) return;
  const float s = step->clip;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    po_tensor t;
    int32_t start;
    int len;
    if (!chunk_of(tensors, T, chunks, c, t, start, len) || t.state < 0) continue;
    const po_scalars k = scalars[t.state];
    float *p = t.p + start, *m = t.m + start, *v = t.v + start;
    const float *g = t.g + start;
    const bool vec = aligned16(t.p, t.g, t.m, t.v);
    if (vec && len == PO_CHUNK) {
      float4 qp[ITER], qg[ITER], qm[ITER], qv[ITER];
#pragma unroll
      for (int i = 0; i < ITER; ++i) {
        const int e = 4 * ((int)threadIdx.x + i * BLOCK);
        qp[i] = *reinterpret_cast<const float4 *>(p + e);
        qg[i] = *reinterpret_cast<const float4 *>(g + e);
        qm[i] = *reinterpret_cast<const float4 *>(m + e);
        qv[i] = *reinterpret_cast<const float4 *>(v + e);
      }
#pragma unroll
      for (int i = 0; i < ITER; ++i) {
        const int e = 4 * ((int)threadIdx.x + i * BLOCK);
        update4(qp[i], qg[i], qm[i], qv[i], s, k);
        *reinterpret_cast<float4 *>(p + e) = qp[i];
        *reinterpret_cast<float4 *>(m + e) = qm[i];
        *reinterpret_cast<float4 *>(v + e) = qv[i];
      }
      continue;
    }
    for (int i = 0; i < ITER; ++i) {
      const int e = 4 * ((int)threadIdx.x + i * BLOCK);
      if (e >= len) break;
      if (vec && e + 4 <= len) {
        float4 qp = *reinterpret_cast<const float4 *>(p + e), qm = *reinterpret_cast<const float4 *>(m + e),
               qv = *reinterpret_cast<const float4 *>(v + e);
        const float4 qg = *reinterpret_cast<const float4 *>(g + e);
        update4(qp, qg, qm, qv, s, k);
        *reinterpret_cast<float4 *>(p + e) = qp;
        *reinterpret_cast<float4 *>(m + e) = qm;
        *reinterpret_cast<float4 *>(v + e) = qv;
      } else {
        for (int j = 0; j < 4 && e + j < len; ++j) {
          float xp = p[e + j], xm = m[e + j], xv = v[e + j];
          update(xp, g[e + j], xm, xv, s, k);
          p[e + j] = xp, m[e + j] = xm, v[e + j] = xv;
        }
      }
    }
  }
}

inline hipStream_t st_of(void *stream) { return static_cast<hipStream_t>(stream); }

// nullptr = fine, else what is wrong
const char *table_error(int64_t T, int64_t C) {
  if (T < 0 || T >= ((int64_t)1 << 31)) return "T outside [0, 2^31)";
  if (C < 0 || C > MAX_CHUNKS) return "C outside [0, 2^40 / PO_CHUNK + 2^31]";
  return nullptr;
}

unsigned grid_of(int64_t C) { return (unsigned)(C < MAX_GRID ? C : MAX_GRID); }

}  // namespace

SIDE_EXPORTS(PO_FN, PO_ABI_VERSION)

extern "C" int PO_FN(table_check)(int64_t T, int64_t max_n, int64_t total, int32_t n_groups) {
  if (T < 0 || T >= ((int64_t)1 << 31)) return fail("table_check: %lld tensors, served are [0, 2^31)", (long long)T);
  if (max_n < 0 || max_n >= ((int64_t)1 << 31))
    return fail("table_check: a tensor of %lld elements, served are fewer than 2^31 per tensor", (long long)max_n);
  if (total < 0 || total >= MAX_TOTAL)
    return fail("table_check: %lld elements in all, served are fewer than 2^40", (long long)total);
  if (n_groups < 1 || n_groups > PO_MAX_GROUPS)
    return fail("table_check: %d parameter groups, served are 1 .. PO_MAX_GROUPS = %d", n_groups, PO_MAX_GROUPS);
  return 0;
}

extern "C" int PO_FN(sqnorm)(const po_tensor *tensors, int32_t T, const po_chunk *chunks, int64_t C, double *partials,
                             void *stream) {
  if (const char *e = table_error(T, C)) return fail("sqnorm: T = %d, C = %lld: %s", T, (long long)C, e);
  if (C == 0) return 0;
  if (tensors == nullptr || chunks == nullptr || partials == nullptr || T == 0) return fail("sqnorm: chunks without a table");
  hipLaunchKernelGGL(k_sqnorm, dim3(grid_of(C)), dim3(BLOCK), 0, st_of(stream), tensors, T, chunks, C, partials);
  SIDE_CHECK_LAUNCH("k_sqnorm");
  return 0;
}

extern "C" int PO_FN(prepare)(const po_tensor *tensors, int32_t T, const double *partials, int64_t C, po_groups groups,
                              int32_t n_groups, double max_norm, double grad_scale, int32_t policy, po_state *states,
                              po_scalars *scalars, po_result *result, po_step *step, void *stream) {
  if (const char *e = table_error(T, C)) return fail("prepare: T = %d, C = %lld: %s", T, (long long)C, e);
  if (n_groups < 1 || n_groups > PO_MAX_GROUPS)
    return fail("prepare: %d parameter groups, served are 1 .. PO_MAX_GROUPS = %d", n_groups, PO_MAX_GROUPS);
  if (policy != PO_POLICY_PROPAGATE && policy != PO_POLICY_SKIP) return fail("prepare: policy = %d", policy);
  if (!(grad_scale > 0.0) || !(grad_scale <= 1.79e308)) return fail("prepare: grad_scale = %g, must be positive and finite", grad_scale);
  if (max_norm != max_norm) return fail("prepare: max_norm is NaN");
  if (result == nullptr || step == nullptr) return fail("prepare: null result or step record");
  if ((C > 0 && partials == nullptr) || (T > 0 && (tensors == nullptr || states == nullptr || scalars == nullptr)))
    return fail("prepare: null pointer");
  hipLaunchKernelGGL(k_prepare, dim3(1), dim3(BLOCK), 0, st_of(stream), tensors, T, partials, C, groups, n_groups, max_norm,
                     grad_scale, policy, states, scalars, result, step);
  SIDE_CHECK_LAUNCH("k_prepare");
  return 0;
}

extern "C" int PO_FN(adamw)(const po_tensor *tensors, int32_t T, const po_chunk *chunks, int64_t C, const po_scalars *scalars,
                            const po_step *step, void *stream) {
  if (const char *e = table_error(T, C)) return fail("adamw: T = %d, C = %lld: %s", T, (long long)C, e);
  if (C == 0) return 0;
  if (tensors == nullptr || chunks == nullptr || scalars == nullptr || step == nullptr || T == 0)
    return fail("adamw: chunks without a table");
  hipLaunchKernelGGL(k_adamw, dim3(grid_of(C)), dim3(BLOCK), 0, st_of(stream), tensors, T, chunks, C, scalars, step);
  SIDE_CHECK_LAUNCH("k_adamw");
  return 0;
}

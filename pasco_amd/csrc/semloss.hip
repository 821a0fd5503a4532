// The semantic completion losses for gfx950 (include/pasco_semloss.h): the class-weighted cross entropy and the Lovasz-softmax
// loss of [N, C] logits against a dense label grid, forward and backward.
//
// k_rows_part: one row per lane.  The box test, the label gather, a max-subtracted softmax (the row's C logits are read three
// times: 80 bytes a row, the second and third pass hit L1), the cross-entropy partials of the row range and, per class, the
// bits of err = |[y == c] - p_c| as the sort key (a non-negative float orders as its bit pattern).  1 - p_y is formed as the sum
// of the OTHER exponentials over the sum, never by subtraction.  A workgroup owns one range of rows; k_rows_final adds the
// ranges in ascending order (the two CE sums in fp64, rounded once).
//
// ps_sort_desc: a least-significant-digit radix sort of (key, index) pairs over 8-bit digits of ~key (ascending in ~key =
// descending in key; LSD passes are stable and the indices start ascending, so equal keys stay in ascending index order).  Per
// pass k_sort_hist counts the digits of every tile of PS_SORT_TILE keys (LDS integer atomics), k_sort_scan turns the
// [tiles, 256] counts of a segment into the first output position of every (tile, digit), and k_sort_scatter ranks stably
// within the tile: a wave owns 512 consecutive keys and takes them 64 at a time in ascending order; lanes holding the same
// digit find each other with eight ballots (MI355X_MICROARCH.md: a wave64 ballot is one v_cmp into an SGPR pair), a lane's
// rank is the wave's running count of the digit plus the popcount of its peers below it; the four waves' counts are then
// stacked in wave order.  All segments go in one grid per kernel (blockIdx.y = the segment).
//
// k_lov_count / k_lov_scan / k_lov_tile: the int32 prefix sums of (foreground, inside the box) along a class's sorted order -
// per tile counts, a scan over the tiles, and the tile itself, which forms the closed-form increments (in fp64 from the
// integers, rounded once), the tile's part of dot(err_sorted, increment) and coef.  k_lov_final adds the tiles in ascending
// order.  k_loss_bwd is one pass over the rows.
// Determinism: every float sum is per-thread in ascending order, a fixed LDS tree, then ascending over workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_semloss.h"
#include "side_common.h"

#pragma clang fp contract(off)

SIDE_EXPORTS(PS_FN, PS_ABI_VERSION)

namespace {

constexpr int BLOCK = 256;
constexpr int TILE = PS_SORT_TILE;       // keys per workgroup
constexpr int KPT = TILE / BLOCK;        // keys per thread (8)
constexpr int WAVE_KEYS = TILE / 4;      // consecutive keys a wave owns (512)
constexpr int MIN_RANGE = 256;           // rows of a range at least
constexpr int MAX_RANGES = 256;          // ranges at most
constexpr int PART_WORDS = 40;           // one range's partials: ce_num, ce_den, class_count [C], rows, bad index, bad label
constexpr int PASSES = 4;

hipStream_t st_of(void *s) { return reinterpret_cast<hipStream_t>(s); }

int64_t pad256(int64_t v) { return (v + 255) / 256 * 256; }

bool served(int64_t n, int32_t c) { return n >= 0 && n <= PS_MAX_N && c >= PS_MIN_C && c <= PS_MAX_C; }

int64_t range_rows_of(int64_t n) {
  int64_t r = (n + MAX_RANGES - 1) / MAX_RANGES;
  r = (r + MIN_RANGE - 1) / MIN_RANGE * MIN_RANGE;
  return r < MIN_RANGE ? MIN_RANGE : r;
}

int64_t tiles_of(int64_t m) { return (m + TILE - 1) / TILE; }

int64_t sort_bytes_of(int64_t s, int64_t m) {
  if (s < 1 || s > 65535 || m < 0 || m > PS_MAX_N) return 0;
  // key A, key B, index B (index A is the output), the [S, tiles, 256] digit counts
  return 3 * pad256(4 * s * m) + pad256(4 * s * tiles_of(m) * 256);
}

struct Geometry {
  int64_t tile, tiles, range_rows, ranges, keys_bytes, perm_bytes, sort_bytes, rows_bytes, lovasz_bytes, workspace_bytes;
};

Geometry geometry_of(int64_t n, int32_t c) {
  Geometry g = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!served(n, c)) return g;
  g.tile = TILE;
  g.tiles = tiles_of(n);
  g.range_rows = range_rows_of(n);
  g.ranges = (n + g.range_rows - 1) / g.range_rows;
  g.keys_bytes = pad256(4 * (int64_t)c * n);
  g.perm_bytes = pad256(4 * (int64_t)c * n);
  g.sort_bytes = sort_bytes_of(c, n);
  g.rows_bytes = pad256(4 * PART_WORDS * g.ranges);
  g.lovasz_bytes = pad256(12 * (int64_t)c * g.tiles);      // (foreground, inside) int32 and one float per class and tile
  g.workspace_bytes = g.keys_bytes + g.perm_bytes + g.sort_bytes + g.rows_bytes + g.lovasz_bytes;
  return g;
}

// ---------------------------------------------------------------------------------------------------------------- rows

struct RowsArgs {
  const float *logits;
  const int32_t *coords;
  const uint8_t *target;
  const int32_t *box;
  const float *weights;
  uint8_t *label;
  uint32_t *keys;
  float *part;
  int64_t n, range_rows;
  int c, scale, dx, dy, dz;
};

// Fixed tree over the 256 per-thread values of s[]; the result is s[0].
__device__ __forceinline__ void tree_sum(float *s, int tid) {
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    __syncthreads();
    if (tid < w) s[tid] = s[tid] + s[tid + w];
  }
  __syncthreads();
}

__global__ void __launch_bounds__(BLOCK) k_rows_part(RowsArgs a) {
  __shared__ float s_num[BLOCK], s_den[BLOCK];
  __shared__ int s_cnt[PS_MAX_C + 3];
  const int tid = threadIdx.x;
  const int c = a.c;
  if (tid < PS_MAX_C + 3) s_cnt[tid] = 0;
  __syncthreads();
  const int64_t begin = (int64_t)blockIdx.x * a.range_rows;
  const int64_t end = begin + a.range_rows < a.n ? begin + a.range_rows : a.n;
  const int lox = a.box[0], loy = a.box[1], loz = a.box[2], hix = a.box[3], hiy = a.box[4], hiz = a.box[5];
  float num = 0.f, den = 0.f;
  for (int64_t row = begin + tid; row < end; row += BLOCK) {
    const int x = a.coords[row * 4 + 1], y = a.coords[row * 4 + 2], z = a.coords[row * 4 + 3];
    const bool inside = x >= lox && x <= hix && y >= loy && y <= hiy && z >= loz && z <= hiz;
    int lab = PS_LABEL_OUTSIDE;
    if (!inside) {
      for (int k = 0; k < c; ++k) a.keys[(int64_t)k * a.n + row] = 0u;
    } else {
      atomicAdd(&s_cnt[c], 1);
      const int64_t ix = ((int64_t)x - lox) / a.scale, iy = ((int64_t)y - loy) / a.scale, iz = ((int64_t)z - loz) / a.scale;
      if (ix >= a.dx || iy >= a.dy || iz >= a.dz) {
        atomicAdd(&s_cnt[c + 1], 1);
        lab = PS_LABEL_IGNORE;
      } else {
        lab = a.target[(ix * a.dy + iy) * a.dz + iz];
        if (lab >= c && lab != PS_LABEL_IGNORE) {
          atomicAdd(&s_cnt[c + 2], 1);
          lab = PS_LABEL_IGNORE;
        }
      }
      const float *f = a.logits + row * c;
      float m = f[0];
      for (int k = 1; k < c; ++k) m = fmaxf(m, f[k]);
      float sum = 0.f, others = 0.f;
      for (int k = 0; k < c; ++k) {
        const float e = expf(f[k] - m);
        sum += e;
        if (k != lab) others += e;
      }
      for (int k = 0; k < c; ++k) {
        const float err = k == lab ? others / sum : expf(f[k] - m) / sum;
        a.keys[(int64_t)k * a.n + row] = __float_as_uint(err);
      }
      if (lab < c) {
        atomicAdd(&s_cnt[lab], 1);
        const float w = a.weights[lab];
        num += w * ((logf(sum) + m) - f[lab]);
        den += w;
      }
    }
    a.label[row] = (uint8_t)lab;
  }
  s_num[tid] = num;
  s_den[tid] = den;
  tree_sum(s_num, tid);
  tree_sum(s_den, tid);
  float *dst = a.part + (int64_t)blockIdx.x * PART_WORDS;
  if (tid == 0) {
    dst[0] = s_num[0];
    dst[1] = s_den[0];
  }
  if (tid < c + 3) dst[2 + tid] = __int_as_float(s_cnt[tid]);
}

__global__ void __launch_bounds__(64) k_rows_final(const float *__restrict__ part, int64_t ranges, int c, float *__restrict__ ce,
                                                   int32_t *__restrict__ class_count, int32_t *__restrict__ info) {
  const int tid = threadIdx.x;
  if (tid < c + 3) {
    int s = 0;
    for (int64_t r = 0; r < ranges; ++r) s += __float_as_int(part[r * PART_WORDS + 2 + tid]);
    if (tid < c)
      class_count[tid] = s;
    else
      info[tid - c] = s;
  }
  if (tid == 63) {
    // the ranges' fp32 partials are folded in fp64 and rounded once: a chain of up to 256 fp32 additions would put its own
    // error (2e-7 of den at 171 ranges) into every element of the CE gradient, which divides by den
    double num64 = 0.0, den64 = 0.0;
    for (int64_t r = 0; r < ranges; ++r) {
      num64 += (double)part[r * PART_WORDS];
      den64 += (double)part[r * PART_WORDS + 1];
    }
    const float num = (float)num64, den = (float)den64;
    ce[0] = num / den;
    ce[1] = num;
    ce[2] = den;
    info[3] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- sort

__device__ __forceinline__ uint32_t digit_of(uint32_t key, int shift) { return ((~key) >> shift) & 255u; }

__global__ void __launch_bounds__(BLOCK) k_sort_hist(const uint32_t *__restrict__ kin, int64_t m, int64_t tiles, int shift,
                                                     uint32_t *__restrict__ counts) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.x;
  hist[tid] = 0u;
  __syncthreads();
  const int64_t seg = blockIdx.y, t0 = (int64_t)blockIdx.x * TILE;
  const uint32_t *k = kin + seg * m;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int64_t pos = t0 + r * BLOCK + tid;
    if (pos < m) atomicAdd(&hist[digit_of(k[pos], shift)], 1u);
  }
  __syncthreads();
  counts[(seg * tiles + blockIdx.x) * 256 + tid] = hist[tid];
}

// One workgroup per segment, thread d = digit d: counts[seg][tile][d] becomes the first output position of the tile's keys with
// digit d = (all keys with a smaller digit) + (the keys with digit d in earlier tiles).
__global__ void __launch_bounds__(BLOCK) k_sort_scan(uint32_t *__restrict__ counts, int64_t tiles) {
  __shared__ uint32_t tot[256];
  const int d = threadIdx.x;
  uint32_t *c = counts + (int64_t)blockIdx.x * tiles * 256;
  uint32_t run = 0u;
  for (int64_t t = 0; t < tiles; ++t) {
    const uint32_t v = c[t * 256 + d];
    c[t * 256 + d] = run;
    run += v;
  }
  tot[d] = run;
  __syncthreads();
  uint32_t base = 0u;
  for (int j = 0; j < d; ++j) base += tot[j];
  for (int64_t t = 0; t < tiles; ++t) c[t * 256 + d] += base;
}

// iin == nullptr: the indices are the positions (the first pass).  kout == nullptr: only the indices are written (the last).
__global__ void __launch_bounds__(BLOCK) k_sort_scatter(const uint32_t *__restrict__ kin, const int32_t *__restrict__ iin, int64_t m,
                                                        int64_t tiles, int shift, const uint32_t *__restrict__ counts,
                                                        uint32_t *__restrict__ kout, int32_t *__restrict__ iout) {
  __shared__ uint32_t cnt[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < 4 * 256; j += BLOCK) (&cnt[0][0])[j] = 0u;
  __syncthreads();
  const int64_t seg = blockIdx.y;
  const int64_t start = (int64_t)blockIdx.x * TILE + (int64_t)wave * WAVE_KEYS;
  const uint32_t *k = kin + seg * m;
  const int32_t *ix = iin == nullptr ? nullptr : iin + seg * m;
  uint32_t key[KPT], rank[KPT];
  int32_t idx[KPT];
  int dig[KPT];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < KPT; ++r) {
    const int64_t pos = start + r * 64 + lane;
    const bool valid = pos < m;
    key[r] = valid ? k[pos] : 0u;
    idx[r] = valid ? (ix == nullptr ? (int32_t)pos : ix[pos]) : 0;
    const uint32_t d = digit_of(key[r], shift);
    dig[r] = valid ? (int)d : -1;
    uint64_t peers = __ballot(valid);
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
    uint32_t run = counts[(seg * tiles + blockIdx.x) * 256 + tid];
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
    if (dst >= m) continue;      // cannot happen while the counts come from k_sort_hist on the same keys
    if (kout != nullptr) kout[seg * m + dst] = key[r];
    iout[seg * m + dst] = idx[r];
  }
}

// -------------------------------------------------------------------------------------------------------------- lovasz

__device__ __forceinline__ int label_at(const int32_t *perm, const uint8_t *label, int64_t n, int64_t pos, int32_t *row) {
  const int32_t r = perm[pos];
  *row = r;
  return (r < 0 || r >= n) ? PS_LABEL_OUTSIDE : (int)label[r];
}

__global__ void __launch_bounds__(BLOCK) k_lov_count(const int32_t *__restrict__ perm, const uint8_t *__restrict__ label, int64_t n,
                                                     int64_t tiles, int32_t *__restrict__ tilecnt) {
  __shared__ int s[2];
  const int tid = threadIdx.x, c = blockIdx.y;
  if (tid < 2) s[tid] = 0;
  __syncthreads();
  const int64_t p0 = (int64_t)blockIdx.x * TILE + (int64_t)tid * KPT;
  int fg = 0, in = 0;
  for (int j = 0; j < KPT; ++j) {
    if (p0 + j >= n) break;
    int32_t row;
    const int lab = label_at(perm + (int64_t)c * n, label, n, p0 + j, &row);
    fg += lab == c;
    in += lab != PS_LABEL_OUTSIDE;
  }
  if (fg) atomicAdd(&s[0], fg);
  if (in) atomicAdd(&s[1], in);
  __syncthreads();
  if (tid < 2) tilecnt[((int64_t)c * tiles + blockIdx.x) * 2 + tid] = s[tid];
}

// Exclusive scan over the tiles of a class: one thread per class and counter (the tiles are few: N / 2048).
__global__ void __launch_bounds__(64) k_lov_scan(int32_t *__restrict__ tilecnt, int64_t tiles) {
  const int tid = threadIdx.x;
  if (tid >= 2) return;
  int32_t *t = tilecnt + (int64_t)blockIdx.x * tiles * 2 + tid;
  int run = 0;
  for (int64_t i = 0; i < tiles; ++i) {
    const int v = t[2 * i];
    t[2 * i] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(BLOCK) k_lov_tile(const int32_t *__restrict__ perm, const uint8_t *__restrict__ label,
                                                    const uint32_t *__restrict__ keys, const int32_t *__restrict__ class_count,
                                                    const int32_t *__restrict__ tilecnt, int64_t n, int nc, int64_t tiles,
                                                    float *__restrict__ coef, float *__restrict__ partial) {
  __shared__ int s_fg[BLOCK], s_in[BLOCK];
  __shared__ float s_sum[BLOCK];
  const int tid = threadIdx.x, c = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * TILE + (int64_t)tid * KPT;
  const int32_t *pc = perm + (int64_t)c * n;
  int32_t row[KPT];
  int lab[KPT];
  int fg = 0, in = 0;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    row[j] = -1;
    lab[j] = PS_LABEL_OUTSIDE;
    if (p0 + j < n) lab[j] = label_at(pc, label, n, p0 + j, &row[j]);
    fg += lab[j] == c;
    in += lab[j] != PS_LABEL_OUTSIDE;
  }
  s_fg[tid] = fg;
  s_in[tid] = in;
  __syncthreads();
  // inclusive Hillis-Steele scan over the 256 per-thread counts
  for (int o = 1; o < BLOCK; o <<= 1) {
    const int a = tid >= o ? s_fg[tid - o] : 0, b = tid >= o ? s_in[tid - o] : 0;
    __syncthreads();
    s_fg[tid] += a;
    s_in[tid] += b;
    __syncthreads();
  }
  const int32_t *tc = tilecnt + ((int64_t)c * tiles + blockIdx.x) * 2;
  int cf = tc[0] + s_fg[tid] - fg;      // foreground rows before this thread's first position
  int i = tc[1] + s_in[tid] - in;       // rows inside the box before it = the position among the rows that count
  const int g = class_count[c];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (row[j] < 0 || row[j] >= n) continue;
    float v = 0.f;
    if (lab[j] != PS_LABEL_OUTSIDE) {
      if (g > 0) {
        double inc;
        if (lab[j] == c) {
          cf += 1;
          inc = 1.0 / (double)(g + (i + 1) - cf);
        } else {
          const double u = (double)(g + (i + 1) - cf);
          inc = (double)(g - cf) / ((u - 1.0) * u);
        }
        const float incf = (float)inc;
        sum += __uint_as_float(keys[(int64_t)c * n + row[j]]) * incf;
        v = lab[j] == c ? -incf : incf;
      } else if (lab[j] == c) {
        cf += 1;
      }
      i += 1;
    }
    coef[(int64_t)row[j] * nc + c] = v;
  }
  s_sum[tid] = sum;
  tree_sum(s_sum, tid);
  if (tid == 0) partial[(int64_t)c * tiles + blockIdx.x] = s_sum[0];
}

__global__ void __launch_bounds__(64) k_lov_final(const float *__restrict__ partial, const int32_t *__restrict__ class_count,
                                                  int64_t tiles, int c, float *__restrict__ loss_c, float *__restrict__ lovasz,
                                                  int32_t *__restrict__ present) {
  __shared__ float s[64];
  const int tid = threadIdx.x;
  float v = 0.f;
  if (tid < c && class_count[tid] > 0)
    for (int64_t t = 0; t < tiles; ++t) v += partial[(int64_t)tid * tiles + t];
  s[tid] = v;
  if (tid < c) loss_c[tid] = v;
  __syncthreads();
  if (tid == 0) {
    int p = 0;
    float total = 0.f;
    for (int k = 0; k < c; ++k) {
      if (class_count[k] > 0) {
        p += 1;
        total += s[k];
      }
    }
    *present = p;
    *lovasz = p > 0 ? total / (float)p : 0.f;
  }
}

__global__ void __launch_bounds__(BLOCK) k_loss_bwd(const float *__restrict__ logits, const uint8_t *__restrict__ label,
                                                    const float *__restrict__ coef, const float *__restrict__ weights,
                                                    const float *__restrict__ ce, const int32_t *__restrict__ present,
                                                    const float *__restrict__ g, int64_t n, int c, float *__restrict__ dlogits) {
  const int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  const int lab = label[row];
  float *d = dlogits + row * c;
  if (lab == PS_LABEL_OUTSIDE) {
    for (int k = 0; k < c; ++k) d[k] = 0.f;
    return;
  }
  const float *f = logits + row * c;
  const float *cf = coef + row * c;
  float m = f[0];
  for (int k = 1; k < c; ++k) m = fmaxf(m, f[k]);
  float sum = 0.f, others = 0.f;
  for (int k = 0; k < c; ++k) {
    const float e = expf(f[k] - m);
    sum += e;
    if (k != lab) others += e;
  }
  float dot = 0.f;
  for (int k = 0; k < c; ++k) dot += cf[k] * (expf(f[k] - m) / sum);
  const int np = *present;
  const float gl = np > 0 ? g[1] / (float)np : 0.f;
  const float gc = lab < c ? g[0] * weights[lab] / ce[2] : 0.f;
  for (int k = 0; k < c; ++k) {
    const float p = expf(f[k] - m) / sum;
    const float dce = k == lab ? -(others / sum) : p;      // p_k - [k == y] without the subtraction
    d[k] = (gc * dce + gl * p * (cf[k] - dot)) + 0.f;      // + 0: a zero is +0
  }
}

}  // namespace

extern "C" int PS_FN(geometry)(int64_t n, int32_t c, int64_t *g) {
  if (g == nullptr) return fail("ps_geometry: null pointer");
  const Geometry v = geometry_of(n, c);
  const int64_t w[PS_GEOMETRY_WORDS] = {v.tile,       v.tiles,      v.range_rows,   v.ranges,         v.keys_bytes,
                                        v.perm_bytes, v.sort_bytes, v.rows_bytes,   v.lovasz_bytes,   v.workspace_bytes};
  for (int i = 0; i < PS_GEOMETRY_WORDS; ++i) g[i] = w[i];
  return 0;
}

extern "C" int64_t PS_FN(workspace_bytes)(int64_t n, int32_t c) { return geometry_of(n, c).workspace_bytes; }

extern "C" int64_t PS_FN(sort_workspace_bytes)(int64_t s, int64_t m) { return sort_bytes_of(s, m); }

extern "C" int PS_FN(rows_fwd)(const float *logits, const int32_t *coords, const uint8_t *target, const int32_t *box, int32_t scale,
                               const float *weights, int64_t n, int32_t c, int32_t dx, int32_t dy, int32_t dz, uint8_t *label,
                               float *ce, int32_t *class_count, int32_t *info, uint32_t *keys, void *ws, int64_t ws_bytes,
                               void *stream) {
  if (c < PS_MIN_C || c > PS_MAX_C) return fail("ps_rows_fwd: %d classes not served (%d..%d)", c, PS_MIN_C, PS_MAX_C);
  if (n < 0 || n > PS_MAX_N) return fail("ps_rows_fwd: n = %lld rows not served (0..%d)", (long long)n, PS_MAX_N);
  if (scale < 1) return fail("ps_rows_fwd: scale %d", scale);
  if (dx < 1 || dy < 1 || dz < 1) return fail("ps_rows_fwd: grid %d x %d x %d", dx, dy, dz);
  if (ce == nullptr || class_count == nullptr || info == nullptr ||
      (n > 0 && (logits == nullptr || coords == nullptr || target == nullptr || box == nullptr || weights == nullptr ||
                 label == nullptr || keys == nullptr)))
    return fail("ps_rows_fwd: null pointer (logits %p coords %p target %p box %p weights %p label %p ce %p class_count %p info %p keys %p)",
                (const void *)logits, (const void *)coords, (const void *)target, (const void *)box, (const void *)weights,
                (void *)label, (void *)ce, (void *)class_count, (void *)info, (void *)keys);
  const Geometry g = geometry_of(n, c);
  if (g.rows_bytes > 0 && (ws == nullptr || ws_bytes < g.rows_bytes || ((uintptr_t)ws & 3) != 0))
    return fail("ps_rows_fwd: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)ws_bytes, (long long)g.rows_bytes);
  RowsArgs a;
  a.logits = logits;
  a.coords = coords;
  a.target = target;
  a.box = box;
  a.weights = weights;
  a.label = label;
  a.keys = keys;
  a.part = static_cast<float *>(ws);
  a.n = n;
  a.range_rows = g.range_rows;
  a.c = c;
  a.scale = scale;
  a.dx = dx;
  a.dy = dy;
  a.dz = dz;
  if (g.ranges > 0) {
    hipLaunchKernelGGL(k_rows_part, dim3((unsigned)g.ranges), dim3(BLOCK), 0, st_of(stream), a);
    SIDE_CHECK_LAUNCH("k_rows_part");
  }
  hipLaunchKernelGGL(k_rows_final, dim3(1), dim3(64), 0, st_of(stream), a.part, g.ranges, c, ce, class_count, info);
  SIDE_CHECK_LAUNCH("k_rows_final");
  return 0;
}

extern "C" int PS_FN(sort_desc)(const uint32_t *keys, int64_t s, int64_t m, int32_t *perm, void *ws, int64_t ws_bytes, void *stream) {
  if (s < 1 || s > 65535) return fail("ps_sort_desc: %lld segments not served (1..65535)", (long long)s);
  if (m < 0 || m > PS_MAX_N) return fail("ps_sort_desc: m = %lld keys a segment not served (0..%d)", (long long)m, PS_MAX_N);
  if (m == 0) return 0;
  if (keys == nullptr || perm == nullptr) return fail("ps_sort_desc: null pointer (keys %p perm %p)", (const void *)keys, (void *)perm);
  const int64_t need = sort_bytes_of(s, m);
  if (ws == nullptr || ws_bytes < need || ((uintptr_t)ws & 3) != 0)
    return fail("ps_sort_desc: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)ws_bytes, (long long)need);
  const int64_t tiles = tiles_of(m), part = pad256(4 * s * m);
  char *base = static_cast<char *>(ws);
  uint32_t *key_a = reinterpret_cast<uint32_t *>(base), *key_b = reinterpret_cast<uint32_t *>(base + part);
  int32_t *idx_b = reinterpret_cast<int32_t *>(base + 2 * part);
  uint32_t *counts = reinterpret_cast<uint32_t *>(base + 3 * part);
  const dim3 grid((unsigned)tiles, (unsigned)s), block(BLOCK);
  // keys -> B -> (A, perm) -> B -> perm
  const uint32_t *kin[PASSES] = {keys, key_b, key_a, key_b};
  const int32_t *iin[PASSES] = {nullptr, idx_b, perm, idx_b};
  uint32_t *kout[PASSES] = {key_b, key_a, key_b, nullptr};
  int32_t *iout[PASSES] = {idx_b, perm, idx_b, perm};
  for (int p = 0; p < PASSES; ++p) {
    hipLaunchKernelGGL(k_sort_hist, grid, block, 0, st_of(stream), kin[p], m, tiles, 8 * p, counts);
    SIDE_CHECK_LAUNCH("k_sort_hist");
    hipLaunchKernelGGL(k_sort_scan, dim3((unsigned)s), block, 0, st_of(stream), counts, tiles);
    SIDE_CHECK_LAUNCH("k_sort_scan");
    hipLaunchKernelGGL(k_sort_scatter, grid, block, 0, st_of(stream), kin[p], iin[p], m, tiles, 8 * p, counts, kout[p], iout[p]);
    SIDE_CHECK_LAUNCH("k_sort_scatter");
  }
  return 0;
}

extern "C" int PS_FN(lovasz_fwd)(const int32_t *perm, const uint8_t *label, const uint32_t *keys, const int32_t *class_count,
                                 int64_t n, int32_t c, float *loss_c, float *coef, float *lovasz, int32_t *present, void *ws,
                                 int64_t ws_bytes, void *stream) {
  if (c < PS_MIN_C || c > PS_MAX_C) return fail("ps_lovasz_fwd: %d classes not served (%d..%d)", c, PS_MIN_C, PS_MAX_C);
  if (n < 0 || n > PS_MAX_N) return fail("ps_lovasz_fwd: n = %lld rows not served (0..%d)", (long long)n, PS_MAX_N);
  if (class_count == nullptr || loss_c == nullptr || lovasz == nullptr || present == nullptr ||
      (n > 0 && (perm == nullptr || label == nullptr || keys == nullptr || coef == nullptr)))
    return fail("ps_lovasz_fwd: null pointer (perm %p label %p keys %p class_count %p loss_c %p coef %p lovasz %p present %p)",
                (const void *)perm, (const void *)label, (const void *)keys, (const void *)class_count, (void *)loss_c,
                (void *)coef, (void *)lovasz, (void *)present);
  const Geometry g = geometry_of(n, c);
  if (g.lovasz_bytes > 0 && (ws == nullptr || ws_bytes < g.lovasz_bytes || ((uintptr_t)ws & 3) != 0))
    return fail("ps_lovasz_fwd: workspace of %lld bytes, %lld needed (4-byte aligned)", (long long)ws_bytes, (long long)g.lovasz_bytes);
  int32_t *tilecnt = static_cast<int32_t *>(ws);
  float *partial = reinterpret_cast<float *>(tilecnt + 2 * (int64_t)c * g.tiles);
  if (g.tiles > 0) {
    const dim3 grid((unsigned)g.tiles, (unsigned)c), block(BLOCK);
    hipLaunchKernelGGL(k_lov_count, grid, block, 0, st_of(stream), perm, label, n, g.tiles, tilecnt);
    SIDE_CHECK_LAUNCH("k_lov_count");
    hipLaunchKernelGGL(k_lov_scan, dim3((unsigned)c), dim3(64), 0, st_of(stream), tilecnt, g.tiles);
    SIDE_CHECK_LAUNCH("k_lov_scan");
    hipLaunchKernelGGL(k_lov_tile, grid, block, 0, st_of(stream), perm, label, keys, class_count, tilecnt, n, c, g.tiles, coef,
                       partial);
    SIDE_CHECK_LAUNCH("k_lov_tile");
  }
  hipLaunchKernelGGL(k_lov_final, dim3(1), dim3(64), 0, st_of(stream), partial, class_count, g.tiles, c, loss_c, lovasz, present);
  SIDE_CHECK_LAUNCH("k_lov_final");
  return 0;
}

extern "C" int PS_FN(loss_bwd)(const float *logits, const uint8_t *label, const float *coef, const float *weights, const float *ce,
                               const int32_t *present, const float *g, int64_t n, int32_t c, float *dlogits, void *stream) {
  if (c < PS_MIN_C || c > PS_MAX_C) return fail("ps_loss_bwd: %d classes not served (%d..%d)", c, PS_MIN_C, PS_MAX_C);
  if (n < 0 || n > PS_MAX_N) return fail("ps_loss_bwd: n = %lld rows not served (0..%d)", (long long)n, PS_MAX_N);
  if (n == 0) return 0;
  if (logits == nullptr || label == nullptr || coef == nullptr || weights == nullptr || ce == nullptr || present == nullptr ||
      g == nullptr || dlogits == nullptr)
    return fail("ps_loss_bwd: null pointer (logits %p label %p coef %p weights %p ce %p present %p g %p dlogits %p)",
                (const void *)logits, (const void *)label, (const void *)coef, (const void *)weights, (const void *)ce,
                (const void *)present, (const void *)g, (void *)dlogits);
  hipLaunchKernelGGL(k_loss_bwd, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st_of(stream), logits, label, coef,
                     weights, ce, present, g, n, c, dlogits);
  SIDE_CHECK_LAUNCH("k_loss_bwd");
  return 0;
}

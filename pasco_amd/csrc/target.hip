// Training targets (include/pasco_target.h): the label grids of M subnets resampled under their transforms and the training
// crop, the multi-scale labels, the presence tables behind the mask targets, the masks themselves and the packed target words.
//
// pt_resample is pf_label_bounds' two passes with the second one writing what it finds: pass 1 the box of the transformed
// known voxels, pass 2 every cell of the host-side upper bound of that box, mapped back with T^-1 when it lies in the exact
// box, stored as one byte per grid (255 = nothing) and reduced to the semantic-only and instance-only bounds.  pt_labels
// runs one wave per 4^3 block of a subnet's scene: lane = voxel, the scale-4 cell is the wave and the eight scale-2 cells
// are eight fixed lane masks, so every count is a popcount of a ballot and the vote is a loop over the classes PRESENT in
// the block (no per-thread table).  Reductions are integer min / max (block, then one atomic per block and value) and an
// integer atomicMin for an instance's first voxel: all order independent, so two runs give the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_target.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

#include "transform_chain.h"

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = 2048;

struct Mats {
  float t[PT_MAX_M][16];
};

// the upper-bound boxes: lo and extent per subnet
struct Boxes {
  int32_t lo[PT_MAX_M][3];
  int32_t ext[PT_MAX_M][3];
};

struct Windows {
  double w[PT_MAX_M][4];
  int32_t on;
};

struct Outs {
  pt_subnet_out o[PT_MAX_M];
};

__device__ __forceinline__ bool in_window(const double *w, int x, int y) {
  const double dx = static_cast<double>(x), dy = static_cast<double>(y);
  return dx >= w[0] && dx < w[1] && dy >= w[2] && dy < w[3];
}

// v[0..5] as (min, min, min, max, max, max) over the block; thread j < 6 adds value j to dst with an integer atomic
__device__ __forceinline__ void block_minmax6(int v[6], int (*lds)[6], int32_t *dst) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    for (int o = 32; o > 0; o >>= 1) {
      int u = __shfl_down(v[j], o, 64);
      v[j] = j < 3 ? min(v[j], u) : max(v[j], u);
    }
  }
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) lds[w][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    int j = threadIdx.x;
    int r = lds[0][j];
    for (int q = 1; q < WAVES; ++q) r = j < 3 ? min(r, lds[q][j]) : max(r, lds[q][j]);
    if (j < 3) {
      if (r != INT32_MAX) atomicMin(dst + j, r);
    } else {
      if (r != INT32_MIN) atomicMax(dst + j, r);
    }
  }
}

__device__ __forceinline__ void take(int v[6], int x, int y, int z) {
  v[0] = min(v[0], x);
  v[1] = min(v[1], y);
  v[2] = min(v[2], z);
  v[3] = max(v[3], x);
  v[4] = max(v[4], y);
  v[5] = max(v[5], z);
}

#define EMPTY6 {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN}

__global__ void k_init_bounds(int32_t *out, int total, int32_t *flag) {
  for (int t = threadIdx.x; t < total; t += blockDim.x) out[t] = ((t / 3) % 2 == 0) ? INT32_MAX : INT32_MIN;
  if (flag && threadIdx.x == 0) flag[0] = 0;
}

// ---- pt_resample --------------------------------------------------------------------------------------------
// pass 1: box of transform_coords(known voxel, T_m); any non-zero instance id
__global__ __launch_bounds__(BLOCK) void k_box(const uint8_t *__restrict__ sem, const uint8_t *__restrict__ ins, int X, int Y,
                                               int Z, Mats T, int32_t *__restrict__ bounds, int32_t *__restrict__ flag) {
  __shared__ int lds[WAVES][6];
  const int64_t S = (int64_t)X * Y * Z;
  const int m = blockIdx.y;
  int v[6] = EMPTY6;
  bool any_ins = false;
  for (int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x; s < S; s += (int64_t)gridDim.x * BLOCK) {
    if (m == 0) any_ins = any_ins || ins[s] != 0;
    if (sem[s] == 255) continue;
    int64_t c[3] = {s / ((int64_t)Y * Z), (s / Z) % Y, s % Z};
    float h[3];
    metres_i64(c, h);
    int64_t o[3];
    apply_T(T.t[m], h, o);
    take(v, (int)o[0], (int)o[1], (int)o[2]);
  }
  if (m == 0 && __any(any_ins) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
  block_minmax6(v, lds, bounds + m * PT_BOUNDS);
}

// pass 2: every cell of the upper-bound box; inside the exact box the sample is mapped back with T_m^-1
__global__ __launch_bounds__(BLOCK) void k_samples(const uint8_t *__restrict__ sem, const uint8_t *__restrict__ ins, int X, int Y,
                                                   int Z, Mats Tinv, Boxes ub, uint8_t *__restrict__ sem_box,
                                                   uint8_t *__restrict__ ins_box, int64_t stride,
                                                   int32_t *__restrict__ bounds, const int32_t *__restrict__ flag) {
  __shared__ int lds[WAVES][6];
  const int m = blockIdx.y;
  const int32_t *box = bounds + m * PT_BOUNDS;
  const int blo[3] = {box[0], box[1], box[2]}, bhi[3] = {box[3], box[4], box[5]};
  const bool has_ins = flag[0] != 0;
  const int64_t ey = ub.ext[m][1], ez = ub.ext[m][2];
  const int64_t V = (int64_t)ub.ext[m][0] * ey * ez;
  int vs[6] = EMPTY6, vi[6] = EMPTY6;
  for (int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x; s < V; s += (int64_t)gridDim.x * BLOCK) {
    const int64_t c[3] = {ub.lo[m][0] + s / (ey * ez), ub.lo[m][1] + (s / ez) % ey, ub.lo[m][2] + s % ez};
    uint8_t a = 255, b = 255;
    if (c[0] >= blo[0] && c[0] <= bhi[0] && c[1] >= blo[1] && c[1] <= bhi[1] && c[2] >= blo[2] && c[2] <= bhi[2]) {
      float h[3];
      metres_i64(c, h);
      int64_t p[3];
      apply_T(Tinv.t[m], h, p);
      if (p[0] >= 0 && p[0] < X && p[1] >= 0 && p[1] < Y && p[2] >= 0 && p[2] < Z) {
        const int64_t site = (p[0] * Y + p[1]) * Z + p[2];
        a = sem[site];
        if (has_ins) b = ins[site];
        if (a != 255) take(vs, (int)c[0], (int)c[1], (int)c[2]);
        if (b != 255) take(vi, (int)c[0], (int)c[1], (int)c[2]);
      }
    }
    sem_box[m * stride + s] = a;
    ins_box[m * stride + s] = b;
  }
  block_minmax6(vs, lds, bounds + m * PT_BOUNDS + 6);
  block_minmax6(vi, lds, bounds + m * PT_BOUNDS + 12);
}

// ---- pt_crop_bounds -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_crop_bounds(const uint8_t *__restrict__ sem_box, const uint8_t *__restrict__ ins_box,
                                                       int64_t stride, Boxes ub, Windows win, int32_t *__restrict__ out) {
  __shared__ int lds[WAVES][6];
  const int m = blockIdx.y;
  const int64_t ey = ub.ext[m][1], ez = ub.ext[m][2];
  const int64_t V = (int64_t)ub.ext[m][0] * ey * ez;
  int vs[6] = EMPTY6, vi[6] = EMPTY6;
  for (int64_t s = blockIdx.x * (int64_t)BLOCK + threadIdx.x; s < V; s += (int64_t)gridDim.x * BLOCK) {
    const uint8_t a = sem_box[m * stride + s], b = ins_box[m * stride + s];
    if (a == 255 && b == 255) continue;
    const int x = ub.lo[m][0] + (int)(s / (ey * ez)), y = ub.lo[m][1] + (int)((s / ez) % ey), z = ub.lo[m][2] + (int)(s % ez);
    if (!in_window(win.w[m], x, y)) continue;
    if (a != 255) take(vs, x, y, z);
    if (b != 255) take(vi, x, y, z);
  }
  block_minmax6(vs, lds, out + m * PT_CROP_BOUNDS);
  block_minmax6(vi, lds, out + m * PT_CROP_BOUNDS + 6);
}

// ---- presence -----------------------------------------------------------------------------------------------
__global__ void k_init_tables(int32_t *table, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M * PT_TABLE) table[i] = ((i % PT_TABLE) / 256 == 1) ? INT32_MAX : 0;
}

// Wave-wide: instance id `id` of this lane's voxel at row-major index `idx` (lanes ascend in idx).  One atomicMin per wave and
// id: the lowest lane holding the id has the smallest index.
__device__ __forceinline__ void note_instances(uint8_t id, int32_t idx, int32_t *table) {
  const int lane = threadIdx.x & 63;
  bool pending = id != 0;
  unsigned long long rem;
  while ((rem = __ballot(pending)) != 0ull) {
    const int leader = __ffsll((long long)rem) - 1;
    const int cur = __shfl((int)id, leader, 64);
    if (lane == leader) atomicMin(table + 256 + cur, idx);
    if ((int)id == cur) pending = false;
  }
}

// after the tables' first indices are final: the class found there
__global__ void k_first_class(int32_t *table, int M, Outs outs, const uint8_t *single) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * 256) return;
  const int m = i / 256, id = i % 256;
  int32_t *t = table + m * PT_TABLE;
  const int32_t first = t[256 + id];
  const uint8_t *semantic = single ? single : outs.o[m].semantic;
  t[512 + id] = first == INT32_MAX ? 0 : semantic[first];
}

__global__ __launch_bounds__(BLOCK) void k_presence(const uint8_t *__restrict__ semantic, const uint8_t *__restrict__ instance,
                                                    int64_t n, int32_t *__restrict__ table) {
  const int lane = threadIdx.x & 63;
  // whole waves iterate together: the ballots inside need every lane of the wave in the loop
  const int64_t wave_first = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) - lane;
  for (int64_t base = wave_first; base < n; base += (int64_t)gridDim.x * BLOCK) {
    const int64_t i = base + lane;
    const uint8_t c = i < n ? semantic[i] : 255, id = i < n ? instance[i] : 0;
    bool pending = c != 0 && c != 255;
    unsigned long long rem;
    while ((rem = __ballot(pending)) != 0ull) {
      const int leader = __ffsll((long long)rem) - 1;
      const int cur = __shfl((int)c, leader, 64);
      if (lane == leader) table[cur] = 1;
      if ((int)c == cur) pending = false;
    }
    note_instances(id, (int32_t)i, table);
  }
}

// ---- pt_labels ----------------------------------------------------------------------------------------------
// lanes of the scale-2 cell (0, 0, 0) of a 4^3 block whose lane index is (x << 4) | (y << 2) | z
constexpr unsigned long long CELL2 = 0x330033ull;

__device__ __forceinline__ uint32_t pack4(uint32_t v) {
  // the four z-neighbours' bytes in the lane with z == 0 (little endian = ascending z)
  uint32_t r = v;
  r |= (uint32_t)__shfl_down((int)v, 1, 64) << 8;
  r |= (uint32_t)__shfl_down((int)v, 2, 64) << 16;
  r |= (uint32_t)__shfl_down((int)v, 3, 64) << 24;
  return r;
}

__global__ __launch_bounds__(BLOCK) void k_labels(const uint8_t *__restrict__ sem_box, const uint8_t *__restrict__ ins_box,
                                                  int64_t stride, Boxes ub, Windows win, Outs outs, int n_classes,
                                                  int32_t *__restrict__ table) {
  const int m = blockIdx.y;
  const pt_subnet_out &o = outs.o[m];
  const int lane = threadIdx.x & 63;
  const int SX = o.scene[0], SY = o.scene[1], SZ = o.scene[2];
  const int bx = SX >> 2, by = SY >> 2, bz = SZ >> 2;
  const int64_t n_blocks = (int64_t)bx * by * bz;
  const int lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
  const unsigned long long mine = CELL2 << (lane & 42);        // the lanes of this lane's scale-2 cell (42 = 0b101010)
  const bool first2 = (lane & 21) == 0;                          // the first lane of its scale-2 cell
  int32_t *tab = table + m * PT_TABLE;
  for (int64_t blk = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); blk < n_blocks; blk += (int64_t)gridDim.x * WAVES) {
    const int cx = (int)(blk / ((int64_t)by * bz)), cy = (int)((blk / bz) % by), cz = (int)(blk % bz);
    const int x = cx * 4 + lx, y = cy * 4 + ly, z = cz * 4 + lz;
    const int gx = o.min_C[0] + x, gy = o.min_C[1] + y, gz = o.min_C[2] + z;
    const int rx = gx - ub.lo[m][0], ry = gy - ub.lo[m][1], rz = gz - ub.lo[m][2];
    uint32_t c = 255, id = 255;
    if (rx >= 0 && rx < ub.ext[m][0] && ry >= 0 && ry < ub.ext[m][1] && rz >= 0 && rz < ub.ext[m][2] &&
        (!win.on || in_window(win.w[m], gx, gy))) {
      const int64_t cell = m * stride + ((int64_t)rx * ub.ext[m][1] + ry) * ub.ext[m][2] + rz;
      c = sem_box[cell];
      id = ins_box[cell];
    }
    if (id == 255) id = 0;
    const uint32_t g = c == 255 ? 255u : (c > 0 ? 1u : 0u);
    const int64_t idx = ((int64_t)x * SY + y) * SZ + z;
    const uint32_t pc = pack4(c), pi = pack4(id), pg = pack4(g);
    if (lz == 0) {                                                  // SZ and z are multiples of 4: aligned dwords
      *reinterpret_cast<uint32_t *>(o.semantic + idx) = pc;
      *reinterpret_cast<uint32_t *>(o.instance + idx) = pi;
      *reinterpret_cast<uint32_t *>(o.geo_1 + idx) = pg;
    }
    // the vote: over the classes present in the block, lowest class first on equal counts
    const unsigned long long unknown = __ballot(c == 255), occupied = __ballot(c != 0 && c != 255);
    int best4 = 0, cls4 = 0, best2 = 0, cls2 = 0;
    bool pending = c != 0 && c != 255;
    unsigned long long rem;
    while ((rem = __ballot(pending)) != 0ull) {
      const int leader = __ffsll((long long)rem) - 1;
      const int cur = __shfl((int)c, leader, 64);
      const unsigned long long same = __ballot((int)c == cur);
      if (lane == leader) tab[cur] = 1;
      if (cur < n_classes) {
        const int n4 = __popcll(same), n2 = __popcll(same & mine);
        if (n4 > best4 || (n4 == best4 && n4 > 0 && cur < cls4)) {
          best4 = n4;
          cls4 = cur;
        }
        if (n2 > best2 || (n2 == best2 && n2 > 0 && cur < cls2)) {
          best2 = n2;
          cls2 = cur;
        }
      }
      if ((int)c == cur) pending = false;
    }
    if (lane == 0) {
      const bool all_unknown = unknown == ~0ull;
      const int64_t i4 = ((int64_t)cx * by + cy) * bz + cz;
      o.sem_4[i4] = (uint8_t)(best4 > 0 ? cls4 : (all_unknown ? 0 : 255));
      o.geo_4[i4] = (uint8_t)(all_unknown ? 255 : (occupied != 0ull ? 1 : 0));
    }
    if (first2) {
      const bool all_unknown = (unknown & mine) == mine;
      const int64_t i2 = ((int64_t)(x >> 1) * (SY >> 1) + (y >> 1)) * (SZ >> 1) + (z >> 1);
      o.sem_2[i2] = (uint8_t)(best2 > 0 ? cls2 : (all_unknown ? 0 : 255));
      o.geo_2[i2] = (uint8_t)(all_unknown ? 255 : ((occupied & mine) != 0ull ? 1 : 0));
    }
    note_instances((uint8_t)id, (int32_t)idx, tab);
  }
}

// ---- pt_masks / pt_target_pack ------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_masks(const uint8_t *__restrict__ semantic, const uint8_t *__restrict__ instance,
                                                 int64_t n4, const int32_t *__restrict__ cls_slot,
                                                 const int32_t *__restrict__ ins_slot, int t, uint32_t *__restrict__ masks) {
  __shared__ int32_t cs[256], is[256];
  cs[threadIdx.x] = cls_slot[threadIdx.x];      // BLOCK == 256
  is[threadIdx.x] = ins_slot[threadIdx.x];
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BLOCK) {
    const uint32_t c = reinterpret_cast<const uint32_t *>(semantic)[i], d = reinterpret_cast<const uint32_t *>(instance)[i];
    const int a0 = cs[c & 255], a1 = cs[(c >> 8) & 255], a2 = cs[(c >> 16) & 255], a3 = cs[c >> 24];
    const int b0 = is[d & 255], b1 = is[(d >> 8) & 255], b2 = is[(d >> 16) & 255], b3 = is[d >> 24];
    for (int k = 0; k < t; ++k) {
      const uint32_t w = (uint32_t)(a0 == k || b0 == k) | ((uint32_t)(a1 == k || b1 == k) << 8) |
                         ((uint32_t)(a2 == k || b2 == k) << 16) | ((uint32_t)(a3 == k || b3 == k) << 24);
      masks[(int64_t)k * n4 + i] = w;
    }
  }
}

__global__ void k_target_pack(const uint8_t *__restrict__ semantic, const uint8_t *__restrict__ instance,
                              const int32_t *__restrict__ cls_slot, const int32_t *__restrict__ ins_slot,
                              const uint8_t *__restrict__ unknown, const int32_t *__restrict__ coords, int64_t n, int dx, int dy,
                              int dz, int ox, int oy, int oz, uint32_t *__restrict__ tbits, uint8_t *__restrict__ flags,
                              int32_t *__restrict__ oob) {
  const int64_t row = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (row >= n) return;
  const int64_t x = (int64_t)coords[row * 4 + 1] - ox, y = (int64_t)coords[row * 4 + 2] - oy, z = (int64_t)coords[row * 4 + 3] - oz;
  uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
  uint8_t f = 0;
  if (x < 0 || x >= dx || y < 0 || y >= dy || z < 0 || z >= dz) {
    atomicAdd(oob, 1);
  } else {
    const int64_t idx = (x * dy + y) * dz + z;
    const int slot[2] = {cls_slot[semantic[idx]], ins_slot[instance[idx]]};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = slot[j];
      if (k >= 0) {
        const uint32_t bit = 1u << (k & 31);
        w0 |= (k >> 5) == 0 ? bit : 0u;
        w1 |= (k >> 5) == 1 ? bit : 0u;
        w2 |= (k >> 5) == 2 ? bit : 0u;
        w3 |= (k >> 5) == 3 ? bit : 0u;
      }
    }
    const bool known = unknown == nullptr || unknown[idx] == 0;
    if (known) f = (uint8_t)(1 | ((w0 | w1 | w2 | w3) != 0u ? 2 : 0));
  }
  *reinterpret_cast<uint4 *>(tbits + row * 4) = make_uint4(w0, w1, w2, w3);
  flags[row] = f;
}

int grid_for(int64_t work) {
  int64_t b = (work + BLOCK - 1) / BLOCK;
  if (b < 1) b = 1;
  return static_cast<int>(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

// the upper-bound boxes of a call -> (Boxes, largest volume); 0 = a failure was recorded
int64_t boxes_of(const char *who, const int32_t *h_box_bound, int M, int64_t stride, Boxes &ub) {
  int64_t vmax = 0;
  ub = Boxes{};
  for (int m = 0; m < M; ++m) {
    int64_t v = 1;
    for (int d = 0; d < 3; ++d) {
      const int64_t e = (int64_t)h_box_bound[m * 6 + 3 + d] - h_box_bound[m * 6 + d] + 1;
      if (e <= 0 || e > (1 << 20)) {
        fail("%s: box bound of subnet %d has extent %lld on axis %d", who, m, (long long)e, d);
        return 0;
      }
      ub.lo[m][d] = h_box_bound[m * 6 + d];
      ub.ext[m][d] = (int32_t)e;
      v *= e;
    }
    if (v > stride) {
      fail("%s: box of subnet %d holds %lld cells, box_stride is %lld", who, m, (long long)v, (long long)stride);
      return 0;
    }
    if (v > vmax) vmax = v;
  }
  return vmax;
}

void windows_of(const double *h_window, int M, Windows &win) {
  win.on = h_window != nullptr;
  for (int m = 0; m < PT_MAX_M; ++m)
    for (int j = 0; j < 4; ++j) win.w[m][j] = (h_window && m < M) ? h_window[m * 4 + j] : 0.0;
}

}  // namespace

extern "C" {

SIDE_EXPORTS(PT_FN, PT_ABI_VERSION)

int64_t PT_FN(resample_workspace_bytes)(int32_t) { return 64; }

int PT_FN(resample)(const uint8_t *sem, const uint8_t *ins, int32_t X, int32_t Y, int32_t Z, const float *h_T,
                    const float *h_Tinv, int32_t M, const int32_t *h_box_bound, uint8_t *sem_box, uint8_t *ins_box,
                    int64_t box_stride, int32_t *bounds, void *ws, int64_t ws_bytes, void *stream) {
  if (M < 1 || M > PT_MAX_M) return fail("pt_resample: M = %d outside 1..%d", M, PT_MAX_M);
  if (X <= 0 || Y <= 0 || Z <= 0 || (int64_t)X * Y * Z > INT32_MAX) return fail("pt_resample: grid %d x %d x %d not served", X, Y, Z);
  if (!sem || !ins || !h_T || !h_Tinv || !h_box_bound || !sem_box || !ins_box || !bounds || !ws)
    return fail("pt_resample: null argument");
  if (ws_bytes < PT_FN(resample_workspace_bytes)(M)) return fail("pt_resample: workspace too small");
  Boxes ub;
  const int64_t vmax = boxes_of("pt_resample", h_box_bound, M, box_stride, ub);
  if (vmax == 0) return 1;
  Mats T, Ti;
  for (int m = 0; m < M; ++m)
    for (int j = 0; j < 16; ++j) {
      T.t[m][j] = h_T[m * 16 + j];
      Ti.t[m][j] = h_Tinv[m * 16 + j];
    }
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t *flag = static_cast<int32_t *>(ws);
  hipLaunchKernelGGL(k_init_bounds, dim3(1), dim3(BLOCK), 0, st, bounds, M * PT_BOUNDS, flag);
  SIDE_CHECK_LAUNCH("k_init_bounds");
  const int64_t S = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_box, dim3(grid_for(S), M), dim3(BLOCK), 0, st, sem, ins, X, Y, Z, T, bounds, flag);
  SIDE_CHECK_LAUNCH("k_box");
  hipLaunchKernelGGL(k_samples, dim3(grid_for(vmax), M), dim3(BLOCK), 0, st, sem, ins, X, Y, Z, Ti, ub, sem_box, ins_box,
                     box_stride, bounds, flag);
  SIDE_CHECK_LAUNCH("k_samples");
  return 0;
}

int PT_FN(crop_bounds)(const uint8_t *sem_box, const uint8_t *ins_box, int64_t box_stride, const int32_t *h_box_bound,
                       int32_t M, const double *h_window, int32_t *out, void *stream) {
  if (M < 1 || M > PT_MAX_M) return fail("pt_crop_bounds: M = %d outside 1..%d", M, PT_MAX_M);
  if (!sem_box || !ins_box || !h_box_bound || !h_window || !out) return fail("pt_crop_bounds: null argument");
  Boxes ub;
  const int64_t vmax = boxes_of("pt_crop_bounds", h_box_bound, M, box_stride, ub);
  if (vmax == 0) return 1;
  Windows win;
  windows_of(h_window, M, win);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_init_bounds, dim3(1), dim3(BLOCK), 0, st, out, M * PT_CROP_BOUNDS, (int32_t *)nullptr);
  SIDE_CHECK_LAUNCH("k_init_bounds");
  hipLaunchKernelGGL(k_crop_bounds, dim3(grid_for(vmax), M), dim3(BLOCK), 0, st, sem_box, ins_box, box_stride, ub, win, out);
  SIDE_CHECK_LAUNCH("k_crop_bounds");
  return 0;
}

int PT_FN(labels)(const uint8_t *sem_box, const uint8_t *ins_box, int64_t box_stride, const int32_t *h_box_bound, int32_t M,
                  const double *h_window, const pt_subnet_out *h_out, int32_t n_classes, int32_t *table, void *stream) {
  if (M < 1 || M > PT_MAX_M) return fail("pt_labels: M = %d outside 1..%d", M, PT_MAX_M);
  if (n_classes < 2 || n_classes > 255) return fail("pt_labels: %d classes not served (2..255)", n_classes);
  if (!sem_box || !ins_box || !h_box_bound || !h_out || !table) return fail("pt_labels: null argument");
  Boxes ub;
  if (boxes_of("pt_labels", h_box_bound, M, box_stride, ub) == 0) return 1;
  Windows win;
  windows_of(h_window, M, win);
  Outs outs;
  int64_t bmax = 1;
  for (int m = 0; m < M; ++m) {
    const pt_subnet_out &o = h_out[m];
    int64_t vol = 1;
    for (int d = 0; d < 3; ++d) {
      if (o.scene[d] < 4 || o.scene[d] % 4 != 0) return fail("pt_labels: scene size %d of subnet %d on axis %d is no multiple of 4", o.scene[d], m, d);
      vol *= o.scene[d];
    }
    if (vol > INT32_MAX) return fail("pt_labels: scene of subnet %d holds %lld voxels", m, (long long)vol);
    if (!o.semantic || !o.instance || !o.geo_1 || !o.geo_2 || !o.geo_4 || !o.sem_2 || !o.sem_4)
      return fail("pt_labels: null output of subnet %d", m);
    if ((((uintptr_t)o.semantic | (uintptr_t)o.instance | (uintptr_t)o.geo_1) & 3) != 0)
      return fail("pt_labels: grids of subnet %d not 4-byte aligned", m);
    outs.o[m] = o;
    if (vol / 64 > bmax) bmax = vol / 64;
  }
  for (int m = M; m < PT_MAX_M; ++m) outs.o[m] = h_out[0];
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_init_tables, dim3((M * PT_TABLE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, table, M);
  SIDE_CHECK_LAUNCH("k_init_tables");
  int64_t nb = (bmax + WAVES - 1) / WAVES;
  if (nb > MAX_BLOCKS) nb = MAX_BLOCKS;
  hipLaunchKernelGGL(k_labels, dim3((unsigned)nb, M), dim3(BLOCK), 0, st, sem_box, ins_box, box_stride, ub, win, outs, n_classes,
                     table);
  SIDE_CHECK_LAUNCH("k_labels");
  hipLaunchKernelGGL(k_first_class, dim3(M), dim3(256), 0, st, table, M, outs, (const uint8_t *)nullptr);
  SIDE_CHECK_LAUNCH("k_first_class");
  return 0;
}

int PT_FN(presence)(const uint8_t *semantic, const uint8_t *instance, int64_t n, int32_t *table, void *stream) {
  if (n < 1 || n > INT32_MAX) return fail("pt_presence: n = %lld voxels not served", (long long)n);
  if (!semantic || !instance || !table) return fail("pt_presence: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  Outs outs = {};
  hipLaunchKernelGGL(k_init_tables, dim3((PT_TABLE + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, table, 1);
  SIDE_CHECK_LAUNCH("k_init_tables");
  hipLaunchKernelGGL(k_presence, dim3(grid_for(n)), dim3(BLOCK), 0, st, semantic, instance, n, table);
  SIDE_CHECK_LAUNCH("k_presence");
  hipLaunchKernelGGL(k_first_class, dim3(1), dim3(256), 0, st, table, 1, outs, semantic);
  SIDE_CHECK_LAUNCH("k_first_class");
  return 0;
}

int PT_FN(masks)(const uint8_t *semantic, const uint8_t *instance, int64_t n, const int32_t *cls_slot, const int32_t *ins_slot,
                 int32_t t, uint8_t *masks, void *stream) {
  if (n < 4 || n % 4 != 0 || n > INT32_MAX) return fail("pt_masks: n = %lld voxels not served (a multiple of 4)", (long long)n);
  if (t < 0 || t > 510) return fail("pt_masks: %d targets", t);
  if (t == 0) return 0;
  if (!semantic || !instance || !cls_slot || !ins_slot || !masks) return fail("pt_masks: null argument");
  if ((((uintptr_t)semantic | (uintptr_t)instance | (uintptr_t)masks) & 3) != 0) return fail("pt_masks: arrays not 4-byte aligned");
  hipLaunchKernelGGL(k_masks, dim3(grid_for(n / 4)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), semantic, instance, n / 4,
                     cls_slot, ins_slot, t, reinterpret_cast<uint32_t *>(masks));
  SIDE_CHECK_LAUNCH("k_masks");
  return 0;
}

int PT_FN(target_pack)(const uint8_t *semantic, const uint8_t *instance, const int32_t *cls_slot, const int32_t *ins_slot,
                       const uint8_t *unknown, const int32_t *coords, int64_t n, int32_t t, int32_t dx, int32_t dy, int32_t dz,
                       int32_t ox, int32_t oy, int32_t oz, uint32_t *tbits, uint8_t *flags, int32_t *oob, void *stream) {
  if (n < 0 || n > INT32_MAX) return fail("pt_target_pack: n = %lld rows not served", (long long)n);
  if (t < 1 || t > PT_MAX_T) return fail("pt_target_pack: %d targets not served (1..%d)", t, PT_MAX_T);
  if (dx < 1 || dy < 1 || dz < 1) return fail("pt_target_pack: grid %d x %d x %d", dx, dy, dz);
  if (!semantic || !instance || !cls_slot || !ins_slot || !oob || (n > 0 && (!coords || !tbits || !flags)))
    return fail("pt_target_pack: null pointer");
  if (((uintptr_t)tbits & 15) != 0) return fail("pt_target_pack: tbits not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SIDE_CHECK_HIP(hipMemsetAsync(oob, 0, sizeof(int32_t), st));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_target_pack, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, semantic, instance, cls_slot,
                     ins_slot, unknown, coords, n, dx, dy, dz, ox, oy, oz, tbits, flags, oob);
  SIDE_CHECK_LAUNCH("k_target_pack");
  return 0;
}

}  // extern "C"

// Label generation (include/pasco_label.h): raw SemanticKITTI voxel labels -> the semantic grid, and the semantic grid
// -> panoptic thing instances (26-connected components per thing class, small ones dropped, ordered renumbering).
//
// pl_instances is seven launches on one stream, no host round trip:
//   k_local     one block per 8 x 8 x 32 tile (whole Z columns of the usual grid, eight consecutive sites per thread,
//               one 8-byte load).  Union-find in LDS over the tile's thing voxels, then every site writes the global
//               site index of its tile-local root (-1 on a non-thing voxel) and a zero count.
//   k_merge     every thing voxel unites with those of its 13 lexicographically earlier neighbours that lie in
//               another tile (faces, edges and corners) by atomicMin on the int32 parents.
//   k_flatten   parent[i] = root(i); one add per wave and root into count[root] where lanes share a root.
//   k_blockcnt  per block of 256 sites and per thing class: the surviving roots (count >= min_size); dropped components
//               and their voxels go to the record.
//   k_scan      exclusive scan of the [class position][block] table: one block, 4096 entries per round.
//   k_rank      final id of a surviving root = 1 + scanned offset + its raster rank among the same-class survivors of
//               its block (wave ballots); count[root] = -id, sizes[id - 1] = count.
//   k_write     both output grids.
//
// Why the result is unique.  A link always points from a site to a smaller site of the same component, and a union
// returns only after it has linked a root or found both ends under one root.  So when k_merge has finished, every
// component is one tree and its root is its smallest site, in whatever order the atomics landed; counts are integer
// sums; ids come from a scan in (class position, site) order.  Nothing depends on timing or placement.
//
// Why every loop ends.  find follows strictly decreasing parents.  In a union, each round that does not return replaces
// (a, b) by two sites both smaller than max(a, b), so it ends after at most S rounds; it still carries a hard cap that
// sets PL_STATUS_LOOP_CAP and returns.  No workgroup waits for another; there is no "repeat until nothing changed".
// A stale read of a parent (another CU's L1) is an older ancestor of the same set, which both loops tolerate; the atomic
// itself returns the true word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_label.h"
#include "side_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int TX = 8, TY = 8, TZ = 32;
constexpr int TILE = TX * TY * TZ;       // 2048 sites, 8 per thread
constexpr int PER = TILE / BLOCK;        // 8 consecutive z per thread
constexpr int UNION_CAP = 1 << 20;
constexpr int SCAN_BLOCK = 1024;
constexpr uint8_t NOT_THING = 0xFF;

struct ClsTab {
  uint8_t pos[256];   // semantic value -> position in thing_ids, NOT_THING otherwise
};

struct Grid {
  int X, Y, Z;
};

// ---- union-find on int parents (LDS: workgroup scope, global: agent scope) ---------------------------------------
template <int SCOPE>
__device__ __forceinline__ int find_root(int *p, int i) {
  for (;;) {
    int q = __hip_atomic_load(p + i, __ATOMIC_RELAXED, SCOPE);
    if (static_cast<unsigned>(q) >= static_cast<unsigned>(i)) return i;
    i = q;
  }
}

template <int SCOPE>
__device__ __forceinline__ bool unite(int *p, int a, int b) {
  for (int it = 0; it < UNION_CAP; ++it) {
    a = find_root<SCOPE>(p, a);
    b = find_root<SCOPE>(p, b);
    if (a == b) return true;
    int hi = a > b ? a : b, lo = a > b ? b : a;
    int old = __hip_atomic_fetch_min(p + hi, lo, __ATOMIC_RELAXED, SCOPE);
    if (old == hi) return true;   // hi was a root and now hangs under lo
    a = old;                      // hi had been linked meanwhile: its former parent and lo are still to be joined
    b = lo;
  }
  return false;
}

__device__ __forceinline__ void stage_tab(uint8_t *tab, const ClsTab &t) {
  tab[threadIdx.x] = t.pos[threadIdx.x];   // BLOCK == 256 entries
  __syncthreads();
}

// ---- pl_instances -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_local(const uint8_t *__restrict__ sem, Grid g, ClsTab t, int tiles_y,
                                                 int tiles_z, int sem_aligned, int *__restrict__ parent,
                                                 int *__restrict__ count, int *__restrict__ record) {
  __shared__ uint8_t tab[256];
  __shared__ uint8_t lab[TILE];
  __shared__ int par[TILE];
  stage_tab(tab, t);
  if (blockIdx.x == 0 && threadIdx.x < PL_RECORD) record[threadIdx.x] = 0;

  int b = blockIdx.x;
  const int tz = b % tiles_z;
  b /= tiles_z;
  const int ty = b % tiles_y, tx = b / tiles_y;
  const int col = threadIdx.x >> 2, lx = col >> 3, ly = col & 7, lz0 = (threadIdx.x & 3) * PER;
  const int x = tx * TX + lx, y = ty * TY + ly, z0 = tz * TZ + lz0;
  const bool in_xy = x < g.X && y < g.Y;
  const int64_t g0 = (static_cast<int64_t>(x) * g.Y + y) * g.Z + z0;
  const bool wide = in_xy && sem_aligned && (g.Z % PER == 0) && z0 < g.Z;   // 8 sites in the grid, 8-byte aligned
  const int l0 = threadIdx.x * PER;

  uint8_t c[PER];
  if (wide) {
    uint64_t v = *reinterpret_cast<const uint64_t *>(sem + g0);
#pragma unroll
    for (int k = 0; k < PER; ++k) c[k] = tab[(v >> (8 * k)) & 0xFF];
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) c[k] = (in_xy && z0 + k < g.Z) ? tab[sem[g0 + k]] : NOT_THING;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    lab[l0 + k] = c[k];
    par[l0 + k] = l0 + k;
  }
  __syncthreads();

  // the 13 neighbours that come earlier in site order; local index order is site order inside a tile
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (c[k] == NOT_THING) continue;
    const int lz = lz0 + k, me = l0 + k;
    for (int dx = -1; dx <= 0; ++dx) {
      const int nx = lx + dx;
      if (nx < 0) continue;
      const int dy_hi = dx < 0 ? 1 : 0;
      for (int dy = -1; dy <= dy_hi; ++dy) {
        const int ny = ly + dy;
        if (ny < 0 || ny >= TY) continue;
        const int dz_hi = (dx < 0 || dy < 0) ? 1 : -1;
        for (int dz = -1; dz <= dz_hi; ++dz) {
          const int nz = lz + dz;
          if (nz < 0 || nz >= TZ) continue;
          const int n = (nx * TY + ny) * TZ + nz;
          if (lab[n] == c[k]) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, me, n);   // ends within TILE rounds
        }
      }
    }
  }
  __syncthreads();

  int out[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (c[k] == NOT_THING) {
      out[k] = -1;
    } else {
      const int r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l0 + k);
      const int rx = r >> 8, ry = (r >> 5) & 7, rz = r & 31;
      out[k] = ((tx * TX + rx) * g.Y + ty * TY + ry) * g.Z + tz * TZ + rz;
    }
  }
  if (wide) {
    int4 *pp = reinterpret_cast<int4 *>(parent + g0), *pc = reinterpret_cast<int4 *>(count + g0);
    pp[0] = make_int4(out[0], out[1], out[2], out[3]);
    pp[1] = make_int4(out[4], out[5], out[6], out[7]);
    pc[0] = make_int4(0, 0, 0, 0);
    pc[1] = make_int4(0, 0, 0, 0);
  } else if (in_xy) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      if (z0 + k < g.Z) {
        parent[g0 + k] = out[k];
        count[g0 + k] = 0;
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_merge(const uint8_t *__restrict__ sem, Grid g, ClsTab t, int S, int *parent,
                                                 int *__restrict__ record) {
  __shared__ uint8_t tab[256];
  stage_tab(tab, t);
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= S) return;
  const uint8_t s = sem[i];
  if (tab[s] == NOT_THING) return;
  const int z = i % g.Z, xy = i / g.Z, y = xy % g.Y, x = xy / g.Y;
  bool ok = true;
  for (int dx = -1; dx <= 0; ++dx) {
    const int nx = x + dx;
    if (nx < 0) continue;
    const int dy_hi = dx < 0 ? 1 : 0;
    for (int dy = -1; dy <= dy_hi; ++dy) {
      const int ny = y + dy;
      if (ny < 0 || ny >= g.Y) continue;
      const int dz_hi = (dx < 0 || dy < 0) ? 1 : -1;
      for (int dz = -1; dz <= dz_hi; ++dz) {
        const int nz = z + dz;
        if (nz < 0 || nz >= g.Z) continue;
        if ((nx / TX == x / TX) && (ny / TY == y / TY) && (nz / TZ == z / TZ)) continue;   // joined in k_local
        const int n = (nx * g.Y + ny) * g.Z + nz;
        if (sem[n] == s) ok = unite<__HIP_MEMORY_SCOPE_AGENT>(parent, i, n) && ok;
      }
    }
  }
  if (!ok) atomicOr(record + PL_REC_STATUS, PL_STATUS_LOOP_CAP);
}

__global__ __launch_bounds__(BLOCK) void k_flatten(int S, int *parent, int *__restrict__ count) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int r = -1;
  if (i < S && parent[i] >= 0) {
    r = find_root<__HIP_MEMORY_SCOPE_AGENT>(parent, i);
    parent[i] = r;   // a smaller site of the same set: other walkers may see either value
  }
  // one add per wave and root for the first few distinct roots of the wave, the rest one by one
  bool active = r >= 0;
  for (int round = 0; round < 4; ++round) {
    const uint64_t am = __ballot(active);
    if (am == 0) break;
    const int leader = __ffsll(static_cast<long long>(am)) - 1;
    const int r0 = __shfl(r, leader);
    const bool mine = active && r == r0;
    const uint64_t mm = __ballot(mine);
    if (lane == leader) atomicAdd(count + r0, __popcll(mm));
    if (mine) active = false;
  }
  if (active) atomicAdd(count + r, 1);
}

// is site i a surviving root / a dropped root
__device__ __forceinline__ int root_count(const int *parent, const int *count, int i, int S) {
  return (i < S && parent[i] == i) ? count[i] : 0;
}

__global__ __launch_bounds__(BLOCK) void k_blockcnt(const uint8_t *__restrict__ sem, ClsTab t, int S, int n_things,
                                                    int min_size, const int *__restrict__ parent,
                                                    const int *__restrict__ count, int *__restrict__ blockcnt,
                                                    int *__restrict__ record) {
  __shared__ uint8_t tab[256];
  __shared__ int surv[PL_MAX_THINGS];
  __shared__ int drop[2];
  if (threadIdx.x < PL_MAX_THINGS) surv[threadIdx.x] = 0;
  if (threadIdx.x < 2) drop[threadIdx.x] = 0;
  stage_tab(tab, t);
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const int n = root_count(parent, count, i, S);
  if (n > 0) {
    if (n >= min_size) {
      atomicAdd(&surv[tab[sem[i]]], 1);
    } else {
      atomicAdd(&drop[0], 1);
      atomicAdd(&drop[1], n);
    }
  }
  __syncthreads();
  if (threadIdx.x < n_things) blockcnt[static_cast<int64_t>(threadIdx.x) * gridDim.x + blockIdx.x] = surv[threadIdx.x];
  if (threadIdx.x == 0 && drop[0] != 0) {
    atomicAdd(record + PL_REC_DROPPED, drop[0]);
    atomicAdd(record + PL_REC_UNKNOWN, drop[1]);
  }
}

// in-place exclusive scan of n ints by one block, 4096 per round (one 16-byte load per lane, wave scans by shuffle, the
// 16 wave totals through LDS); the total goes to record[PL_REC_INSTANCES].  v is 16-byte aligned.
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan(int *__restrict__ v, int64_t n, int *__restrict__ record) {
  constexpr int SCAN_WAVES = SCAN_BLOCK / 64;
  __shared__ int wsum[SCAN_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int64_t base = 0; base < n; base += 4 * SCAN_BLOCK) {
    const int64_t j = base + 4 * threadIdx.x;
    int x[4] = {0, 0, 0, 0};
    if (j + 3 < n) {
      const int4 q = *reinterpret_cast<const int4 *>(v + j);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = j + k < n ? v[j + k] : 0;
    }
    const int s = x[0] + x[1] + x[2] + x[3];
    int inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
      const int t = wsum[w];
      before += w < wave ? t : 0;
      total += t;
    }
    int run = carry + before + inc - s;
    if (j + 3 < n) {
      *reinterpret_cast<int4 *>(v + j) = make_int4(run, run + x[0], run + x[0] + x[1], run + x[0] + x[1] + x[2]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (j + k < n) v[j + k] = run;
        run += x[k];
      }
    }
    carry += total;
    __syncthreads();   // wsum is rewritten in the next round
  }
  if (threadIdx.x == 0) record[PL_REC_INSTANCES] = carry;
}

__global__ __launch_bounds__(BLOCK) void k_rank(const uint8_t *__restrict__ sem, ClsTab t, int S, int min_size,
                                                const int *__restrict__ parent, int *__restrict__ count,
                                                const int *__restrict__ blockoff, int *__restrict__ sizes,
                                                int sizes_cap) {
  __shared__ uint8_t tab[256];
  __shared__ int wcnt[WAVES][PL_MAX_THINGS];
  if (threadIdx.x < WAVES * PL_MAX_THINGS) (&wcnt[0][0])[threadIdx.x] = 0;
  stage_tab(tab, t);
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = root_count(parent, count, i, S);
  const bool surv = n > 0 && n >= min_size;
  const int c = surv ? tab[sem[i]] : -1;
  // raster rank among the wave's survivors of the same class: one round per class present (at most PL_MAX_THINGS)
  int rank = 0;
  bool active = surv;
  for (int round = 0; round < PL_MAX_THINGS; ++round) {
    const uint64_t am = __ballot(active);
    if (am == 0) break;
    const int leader = __ffsll(static_cast<long long>(am)) - 1;
    const int c0 = __shfl(c, leader);
    const bool mine = active && c == c0;
    const uint64_t mm = __ballot(mine);
    if (mine) {
      rank = __popcll(mm & ((1ull << lane) - 1ull));
      active = false;
    }
    if (lane == leader) wcnt[wave][c0] = __popcll(mm);
  }
  __syncthreads();
  if (!surv) return;
  int before = blockoff[static_cast<int64_t>(c) * gridDim.x + blockIdx.x];
  for (int w = 0; w < wave; ++w) before += wcnt[w][c];
  const int id = 1 + before + rank;
  if (sizes != nullptr && id - 1 < sizes_cap) sizes[id - 1] = n;
  count[i] = -id;
}

template <int VEC>
__global__ __launch_bounds__(BLOCK) void k_write(const uint8_t *__restrict__ sem, ClsTab t, int S,
                                                 const int *__restrict__ parent, const int *__restrict__ count,
                                                 int *__restrict__ instance, uint8_t *__restrict__ sem_out) {
  __shared__ uint8_t tab[256];
  stage_tab(tab, t);
  const int i0 = (blockIdx.x * BLOCK + threadIdx.x) * VEC;
  if (i0 >= S) return;
  uint8_t s[VEC];
  int ins[VEC];
  if (VEC == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t *>(sem + i0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = (v >> (8 * k)) & 0xFF;
  } else {
    s[0] = sem[i0];
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    ins[k] = 0;
    if (tab[s[k]] != NOT_THING) {
      const int v = count[parent[i0 + k]];   // -id of a survivor, the voxel count of a dropped component
      if (v < 0) {
        ins[k] = -v;
      } else {
        s[k] = 255;
      }
    }
  }
  if (VEC == 4) {
    *reinterpret_cast<int4 *>(instance + i0) = make_int4(ins[0], ins[1], ins[2], ins[3 % VEC]);
    *reinterpret_cast<uint32_t *>(sem_out + i0) =
        static_cast<uint32_t>(s[0]) | (static_cast<uint32_t>(s[1 % VEC]) << 8) |
        (static_cast<uint32_t>(s[2 % VEC]) << 16) | (static_cast<uint32_t>(s[3 % VEC]) << 24);
  } else {
    instance[i0] = ins[0];
    sem_out[i0] = s[0];
  }
}

// ---- pl_semantic_grid: 8 voxels (one byte of the invalid mask) per thread ------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void k_semantic(const uint16_t *__restrict__ raw, const uint8_t *__restrict__ invalid,
                                                    const uint8_t *__restrict__ lut, int n_lut, int64_t n_bytes,
                                                    uint8_t *__restrict__ sem, int *__restrict__ status) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
  if (j >= n_bytes) return;
  const uint32_t bits = invalid[j];
  uint16_t r[8];
  if (WIDE) {
    const uint4 v = *reinterpret_cast<const uint4 *>(raw + j * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFF;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = raw[j * 8 + k];
  }
  uint64_t out = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint32_t v = 255;
    if (r[k] >= n_lut) {
      bad = true;
    } else if (((bits >> (7 - k)) & 1u) == 0) {
      v = lut[r[k]];
    }
    out |= static_cast<uint64_t>(v) << (8 * k);
  }
  if (WIDE) {
    *reinterpret_cast<uint64_t *>(sem + j * 8) = out;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) sem[j * 8 + k] = (out >> (8 * k)) & 0xFF;
  }
  if (bad) atomicOr(status, PL_STATUS_RAW_RANGE);
}

int64_t blocks_of(int64_t n, int per) { return (n + per - 1) / per; }

bool grid_ok(int32_t X, int32_t Y, int32_t Z) {
  return X >= 1 && Y >= 1 && Z >= 1 && static_cast<int64_t>(X) * Y * Z <= PL_MAX_SITES;
}

}  // namespace

extern "C" {

SIDE_EXPORTS(PL_FN, PL_ABI_VERSION)

int PL_FN(semantic_grid)(const uint16_t *raw, const uint8_t *invalid, const uint8_t *lut, int32_t n_lut, int64_t S,
                         uint8_t *sem, int32_t *d_status, void *stream) {
  if (S < 0 || S % 8 != 0) return fail("pl_semantic_grid: %lld voxels, a multiple of 8 is required", (long long)S);
  if (n_lut < 1 || n_lut > 65536) return fail("pl_semantic_grid: lookup table of %d entries", n_lut);
  if (S == 0) return 0;
  if (!raw || !invalid || !lut || !sem || !d_status) return fail("pl_semantic_grid: null pointer");
  const int64_t n_bytes = S / 8, blocks = blocks_of(n_bytes, BLOCK);
  if (blocks > INT32_MAX) return fail("pl_semantic_grid: %lld voxels are too many", (long long)S);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool wide = reinterpret_cast<uintptr_t>(raw) % 16 == 0 && reinterpret_cast<uintptr_t>(sem) % 8 == 0;
  if (wide) {
    k_semantic<true><<<static_cast<unsigned>(blocks), BLOCK, 0, st>>>(raw, invalid, lut, n_lut, n_bytes, sem, d_status);
  } else {
    k_semantic<false><<<static_cast<unsigned>(blocks), BLOCK, 0, st>>>(raw, invalid, lut, n_lut, n_bytes, sem, d_status);
  }
  SIDE_CHECK_LAUNCH("k_semantic");
  return 0;
}

int64_t PL_FN(instances_workspace_bytes)(int32_t X, int32_t Y, int32_t Z, int32_t n_things) {
  if (!grid_ok(X, Y, Z) || n_things < 0 || n_things > PL_MAX_THINGS) return -1;
  const int64_t S = static_cast<int64_t>(X) * Y * Z;
  const int64_t S4 = (S + 3) / 4 * 4;   // keeps the three arrays 16-byte aligned
  const int64_t table = (static_cast<int64_t>(n_things > 0 ? n_things : 1) * blocks_of(S, BLOCK) + 3) / 4 * 4;
  return 4 * (2 * S4 + table);
}

int PL_FN(instances)(const uint8_t *sem, int32_t X, int32_t Y, int32_t Z, const int32_t *h_thing_ids, int32_t n_things,
                     int32_t min_size, int32_t *instance, uint8_t *semantic_out, int32_t *record, int32_t *sizes,
                     int32_t sizes_cap, void *ws, int64_t ws_bytes, void *stream) {
  if (!grid_ok(X, Y, Z)) return fail("pl_instances: grid %d x %d x %d (1 <= X, Y, Z and at most %d sites)", X, Y, Z, PL_MAX_SITES);
  if (n_things < 0 || n_things > PL_MAX_THINGS) return fail("pl_instances: %d thing ids, at most %d", n_things, PL_MAX_THINGS);
  if (n_things > 0 && !h_thing_ids) return fail("pl_instances: null thing ids");
  if (min_size < 0) return fail("pl_instances: min_size %d", min_size);
  if (!sem || !instance || !semantic_out || !record || !ws) return fail("pl_instances: null pointer");
  if (sem == semantic_out) return fail("pl_instances: semantic_out may not alias sem");
  if (sizes_cap < 0) return fail("pl_instances: sizes_cap %d", sizes_cap);
  ClsTab tab;
  for (int i = 0; i < 256; ++i) tab.pos[i] = NOT_THING;
  for (int i = 0; i < n_things; ++i) {
    const int32_t id = h_thing_ids[i];
    if (id < 1 || id > 254) return fail("pl_instances: thing id %d (1..254)", id);
    if (tab.pos[id] != NOT_THING) return fail("pl_instances: thing id %d given twice", id);
    tab.pos[id] = static_cast<uint8_t>(i);
  }
  const int64_t need = PL_FN(instances_workspace_bytes)(X, Y, Z, n_things);
  if (ws_bytes < need) return fail("pl_instances: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return fail("pl_instances: workspace not 16-byte aligned");

  const int S = X * Y * Z;
  const int S4 = (S + 3) / 4 * 4;
  int *parent = static_cast<int *>(ws), *count = parent + S4, *table = count + S4;
  const int nb = static_cast<int>(blocks_of(S, BLOCK));
  const int tiles_x = (X + TX - 1) / TX, tiles_y = (Y + TY - 1) / TY, tiles_z = (Z + TZ - 1) / TZ;
  const int64_t tiles = static_cast<int64_t>(tiles_x) * tiles_y * tiles_z;
  if (tiles > INT32_MAX) return fail("pl_instances: %lld tiles are too many", (long long)tiles);
  const Grid g{X, Y, Z};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nt = n_things > 0 ? n_things : 1;

  k_local<<<static_cast<unsigned>(tiles), BLOCK, 0, st>>>(sem, g, tab, tiles_y, tiles_z,
                                                          reinterpret_cast<uintptr_t>(sem) % 8 == 0, parent, count, record);
  SIDE_CHECK_LAUNCH("k_local");
  k_merge<<<nb, BLOCK, 0, st>>>(sem, g, tab, S, parent, record);
  SIDE_CHECK_LAUNCH("k_merge");
  k_flatten<<<nb, BLOCK, 0, st>>>(S, parent, count);
  SIDE_CHECK_LAUNCH("k_flatten");
  k_blockcnt<<<nb, BLOCK, 0, st>>>(sem, tab, S, nt, min_size, parent, count, table, record);
  SIDE_CHECK_LAUNCH("k_blockcnt");
  k_scan<<<1, SCAN_BLOCK, 0, st>>>(table, static_cast<int64_t>(nt) * nb, record);
  SIDE_CHECK_LAUNCH("k_scan");
  k_rank<<<nb, BLOCK, 0, st>>>(sem, tab, S, min_size, parent, count, table, sizes, sizes_cap);
  SIDE_CHECK_LAUNCH("k_rank");
  const bool vec = S % 4 == 0 && reinterpret_cast<uintptr_t>(sem) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(semantic_out) % 4 == 0 && reinterpret_cast<uintptr_t>(instance) % 16 == 0;
  if (vec) {
    k_write<4><<<static_cast<unsigned>(blocks_of(S / 4, BLOCK)), BLOCK, 0, st>>>(sem, tab, S, parent, count, instance, semantic_out);
  } else {
    k_write<1><<<nb, BLOCK, 0, st>>>(sem, tab, S, parent, count, instance, semantic_out);
  }
  SIDE_CHECK_LAUNCH("k_write");
  return 0;
}

}  // extern "C"

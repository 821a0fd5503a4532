// Visualisation (include/pasco_view.h): majority pooling, the 3 x 3 x 3 window filter, the colour-index grid of a view,
// brick occupancy bits, the ray caster and the box downsample.  pasco_amd/viz/host.py restates every kernel in numpy with
// the same operations in the same order; the tests hold the two equal on every byte.
//
// Layout choices:
//   k_pool      one thread per output cell; the 32-bin histogram of a thread lives in LDS (bin-major, so the lanes of a wave
//               hit different banks) because a runtime-indexed register array would go to scratch.
//   k_filter    one thread per voxel; the 27 values stay in registers (every index is a compile-time constant), the median
//               sorts them with an odd-even transposition network, invalid slots padded with +inf.
//   k_compose   the segment table (<= 128 entries) and the thing ranks are staged in LDS once per block; a voxel whose
//               panoptic id is 0 never searches it.
//   k_bricks    one block per output word (32 bricks), one wave per 8 of them, eight consecutive z per lane (32 bytes);
//               every word is written whole by one thread: no atomics, nothing to zero first.
//   k_render    16 x 16 pixels per block, one 8 x 8 tile per wave: neighbouring rays walk neighbouring voxels, so the
//               lanes of a wave read the same few cache lines and leave the loop after similar step counts.  The grid
//               (2 - 8 MB) and the brick bits (512 B) are read through the caches; a ray keeps its whole state in registers.
//
// Why every loop ends: each turn of the walk takes either a voxel step or a brick step and both counters carry a hard cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pasco_view.h"
#include "side_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int B = PV_BRICK;
constexpr int B_SHIFT = 3;
static_assert((1 << B_SHIFT) == B, "brick size");
constexpr float INF = __builtin_huge_valf();

struct Grid {
  int X, Y, Z;
};

bool bad_grid(int32_t X, int32_t Y, int32_t Z) {
  return X <= 0 || Y <= 0 || Z <= 0 || static_cast<int64_t>(X) * Y * Z >= (int64_t{1} << 31);
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + BLOCK - 1) / BLOCK); }

// ---- pv_majority_pool -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_pool(const uint8_t *__restrict__ grid, Grid g, int k, Grid o, int cells,
                                                uint8_t *__restrict__ out, int *__restrict__ status) {
  __shared__ uint16_t hist[PV_MAX_LABEL][BLOCK];
  const int tid = threadIdx.x;
  const int cell = blockIdx.x * BLOCK + tid;
  if (cell >= cells) return;          // no barrier below
  for (int l = 0; l < PV_MAX_LABEL; ++l) hist[l][tid] = 0;
  const int zz = cell % o.Z, yy = (cell / o.Z) % o.Y, xx = cell / (o.Z * o.Y);
  bool has0 = false, bad = false;
  for (int dx = 0; dx < k; ++dx)
    for (int dy = 0; dy < k; ++dy) {
      const uint8_t *row = grid + (static_cast<int64_t>(xx * k + dx) * g.Y + (yy * k + dy)) * g.Z + zz * k;
      for (int dz = 0; dz < k; ++dz) {
        const int v = row[dz];
        if (v == 0) has0 = true;
        else if (v < PV_MAX_LABEL) hist[v][tid] += 1;
        else if (v != 255) bad = true;
      }
    }
  int best = 0, best_n = 0;
  for (int l = 1; l < PV_MAX_LABEL; ++l) {
    const int n = hist[l][tid];
    if (n > best_n) {
      best_n = n;
      best = l;
    }
  }
  out[cell] = static_cast<uint8_t>(best_n > 0 ? best : (has0 ? 0 : 255));
  if (bad) atomicOr(status, PV_STATUS_LABEL_RANGE);
}

// ---- pv_window_filter -------------------------------------------------------------------------------------------
__device__ __forceinline__ void cswap(float &a, float &b) {
  const float lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

template <int OP>
__global__ __launch_bounds__(BLOCK) void k_filter(const float *__restrict__ in, const uint8_t *__restrict__ mask, Grid g,
                                                  int sites, float *__restrict__ out) {
  const int site = blockIdx.x * BLOCK + threadIdx.x;
  if (site >= sites) return;
  const int z = site % g.Z, y = (site / g.Z) % g.Y, x = site / (g.Z * g.Y);
  float v[27];
  int n = 0;
  float sum = 0.0f, mx = -INF;
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        const int slot = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1);
        const int xx = x + dx, yy = y + dy, zz = z + dz;
        bool ok = xx >= 0 && xx < g.X && yy >= 0 && yy < g.Y && zz >= 0 && zz < g.Z;
        float val = INF;
        if (ok) {
          const int s = (xx * g.Y + yy) * g.Z + zz;
          val = in[s];
          ok = val != PV_SENTINEL && (mask == nullptr || mask[s] != 0);
        }
        if (ok) {
          ++n;
          if (OP == PV_OP_AVG) sum = sum + val;
          if (OP == PV_OP_MAX) mx = val > mx ? val : mx;
        }
        v[slot] = ok ? val : INF;
      }
  float r;
  if (n == 0) {
    r = PV_SENTINEL;
  } else if (OP == PV_OP_AVG) {
    r = sum / static_cast<float>(n);
  } else if (OP == PV_OP_MAX) {
    r = mx;
  } else {
#pragma unroll
    for (int pass = 0; pass < 27; ++pass)
#pragma unroll
      for (int i = pass & 1; i + 1 < 27; i += 2) cswap(v[i], v[i + 1]);
    const int lo = (n - 1) >> 1, hi = n >> 1;
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int i = 0; i < 27; ++i) {
      a = i == lo ? v[i] : a;
      b = i == hi ? v[i] : b;
    }
    r = lo == hi ? a : (a + b) * 0.5f;
  }
  out[site] = r;
}

// ---- pv_compose -------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t quantise(float c, float vmin, float vmax) {
  if (!(vmax > vmin)) return 0;
  float t = (c - vmin) / (vmax - vmin);
  t = t > 0.0f ? t : 0.0f;
  t = t < 1.0f ? t : 1.0f;
  return static_cast<uint32_t>(static_cast<int>(t * 255.0f + 0.5f));
}

__global__ __launch_bounds__(BLOCK) void k_compose(const int32_t *__restrict__ pan, const int32_t *__restrict__ seg,
                                                   int n_seg, const uint8_t *__restrict__ sem,
                                                   const float *__restrict__ conf, int sites, int view, float vmin,
                                                   float vmax, uint32_t *__restrict__ out) {
  __shared__ int s_id[PV_MAX_SEGMENTS];
  __shared__ int s_thing[PV_MAX_SEGMENTS];
  __shared__ int s_rank[PV_MAX_SEGMENTS];
  __shared__ uint32_t s_q[PV_MAX_SEGMENTS];
  const int tid = threadIdx.x;
  const bool uses_seg = view == PV_VIEW_PANOPTIC || view == PV_VIEW_MASK || view == PV_VIEW_INS_CONF;
  if (uses_seg) {
    if (tid < n_seg) {
      s_id[tid] = seg[tid];
      s_thing[tid] = seg[n_seg + tid] != 0;
      s_q[tid] = quantise(__int_as_float(seg[3 * n_seg + tid]), vmin, vmax);
    }
    __syncthreads();
    if (tid < n_seg) {
      int r = 0;
      for (int s = 0; s <= tid; ++s) r += s_thing[s];
      s_rank[tid] = r;
    }
    __syncthreads();
  }
  const int site = blockIdx.x * BLOCK + tid;
  if (site >= sites) return;
  uint32_t r = 0;
  if (view == PV_VIEW_SEMANTIC) {
    const int c = sem[site];
    r = (c != 0 && c != 255) ? c : 0;
  } else if (view == PV_VIEW_VOX_CONF) {
    if (sem[site] != 0) r = PV_RAMP_BASE + quantise(conf[site], vmin, vmax);
  } else {
    const int id = pan[site];
    int s = -1;
    if (id != 0) {
      for (int i = 0; i < n_seg; ++i)
        if (s_id[i] == id) {
          s = i;
          break;
        }
    }
    const bool thing = s >= 0 && s_thing[s];
    if (thing) {
      r = view == PV_VIEW_INS_CONF ? PV_RAMP_BASE + s_q[s] : PV_INSTANCE_BASE + s_rank[s] - 1;
    } else if (view == PV_VIEW_PANOPTIC) {
      const int c = sem[site];
      r = (c >= PV_STUFF_FIRST && c <= PV_STUFF_LAST) ? c : 0;
    }
  }
  out[site] = r;
}

// ---- pv_bricks --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_bricks(const uint32_t *__restrict__ colour, Grid g, Grid nb, int n_bricks,
                                                  uint32_t *__restrict__ bits) {
  __shared__ uint32_t part[WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lx = lane >> 3, ly = lane & 7;
  uint32_t word = 0;
  for (int i = 0; i < 32 / WAVES; ++i) {
    const int bit = wave * (32 / WAVES) + i;
    const int b = blockIdx.x * 32 + bit;
    if (b >= n_bricks) break;                     // wave-uniform
    const int bz = b % nb.Z, by = (b / nb.Z) % nb.Y, bx = b / (nb.Z * nb.Y);
    const int x = bx * B + lx, y = by * B + ly, z0 = bz * B;
    bool any = false;
    if (x < g.X && y < g.Y) {
      const uint32_t *p = colour + (static_cast<int64_t>(x) * g.Y + y) * g.Z + z0;
#pragma unroll
      for (int k = 0; k < B; ++k)
        if (z0 + k < g.Z) any |= p[k] != 0;
    }
    if (__ballot(any) != 0) word |= 1u << bit;
  }
  if (lane == 0) part[wave] = word;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t w = 0;
    for (int i = 0; i < WAVES; ++i) w |= part[i];
    bits[blockIdx.x] = w;
  }
}

// ---- pv_render --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp_cell(float p, int lo, int hi) {
  const float flo = static_cast<float>(lo), fhi = static_cast<float>(hi);
  p = p > flo ? p : flo;          // a NaN becomes lo
  p = p < fhi ? p : fhi;
  return static_cast<int>(p);
}

__global__ __launch_bounds__(BLOCK) void k_render(const uint32_t *__restrict__ colour, const uint32_t *__restrict__ bits,
                                                  Grid g, Grid nbr, const float *__restrict__ cam, int W, int H,
                                                  const uint8_t *__restrict__ palette, int n_palette, int fx, int fy, int fz,
                                                  uint32_t background, int cap_fine, int cap_coarse,
                                                  int32_t *__restrict__ hit, uint8_t *__restrict__ face_out,
                                                  uint8_t *__restrict__ rgb, int *__restrict__ status) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int j = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (i >= W || j >= H) return;

  const int n[3] = {g.X, g.Y, g.Z}, nb[3] = {nbr.X, nbr.Y, nbr.Z};
  const float fi = static_cast<float>(i), fj = static_cast<float>(j);
  float o[3], d[3], inv[3];
  int st[3];
  bool miss = false;
  float t0 = 0.0f, t1 = INF;
  int ea = -1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = cam[a];
    d[a] = (cam[3 + a] + fi * cam[6 + a]) + fj * cam[9 + a];
    const float ext = static_cast<float>(n[a]);
    if (d[a] == 0.0f) {
      st[a] = 0;
      inv[a] = 0.0f;
      if (!(o[a] >= 0.0f && o[a] < ext)) miss = true;
    } else {
      st[a] = d[a] > 0.0f ? 1 : -1;
      inv[a] = 1.0f / d[a];
      const float ta = (0.0f - o[a]) * inv[a], tb = (ext - o[a]) * inv[a];
      const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
      if (tn > t0) {
        t0 = tn;
        ea = a;
      }
      if (tf < t1) t1 = tf;
    }
  }
  if (!(t0 <= t1)) miss = true;

  int c[3], bc[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = clamp_cell(o[a] + t0 * d[a], 0, n[a] - 1);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (a == ea) c[a] = st[a] > 0 ? 0 : n[a] - 1;
  int face = PV_FACE_INSIDE;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (a == ea) face = 2 * a + (st[a] < 0 ? 1 : 0);
    bc[a] = c[a] >> B_SHIFT;
  }

  int result = -1, st_bits = 0;
  uint32_t index = 0;
  int fine = 0, coarse = 0;
  bool fresh = true, occ = false;
  while (!miss) {
    if (fresh) {
      const int b = (bc[0] * nb[1] + bc[1]) * nb[2] + bc[2];
      occ = (bits[b >> 5] >> (b & 31)) & 1u;
      fresh = false;
    }
    float tm[3];
    int a = 0;
    if (occ) {
      const int site = (c[0] * n[1] + c[1]) * n[2] + c[2];
      const uint32_t v = colour[site];
      if (v != 0) {
        result = site;
        index = v;
        break;
      }
      if (fine >= cap_fine) {
        st_bits = PV_STATUS_STEP_CAP;
        break;
      }
      ++fine;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        tm[k] = st[k] == 0 ? INF : (static_cast<float>(c[k] + (st[k] > 0 ? 1 : 0)) - o[k]) * inv[k];
      if (tm[1] < tm[a]) a = 1;
      if (tm[2] < tm[a]) a = 2;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k == a) {
          c[k] += st[k];
          face = 2 * k + (st[k] < 0 ? 1 : 0);
          if (c[k] < 0 || c[k] >= n[k]) miss = true;
          if ((c[k] >> B_SHIFT) != bc[k]) {
            bc[k] = c[k] >> B_SHIFT;
            fresh = true;
          }
        }
    } else {
      if (coarse >= cap_coarse) {
        st_bits = PV_STATUS_STEP_CAP;
        break;
      }
      ++coarse;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        tm[k] = st[k] == 0 ? INF : (static_cast<float>((bc[k] + (st[k] > 0 ? 1 : 0)) * B) - o[k]) * inv[k];
      if (tm[1] < tm[a]) a = 1;
      if (tm[2] < tm[a]) a = 2;
      float t = tm[0];
      if (a == 1) t = tm[1];
      if (a == 2) t = tm[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k == a) {
          bc[k] += st[k];
          face = 2 * k + (st[k] < 0 ? 1 : 0);
          if (bc[k] < 0 || bc[k] >= nb[k]) miss = true;
          c[k] = st[k] > 0 ? bc[k] * B : bc[k] * B + (B - 1);
        } else {
          const int lo = bc[k] * B;
          const int hi = lo + B - 1 < n[k] - 1 ? lo + B - 1 : n[k] - 1;
          c[k] = clamp_cell(o[k] + t * d[k], lo, hi);
        }
      }
      fresh = true;
    }
  }

  const int px = j * W + i;
  uint32_t colr = background;
  if (result >= 0) {
    if (index >= static_cast<uint32_t>(n_palette)) {
      index = n_palette - 1;
      st_bits |= PV_STATUS_PALETTE;
    }
    const int f = face == PV_FACE_INSIDE ? fz : (face >> 1) == 0 ? fx : (face >> 1) == 1 ? fy : fz;
    const uint8_t *p = palette + 3 * index;
    colr = ((p[0] * f) >> 8) | (((p[1] * f) >> 8) << 8) | (((p[2] * f) >> 8) << 16);
  }
  hit[px] = result;
  face_out[px] = static_cast<uint8_t>(result >= 0 ? face : PV_FACE_NONE);
  rgb[3 * px + 0] = static_cast<uint8_t>(colr & 0xFF);
  rgb[3 * px + 1] = static_cast<uint8_t>((colr >> 8) & 0xFF);
  rgb[3 * px + 2] = static_cast<uint8_t>((colr >> 16) & 0xFF);
  if (st_bits) atomicOr(status, st_bits);
}

// ---- pv_downsample ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_downsample(const uint8_t *__restrict__ in, int W, int s, int n_out,
                                                      uint8_t *__restrict__ out) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n_out) return;
  const int ch = e % 3, i = (e / 3) % W, j = e / (3 * W);
  const int64_t row = static_cast<int64_t>(W) * s * 3;
  int sum = 0;
  for (int dj = 0; dj < s; ++dj)
    for (int di = 0; di < s; ++di) sum += in[(static_cast<int64_t>(j) * s + dj) * row + (i * s + di) * 3 + ch];
  out[e] = static_cast<uint8_t>((sum + s * s / 2) / (s * s));
}

inline hipStream_t S(void *stream) { return static_cast<hipStream_t>(stream); }

}  // namespace

extern "C" {

SIDE_EXPORTS(PV_FN, PV_ABI_VERSION)

int PV_FN(majority_pool)(const uint8_t *grid, int32_t X, int32_t Y, int32_t Z, int32_t k, uint8_t *out, int32_t *d_status,
                         void *stream) {
  if (bad_grid(X, Y, Z)) return fail("pv_majority_pool: grid %d x %d x %d is not supported", X, Y, Z);
  if (k != 2 && k != 4 && k != 8) return fail("pv_majority_pool: k = %d, must be 2, 4 or 8", k);
  if (!grid || !out || !d_status) return fail("pv_majority_pool: null pointer");
  const Grid o{X / k, Y / k, Z / k};
  const int cells = o.X * o.Y * o.Z;
  if (cells == 0) return 0;
  k_pool<<<blocks_for(cells), BLOCK, 0, S(stream)>>>(grid, Grid{X, Y, Z}, k, o, cells, out, d_status);
  SIDE_CHECK_LAUNCH("k_pool");
  return 0;
}

int PV_FN(window_filter)(const float *in, const uint8_t *mask, int32_t X, int32_t Y, int32_t Z, int32_t op, float *out,
                         void *stream) {
  if (bad_grid(X, Y, Z)) return fail("pv_window_filter: grid %d x %d x %d is not supported", X, Y, Z);
  if (!in || !out || in == out) return fail("pv_window_filter: null or aliased pointer");
  const Grid g{X, Y, Z};
  const int sites = X * Y * Z;
  const unsigned nblk = blocks_for(sites);
  if (op == PV_OP_MEDIAN) k_filter<PV_OP_MEDIAN><<<nblk, BLOCK, 0, S(stream)>>>(in, mask, g, sites, out);
  else if (op == PV_OP_MAX) k_filter<PV_OP_MAX><<<nblk, BLOCK, 0, S(stream)>>>(in, mask, g, sites, out);
  else if (op == PV_OP_AVG) k_filter<PV_OP_AVG><<<nblk, BLOCK, 0, S(stream)>>>(in, mask, g, sites, out);
  else return fail("pv_window_filter: op = %d", op);
  SIDE_CHECK_LAUNCH("k_filter");
  return 0;
}

int PV_FN(compose)(const int32_t *panoptic, const int32_t *seg, int32_t n_seg, const uint8_t *sem, const float *conf,
                   int32_t X, int32_t Y, int32_t Z, int32_t view, float vmin, float vmax, uint32_t *out, void *stream) {
  if (bad_grid(X, Y, Z)) return fail("pv_compose: grid %d x %d x %d is not supported", X, Y, Z);
  if (view < PV_VIEW_SEMANTIC || view > PV_VIEW_INS_CONF) return fail("pv_compose: view = %d", view);
  if (n_seg < 0 || n_seg > PV_MAX_SEGMENTS) return fail("pv_compose: %d segments, at most %d", n_seg, PV_MAX_SEGMENTS);
  const bool uses_seg = view == PV_VIEW_PANOPTIC || view == PV_VIEW_MASK || view == PV_VIEW_INS_CONF;
  const bool uses_sem = view == PV_VIEW_SEMANTIC || view == PV_VIEW_PANOPTIC || view == PV_VIEW_VOX_CONF;
  if (!out || (uses_seg && (!panoptic || (n_seg > 0 && !seg))) || (uses_sem && !sem) || (view == PV_VIEW_VOX_CONF && !conf))
    return fail("pv_compose: view %d misses an input", view);
  const int sites = X * Y * Z;
  k_compose<<<blocks_for(sites), BLOCK, 0, S(stream)>>>(panoptic, seg, n_seg, sem, conf, sites, view, vmin, vmax, out);
  SIDE_CHECK_LAUNCH("k_compose");
  return 0;
}

int64_t PV_FN(brick_words)(int32_t X, int32_t Y, int32_t Z) {
  if (bad_grid(X, Y, Z)) return -1;
  const int64_t n = static_cast<int64_t>((X + B - 1) / B) * ((Y + B - 1) / B) * ((Z + B - 1) / B);
  return (n + 31) / 32;
}

int PV_FN(bricks)(const uint32_t *colour, int32_t X, int32_t Y, int32_t Z, uint32_t *bits, void *stream) {
  if (bad_grid(X, Y, Z)) return fail("pv_bricks: grid %d x %d x %d is not supported", X, Y, Z);
  if (!colour || !bits) return fail("pv_bricks: null pointer");
  const Grid nb{(X + B - 1) / B, (Y + B - 1) / B, (Z + B - 1) / B};
  const int n_bricks = nb.X * nb.Y * nb.Z;
  k_bricks<<<static_cast<unsigned>((n_bricks + 31) / 32), BLOCK, 0, S(stream)>>>(colour, Grid{X, Y, Z}, nb, n_bricks, bits);
  SIDE_CHECK_LAUNCH("k_bricks");
  return 0;
}

int PV_FN(render)(const uint32_t *colour, const uint32_t *bits, int32_t X, int32_t Y, int32_t Z, const float *cam,
                  int32_t W, int32_t H, const uint8_t *palette, int32_t n_palette, int32_t fx, int32_t fy, int32_t fz,
                  uint32_t background, int32_t step_cap, int32_t *hit, uint8_t *face, uint8_t *rgb, int32_t *d_status,
                  void *stream) {
  if (bad_grid(X, Y, Z)) return fail("pv_render: grid %d x %d x %d is not supported", X, Y, Z);
  if (W <= 0 || H <= 0 || static_cast<int64_t>(W) * H >= (int64_t{1} << 29)) return fail("pv_render: image %d x %d", W, H);
  if (n_palette < 1) return fail("pv_render: empty palette");
  if (fx < 0 || fx > 256 || fy < 0 || fy > 256 || fz < 0 || fz > 256) return fail("pv_render: face factors must be 0 .. 256");
  if (step_cap < 0) return fail("pv_render: step_cap = %d", step_cap);
  if (!colour || !bits || !cam || !palette || !hit || !face || !rgb || !d_status) return fail("pv_render: null pointer");
  const Grid nb{(X + B - 1) / B, (Y + B - 1) / B, (Z + B - 1) / B};
  int cap_fine = X + Y + Z + 3, cap_coarse = nb.X + nb.Y + nb.Z + 3;
  if (step_cap > 0 && step_cap < cap_fine) cap_fine = step_cap;
  if (step_cap > 0 && step_cap < cap_coarse) cap_coarse = step_cap;
  const dim3 grid(static_cast<unsigned>((W + 15) / 16), static_cast<unsigned>((H + 15) / 16));
  k_render<<<grid, BLOCK, 0, S(stream)>>>(colour, bits, Grid{X, Y, Z}, nb, cam, W, H, palette, n_palette, fx, fy, fz,
                                          background, cap_fine, cap_coarse, hit, face, rgb, d_status);
  SIDE_CHECK_LAUNCH("k_render");
  return 0;
}

int PV_FN(downsample)(const uint8_t *in, int32_t W, int32_t H, int32_t s, uint8_t *out, void *stream) {
  if (W <= 0 || H <= 0 || s < 1 || s > 16 || static_cast<int64_t>(W) * H * s * s * 3 >= (int64_t{1} << 31))
    return fail("pv_downsample: image %d x %d, s = %d", W, H, s);
  if (!in || !out) return fail("pv_downsample: null pointer");
  const int n_out = W * H * 3;
  k_downsample<<<blocks_for(n_out), BLOCK, 0, S(stream)>>>(in, W, s, n_out, out);
  SIDE_CHECK_LAUNCH("k_downsample");
  return 0;
}

}  // extern "C"

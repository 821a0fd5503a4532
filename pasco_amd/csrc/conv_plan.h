// Which kernels a split-precision convolution (ph_conv_desc.mma_mode 1 / 2) runs on: the decision as a pure function.
//
// Plain C++17: no HIP, no pointer is dereferenced, the environment is read only through the ConvKnobs passed in.  The executor
// (ph_conv_fwd_f16x3, conv_f16x3.hip) validates the descriptor, builds the kernel argument block once, calls conv_plan() and runs
// the steps; tests/test_conv_plan_cpu.py holds this file to the decisions recorded in tests/golden/conv_plan.json.
//
// The order of the routes (the first that takes the launch wins):
//   0. tile width bn from cout (32 / 64 / 128), tile height bm and stage depth kc, then the split over the kernel offsets for
//      few-row maps on 128-wide tiles (cost model, else the 2048 / tiles rule);
//   1. dense-grid promise (grid_dims / grid_kernel)           -> k_conv_grid, its own split over the units of work;
//   2. row lists of one-pair-per-row maps                     -> k_conv_dma over the lists (recorded as kernel id 3);
//   3. 3x3x3 maps with window tables, no split chosen         -> the window kernel (k_conv_wop2 / k_conv_win) AND one of the gather
//      kernels below as its partner: a device-side predicate lets exactly one of the two do the work (recorded as id 5);
//   4. 128 / 256 output channels, >= 8 offsets                -> k_conv_wide (whole rounds; a 128-channel head may leave its
//      left-over rows to a k_conv_dma tail that is split over the offsets);
//   5. k = 1 on 128-wide tiles, 64 / 128 padded input channels -> k_conv_lin;
//   6. 128-wide tiles                                         -> k_conv_dma (a last partial round of row tiles goes to a tail
//      launch split over the offsets);
//   7. everything else, and mode 1                            -> k_conv_h2 / k_conv_f16x3.
// Every rule and threshold below is the measured one of the kernel it serves (see the kernel files); the quirks that look like
// oversights are marked "kept on purpose": changing one is a change of behaviour with its own measurements.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pasco_hip.h"

enum ConvKernel { CONV_K_F16X3 = 1, CONV_K_H2, CONV_K_DMA, CONV_K_WIN, CONV_K_WOP2, CONV_K_WIDE, CONV_K_LIN, CONV_K_GRID };

constexpr int CONV_DMA_KMAX = 32;         // kernel offsets in k_conv_dma's index table
constexpr int CONV_DMA_DENSE_KVOL = 100;  // above: the dense GEMMs keep the table's last slot for their stage list
constexpr int CONV_WIDE_KMAX = 27;        // kernel offsets in k_conv_wide's index table

// The inputs of the decision: what the dispatch branches on, nothing else.
struct ConvShape {
  int mma_mode = 2;
  int64_t n_in = 0, n_out = 0;
  int cin = 0, cout = 0, kvol = 1, route = 0;
  int64_t ws_bytes = 0;            // split scratch the caller offered (ph_conv_desc.splitk_ws_bytes; 0 = none)
  bool nbr = false, out = false, out_split = false, w_frag = false, axis = false, residual = false;
  bool win = false;                // all four window tables
  bool rl = false;                 // all three row lists
  int64_t rl_rows = 0;
  int grid_dims[4] = {0, 0, 0, 0}, grid_kernel[3] = {0, 0, 0};
  bool have_zero_line = true;      // ph_dma_zero_line() answered (the DMA / window kernels read it for absent neighbours)
};

// Every development switch of the dispatch.  The product build plans with the defaults; the development build (-DPH_DEV) fills
// one instance from the PASCO_* environment at the first launch and lets the extern "C" setters of tools/ write into it.
struct ConvKnobs {
  bool mid_on = true;              // PASCO_CONVH_MID=0: no 64-row / 64-channel-stage choice for thin 128-channel layers
  bool has_cfg = false;            // PASCO_CONVH_CFG=bm,kc: force tile height / stage depth (k_conv_h2 / k_conv_f16x3 only)
  int cfg_bm = 0, cfg_kc = 0;
  bool has_ksplit = false;         // PASCO_CONVH_KSPLIT=n: force the split over the kernel offsets
  int ksplit = 0;
  bool ksplit_model = true;        // PASCO_CONVH_KSPLIT_MODEL=0: the 2048 / tiles rule instead of the cost model
  bool dma_on = true;              // PASCO_CONV_DMA=0: every launch on the register-staged k_conv_h2
  bool dma_all = false;            // PASCO_CONV_DMA=2: every tile width on k_conv_dma
  bool dma_inter = true;           // PASCO_CONV_DMA_INTER=0: DMA instructions in front of the MFMAs, not between them
  bool tail_on = true;             // PASCO_CONV_TAIL=0: no tail split of k_conv_dma
  bool wide_on = true;             // PASCO_CONV_WIDE=0: no k_conv_wide
  bool win_on = true;              // PASCO_CONV_WIN=0: no window kernel
  bool win_wide = false;           // PASCO_CONV_WIN=2: windows on 128-wide tiles too
  bool wop2 = true;                // PASCO_WOP=0: the row-parallel window kernel for 64-wide outputs
  bool rl_on = true;               // PASCO_CONV_RL=0: ignore row lists
  int lin_on = 1;                  // PASCO_CONV_LIN / ph_conv_lin_set: bit 0 = k_conv_lin on, bits 8.. = workgroups per CU
  int grid_ks = 0;                 // PASCO_GRID_KS=n: slices of k_conv_grid by hand (0 = the model)
  bool grid_upw = true;            // PASCO_GRID_UPW=0: the same slices for every tile of k_conv_grid
  int dma_ablate = 0;              // ph_conv_dma_set_ablate, bits 0..7 (k_conv_dma, the window kernels)
  bool dma_tall = false;           // ph_conv_dma_set_ablate, bit 8: 256-row / 8-wave tiles of k_conv_dma
  int grid_ablate = 0;             // ph_conv_grid_set_ablate
};

struct ConvStep {
  int kernel = 0;                  // ConvKernel
  int bm = 128, bn = 128, kc = 32, waves = 4;      // the template choice, with:
  bool emit = false, inter = false;
  int ksplit = 1;
  bool use_ws = false;             // the partial sums go to the split scratch (and k_splitk_epilogue follows)
  int64_t row0 = 0, rows = 0;      // output rows [row0, row0 + rows) of the map (a row-list step: positions of the lists)
  bool rowlist = false;            // the launch walks the row lists instead of the map
  int grid_upw = 0;                // k_conv_grid: units of work per workgroup
  bool win_pair = false;           // one of a window / gather pair (the launch gets win_stats)
  int win_which = 0, win_gather = 0;
  int lin_wpc = 2;                 // k_conv_lin: workgroups per CU
  int ablate = 0;                  // development build: the kernel's ablation bits
  bool no_axis = false, no_residual = false;       // development build timing experiments (wrong results by design)
};

enum ConvPlanError { CONV_PLAN_OK = 0, CONV_PLAN_NO_ZERO_LINE };

struct ConvPlan {
  int nsteps = 0;
  ConvStep step[3];
  int cfg[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // what ph_record_cfg leaves behind: mode, bm, bn, kc, ksplit, emit, kernel id, waves
  int error = CONV_PLAN_OK;
};

// ---- the repeated pieces ------------------------------------------------------------------------------------------------------
static inline int64_t conv_tiles(int64_t rows, int bm, int64_t ncol = 1) { return (rows + bm - 1) / bm * ncol; }
static inline int conv_kper(int kvol, int ks) { return (kvol + ks - 1) / ks; }
// the kernels give every slice ceil(kvol / ks) offsets, so e.g. 27 offsets in 8 slices of 4 leave the eighth with nothing - its
// workgroups would only write (and the reduction read) zeros: the largest ks' <= ks whose slices all hold an offset
static inline int slices_without_empty(int kvol, int ks) {
  while (ks > 1 && conv_kper(kvol, conv_kper(kvol, ks)) != ks) --ks;
  return ks;
}
// ks partial copies of rows x cout fp32 sums fit the scratch the caller offered
static inline bool split_room(int64_t ks, int64_t rows, int cout, int64_t ws_bytes) {
  return ws_bytes > 0 && ks * rows * cout * 4 <= ws_bytes;
}
static inline int conv_dma_kper_max(int kvol) { return CONV_DMA_KMAX - (kvol > CONV_DMA_DENSE_KVOL ? 1 : 0); }

static inline void conv_plan_record(ConvPlan &p, int mode, int bm, int bn, int kc, int ksplit, int emit, int kid, int waves) {
  const int v[8] = {mode, bm, bn, kc, ksplit, emit, kid, waves};
  for (int q = 0; q < 8; ++q) p.cfg[q] = v[q];
}
static inline ConvStep &conv_plan_push(ConvPlan &p, const ConvStep &s) {
  p.step[p.nsteps] = s;
  return p.step[p.nsteps++];
}

// ---- k_conv_dma: one launch, or a head of whole rounds + a tail split over the offsets; false = declined ---------------------
// `s` carries the launch as the caller chose it (rows, ksplit, win / row-list fields)
static inline bool conv_plan_dma(ConvPlan &p, const ConvShape &sh, const ConvKnobs &kn, ConvStep s, int bn) {
  if (conv_kper(sh.kvol, s.ksplit) > conv_dma_kper_max(sh.kvol)) return false;   // kept on purpose: kvol > 100 loses one index slot
  if (!sh.have_zero_line) return false;
  s.kernel = CONV_K_DMA;
  s.kc = 32;
  s.ablate = kn.dma_ablate & 0x85;
  s.no_axis = (kn.dma_ablate & 0x10) != 0;
  s.no_residual = (kn.dma_ablate & 0x40) != 0;
  s.emit = sh.out_split && s.ksplit == 1;
  const int64_t ncol = conv_tiles(sh.cout, bn);
  // 256-row tiles (8 waves, one workgroup per CU) when they still cover every CU about twice - development build only
  const bool tall = bn >= 64 && conv_tiles(s.rows, 256, ncol) * s.ksplit >= 2 * 256 && kn.dma_tall;
  auto shape = [&](ConvStep &t, int waves, int bm) {
    t.waves = waves, t.bm = bm, t.bn = bn;
    t.inter = kn.dma_inter && waves == 4;
  };
  auto record = [&](const ConvStep &t) { conv_plan_record(p, 2, t.bm, t.bn, 32, t.ksplit, t.emit ? 1 : 0, 4, t.waves); };
  if (bn != 128 || tall) {
    shape(s, (bn != 32 && tall) ? 8 : 4, (bn != 32 && tall) ? 256 : 128);
    record(conv_plan_push(p, s));
    return true;
  }
  shape(s, 4, 128);
  // tail split: every tile of a launch does the same work, so a launch of T tiles runs in ceil(T / 512) rounds of resident
  // workgroups and a small last round leaves most of the chip idle for a whole tile time.  When fewer than half a round of row
  // tiles is left over, they go into a second launch that is split over the offsets; only those rows pay the reduction.
  const int64_t trow = conv_tiles(s.rows, 128);
  const int64_t slots = 512 / ncol;               // row tiles of one full round
  const int64_t rounds = trow / slots, rest = trow - rounds * slots;
  if (kn.tail_on && s.ksplit == 1 && !s.rowlist && sh.nbr && sh.kvol >= 8 && !s.win_gather && rounds >= 1 && rest > 0 &&
      2 * rest <= slots && sh.ws_bytes > 0) {
    int ks = (int)(slots / rest);
    if (ks > sh.kvol / 3) ks = sh.kvol / 3;
    if (ks > 16) ks = 16;                         // kept on purpose: this tail's cap is 16, the wide route's is 12
    ks = slices_without_empty(sh.kvol, ks);
    const int64_t r0 = (trow - rest) * 128, tail_rows = s.rows - r0;
    if (ks >= 2 && split_room(ks, tail_rows, sh.cout, sh.ws_bytes)) {
      ConvStep head = s, tail = s;
      head.rows = r0;
      tail.row0 = s.row0 + r0, tail.rows = tail_rows;
      tail.ksplit = ks, tail.use_ws = true, tail.emit = false;
      conv_plan_push(p, head);
      record(conv_plan_push(p, tail));            // the tail records last: the launch reads as "ksplit"
      return true;
    }
  }
  record(conv_plan_push(p, s));
  return true;
}

// ---- k_conv_wide; false = declined -------------------------------------------------------------------------------------------
static inline bool conv_plan_wide(ConvPlan &p, const ConvShape &sh, const ConvKnobs &kn, const ConvStep &in) {
  if ((sh.cout != 256 && sh.cout != 128) || sh.kvol < 8 || in.win_gather || !sh.nbr) return false;
  const int64_t trow = conv_tiles(sh.n_out, 256);
  if (sh.route & PH_ROUTE_WIDE_NEVER) return false;
  ConvStep s = in;
  s.kernel = CONV_K_WIDE;
  s.bm = 256, s.bn = sh.cout, s.kc = 32, s.waves = 8;
  s.ablate = 0;
  s.ksplit = 1, s.use_ws = false;
  auto record = [&](const ConvStep &t) { conv_plan_record(p, 2, 256, t.bn, 32, t.ksplit, t.emit ? 1 : 0, 6, 8); };
  if (!(sh.route & PH_ROUTE_WIDE_ALWAYS)) {
    if (sh.kvol > CONV_WIDE_KMAX) return false;
    if (sh.cout == 256 && trow < 48) return false;
    if (sh.cout == 128) {      // whole rounds only: the last round at least ~60 % full, no split over the offsets
      const int64_t rest = trow % 256;
      if (trow >= 256 && rest != 0 && rest < 150 && in.ksplit == 1 && sh.ws_bytes > 0) {
        // whole rounds + a few row tiles: the whole rounds here, the left-over rows on k_conv_dma, split over the offsets
        const int64_t r0 = (trow - rest) * 256, tail_rows = sh.n_out - r0;
        int ks = (int)(512 / conv_tiles(tail_rows, 128));
        if (ks > sh.kvol / 3) ks = sh.kvol / 3;
        if (ks > 12) ks = 12;                     // kept on purpose: this tail's cap is 12, k_conv_dma's own is 16
        ks = slices_without_empty(sh.kvol, ks);
        if (ks >= 2 && sh.have_zero_line && split_room(ks, tail_rows, sh.cout, sh.ws_bytes)) {
          ConvStep head = s, tail = in;
          head.rows = r0;
          head.emit = sh.out_split;
          conv_plan_push(p, head);
          // kept on purpose: the tail goes to k_conv_dma<4, 2, 2, 2, 2> through that route's own rules (its tail split is
          // off because a split is already chosen)
          tail.row0 = r0, tail.rows = tail_rows;
          tail.ksplit = ks, tail.use_ws = true;
          return conv_plan_dma(p, sh, kn, tail, 128);
        }
      }
      if (trow < 150 || (rest != 0 && rest < 150)) return false;
    }
  }
  if (!sh.have_zero_line) return false;
  int ks = conv_kper(sh.kvol, CONV_WIDE_KMAX);                       // what the index table demands
  if (trow * ks < 160) {                                             // well under one workgroup per CU: split further
    // kept on purpose: no slices_without_empty here - under PH_ROUTE_WIDE_ALWAYS 27 offsets can get 8 slices of 4 (the eighth empty)
    int want = (int)((256 + trow / 2) / trow);
    const int kmax = sh.kvol / 3 > 0 ? sh.kvol / 3 : 1;
    if (want > kmax) want = kmax;
    if (want > ks) ks = want;
  }
  if (ks > 1) {
    if (!split_room(ks, sh.n_out, sh.cout, sh.ws_bytes)) return false;
    s.ksplit = ks, s.use_ws = true;
  }
  s.emit = sh.out_split && s.ksplit == 1;
  record(conv_plan_push(p, s));
  return true;
}

// ---- k_conv_grid (the dense-grid promise); false = declined, the gather kernels read `nbr` -----------------------------------
// reachable (dx, dz) groups of an average tile: all dx, the dz that stay inside the grid
static inline double conv_grid_groups(const int *gd, const int *gk) {
  double zavg = 0.0;
  for (int z = 0; z < gd[3]; ++z)
    for (int iz = 0; iz < gk[2]; ++iz) zavg += (z + iz - gk[2] / 2 >= 0 && z + iz - gk[2] / 2 < gd[3]) ? 1.0 : 0.0;
  return gk[0] * zavg / gd[3];
}
static inline bool conv_plan_grid(ConvPlan &p, const ConvShape &sh, const ConvKnobs &kn, int cpad) {
  const int *gd = sh.grid_dims, *gk = sh.grid_kernel;
  // every dimension positive: the product of two negative ones would pass the `sites` test below
  if (gd[0] <= 0 || gd[1] <= 0 || gd[2] <= 0 || gd[3] <= 0) return false;
  if (sh.cout % 128 != 0 || sh.axis) return false;
  if (sh.route & PH_ROUTE_GRID_NEVER) return false;
  const int kx = gk[0], ky = gk[1], kz = gk[2];
  if (ky < 3 || ky > 7 || !(kx & 1) || !(ky & 1) || !(kz & 1) || kx * kz > 64 || kx * ky * kz != sh.kvol) return false;
  const int64_t sites = (int64_t)gd[0] * gd[1] * gd[2] * gd[3];
  if (sites != sh.n_out || sites != sh.n_in) return false;
  const int64_t tiles = conv_tiles(sh.n_out, 256, sh.cout / 128);
  const int nchunks = cpad >> 5;
  // the split over the units of work (group x 32-channel chunk) by a cost model: rounds of one workgroup per CU x the longest
  // slice + the reduction's round trip
  const double units = conv_grid_groups(gd, gk) * nchunks;
  const double stage_us = 1.0, fixed_us = 8.0;
  int best = 1;
  double best_us = 1e30;
  for (int ks = 1; ks <= 12; ++ks) {
    if (ks > 1 && !split_room(ks, sh.n_out, sh.cout, sh.ws_bytes)) break;
    if (ks > 1 && units / ks < 2.0) break;
    const double rounds = (double)((tiles * ks + 255) / 256);
    double us = rounds * (ceil(units / ks) * ky * stage_us + fixed_us);
    if (ks > 1) us += (double)ks * (double)sh.n_out * sh.cout * 4.0 / 3.0e6 + 5.0;
    if (us < best_us) best_us = us, best = ks;
  }
  if (kn.grid_ks >= 1 && (kn.grid_ks == 1 || split_room(kn.grid_ks, sh.n_out, sh.cout, sh.ws_bytes))) best = kn.grid_ks;
  int grid_upw = 0;
  if (best > 1 && tiles * best <= 256) {
    // ONE round of workgroups: the launch lasts as long as its longest workgroup, and the model's slices are for a tile with the
    // AVERAGE number of reachable groups - tiles in the grid's inner z planes reach a third more, a tile across two planes more
    // still.  Aim at the same units per workgroup everywhere, with as many slices in the launch as the fullest tile takes.
    // Launches of several rounds balance by themselves and lose to the extra slices.
    const int upw = (int)(units / best + 0.5) > 0 ? (int)(units / best + 0.5) : 1;
    int zmax = 0;
    for (int z = 0; z < gd[3]; ++z) {
      int c = 0;
      for (int iz = 0; iz < kz; ++iz) c += (z + iz - kz / 2 >= 0 && z + iz - kz / 2 < gd[3]) ? 1 : 0;
      zmax = c > zmax ? c : zmax;
    }
    const int zreach = zmax + 1 < kz ? zmax + 1 : kz;               // a tile across a plane boundary
    int ksmax = (kx * zreach * nchunks + upw / 2) / upw;
    ksmax = ksmax > 12 ? 12 : ksmax;
    while (ksmax > best && !split_room(ksmax, sh.n_out, sh.cout, sh.ws_bytes)) --ksmax;
    if (kn.grid_upw) {
      if (ksmax > best) best = ksmax;
      grid_upw = upw;
    }
  }
  ConvStep s;
  s.kernel = CONV_K_GRID;
  s.bm = 256, s.bn = 128, s.kc = 32, s.waves = 8;
  s.rows = sh.n_out;
  s.ksplit = best, s.use_ws = best > 1;
  s.grid_upw = grid_upw;
  s.emit = sh.out_split && best == 1;
  s.ablate = kn.grid_ablate;
  conv_plan_push(p, s);
  conv_plan_record(p, 2, 256, 128, 32, best, s.emit ? 1 : 0, 8, 8);
  return true;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
static inline ConvPlan conv_plan(const ConvShape &sh, const ConvKnobs &kn) {
  ConvPlan p;
  const bool pre = sh.mma_mode == 2;
  const int cpad = (sh.cin + 31) / 32 * 32;
  const int bn = sh.cout <= 32 ? 32 : (sh.cout <= 64 ? 64 : 128);
  const int64_t ncol = conv_tiles(sh.cout, bn);
  const int64_t t128 = conv_tiles(sh.n_out, 128, ncol);
  // tile height: the tallest tile that still gives >= 2 workgroups per CU
  int bm = 128;
  if (bn >= 64 && t128 < 2 * 256) bm = 64;
  if (bn == 128 && bm == 64 && conv_tiles(sh.n_out, 64, ncol) < 2 * 256) bm = 32;
  int kc = (sh.cin % 64 == 0 && sh.cin >= 256) ? 64 : 32;   // deeper stages pay only for wide layers
  // 128-channel layers with fewer than ~1.5 waves of 128-row tiles: 64-row tiles with 64-channel stages
  if (pre && kn.mid_on && bn == 128 && sh.cin == 128 && sh.kvol > 1 && t128 < 3 * 256) {
    if (bm == 128) bm = 64;
    kc = 64;
  }
  if (pre && cpad % 64 != 0) kc = 32;
  const bool env = kn.has_cfg;
  if (env) {
    const int em = kn.cfg_bm, ek = kn.cfg_kc;
    if (em == 128 || (em == 64 && bn >= 64) || (em == 32 && bn == 128)) bm = em;
    if (ek == 32 || (ek == 64 && (!pre || cpad % 64 == 0))) kc = ek;
  }
  // Few-row layers: every workgroup streams the whole W[k] slab sequence from L2, so small row tiles multiply the weight
  // traffic.  Keep the tall 128-row tile and get the parallelism from a split over the kernel offsets instead (partial sums
  // reduced in a fixed order by k_splitk_epilogue).  The caller provides the scratch, else no split.
  int ksplit = 1;
  {
    int want = (int)(2048 / (t128 > 0 ? t128 : 1));
    if (want > 8) want = 8;
    if (want > sh.kvol / 4) want = sh.kvol / 4;
    // the number of slices by a cost model instead (128-wide tiles; both operand modes, so that they keep choosing alike): the
    // launch runs in ceil(tiles x slices / 512) rounds of resident workgroups, a round lasts as long as its longest slice, and
    // every slice adds a partial-sum round trip
    if (kn.ksplit_model && bn == 128 && t128 < 2 * 256 && sh.kvol >= 8 && sh.ws_bytes > 0) {
      const double stage_us = 1.3, fixed_us = 5.0;           // one 32-channel stage of a workgroup sharing its CU; launch / prologue
      const double nchunks = (double)(cpad / 32);
      int best = 1;
      double best_us = 1e30;
      for (int ks = 1; ks <= 12 && ks <= sh.kvol / 3; ++ks) {
        const int kper = conv_kper(sh.kvol, ks);
        if (kper > conv_dma_kper_max(sh.kvol) || slices_without_empty(sh.kvol, ks) != ks) continue;   // beyond the index table / same as fewer slices
        if (ks > 1 && !split_room(ks, sh.n_out, sh.cout, sh.ws_bytes)) continue;
        const double rounds = (double)((t128 * ks + 511) / 512);
        double us = rounds * (kper * nchunks * stage_us + fixed_us);
        if (ks > 1) us += (double)ks * (double)sh.n_out * sh.cout * 4.0 / 3.0e6 + fixed_us;   // the reduction: 3 TB/s
        if (us < best_us) best_us = us, best = ks;
      }
      want = best;
    }
    if (kn.has_ksplit) want = kn.ksplit;
    const bool room = split_room(want, sh.n_out, sh.cout, sh.ws_bytes);
    if (bn == 128 && t128 < 2 * 256 && want >= 2 && room && !env) {
      bm = 128;
      ksplit = want;
    } else if (kn.has_ksplit && want >= 2 && room) {
      ksplit = want;
    }
  }
  ConvStep base;
  base.rows = sh.n_out;
  base.bn = bn;
  // 1. the dense-grid promise
  if (pre && !env && sh.grid_dims[0] > 0 && sh.nbr && conv_plan_grid(p, sh, kn, cpad)) return p;
  // 2. row lists: every 128-position tile of the list is the k = 1 product of one kernel offset
  if (pre && !env && sh.rl && sh.rl_rows > 0 && kn.rl_on && (bn == 64 || bn == 128)) {
    ConvStep s = base;
    s.rowlist = true;
    s.rows = sh.rl_rows;
    if (conv_plan_dma(p, sh, kn, s, bn)) {
      // kept on purpose: the row-list route is k_conv_dma and records kernel id 3
      conv_plan_record(p, 2, 128, bn, 32, 1, sh.out_split ? 1 : 0, 3, 4);
      return p;
    }
  }
  // 3. window / gather pair.  Only where no split over the offsets was chosen (its reduction kernel would run unconditionally);
  // 128-wide tiles lose to the gather kernel and stay there unless asked for
  ConvStep g = base;
  g.ksplit = ksplit, g.use_ws = ksplit > 1;
  if (pre && kn.win_on && !env && sh.kvol == 27 &&
      (bn == 64 || (bn == 128 && (kn.win_wide || (sh.route & PH_ROUTE_WIN_ALWAYS)))) && ksplit == 1 && sh.win) {
    if (!sh.have_zero_line) {
      p.error = CONV_PLAN_NO_ZERO_LINE;
      return p;
    }
    ConvStep w = base;
    w.win_pair = true;
    w.win_which = (bn == 64 ? 0 : 1) |
                  ((sh.route & PH_ROUTE_WIN_ALWAYS) ? 0x100 : ((sh.route & PH_ROUTE_WIN_NEVER) ? 0x200 : 0));
    w.win_gather = 0;
    w.emit = sh.out_split;
    w.ablate = kn.dma_ablate;
    w.kc = 32;
    // 64-wide outputs: offset-parallel waves on 16-channel chunks when the caller gave the fragment-order copy of the kernel
    w.kernel = (bn == 64 && kn.wop2 && sh.cout <= 64 && sh.w_frag) ? CONV_K_WOP2 : CONV_K_WIN;
    w.waves = (bn == 64) ? 4 : 8;
    conv_plan_push(p, w);
    g.win_pair = true;
    g.win_which = w.win_which;
    g.win_gather = 1;
    bm = 128;      // kept on purpose: pairs are only formed on big maps, the gather side keeps its 128-row tile
  }
  const bool pair = g.win_pair;
  auto finish = [&]() -> ConvPlan & {
    // kept on purpose: a pair records (2, 128, bn, 32, 1, emit, 5, 4) after both launches, whichever gather kernel ran
    if (pair) conv_plan_record(p, 2, 128, bn, 32, 1, sh.out_split ? 1 : 0, 5, 4);
    return p;
  };
  // 4. k_conv_wide
  if (pre && kn.wide_on && !env && bn == 128 && (sh.cout == 256 || sh.cout == 128) && sh.kvol >= 8 && sh.nbr &&
      conv_plan_wide(p, sh, kn, g))
    return finish();
  // 5. k = 1 row streams
  if (pre && kn.dma_on && !env && bn == 128 && sh.kvol == 1 && ksplit == 1 && (kn.lin_on & 1) && !(sh.route & PH_ROUTE_LIN_NEVER) &&
      (cpad == 64 || cpad == 128) && sh.n_out >= 1) {
    ConvStep s = g;
    s.kernel = CONV_K_LIN;
    s.bm = 32, s.bn = 128, s.kc = 32, s.waves = 4;
    s.emit = sh.out_split;
    s.lin_wpc = ((kn.lin_on >> 8) & 15) ? ((kn.lin_on >> 8) & 15) : 2;
    conv_plan_push(p, s);
    conv_plan_record(p, 2, 32, 128, 32, 1, s.emit ? 1 : 0, 7, 4);
    return finish();
  }
  // 6. k_conv_dma
  if (pre && kn.dma_on && !env && (bn == 128 || kn.dma_all)) {
    ConvStep s = g;
    if (bm != 128) {
      // kept on purpose: the choice above was made for a shorter tile, so the split is decided again for 128 rows by the
      // 1024 / tiles rule - which overrides the cost model's answer, a 1 included
      int want = (int)(1024 / (t128 > 0 ? t128 : 1));
      if (want > 8) want = 8;
      if (want > sh.kvol / 4) want = sh.kvol / 4;
      if (t128 < 256 && want >= 2 && split_room(want, sh.n_out, sh.cout, sh.ws_bytes)) s.ksplit = want, s.use_ws = true;
    }
    if (conv_plan_dma(p, sh, kn, s, bn)) return finish();
  }
  // 7. k_conv_h2 (mode 2) / k_conv_f16x3 (mode 1), with the split chosen at the top (not the redone one)
  g.kernel = pre ? CONV_K_H2 : CONV_K_F16X3;
  g.bm = bm, g.kc = kc, g.waves = 4;
  g.emit = pre && sh.out_split && ksplit == 1;
  conv_plan_push(p, g);
  conv_plan_record(p, pre ? 2 : 1, bm, bn, kc, ksplit, g.emit ? 1 : 0, pre ? 2 : 1, 4);
  return finish();
}

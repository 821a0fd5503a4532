"""The split-precision convolution dispatch as data: pasco_amd/csrc/conv_plan.h (plain C++17, no GPU) compiled into a ten-line
extern "C" shim and held to

  * tests/golden/conv_plan.json - what the library decided, launch by launch, BEFORE the planner existed
    (tests/golden/make_golden_convplan.py): every row must plan to exactly the recorded eight-integer config;
  * the consistency of every plan (golden rows and a sweep around each rule's thresholds): no empty slice of the kernel
    offsets, partial sums inside the scratch offered, a head and its tail covering the rows exactly once, slices inside the
    kernels' index tables, emit only without a split;
  * the decline of a dense-grid promise with a non-positive dimension;
  * a stand-alone program (own main) around the same shim, built with -fsanitize=address,undefined, over the golden rows.
"""
import ctypes as C
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pasco_amd", "csrc")
CXX = os.environ.get("CXX", "g++")

N_IN, N_STEP = 25, 14
K_F16X3, K_H2, K_DMA, K_WIN, K_WOP2, K_WIDE, K_LIN, K_GRID = range(1, 9)
STEP_FIELDS = ("kernel", "bm", "bn", "kc", "waves", "emit", "ksplit", "use_ws", "row0", "rows", "rowlist", "win_gather",
               "win_which", "grid_upw")
WS_BIG = 401872896

SHIM = r"""
#include "conv_plan.h"
extern "C" void conv_plan_shim(const int64_t *v, int64_t *o) {   // v: the golden inputs, flattened, + have_zero_line
  ConvShape s;
  s.mma_mode = (int)v[0], s.n_in = v[1], s.n_out = v[2], s.cin = (int)v[3], s.cout = (int)v[4], s.kvol = (int)v[5], s.route = (int)v[6];
  s.ws_bytes = v[7], s.nbr = v[8], s.out = v[9], s.out_split = v[10], s.w_frag = v[11], s.axis = v[12], s.residual = v[13];
  s.win = v[14], s.rl = v[15], s.rl_rows = v[16], s.have_zero_line = v[24];
  for (int q = 0; q < 4; ++q) s.grid_dims[q] = (int)v[17 + q];
  for (int q = 0; q < 3; ++q) s.grid_kernel[q] = (int)v[21 + q];
  const ConvPlan p = conv_plan(s, ConvKnobs{});                   // the product knobs
  o[0] = p.nsteps, o[1] = p.error;
  for (int q = 0; q < 8; ++q) o[2 + q] = p.cfg[q];
  for (int i = 0; i < p.nsteps; ++i) {
    const ConvStep &t = p.step[i];
    const int64_t f[14] = {t.kernel, t.bm, t.bn, t.kc, t.waves, t.emit, t.ksplit, t.use_ws, t.row0, t.rows, t.rowlist, t.win_gather,
                           t.win_which, t.grid_upw};
    for (int q = 0; q < 14; ++q) o[10 + 14 * i + q] = f[q];
  }
}
"""

MAIN = r"""
#include <stdint.h>
#include <stdio.h>
extern "C" void conv_plan_shim(const int64_t *v, int64_t *o);
int main(int argc, char **argv) {          // rows of 25 inputs + 8 expected config integers; exit 1 on a mismatch
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  long long x;
  int64_t v[33], o[10 + 3 * 14];
  int n = 0, rows = 0, bad = 0;
  while (fscanf(f, "%lld", &x) == 1) {
    v[n++] = x;
    if (n == 33) {
      conv_plan_shim(v, o);
      for (int q = 0; q < 8; ++q) bad += o[2 + q] != v[25 + q];
      n = 0, ++rows;
    }
  }
  fclose(f);
  printf("%d rows, %d mismatches\n", rows, bad);
  return bad != 0 || rows == 0 || argc != 2;
}
"""


def _flat(inputs, have_zero_line=1):
    *scalars, gd, gk = inputs
    return [int(x) for x in scalars] + list(gd) + list(gk) + [have_zero_line]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as f:
        g = json.load(f)
    assert g["inputs"][:8] == ["mma_mode", "n_in", "n_out", "cin", "cout", "kvol", "route", "ws_bytes"] and len(g["rows"]) > 200
    return g["rows"]


@pytest.fixture(scope="module")
def shim_src(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_plan")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    return d, src


@pytest.fixture(scope="module")
def plan(shim_src):
    d, src = shim_src
    lib = d / "libconvplan.so"
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(lib)], check=True)
    fn = C.CDLL(str(lib)).conv_plan_shim
    fn.argtypes, fn.restype = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)], None

    def run(inputs, have_zero_line=1):
        v = (C.c_int64 * N_IN)(*_flat(inputs, have_zero_line))
        o = (C.c_int64 * (10 + 3 * N_STEP))()
        fn(v, o)
        steps = [dict(zip(STEP_FIELDS, o[10 + N_STEP * i:10 + N_STEP * (i + 1)])) for i in range(o[0])]
        return dict(error=o[1], cfg=list(o[2:10]), steps=steps)
    return run


def _shape(mode=2, n=1000, cin=64, cout=128, kvol=27, route=0, ws=WS_BIG, nbr=1, out=1, out_split=0, w_frag=0, axis=0, residual=0,
           win=0, rl=0, rl_rows=0, gd=(0, 0, 0, 0), gk=(0, 0, 0), n_in=None):
    return [mode, n if n_in is None else n_in, n, cin, cout, kvol, route, ws, nbr, out, out_split, w_frag, axis, residual, win, rl,
            rl_rows, list(gd), list(gk)]


def _check_consistent(inputs, p):
    n_out, cout, kvol, ws = inputs[2], inputs[4], inputs[5], inputs[7]
    what = f"{inputs} -> {p}"
    assert p["error"] == 0 and 1 <= len(p["steps"]) <= 3, what
    cover = []
    for s in p["steps"]:
        ks = s["ksplit"]
        kper = -(-kvol // ks)
        if s["kernel"] != K_GRID:                         # k_conv_grid splits its units of work, not the offsets
            assert -(-kvol // kper) == ks, f"empty slice: {what}"
        if ks > 1:
            assert s["use_ws"] and ks * s["rows"] * cout * 4 <= ws, f"scratch: {what}"
        if s["kernel"] == K_DMA:
            assert kper <= (31 if kvol > 100 else 32), f"k_conv_dma index table: {what}"
        if s["kernel"] == K_WIDE:
            assert kper <= 27, f"k_conv_wide index table: {what}"
        if s["emit"]:
            assert ks == 1, f"emit with a split: {what}"
        if s["kernel"] in (K_WIN, K_WOP2):                # the window side of a pair walks the whole map
            assert (s["row0"], s["rows"], ks) == (0, n_out, 1), what
        elif s["rowlist"]:
            assert (s["row0"], s["rows"]) == (0, inputs[16]), what
        else:
            cover.append((s["row0"], s["rows"]))
    if cover:
        at = 0
        for r0, rows in sorted(cover):
            assert r0 == at and rows > 0, f"rows not covered exactly once: {what}"
            at += rows
        assert at == n_out, f"rows not covered exactly once: {what}"


def test_golden_rows_plan_to_the_recorded_config(golden, plan):
    for inputs, cfg in golden:
        assert plan(inputs)["cfg"] == cfg, f"{inputs}: planned {plan(inputs)}, recorded {cfg}"


def test_golden_plans_are_consistent(golden, plan):
    for inputs, _ in golden:
        _check_consistent(inputs, plan(inputs))


def _sweep_rows():
    rows = set()
    for t in (47, 48, 149, 150, 159, 160, 255, 256, 257, 511, 512, 513):
        for bm in (128, 256):
            rows.update(((t - 1) * bm + 1, t * bm))
    # rest-versus-slots edges of k_conv_dma's tail split (slots = 512 or 256 row tiles of 128 per round) ...
    for slots in (512, 256):
        for rounds in (1, 2):
            for rest in (1, 2, slots // 2 - 1, slots // 2, slots // 2 + 1, slots - 1):
                rows.add((rounds * slots + rest) * 128)
    # ... and of the 128-channel head-plus-tail plan of k_conv_wide (whole rounds of 256 row tiles of 256 + rest < 150)
    for rounds in (1, 2):
        for rest in (1, 2, 75, 149, 150, 151):
            rows.update(((rounds * 256 + rest) * 256, (rounds * 256 + rest) * 256 - 255))
    return sorted(rows)


def test_threshold_sweep_plans_are_consistent(plan):
    n = 0
    for kvol, cout, rows, cin, ws, emit in itertools.product((1, 8, 27, 75, 245), (32, 64, 128, 256), _sweep_rows(), (64, 128),
                                                             (0, 512 * 128 * 128 * 4, WS_BIG), (0, 1)):
        for mode in (2, 1):
            if mode == 1 and (emit or cin == 128):
                continue
            sh = _shape(mode=mode, n=rows, cin=cin, cout=cout, kvol=kvol, ws=ws, nbr=int(kvol > 1), out_split=emit)
            _check_consistent(sh, plan(sh))
            n += 1
    assert n > 10000


def test_nonpositive_grid_dims_are_declined(plan):
    ok = _shape(n=6688, cout=128, kvol=245, gd=(1, 38, 44, 4), gk=(7, 7, 5))
    assert plan(ok)["cfg"][6] == 8 and plan(ok)["steps"][0]["kernel"] == K_GRID
    for gd in ((1, -38, -44, 4), (1, 38, -44, -4), (1, -38, 44, -4), (1, 38, 0, 4), (0, 38, 44, 4), (-1, -38, 44, 4)):
        sites = gd[0] * gd[1] * gd[2] * gd[3]
        p = plan(_shape(n=6688, cout=128, kvol=245, gd=gd, gk=(7, 7, 5)))
        assert all(s["kernel"] != K_GRID for s in p["steps"]) and p["cfg"][6] != 8, (gd, sites, p)


def test_missing_zero_line_declines_the_dma_kernels(plan):
    """ph_dma_zero_line() answering null stays what it was: a decline (k_conv_h2 takes the launch), an error for a window pair."""
    p = plan(_shape(n=3001, cout=128, kvol=3), have_zero_line=0)
    assert [s["kernel"] for s in p["steps"]] == [K_H2]
    assert plan(_shape(n=100000, cout=64, kvol=27, win=1), have_zero_line=0)["error"] != 0


def test_planner_under_sanitizers(golden, shim_src, tmp_path):
    d, src = shim_src
    main = tmp_path / "main.cpp"
    main.write_text(MAIN)
    rows = tmp_path / "rows.txt"
    rows.write_text("\n".join(" ".join(str(x) for x in _flat(i) + c) for i, c in golden) + "\n")
    exe = tmp_path / "plan_asan"
    subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src),
                    str(main), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and "0 mismatches" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr

"""Generate tests/golden/conv_plan.json: which kernel the split-precision convolution dispatch (`ph_conv_fwd`, mma_mode 1 / 2)
chooses for which inputs - the pin that tests/test_conv_plan_cpu.py holds the host-only planner (pasco_amd/csrc/conv_plan.h) to.

Needs a GPU; run by hand (never collected by pytest).  `CBackend.conv_fwd` is wrapped the way tests/launch_checker.py wraps it;
every launch stores one row: the inputs of the decision, read from the very `ph_conv_desc` the call passed to the library (so the
bytes of split scratch are the ones the C side saw - the per-stream buffer only ever grows - and the presence flags are the
pointers it tested), and `conv_last_config()` read straight after the launch.  Rows are de-duplicated and sorted.

The launches: one step of each of the five benchmark configurations tests/test_hip_bench_shapes.py runs (after its warm-up step),
then the base shape of every entry in ROUTES of tests/test_hip_conv_routes.py (plain, with a per-axis table tail, emitting).
Mode-0 launches are not recorded: the exact fp32 kernel has no plan.  Data only - settings and recorded results.

    python tests/golden/make_golden_convplan.py [--out tests/golden/conv_plan.json]
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUTS = ("mma_mode", "n_in", "n_out", "cin", "cout", "kvol", "route", "ws_bytes", "nbr", "out", "out_split", "w_frag", "axis",
          "residual", "win", "rl", "rl_rows", "grid_dims", "grid_kernel")
CONFIG = ("mma_mode", "bm", "bn", "kc", "ksplit", "emit", "kernel", "waves")

BENCH_CONFIGS = [
    ("mimo3", dict(n_infers=3, in_channels=283, n_classes=20)),
    ("mimo1_semantickitti", dict(n_infers=1, in_channels=283, n_classes=20)),
    ("mimo3_sscbench_kitti360", dict(n_infers=3, in_channels=8, n_classes=19)),
    ("mimo8_one_gpu", dict(n_infers=8, in_channels=283, n_classes=20)),
    ("mimo3_heavy_decoder", dict(n_infers=3, in_channels=283, n_classes=20, heavy=True)),
]


class Recorder:
    """Wraps one CBackend's conv_fwd; one row per split-precision launch."""

    def __init__(self, hip):
        self.hip = hip
        self.inner = hip.conv_fwd
        self.rows = set()

    def install(self):
        self.hip.conv_fwd = self

    def remove(self):
        self.hip.conv_fwd = self.inner

    def __call__(self, x, weight, nbr, n_out, **kw):
        seen = []
        fn = self.hip.fn["conv_fwd"]

        def spy(desc_ref, stream):
            seen.append(desc_ref._obj)
            return fn(desc_ref, stream)

        self.hip.fn["conv_fwd"] = spy
        try:
            out = self.inner(x, weight, nbr, n_out, **kw)
        finally:
            self.hip.fn["conv_fwd"] = fn
        for d in seen:
            if d.mma_mode in (1, 2):
                cfg = self.hip.conv_last_config()
                self.rows.add((self.inputs(d), tuple(cfg[k] for k in CONFIG)))
        return out

    @staticmethod
    def inputs(d):
        win = bool(d.win_rows) and bool(d.win_cnt) and bool(d.win_slots) and bool(d.win_stats)
        rl = bool(d.rl_in) and bool(d.rl_out) and bool(d.rl_tile_k)
        return (int(d.mma_mode), int(d.n_in), int(d.n_out), int(d.cin), int(d.cout), int(d.kvol), int(d.route),
                int(d.splitk_ws_bytes) if d.splitk_ws else 0, int(bool(d.nbr)), int(bool(d.out)), int(bool(d.out_split)),
                int(bool(d.w_frag)), int(bool(d.axis_table)), int(bool(d.residual)), int(win), int(rl), int(d.rl_rows),
                tuple(int(v) for v in d.grid_dims), tuple(int(v) for v in d.grid_kernel))


def bench_steps(rec):
    import bench
    from pasco_amd.graph.synth import TeacherKeep, make_scene
    dev = torch.device("cuda", 0)
    for tag, kw in BENCH_CONFIGS:
        net = bench.build_net(kw["n_infers"], kw["in_channels"], dev, heavy=kw.get("heavy", False), n_classes=kw["n_classes"])
        scene = make_scene(seed=0, n_infers=kw["n_infers"], in_channels=kw["in_channels"]).to(dev)
        teacher = TeacherKeep(scene, dev)
        with torch.no_grad():
            bench.run_scene(net, scene, teacher)                  # warm-up: kernel maps, operand caches
            rec.install()
            try:
                bench.run_scene(net, scene, teacher)
            finally:
                rec.remove()
        print(f"[convplan] {tag}: {len(rec.rows)} distinct rows so far", flush=True)
        del net, scene, teacher
        torch.cuda.empty_cache()


def route_bases(rec, hip):
    from tests import test_hip_conv_routes as R
    from tests.conftest import load_oracle
    oracle = load_oracle()
    for c in R.CASES:
        if not c["full"]:
            continue
        key, mode, bits, kind = R.ROUTES[c["route"]]
        if mode == 0:
            continue
        p = R._problem(hip, oracle, c)
        v = R._vectors(c, p["g"], p["n_out"])
        split = hip.split_weight_rows(p["w"]) if mode == 2 else hip.split_weight_f16(p["w"])
        calls = [dict(bias=v["bias"])]
        if mode == 2:
            calls.append(dict(bias=v["bias"], axis=(v["tab"], v["acoords"], R.LO_AXIS), residual=v["res"]))
            if c["cout"] % 32 == 0:
                calls.append(dict(bias=v["bias"], emit_split=(None, None, 0)))
                calls.append(dict(bias=v["bias"], emit_split=(None, None, 0), want_out=False))
        rec.install()
        try:
            with hip.routing(bits):
                for kw in calls:
                    hip.conv_fwd(p["x"], p["w"], p["nbr"], p["n_out"], split=split, **kw, **p["extra"])
        finally:
            rec.remove()
        try:
            hip.check_status(p["x"].device)
        except Exception:                       # flags of the forced shapes are the route tests' business
            pass
    print(f"[convplan] routes: {len(rec.rows)} distinct rows", flush=True)


def main():
    out_path = os.path.join(HERE, "conv_plan.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    from pasco_amd.me.backend import hip_backend
    hip = hip_backend()
    rec = Recorder(hip)
    bench_steps(rec)
    route_bases(rec, hip)
    torch.cuda.synchronize()
    rows = sorted(rec.rows)
    with open(out_path, "w") as f:
        f.write('{"inputs": %s,\n "config": %s,\n "rows": [\n' % (json.dumps(list(INPUTS)), json.dumps(list(CONFIG))))
        f.write(",\n".join("  " + json.dumps([list(i), list(c)]) for i, c in rows))
        f.write("\n ]}\n")
    print(f"[convplan] wrote {len(rows)} rows to {out_path}")


if __name__ == "__main__":
    main()

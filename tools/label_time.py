"""Time the instance-label generator on the two full-size scenes of tests/test_hip_instances.py (seeded blobs, dense noise):

  (i)   pl_instances alone: device events around one call, warm-up, then N repeats (median / min / max);
  (ii)  a whole frame through `python -m pasco_amd.data.gen_instances` (file reads, pl_semantic_grid, pl_instances,
        the device-to-host copies and the pickle write): wall seconds per frame over a small tree written to a temporary
        directory;
  (iii) the numpy / scipy host restatement of the same call on this box (`data.instances.instance_labels_host`).

    python tools/label_time.py [--repeats 30] [--frames 6] [--out FILE.json]
    python tools/label_time.py --write-tree DIR [--frames 6]     # only write the blob scene as a dataset tree (to profile
                                                                 # a CLI run on it: rocprofv3 --kernel-trace --stats -- ...)

A missing GPU is an error: there is nothing to fall back to."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CONFIG = os.path.join(ROOT, "tests", "golden", "semantic-kitti.yaml")


def device_ms(sem, things, repeats, warmup=5):
    from pasco_amd.data.label_lib import label_lib
    lib = label_lib()
    ws = torch.empty(lib.workspace_bytes(sem.shape, len(things)), dtype=torch.uint8, device=sem.device)
    for _ in range(warmup):
        out = lib.instances(sem, things, 8, sizes_cap=4096, ws=ws)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = lib.instances(sem, things, 8, sizes_cap=4096, ws=ws)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms, out


def write_tree(root, grid, frames):
    """The scene as `frames` SemanticKITTI voxel file pairs (raw label = the first yaml key of each class)."""
    lm = yaml.safe_load(open(CONFIG))["learning_map"]
    inv = np.zeros(256, np.uint16)
    for k in sorted(lm, reverse=True):
        inv[lm[k]] = k
    inv[255] = 1          # "outlier": maps to 0 in the yaml, hence to 255 in the lookup table
    inv[0] = 0
    vox = os.path.join(root, "dataset", "sequences", "08", "voxels")
    os.makedirs(vox)
    raw = inv[grid]
    for f in range(frames):
        raw.tofile(os.path.join(vox, f"{5 * f:06d}.label"))
        np.zeros(grid.size // 8, np.uint8).tofile(os.path.join(vox, f"{5 * f:06d}.invalid"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--out", default="")
    ap.add_argument("--write-tree", default="")
    a = ap.parse_args()
    if a.write_tree:
        from test_hip_instances import blob_scene
        write_tree(a.write_tree, blob_scene(11), a.frames)
        return
    if not torch.cuda.is_available():
        raise SystemExit("label_time.py needs the GPU")
    from test_hip_instances import blob_scene, noise_scene
    from pasco_amd.data import gen_instances as G
    from pasco_amd.data.instances import instance_labels_host
    dev = torch.device("cuda", 0)
    things = list(range(1, 9))
    result = {"repeats": a.repeats, "cpus": len(os.sched_getaffinity(0)), "omp": os.environ.get("OMP_NUM_THREADS")}
    for name, grid in (("blobs", blob_scene(11)), ("noise", noise_scene(3))):
        host_s = []
        for _ in range(3):
            t0 = time.perf_counter()
            e_ins, e_sem, info = instance_labels_host(grid, things, 8)
            host_s.append(time.perf_counter() - t0)
        ms, (ins, sem, rec, _) = device_ms(torch.from_numpy(grid).to(dev), things, a.repeats)
        same = bool(torch.equal(ins.cpu(), torch.from_numpy(e_ins)) and torch.equal(sem.cpu(), torch.from_numpy(e_sem)))
        with tempfile.TemporaryDirectory() as tmp:
            write_tree(tmp, grid, a.frames + 1)
            args = ["--root", tmp, "--config", CONFIG, "--sequences", "08"]
            warm = G.parser().parse_args(args + ["--preprocess-root", os.path.join(tmp, "warm"), "--frame-interval", str(5 * (a.frames + 1))])
            G.generate(warm)                               # one frame: code objects, allocator
            r = G.generate(G.parser().parse_args(args + ["--preprocess-root", os.path.join(tmp, "pre")]))
            rh = G.generate(G.parser().parse_args(args + ["--preprocess-root", os.path.join(tmp, "pre_host"), "--device", "cpu"]))
        result[name] = {"instances": info["n_instances"], "dropped": info["n_dropped"], "device_equals_host": same,
                        "record": rec.cpu().tolist(),
                        "pl_instances_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)},
                        "cli_device_s_per_frame": r["seconds"] / r["frames"], "cli_frames": r["frames"],
                        "cli_host_s_per_frame": rh["seconds"] / rh["frames"],
                        "host_restatement_s": {"median": statistics.median(host_s), "min": min(host_s)}}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Raw scenes -> collated training batch through augment.Compose (csrc/augment.hip + device GridSample / SphereCrop), timed with device
events, from device-resident scenes and from host numpy arrays (the host -> device upload included).  Default: 2 x 1,000,000 raw float64
points through the S3DIS PT list; `--list scannet/openseg-pt-v1-0-pointpdf-v1m1-base --points 150000 --dtype float32 --normal` for
ScanNet.  Prints one JSON line.  `--stats kernel_stats.csv` (rocprofv3 --kernel-trace --stats of a run of this tool) adds per-kernel
times and GB/s from the byte formulas below (bytes per point or voxel and call; the point count per call is at most the raw count)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PASS_BYTES, BOUNDS_BYTES = 96, 48     # fused point pass: coord + colour fp64 rows read and written; bounds pass: both rows read
NORMAL_BYTES = 48                      # + the normal row of the point pass when the scenes carry normals
BYTES = {"k_aug_points": lambda a: PASS_BYTES + (NORMAL_BYTES if a.normal else 0), "k_aug_bounds_part": lambda a: BOUNDS_BYTES,
         "k_aug_keys": lambda a: 8, "k_elastic_apply": lambda a: 48, "k_grid_hash_f64": lambda a: 24 + 24 + 8}


def kernel_stats(path, a, calls_per_iter):
    """Per-kernel mean time and GB/s (bytes per point x raw points per call over the mean time) from rocprofv3's kernel_stats.csv."""
    import csv
    rows = {}
    for r in csv.DictReader(open(path)):
        for k, f in BYTES.items():
            if k in r["Name"]:
                mean_ns = float(r["AverageNs"])
                rows[k] = dict(calls=int(r["Calls"]), mean_us=mean_ns / 1e3, gbs=f(a) * a.points * a.scenes / mean_ns)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="s3dis/openseg-pt-v1-0-pointpdf-v1m1-base")
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="float64", choices=("float32", "float64"))
    ap.add_argument("--normal", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    from pointcloudpdf_amd import augment

    with open(os.path.join(ROOT, "tests", "golden", "pdf_train_transforms.json")) as f:
        cfgs = json.load(f)[a.list]
    rng = np.random.default_rng(0)
    dt = np.dtype(a.dtype)
    scenes = []
    for _ in range(a.scenes):
        s = dict(coord=np.round(rng.uniform(0, [10, 8, 3], (a.points, 3)), 3).astype(dt), color=np.floor(rng.uniform(0, 256, (a.points, 3))).astype(dt),
                 segment=rng.integers(0, 13, a.points))
        if a.normal:
            v = rng.normal(size=(a.points, 3))
            s["normal"] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dt)
        scenes.append(s)
    dev = torch.device("cuda", 0)
    dscenes = [{k: torch.from_numpy(v).to(dev) for k, v in s.items()} for s in scenes]
    pipe = augment.Compose(cfgs)
    res = {}
    for label, inp in (("device_input", dscenes), ("host_input", scenes)):
        times = []
        for it in range(a.warmup + a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            batch = pipe(inp, [1000 * it + s for s in range(a.scenes)], device=dev)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times.append(e0.elapsed_time(e1))
        res[f"ms_median_{label}"], res[f"ms_min_{label}"] = float(np.median(times)), float(np.min(times))
    line = dict(list=a.list, scenes=a.scenes, points=a.points, dtype=a.dtype, normal=a.normal, **res, out_points=int(batch["coord"].shape[0]),
                pass_bytes_per_point=PASS_BYTES + (NORMAL_BYTES if a.normal else 0), bounds_bytes_per_point=BOUNDS_BYTES)
    if a.stats:
        line["kernels"] = kernel_stats(a.stats, a, None)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

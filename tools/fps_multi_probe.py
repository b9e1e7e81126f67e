#!/usr/bin/env python3
"""GPU probe of the bucketed FPS kernels, per level of the headline config (100k-point scenes, 4 levels of n -> n / 4): time of the
automatic choice and of every kernel PDFOPS_FPS_KERNEL can force (single | multi | mw8 | mw16; read at every launch), identical
indices, samples per round from the work counters.

    python tools/fps_multi_probe.py [--scenes 2] [--reps 5] [--kernels auto,single,multi,mw8,mw16] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pointcloudpdf_amd import _native, synthetic

KERNELS = ("auto", "single", "multi", "mw8", "mw16")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="timed launches per kernel and level (after one warm-up launch); the median is reported")
    ap.add_argument("--kernels", default=",".join(KERNELS))
    ap.add_argument("--json", metavar="FILE", help="also write the per-level results there")
    args = ap.parse_args()
    kernels = args.kernels.split(",")
    assert set(kernels) <= set(KERNELS), kernels

    be = _native.hip_backend()
    batch = synthetic.make_batch([100000] * args.scenes, device="cuda")
    xyz, off = batch["coord"], batch["offset"]
    sizes = [100000] * args.scenes
    levels = []
    for lvl in range(4):
        msizes = [s // 4 for s in sizes]
        noff = torch.tensor(msizes, device="cuda").cumsum(0).int()
        ref, row, line = None, {}, []
        for k in kernels:
            os.environ.pop("PDFOPS_FPS_KERNEL", None)
            if k != "auto":
                os.environ["PDFOPS_FPS_KERNEL"] = k
            be.collect_fps_stats = True   # (forces a sync and a copy: only on the warm-up launch)
            idx = be.farthest_point_sampling(xyz, off, noff, max(sizes), sum(msizes))
            st = be.last_fps_stats.tolist()[0]
            be.collect_fps_stats = False
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                idx = be.farthest_point_sampling(xyz, off, noff, max(sizes), sum(msizes))
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            os.environ.pop("PDFOPS_FPS_KERNEL", None)
            if ref is None:
                ref = idx.clone()
            same = bool(torch.equal(ref, idx))
            # the fourth counter is the round count, except for k_fps (one sample per round; it stores the scene's bucket count there;
            # the automatic choice takes it only below 768 points, which no level of this config reaches)
            rounds = st[2] if k == "single" else st[3]
            row[k] = {"ms": ms, "median_ms": statistics.median(ms), "same_indices": same, "samples_per_round": st[2] / max(rounds, 1),
                      "bucket_updates_per_sample": st[0] / max(st[2], 1)}
            line.append(f"{k}: {row[k]['median_ms']:7.2f} ms same={same} samples/round {row[k]['samples_per_round']:.2f} "
                        f"bucket-updates/sample {row[k]['bucket_updates_per_sample']:.2f}")
        print(f"level {lvl + 1}: n={sizes[0]} -> m={msizes[0]} x{args.scenes} | " + " | ".join(line), flush=True)
        levels.append({"level": lvl + 1, "n": sizes[0], "m": msizes[0], "scenes": args.scenes, "kernels": row})
        xyz = xyz.index_select(0, ref.long()).contiguous()
        off = noff
        sizes = msizes
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"reps": args.reps, "levels": levels}, f, indent=1)
    if not all(r["same_indices"] for lv in levels for r in lv["kernels"].values()):
        sys.exit("indices differ between kernels")


if __name__ == "__main__":
    main()

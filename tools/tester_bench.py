#!/usr/bin/env python3
"""Times the precise tester on one ScanNet-shaped synthetic scene through three paths, in one process:

  (a) ``testing.fragment_inference``: one fragment per forward, geometry inline, fragments from ``voxelize.grid_sample(mode="test")``;
  (b) ``testing.SceneTester(group=0)``: batched fragments (one gather kernel per batch), geometry inline, batched vote;
  (c) ``testing.SceneTester`` with its defaults: the same with the geometry pre-pass one group of batches ahead on a side stream;
  (d) ``testing.SceneTester(group=--small-group)``: as (c) with small groups.  A scene with fewer batches than the default group is ONE
      group in (c) -- its whole geometry is computed in a single grouped pre-pass (every fragment's farthest-point chain side by side)
      BEFORE the first forward, nothing overlaps -- while (d) has several groups, so a group's forwards run while the next group's
      geometry is computed.  The JSON records the batch and group counts of both.

Each path is warmed once and then timed ``--reps`` times with synchronised wall time over the WHOLE scene (fragment table, fragments,
forwards, votes).  Writes one JSON document (``--out``) with ms per scene, fragments per second and the (a) / (c) ratio.

    python tools/tester_bench.py --out profiles/tester_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudpdf_amd import point_transformer, segmentor, synthetic, testing, voxelize  # noqa: E402,F401  (the first two register the models)
from pointcloudpdf_amd.registry import MODELS  # noqa: E402

GRID = 0.02
TEST_CFG = dict(   # the ScanNet test section of the reference's openseg configs, one augmentation
    transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
    test_mode=True,
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=GRID, hash_type="fnv", mode="test", keys=("coord", "color", "normal")),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "index"), feat_keys=("coord", "color", "normal"))],
        aug_transform=[[dict(type="RandomScale", scale=[1, 1])]]))


def make_scene(voxels, seed=0):
    """One point per voxel from ``synthetic.make_scene`` plus jittered copies: a geometric number per point (most voxels keep one or two
    points) and 16 for a few, so that count.max() >= 16 as in a raw ScanNet scan at the config's grid."""
    base = synthetic.make_scene(voxels, scene_id=seed, kind="scannet")
    rng = np.random.default_rng(seed)
    copies = np.minimum(rng.geometric(0.6, voxels) - 1, 6)
    copies[rng.choice(voxels, 64, replace=False)] = 17
    rep = np.repeat(np.arange(voxels), copies)
    idx = np.concatenate([np.arange(voxels), rep])
    coord = base["coord"][idx].copy()
    coord[voxels:] += rng.normal(0, 0.0005, (rep.shape[0], 3)).astype(np.float32)
    return dict(coord=coord, color=(base["color"][idx] * 255).astype(np.float32), normal=base["normal"][idx], segment=base["segment"][idx],
                name=f"synthetic{seed}")


def timed(fn, reps):
    fn()                                   # warm-up: allocator pools, side streams, first-use kernel loads
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=225000, help="one-point-per-voxel base points (about 150k occupied voxels after the copies)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--backbone", default="PointTransformer-Seg50")
    ap.add_argument("--fragments-per-batch", type=int, default=4)
    ap.add_argument("--small-group", type=int, default=2, help="batches per look-ahead pre-pass of path (d)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    scene = make_scene(args.voxels)
    seg = MODELS.build(dict(type="DefaultSegmentor", backbone=dict(type=args.backbone, in_channels=9, num_classes=20))).cuda().eval()
    synthetic.fill_parameters_deterministic(seg, seed=5)
    pipe = testing.TestPipeline(TEST_CFG)
    msp = lambda part, logits: -logits.log_softmax(-1).max(-1)[0]

    def forward(batch):
        logits = seg({k: batch[k] for k in ("coord", "feat", "offset", "offset_host", "pdf_geometry") if k in batch})["seg_logits"]
        return logits, msp(None, logits)

    st = pipe.prepare(scene, "cuda")
    table = testing._table(st["coord"].contiguous(), GRID)
    n, v, cmax = int(st["coord"].shape[0]), int(table["count"].shape[0]), int(table["cmax"])
    assert cmax >= 16, cmax

    def path_a():
        s = pipe.prepare(scene, "cuda")
        coord = s["coord"].contiguous()
        feat = torch.cat([coord, s["color"], s["normal"]], 1)
        frags = voxelize.grid_sample(coord, torch.tensor([n], dtype=torch.int32, device="cuda"), GRID, mode="test", offset_host=[n])["fragments"]
        return testing.fragment_inference(seg, msp, dict(coord=coord, feat=feat), frags, 20)

    serial = testing.SceneTester(forward, 20, pipe, fragments_per_batch=args.fragments_per_batch, group=0, device="cuda")
    ahead = testing.SceneTester(forward, 20, pipe, fragments_per_batch=args.fragments_per_batch, device="cuda")
    small = testing.SceneTester(forward, 20, pipe, fragments_per_batch=args.fragments_per_batch, group=args.small_group, device="cuda")
    batches = -(-cmax // args.fragments_per_batch)
    with torch.no_grad():
        times = dict(a_fragment_inference=timed(path_a, args.reps), b_scene_tester_group0=timed(lambda: serial.run(scene), args.reps),
                     c_scene_tester_default=timed(lambda: ahead.run(scene), args.reps),
                     d_scene_tester_small_group=timed(lambda: small.run(scene), args.reps))
        pa, pb, pc = path_a()[0], serial.run(scene)[0], ahead.run(scene)[0]
    res = dict(tool="tools/tester_bench.py", device=torch.cuda.get_device_name(0), backbone=args.backbone, points=n, voxels=v, fragments=cmax,
               grid_size=GRID, fragments_per_batch=args.fragments_per_batch, batches=batches, group=ahead.group,
               look_ahead_groups=dict(c_scene_tester_default=-(-batches // ahead.group), d_scene_tester_small_group=-(-batches // small.group)),
               small_group=small.group, reps=args.reps,
               timing="synchronised wall time over the whole scene (prepare, fragment table, fragments, forwards, votes); one warm-up run per path",
               ms_per_scene={k: dict(runs=[round(x, 2) for x in t], median=round(float(np.median(t)), 2)) for k, t in times.items()},
               fragments_per_second={k: round(cmax / (float(np.median(t)) * 1e-3), 1) for k, t in times.items()},
               ratio_a_over_c=round(float(np.median(times["a_fragment_inference"]) / np.median(times["c_scene_tester_default"])), 3),
               ratio_a_over_b=round(float(np.median(times["a_fragment_inference"]) / np.median(times["b_scene_tester_group0"])), 3),
               pred_b_equals_c=bool(torch.equal(pb, pc)), pred_c_equals_d=bool(torch.equal(pc, small.run(scene)[0])),
               pred_agreement_a_vs_c=round(float((pa == pc).float().mean()), 6),
               note="(a) gathers the scene's own coordinates; (b) / (c) shift every fragment (post_transform CenterShift) as the reference does, "
                    "so (a) and (c) see translated inputs: agreement is reported, not asserted")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

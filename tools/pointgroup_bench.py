#!/usr/bin/env python3
"""Device time of the PointGroup passes of csrc/point_group.hip.  Prints ONE JSON line and writes it to profiles/pointgroup_bench.json.

(a) The eval clustering stage -- ball table, clustering, proposals -- on one synthetic ScanNet-shaped scene: about 150,000 object points in 30
    instances, predicted centres collapsed to within a voxel (every row saturates at 1,000 entries), and the same scene with the centres
    NOT collapsed (blobs of 8 voxels standard deviation).  Per stage (the whole wrapper call: kernels, allocations and host reads): median time between two HIP events; rounds of the label propagation; table bytes.
    For scale, the module's own host path on the same table: device -> host copy + the NumPy restatement of bfs_cluster, at a REDUCED
    size (--host-points, default 15,000 points: the restatement walks ~10^3 entries per point in Python).  Information only.
(b) The bias-loss node, forward + backward at 2 x 100,000 rows with a float64 centroid, against the torch composition on the same tensors.
    Bound: not slower (ratio <= 1.0, as criteria_bench.py); exits non-zero otherwise.
(c) The training step and one eval forward of the ScanNet recipe's model (PG-v1m1 over SpUNet-v1m1) at 2 x 100,000 voxels / one scene.
    Information only (--recipe-rounds, default 10).

How the time is taken (as tools/criteria_bench.py): one process, two HIP events per sample, the variants of a pair alternate inside every
round, median over --rounds (30) after --warmup (5).

    python tools/pointgroup_bench.py --rounds 30
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(v):
    import numpy as np

    return round(float(np.median(np.asarray(v))), 2)


def timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1) * 1e3


def scene(points, instances, collapsed, seed, dev):
    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    per = points // instances
    centre = rng.uniform(0, 400, (instances, 3))
    owner = rng.permutation(np.repeat(np.arange(instances), per))
    spread = rng.uniform(-0.5, 0.5, (owner.shape[0], 3)) if collapsed else rng.normal(0, 8.0, (owner.shape[0], 3))
    xyz = torch.from_numpy((centre[owner] + spread).astype(np.float32)).to(dev)
    label = torch.from_numpy((2 + owner % 18).astype(np.int32)).to(dev)
    logits = torch.randn(owner.shape[0], 20, device=dev)
    logits[torch.arange(owner.shape[0], device=dev), label.long()] += 6
    return xyz, label, torch.softmax(logits, -1).contiguous()


def clustering_stage(be, points, collapsed, rounds, warmup, dev):
    import torch

    xyz, label, prob = scene(points, 30, collapsed, 3, dev)
    offset = torch.tensor([xyz.shape[0]], dtype=torch.int32, device=dev)
    t = {"table": [], "cluster": [], "proposals": []}
    for rnd in range(warmup + rounds):
        (idx, start_len), a = timed(lambda: be.pg_ball_table(xyz, offset, 1.5))
        (cidx, coff, stats), b = timed(lambda: be.pg_cluster(label, idx, start_len, 50, with_stats=True))
        res, c = timed(lambda: be.pg_proposals(cidx, coff, label, None, prob, 100))
        if rnd >= warmup:
            t["table"].append(a); t["cluster"].append(b); t["proposals"].append(c)
    torch.cuda.synchronize()
    return dict(stage_times_contain="the whole wrapper call between two HIP events: its kernels, its allocations and its host reads (table: grid "
                "build, count, scan, one read of the total, fill; cluster: all rounds with one read per batch, read-off, the stable sort, fill; "
                "proposals: select, one read of the counts, fill) -- a stage, not a single kernel",
                points=int(xyz.shape[0]), collapsed=collapsed, table_entries=int(idx.numel()), table_bytes=int(idx.numel()) * 4 + int(start_len.numel()) * 4,
                saturated_rows=int((start_len[:, 1] == 1000).sum()), rounds=int(stats["rounds"]), clusters=int(coff.numel()) - 1,
                proposals=int(res["classes"].numel()), us_table=med(t["table"]), us_cluster=med(t["cluster"]), us_proposals=med(t["proposals"]),
                us_stage=med([x + y + z for x, y, z in zip(t["table"], t["cluster"], t["proposals"])]))


def host_path(be, points, dev):
    import torch

    from pointcloudpdf_amd import pointgroup_ops

    xyz, label, _ = scene(points, 30, True, 3, dev)
    idx, start_len = be.pg_ball_table(xyz, torch.tensor([xyz.shape[0]], dtype=torch.int32, device=dev), 1.5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h_idx, h_sl, h_label = idx.cpu(), start_len.cpu(), label.cpu()
    t1 = time.perf_counter()
    out, off = pointgroup_ops.bfs_cluster(h_label, h_idx, h_sl, 50)
    t2 = time.perf_counter()
    _, dev_us = timed(lambda: be.pg_cluster(label, idx, start_len, 50))
    return dict(points=int(xyz.shape[0]), table_bytes=int(idx.numel()) * 4 + int(start_len.numel()) * 4, ms_copy_to_host=round((t1 - t0) * 1e3, 2),
                ms_host_restatement=round((t2 - t1) * 1e3, 2), clusters=int(off.numel()) - 1, us_device_clustering_same_table=round(dev_us, 2),
                note="the host restatement is NumPy, not the reference's C++: for scale only")


def bias_pair(rows, rounds, warmup, dev):
    import torch

    from pointcloudpdf_amd import point_group

    g = torch.Generator().manual_seed(1)
    pred = torch.randn(rows, 3, generator=g).to(dev)
    coord = (torch.rand(rows, 3, generator=g) * 6).to(dev)
    centroid = (coord.cpu() + torch.randn(rows, 3, generator=g) * 0.3).double().to(dev)
    instance = torch.randint(-1, 40, (rows,), generator=g).to(dev)
    kept = {}

    def run(name, fn):
        p = pred.detach().requires_grad_()
        l1, cos = fn(p, coord, centroid, instance, -1)
        (l1 + cos).backward()
        kept[name] = (float(l1), float(cos), p.grad)

    variants = {"fused": point_group.bias_losses, "composition": point_group.bias_losses_composition}
    times = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants.items():
            _, us = timed(lambda: run(name, fn))
            if rnd >= warmup:
                times[name].append(us)
    f, c = kept["fused"], kept["composition"]
    res = dict(rows=rows, us_fused=med(times["fused"]), us_composition=med(times["composition"]),
               l1_rel_diff=abs(f[0] - c[0]) / abs(c[0]), cosine_rel_diff=abs(f[1] - c[1]) / abs(c[1]),
               grad_max_diff_over_max=float((f[2] - c[2]).abs().max() / c[2].abs().max()))
    res["fused_over_composition"] = round(res["us_fused"] / res["us_composition"], 4)
    res["within_bound"] = bool(res["fused_over_composition"] <= 1.0)
    return res


def recipe(voxels, rounds, dev):
    import numpy as np
    import torch

    from pointcloudpdf_amd import data_path, engine

    model = dict(type="PG-v1m1", backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                                               layers=(2, 3, 4, 6, 2, 2, 2, 2)),
                 backbone_out_channels=96, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
                 instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50)
    rng = np.random.default_rng(2)

    def make(scenes):
        grids = []
        for _ in range(scenes):   # a surface-like scene: the cells of a 400 x 400 height field
            cells = rng.permutation(400 * 400)[:voxels]
            x, y = cells // 400, cells % 400
            grids.append(np.stack([x, y, (20 + 10 * np.sin(x / 30.0) * np.cos(y / 40.0)).astype(np.int64)], 1))
        grid = torch.from_numpy(np.concatenate(grids).astype(np.int32)).to(dev)
        coord = grid.float() * 0.02
        blob = (grid[:, 0] // 80) * 5 + grid[:, 1] // 80
        segment, offset = (blob % 20).long(), torch.tensor(np.cumsum([voxels] * scenes), dtype=torch.int32, device=dev)
        parsed = data_path.instance_parser(coord, segment, blob.long(), offset=offset)
        return dict(coord=coord, grid_coord=grid, feat=torch.randn(grid.shape[0], 6, device=dev), offset=offset, segment=segment,
                    instance=parsed["instance"], instance_centroid=parsed["instance_centroid"])

    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=model)).to(dev)
    train, one = make(2), make(1)

    def train_step():
        step.zero_grad(set_to_none=True)
        step(train)["loss"].backward()

    def eval_forward():
        with torch.no_grad():
            return step(one)

    out = {}
    for name, fn, mode in (("train_step_2x", train_step, True), ("eval_forward_1x", eval_forward, False)):
        step.train(mode)
        t = [timed(fn)[1] for _ in range(2 + rounds)][2:]
        out["ms_" + name] = round(med(t) / 1e3, 3)
    out.update(voxels_per_scene=voxels, rounds=rounds, note="untrained weights: the eval forward clusters whatever the random heads predict")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--host-points", type=int, default=15000)
    ap.add_argument("--rows", type=int, default=100000, help="rows per scene of the bias-loss measurement (two scenes)")
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--recipe-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointgroup_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from pointcloudpdf_amd import _native

    assert torch.cuda.is_available(), "pointgroup_bench.py measures on the GPU; there is no CPU fall-back"
    dev, be = "cuda", _native.hip_backend()
    res = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, warmup=args.warmup,
               clustering_collapsed=clustering_stage(be, args.points, True, args.rounds, args.warmup, dev),
               clustering_spread=clustering_stage(be, args.points, False, args.rounds, args.warmup, dev),
               host_path_reduced=host_path(be, args.host_points, dev),
               bias_loss=bias_pair(2 * args.rows, args.rounds, args.warmup, dev))
    if args.recipe_rounds > 0:
        res["recipe"] = recipe(args.voxels, args.recipe_rounds, dev)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    sys.exit(0 if res["bias_loss"]["within_bound"] else 1)


if __name__ == "__main__":
    main()

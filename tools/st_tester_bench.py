#!/usr/bin/env python3
"""Times the precise tester with the StratifiedTransformer (ST-v1m1, the S3DIS recipe's settings, MSP score) on one S3DIS-shaped
synthetic scene at the recipe's grid (0.04 m), through three paths of this build:

  (a) ``SceneTester(st_backbone=..., fragments_per_batch=1, group=0)``: one fragment per forward, geometry inline;
  (b) ``fragments_per_batch=4, group=0``: batched fragments (one window origin per fragment), geometry inline;
  (c) ``fragments_per_batch=4`` with the default look-ahead: the geometry of a group of batches from one grouped pre-pass on a side stream.

``--baseline-root DIR`` adds the figure of ANOTHER built checkout (the commit this one is compared with) on the same scene: one
fragment per forward through ``TestPipeline.batches`` + the model's own inline geometry + ``fragment_vote`` -- the only calls an ST
model can take there with the reference's partition (no geometry hand-over, no per-fragment origin), without the PT-v1 pre-pass
``SceneTester`` would add to it.

Every path runs in a fresh child process under its own ``timeout``; a child that fails ends the run (nothing more is started on the
device).  Per path: one warm-up, then ``--reps`` runs of synchronised wall time over the WHOLE scene (prepare, fragment table, fragments,
geometry, forwards, votes); median and spread (max - min) are recorded.  No kernel trace is taken: (c) measures one grouped pre-pass
followed by the forwards whenever the scene's batches fit one group.

    python tools/st_tester_bench.py --out profiles/st_tester_bench.json [--baseline-root ../parent-checkout]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = 0.04
MODES = {"a": dict(fragments_per_batch=1, group=0), "b": dict(fragments_per_batch=4, group=0), "c": dict(fragments_per_batch=4, group=None)}
TEST_CFG = dict(   # the S3DIS test section of the reference's openseg-st-v1m1 configs, one augmentation
    transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
    test_mode=True,
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=GRID, hash_type="fnv", mode="test", keys=("coord", "color"), return_grid_coord=True),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=("coord", "color"))],
        aug_transform=[[dict(type="RandomScale", scale=[1, 1])]]))


def make_scene(voxels, seed=0):
    """The points of ``synthetic.make_scene(kind="s3dis")`` plus jittered copies (a geometric number per point, seven for 64 of them): a
    raw room denser than the recipe's grid, so that GridSample(mode="test") gives a dozen or so fragments.  The JSON records the point,
    voxel and fragment counts the tester sees."""
    import numpy as np
    from pointcloudpdf_amd import synthetic

    base = synthetic.make_scene(voxels, scene_id=seed, kind="s3dis")
    rng = np.random.default_rng(seed)
    copies = np.minimum(rng.geometric(0.6, voxels) - 1, 4)
    copies[rng.choice(voxels, 64, replace=False)] = 7
    rep = np.repeat(np.arange(voxels), copies)
    idx = np.concatenate([np.arange(voxels), rep])
    coord = base["coord"][idx].copy()
    coord[voxels:] += rng.normal(0, 0.0005, (rep.shape[0], 3)).astype(np.float32)
    return dict(coord=coord, color=(base["color"][idx] * 255).astype(np.float32), segment=base["segment"][idx], name=f"synthetic{seed}")


def child(args):
    """One path in this process -> one JSON line."""
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from pointcloudpdf_amd import _native, engine, segmentor, stratified, synthetic, testing  # noqa: F401  (registers the models)
    from pointcloudpdf_amd.registry import MODELS

    torch.backends.cuda.matmul.allow_tf32 = False
    scene = make_scene(args.voxels)
    seg = MODELS.build(dict(type="DefaultSegmentor", backbone=dict(engine.ST_V1M1_BACKBONE, num_classes=13))).cuda().eval()
    synthetic.fill_parameters_deterministic(seg, seed=5)
    pipe = testing.TestPipeline(TEST_CFG)

    def forward(batch):
        logits = seg({k: batch[k] for k in ("coord", "feat", "offset", "offset_host", "st_geometry") if k in batch})["seg_logits"]
        return logits, -logits.log_softmax(-1).max(-1)[0]

    st = pipe.prepare(scene, "cuda")
    table = testing._table(st["coord"].contiguous(), GRID)
    n, v, cmax = int(st["coord"].shape[0]), int(table["count"].shape[0]), int(table["cmax"])
    if args.child == "baseline":
        def run():
            s = pipe.prepare(scene, "cuda")
            votes = torch.zeros(n, 13, device="cuda")
            ssum, scnt = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
            for batch in pipe.batches(s, 1):
                logits, score = forward(batch)
                fr = batch["fragment"]
                _native.backend_for(logits).fragment_vote(logits.float().contiguous(), score.float().contiguous(), fr["table"], fr["f0"], fr["g"],
                                                          votes, ssum, scnt)
            return votes.max(1)[1]
        info = dict(fragments_per_batch=1, group=0)
    else:
        opts = {k: w for k, w in MODES[args.child].items() if w is not None}
        tester = testing.SceneTester(forward, 13, pipe, device="cuda", st_backbone=seg.backbone, **opts)
        run = lambda: tester.run(scene)[0]
        info = dict(fragments_per_batch=tester.fragments_per_batch, group=tester.group)
    with torch.no_grad():
        pred = run()                           # warm-up: allocator pools, side streams, first-use kernel loads
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
    if args.child != "baseline":
        tester.close()
    batches = -(-cmax // info["fragments_per_batch"])
    print(json.dumps(dict(mode=args.child, device=torch.cuda.get_device_name(0), points=n, voxels=v, fragments=cmax, batches=batches,
                          look_ahead_groups=(-(-batches // info["group"]) if info["group"] else 0), **info,
                          runs_ms=[round(x, 2) for x in runs], median_ms=round(float(np.median(runs)), 2),
                          spread_ms=round(float(max(runs) - min(runs)), 2),
                          pred_checksum=int(pred.long().sum()), pred_hist=torch.bincount(pred, minlength=13).tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=100000, help="points of the synthetic room before the jittered copies")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--baseline-root", default=None, help="another built checkout to time the one-fragment-per-forward path of")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=sorted(MODES) + ["baseline"], help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res, order = {}, [(m, os.path.dirname(HERE)) for m in sorted(MODES)]
    if args.baseline_root:
        order.append(("baseline", os.path.abspath(args.baseline_root)))
    for mode, root in order:   # one fresh process per path, each under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root,
               "--voxels", str(args.voxels), "--reps", str(args.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(root))
        if p.returncode != 0:
            print(f"st_tester_bench: path {mode!r} ended with status {p.returncode}; nothing more is started", file=sys.stderr)
            sys.exit(p.returncode)
        res[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(res[mode]), flush=True)
    first = res["a"]
    key = {"a": "a_one_fragment_inline", "b": "b_batched_inline", "c": "c_batched_look_ahead", "baseline": "baseline_one_fragment_inline"}
    out = dict(tool="tools/st_tester_bench.py", device=first["device"], backbone="ST-v1m1 (S3DIS recipe), MSP score", grid_size=GRID,
               points=first["points"], voxels=first["voxels"], fragments=first["fragments"], reps=args.reps,
               timing="synchronised wall time over the whole scene (prepare, fragment table, fragments, geometry, forwards, votes); one warm-up "
                      "run per path; every path in a fresh process; spread = max - min of the runs; no kernel trace: (c) is one grouped "
                      "pre-pass followed by the forwards when the scene's batches fit one group",
               paths={key[m]: {k: r[k] for k in ("fragments_per_batch", "group", "batches", "look_ahead_groups", "runs_ms", "median_ms", "spread_ms")}
                      for m, r in res.items()},
               ratio_a_over_c=round(res["a"]["median_ms"] / res["c"]["median_ms"], 3),
               ratio_b_over_c=round(res["b"]["median_ms"] / res["c"]["median_ms"], 3),
               pred_b_equals_c=res["b"]["pred_hist"] == res["c"]["pred_hist"] and res["b"]["pred_checksum"] == res["c"]["pred_checksum"],
               pred_hist_a=res["a"]["pred_hist"], pred_hist_c=res["c"]["pred_hist"])
    if "baseline" in res:
        b, c = res["baseline"], res["c"]
        out.update(ratio_baseline_over_c=round(b["median_ms"] / c["median_ms"], 3),
                   c_faster_than_baseline_by_more_than_the_spreads=bool(b["median_ms"] - c["median_ms"] > b["spread_ms"] + c["spread_ms"]),
                   pred_hist_baseline=b["pred_hist"])
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

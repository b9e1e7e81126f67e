#!/usr/bin/env python3
"""Device time of the open-set metrics pass (evaluator.openset_metrics on device tensors: csrc/openset_metrics.hip, result read back once)
against the torch composition it replaces on the same device tensors (evaluator.intersection_and_union + evaluator.aupr_and_auroc with
their host reads), at three sizes: the tester bench's scene (374,732 rows), 1,000,000 rows and an all-points call of 20,000,000 rows;
13 classes, 8 % of the rows ignored, scores rounded to 1e-4 (ties).  Prints ONE JSON line and writes it to profiles/metrics_bench.json;
exits non-zero when the pass is slower than the composition at any size (bound: ratio <= 1.0) or the two disagree.

Timing: one process, HIP events around each call (both variants end with their result on the host), the variants alternating inside every
round, the median of the rounds after the warm-up ones.  `kernels`: the pass's per-kernel split of one call (its own k_om_* kernels and
the k_ts_* ones of csrc/tile_sort.h; torch profiler, 1,000,000 rows; information only).

`--tester`: additionally times `testing.OpenSegTester.test` on the synthetic scene of tools/tester_bench.py (Seg50, MSP scores; the whole
call, metrics included; synchronised wall time, one warm-up) in a child process of its own, and with `--baseline-tree PATH` (a checkout
of the parent commit with its library built) the same call of the parent's package before and after, plus the time the parent's host
metrics take on that scene's arrays.  Bound: this tree's tester is not slower than the parent's.

    python tools/metrics_bench.py --tester --baseline-tree ../parent
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (374732, 1000000, 20000000)
K, UNKNOWN, IGNORE = 13, (5, 9), -1


def summary(us):
    import numpy as np

    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def make_inputs(dev, rows, seed=0):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    target = torch.randint(0, K, (rows,), device=dev, generator=g)
    target[torch.rand(rows, device=dev, generator=g) < 0.08] = IGNORE
    pos = torch.isin(target, torch.tensor(UNKNOWN, device=dev))
    score = torch.round((torch.randn(rows, device=dev, generator=g) + 0.8 * pos) * 1e4) / 1e4
    pred = torch.where(torch.rand(rows, device=dev, generator=g) < 0.7, target.clamp(min=0), torch.randint(0, K, (rows,), device=dev, generator=g))
    return pred, score, target


def pass_times(dev, rows, rounds, warmup):
    import torch

    from pointcloudpdf_amd import evaluator

    pred, score, target = make_inputs(dev, rows)
    evaluator.unknown_mask(K, UNKNOWN, dev)
    kept = {}

    def fused():
        hist, rec = evaluator.openset_metrics(pred, score, target, K, UNKNOWN, IGNORE)
        kept["fused"] = torch.cat([hist.reshape(-1).double(), rec]).cpu()           # the one host read

    def composition():
        i, u, t = evaluator.intersection_and_union(pred, target, K, IGNORE)
        aupr, auroc = evaluator.aupr_and_auroc(score, target, UNKNOWN, IGNORE)       # (reads the host three times)
        kept["composition"] = torch.cat([torch.stack([i, u, t]).reshape(-1).double().cpu(), torch.tensor([aupr, auroc], dtype=torch.float64)])

    variants = {"fused": fused, "composition": composition}
    times = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for name, run in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    torch.cuda.synchronize()
    f, c = kept["fused"], kept["composition"]
    res = dict(rows=rows, rounds=rounds, warmup=warmup, hist_equal=bool(torch.equal(f[:3 * K], c[:3 * K])),
               aupr_diff=abs(float(f[3 * K] - c[3 * K])), auroc_diff=abs(float(f[3 * K + 1] - c[3 * K + 1])),
               **{k: summary(v) for k, v in times.items()})
    res["fused_over_composition"] = round(res["fused"]["us_median"] / res["composition"]["us_median"], 4)
    res["within_bound"] = bool(res["fused_over_composition"] <= 1.0 and res["hist_equal"] and res["aupr_diff"] <= 1e-9 and res["auroc_diff"] <= 1e-9)
    return res, fused


def kernel_split(run, calls=5):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            at = max(ev.key.find("k_om_"), ev.key.find("k_ts_"))   # the pass's own kernels and the shared sort's
            if at < 0:
                continue
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            name = ev.key[at:].split("(")[0].split("<")[0]
            per[name] = round(per.get(name, 0.0) + t / calls, 2)
        if not per:
            return "not measured"
        return dict(kernel_us_per_call=per, total_us=round(sum(per.values()), 2))
    except Exception as e:   # noqa: BLE001 -- information only
        return f"not measured ({type(e).__name__})"


def tester_child(tree, voxels, reps):
    """Runs in a child process: OpenSegTester.test of the package under `tree` on the synthetic scene; prints one JSON line."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tools"))
    import numpy as np
    import torch

    import tester_bench
    from pointcloudpdf_amd import evaluator, recognizer, synthetic, testing
    from pointcloudpdf_amd.registry import MODELS

    unknown = [4, 7, 14, 16]
    scene = tester_bench.make_scene(voxels)
    seg = MODELS.build(dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg50", in_channels=9, num_classes=20))).cuda().eval()
    synthetic.fill_parameters_deterministic(seg, seed=5)
    cfg = dict(data=dict(num_classes=20, ignore_index=-1, test=tester_bench.TEST_CFG), unknown_label=unknown, device="cuda", fragments_per_batch=4)
    tester = testing.OpenSegTester((seg, recognizer.MaxProbability("msp")), cfg)
    times, out = [], None
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tester.test([scene])
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    res = dict(points=int(scene["coord"].shape[0]), ms_per_call=[round(t, 2) for t in times],
               ms_median=round(float(np.median(times)), 2), mIoU=out["mIoU"], aupr=out["aupr"], auroc=out["auroc"], all_aupr=out["all_aupr"],
               all_auroc=out["all_auroc"])
    if hasattr(tester, "_histogram"):   # the parent's tester: what its host metrics take on this scene's arrays (per scene + all points)
        _, pred, score, segment = tester._scene(scene, None, need_score=True)
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            tester._histogram(pred, segment)
            for _ in range(2):
                evaluator.aupr_and_auroc(torch.from_numpy(score), torch.from_numpy(segment), unknown, -1)
            host.append((time.perf_counter() - t0) * 1e3)
        res["host_metrics_ms"] = round(float(np.median(host)), 2)
        res["host_metrics_share"] = round(res["host_metrics_ms"] / res["ms_median"], 4)
    print(json.dumps(res))


def run_child(tree, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--tester-child", os.path.abspath(tree), "--voxels", str(args.voxels), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    except subprocess.TimeoutExpired:
        return dict(returncode=124, error="the child did not finish within 420 s")
    if r.returncode != 0:
        return dict(returncode=r.returncode, error=(r.stderr or r.stdout)[-400:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--tester", action="store_true", help="also time OpenSegTester.test on the synthetic scene of tools/tester_bench.py")
    ap.add_argument("--baseline-tree", default=None, help="checkout of the parent commit, library built: its tester in the same run")
    ap.add_argument("--voxels", type=int, default=225000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tester-child", metavar="TREE", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    args = ap.parse_args()
    if args.tester_child:
        return tester_child(args.tester_child, args.voxels, args.reps)
    sys.path.insert(0, ROOT)
    import torch

    import pointcloudpdf_amd  # noqa: F401  (before the first device call: the package sets the runtime's capture switch at import)

    assert torch.cuda.is_available(), "metrics_bench.py measures on the GPU; there is no CPU fall-back"
    assert args.rounds >= 20, "at least 20 timed rounds per variant"
    dev = torch.device("cuda", 0)
    res = dict(workload="open-set metrics: class histograms + AUPR / AUROC of one call", device=torch.cuda.get_device_name(dev), classes=K,
               sizes=[])
    for rows in args.sizes:
        r, fused = pass_times(dev, rows, args.rounds, args.warmup)
        if rows == 1000000 or len(args.sizes) == 1:
            res["kernels"] = dict(rows=rows, **(lambda s: s if isinstance(s, dict) else dict(note=s))(kernel_split(fused)))
        res["sizes"].append(r)
        del fused
        torch.cuda.empty_cache()
    res["within_bound"] = all(r["within_bound"] for r in res["sizes"])
    failed_child = None
    if args.tester:
        # children one after the other (this process keeps its device context but queues nothing meanwhile)
        order = ([("parent", args.baseline_tree)] if args.baseline_tree else []) + [("this", ROOT)]
        if args.baseline_tree:
            order.append(("parent_again", args.baseline_tree))
        res["tester"] = dict(scene="tools/tester_bench.py make_scene", model="Seg50, 9 channels, 20 classes, MSP score", reps=args.reps)
        for k, tree in order:
            res["tester"][k] = run_child(tree, args)
            if "error" in res["tester"][k]:   # a child that failed, aborted, faulted or hung: nothing more is started on the device
                failed_child = k
                break
        if failed_child is None and args.baseline_tree:
            parent = min(res["tester"]["parent"]["ms_median"], res["tester"]["parent_again"]["ms_median"])
            res["tester"]["this_over_parent"] = round(res["tester"]["this"]["ms_median"] / parent, 4)
            res["tester"]["within_bound"] = bool(res["tester"]["this_over_parent"] <= 1.0)
            res["within_bound"] = res["within_bound"] and res["tester"]["within_bound"]
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if failed_child is not None:
        sys.exit(f"--tester: child `{failed_child}` ended with status {res['tester'][failed_child]['returncode']}; the remaining children "
                 "were not started")
    if not res["within_bound"]:
        sys.exit("outside the bound: " + json.dumps([(r["rows"], r["fused_over_composition"]) for r in res["sizes"]])
                 + (f", tester {res['tester'].get('this_over_parent')}" if "tester" in res else ""))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the adaptive-radius neighbour table (pdf_radius_neighbors_self_adaptive: the per-scene radius derived inside the grid
setup) against the fixed-radius entry (pdf_radius_neighbors_self) on a batch made of two copies of ONE 150,000-point ScanNet-shaped scene:
both scenes then share one adaptive radius, which the fixed entry gets as its scalar, so the two entries do the same work and differ by the
per-scene load of the radius.  Prints ONE JSON line and writes it to profiles/adaptive_radius_bench.json; exits non-zero when the
adaptive entry takes more than 1.10 x the reference (or than the measured spread allows), or the tables differ (`within_bound`).

How the time is taken: every sample is one call of the C entry (zero-fill, setup, histogram, scan, scatter, query: six launches on
preallocated buffers -- the same buffers for every variant) between two HIP events; the variants alternate inside every round; reported per
variant: median, min and the 10th / 90th percentile over the rounds after a warm-up, one process.

``--baseline-lib PATH``: a libpdfops.so built from another commit (its pdf_radius_neighbors_self is called through ctypes on the same
buffers, twice per round as `baseline_a` / `baseline_b`: the difference of their medians is the run-to-run spread of this measurement).
``--step``: adds the config-4-shaped training step (2 x 150k points, Seg50, 9 channels, 20 classes) with the adaptive pass built from the
config through engine.build_open_seg_step, replayed by engine.TrainStep behind the look-ahead pre-pass: wall ms per step, information only.

    python tools/adaptive_radius_bench.py --rounds 40 --step
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pointcloudpdf_amd import _native, engine, pseudo_label, synthetic  # noqa: E402

I, F, P, L = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_long
FIXED_ARGS = [I, I, F, P, P, I, P, P, P, L, P]


def summary(us):
    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def entry_times(dev, points, nsample, rounds, warmup, baseline_lib):
    scene = torch.from_numpy(synthetic.make_scene(points, scene_id=70, kind="scannet")["coord"]).float().to(dev)
    coord = torch.cat([scene, scene]).contiguous()
    offset = torch.tensor([points, 2 * points], dtype=torch.int32, device=dev)
    n, b = coord.shape[0], 2
    be = _native.hip_backend()
    r = pseudo_label.adaptive_radii(coord, offset)
    assert float(r[0]) == float(r[1])
    radius = float(r[0])
    nbytes = int(be.lib.pdf_knn_workspace_bytes(b, n, 0))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = {k: (torch.empty((n, nsample), dtype=torch.int32, device=dev), torch.empty((n, nsample), dtype=torch.float32, device=dev))
           for k in ("fixed", "adaptive", "baseline")}
    radii = torch.empty((b,), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(_native.raw_stream())
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def fixed_of(lib):
        fn = lib.pdf_radius_neighbors_self
        fn.restype, fn.argtypes = I, FIXED_ARGS

        def call(key):
            rc = fn(n, nsample, radius, ptr(coord), ptr(offset), b, ptr(out[key][0]), ptr(out[key][1]), ptr(ws), nbytes, stream)
            assert rc == 0, rc
        return call

    own = ctypes.CDLL(_native.LIB_PATH)
    adaptive_fn = own.pdf_radius_neighbors_self_adaptive
    adaptive_fn.restype, adaptive_fn.argtypes = I, [I, I, F, F, P, P, I, P, P, P, P, L, P]
    fixed = fixed_of(own)

    def adaptive():
        rc = adaptive_fn(n, nsample, 16.0, 1e-6, ptr(coord), ptr(offset), b, ptr(out["adaptive"][0]), ptr(out["adaptive"][1]), ptr(radii),
                         ptr(ws), nbytes, stream)
        assert rc == 0, rc

    variants = {"fixed": lambda: fixed("fixed"), "adaptive": adaptive}
    if baseline_lib:
        base = fixed_of(ctypes.CDLL(os.path.abspath(baseline_lib)))
        variants["baseline_a"] = lambda: base("baseline")
        variants["baseline_b"] = lambda: base("baseline")
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
    same = torch.equal(out["fixed"][0], out["adaptive"][0]) and torch.equal(out["fixed"][1], out["adaptive"][1]) and torch.equal(radii.cpu(), r.cpu())
    if baseline_lib:
        same = same and torch.equal(out["fixed"][0], out["baseline"][0]) and torch.equal(out["fixed"][1], out["baseline"][1])
    res = dict(points=[points, points], nsample=nsample, radius=radius, rounds=rounds, warmup=warmup, results_identical=bool(same),
               mean_neighbours=round(float((out["adaptive"][0] >= 0).float().sum(1).mean()), 2), **{k: summary(v) for k, v in times.items()})
    ref = "baseline_a" if baseline_lib else "fixed"
    res["reference"] = ref + (" (pdf_radius_neighbors_self of the baseline library)" if baseline_lib else " (pdf_radius_neighbors_self of this build)")
    res["adaptive_over_reference"] = round(res["adaptive"]["us_median"] / res[ref]["us_median"], 4)
    res["fixed_over_reference"] = round(res["fixed"]["us_median"] / res[ref]["us_median"], 4)
    if baseline_lib:
        res["baseline_spread"] = round(abs(res["baseline_a"]["us_median"] - res["baseline_b"]["us_median"]) / min(res["baseline_a"]["us_median"], res["baseline_b"]["us_median"]), 4)
    # the adaptive entry may take at most 1.10 x the reference (10 % stands for run-to-run spread), or the measured spread if that is larger
    res["bound"] = round(1.0 + max(0.10, res.get("baseline_spread", 0.0)), 4)
    res["within_bound"] = bool(res["results_identical"] and res["adaptive_over_reference"] <= res["bound"])
    return res


def train_step_ms(dev, points, adaptive, steps, warmup, group):
    """Mean wall ms per config-4-shaped training step (optim_bench.py's loop) with the pass the recognizer builds from its section."""
    ce = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg50", in_channels=9, num_classes=20), criteria=ce),
               recognizer=dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=ce, loss_weight=0.04,
                               step_loss_weight=False, num_classes=20, start_epoch=0, kp_ball_radius=0.02 * 5, kp_max_neighbor=64,
                               condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100, slide_window=True,
                               adaptive_radius=bool(adaptive)))
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    step = engine.build_open_seg_step(cfg).to(dev)
    synthetic.fill_parameters_deterministic(step, seed=1)
    step.train()
    opt = engine.FusedSGD(step.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    train = engine.TrainStep(step, opt, graph=True)
    batches = [synthetic.make_batch([points, points], first_scene_id=50 + 5 * i, kind="scannet", unknown=(4, 7, 14, 16)) for i in range(4)]
    loader = engine.GroupedGeometryLoader([batches[i % 4] for i in range(warmup + steps)], group=group, device=dev, **step.prepass_plan)
    t0, last = None, None
    for i, b in enumerate(loader):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        last = train(b)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    res = dict(ms_per_step=round(ms, 3), captured=train.captured is not None, one_graph=train.captured is not None and train.captured.graph2 is None,
               capture_error=train.capture_error, loss_last=float(last["loss"].detach()), recognizer_loss_last=float(last["recognizer_loss"]),
               prepass_plan={k: list(v) for k, v in step.prepass_plan.items()})
    engine.release_autograd_state(step)
    del train, opt, step, loader
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000, help="points of the scene (the batch holds it twice)")
    ap.add_argument("--nsample", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None, help="libpdfops.so of another commit: its fixed entry is the reference (measured twice: spread)")
    ap.add_argument("--step", action="store_true", help="also time the config-4-shaped training step with the fixed and the adaptive pass")
    ap.add_argument("--train-steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_radius_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "adaptive_radius_bench.py measures on the GPU; there is no CPU fall-back"
    assert args.rounds >= 20, "at least 20 timed launches per variant"
    dev = torch.device("cuda", 0)
    res = dict(workload="radius_neighbors_self", device=torch.cuda.get_device_name(dev),
               **entry_times(dev, args.points, args.nsample, args.rounds, args.warmup, args.baseline_lib))
    if args.step:
        gc.collect()
        torch.cuda.empty_cache()
        res["train_step"] = dict(points=[args.points, args.points], steps=args.train_steps, model="Seg50 + U-decoder, 9 channels, 20 classes",
                                 fixed_radius=train_step_ms(dev, args.points, False, args.train_steps, 4, 2),
                                 adaptive_radius=train_step_ms(dev, args.points, True, args.train_steps, 4, 2))
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not res["within_bound"]:
        sys.exit(f"adaptive entry {res['adaptive_over_reference']} x the reference (bound {res['bound']} x), identical results: {res['results_identical']}")


if __name__ == "__main__":
    main()

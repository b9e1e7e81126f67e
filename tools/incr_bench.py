#!/usr/bin/env python3
"""Incremental-stage step (engine.IncrSegStep: frozen Seg50 teacher + Seg50 student with a 13 + 2 class head, fused distillation loss)
at BASELINE config 2's shape: 2 x 100k points per step, geometry recomputed for every batch by the look-ahead pre-pass
(engine.GroupedGeometryLoader), FusedSGD over the student.  Prints ONE JSON line:

  * ms/step, fp32 and under fp16 autocast + DeviceGradScaler (--amp adds the second), captured (TrainStep replaying one hipGraph) and
    eager (the same step issued op by op);
  * the teacher forward's share of an eager fp32 step (HIP events around ``PointPdfIncrV1.get_teacher_output``).

    python tools/incr_bench.py --steps 10 --warmup 3 --amp
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pointcloudpdf_amd import data_path, engine, synthetic  # noqa: E402


def make_batches(count, sizes):
    out = []
    for i in range(count):
        b = synthetic.make_batch(sizes, first_scene_id=500 + 10 * i, unknown=())
        _, b["segment_incr"] = data_path.remap_label(b["segment"], {5: 13, 9: 14})
        out.append(b)
    return out


def build_step(dev):
    step = engine.IncrSegStep(backbone="PointTransformer-Seg50")
    synthetic.fill_parameters_deterministic(step.teacher, seed=1)
    synthetic.fill_parameters_deterministic(step.student, seed=2)
    return step.to(dev).train()


def run(batches, dev, steps, warmup, amp, graph, group):
    """Mean wall ms per step over ``steps`` steps after ``warmup`` (the first includes the capture)."""
    step = build_step(dev)
    opt = engine.FusedSGD(step.student.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    train = engine.TrainStep(step, opt, scaler=engine.DeviceGradScaler(dev) if amp else None, autocast=torch.float16 if amp else None,
                             graph=graph)
    stream = [batches[i % len(batches)] for i in range(warmup + steps)]
    loader = engine.GroupedGeometryLoader(stream, group=group, device=dev)
    losses, t0 = [], None
    for i, b in enumerate(loader):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        out = train(b)
        losses.append(out["loss"].detach().clone())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    res = dict(ms_per_step=round(ms, 3), captured=train.captured is not None, capture_error=train.capture_error,
               loss_first=float(losses[0]), loss_last=float(losses[-1]))
    del train, opt, step, loader
    gc.collect()
    torch.cuda.empty_cache()
    return res


def teacher_share(batches, dev, steps):
    """Eager fp32 steps with HIP events around the teacher's forward and around the whole step (forward + backward)."""
    from pointcloudpdf_amd.geometry import Geometry

    step = build_step(dev)
    learner = step.learner
    orig = learner.get_teacher_output
    marks = []

    def timed(input_dict):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = orig(input_dict)
        b.record()
        marks.append((a, b))
        return out

    learner.get_teacher_output = timed
    teacher_ms, step_ms = [], []
    try:
        for i in range(steps + 1):
            b = dict(batches[i % len(batches)])
            b = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
            b["pdf_geometry"] = Geometry(b["coord"], b["offset"], b["offset_host"]).precompute()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for p in step.student.parameters():
                p.grad = None
            step(b)["loss"].backward()
            e.record()
            torch.cuda.synchronize()
            if i > 0:   # (the first step warms caches and handles)
                teacher_ms.append(marks[-1][0].elapsed_time(marks[-1][1]))
                step_ms.append(s.elapsed_time(e))
    finally:
        learner.get_teacher_output = orig
    t, s = sum(teacher_ms) / len(teacher_ms), sum(step_ms) / len(step_ms)
    del step
    gc.collect()
    torch.cuda.empty_cache()
    return dict(teacher_forward_ms=round(t, 3), eager_step_device_ms=round(s, 3), teacher_share=round(t / s, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--amp", action="store_true", help="also measure under fp16 autocast + DeviceGradScaler")
    ap.add_argument("--group", type=int, default=2, help="look-ahead group of the geometry pre-pass")
    ap.add_argument("--points", type=int, default=100000, help="points per scene (two scenes per step)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    sizes = [args.points, args.points]
    batches = make_batches(4, sizes)
    res = dict(workload="incr_seg_step", backbone="PointTransformer-Seg50", points=sizes, head="13+2", steps=args.steps, warmup=args.warmup,
               group=args.group, device=torch.cuda.get_device_name(dev))
    modes = [("fp32", False)] + ([("amp_fp16", True)] if args.amp else [])
    for name, amp in modes:
        for graph in (True, False):
            res[f"{name}_{'captured' if graph else 'eager'}"] = run(batches, dev, args.steps, args.warmup, amp, graph, args.group)
    res["teacher"] = teacher_share(batches, dev, max(args.steps // 2, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of ONE optimizer step over the parameter set of engine.OpenSegStep (PointTransformer-Seg50 + PDF U-decoder) with
synthetic gradients: FusedAdamW (csrc/optim.hip: k_adam_tick + k_adam) against torch.optim.AdamW(fused=True), torch.optim.AdamW(
foreach=True) and FusedSGD.  Prints ONE JSON line and writes it to profiles/optim_bench.json.

How the time is taken: a step is tens of microseconds on the device and longer than that on the host, so the steps of one sample are
queued behind a blocker (a few large matrix products) and bracketed by two device events -- the host is ahead of the device for the
whole sample and the events see device time only.  Every variant works on ``--copies`` independent copies of the parameter set in
turn (4 x 137 MB for AdamW: more than the 256 MiB Infinity Cache), so each step reads its tensors from HBM as it does in training,
where a whole forward + backward passes between two optimizer steps.  The variants alternate inside every round; reported per
variant: median, min and the 10th / 90th percentile of the per-step time over the rounds, bytes per step from the algorithm
(28 B per value for Adam: read p, g, m, v, write p, m, v; 20 B for SGD), that over the median as GB/s and as a share of the 8 TB/s
HBM peak, and the kernel launches per step (torch profiler, in a pass of its own).

``--step`` adds the full 2-scene training step through engine.TrainStep (captured forward + backward, look-ahead pre-pass) with
FusedSGD and with FusedAdamW + OneCycleLR: wall ms per step, reported, not gated.

    python tools/optim_bench.py --rounds 40 --step
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pointcloudpdf_amd import engine, synthetic  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s (MI355X data sheet)


def parameter_shapes():
    step = engine.OpenSegStep()
    return [tuple(p.shape) for p in step.parameters() if p.requires_grad]


def make_copy(shapes, dev, gen):
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.1) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.01
    return ps


VARIANTS = {
    "fused_adamw": (lambda ps: engine.FusedAdamW(ps, lr=0.005, weight_decay=0.02), 28),
    "torch_adamw_fused": (lambda ps: torch.optim.AdamW(ps, lr=0.005, weight_decay=0.02, fused=True), 28),
    "torch_adamw_foreach": (lambda ps: torch.optim.AdamW(ps, lr=0.005, weight_decay=0.02, foreach=True), 28),
    "fused_sgd": (lambda ps: engine.FusedSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-4), 20),
}


def count_launches(opt):
    """Kernels of one step (torch profiler; None when the profiler is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:   # noqa: BLE001
        return None


def optimizer_times(dev, rounds, per_sample, copies, warmup):
    shapes = parameter_shapes()
    values = int(sum(int(np.prod(s)) for s in shapes))
    gen = torch.Generator(device=dev).manual_seed(0)
    opts = {name: [make(make_copy(shapes, dev, gen)) for _ in range(copies)] for name, (make, _) in VARIANTS.items()}
    block = torch.randn(8192, 8192, device=dev)

    host = {name: [] for name in opts}

    def sample(name):
        b0, a, b = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        b0.record()
        for _ in range(5):
            torch.mm(block, block)           # the blocker: the host queues the whole sample while these run
        a.record()
        t0 = time.perf_counter()
        for i in range(per_sample):
            opts[name][i % copies].step()
        host[name].append((time.perf_counter() - t0) * 1e3)
        b.record()
        return a, b, b0

    for _ in range(warmup):
        for name in opts:
            sample(name)
    torch.cuda.synchronize()
    marks = {name: [] for name in opts}
    for _ in range(rounds):
        for name in opts:                    # (the variants alternate inside every round)
            marks[name].append(sample(name))
        torch.cuda.synchronize()
    out = {}
    for name, (_, per_value) in VARIANTS.items():
        us = np.array([a.elapsed_time(b) for a, b, _ in marks[name]]) * 1e3 / per_sample
        blocker = float(np.median([b0.elapsed_time(a) for a, _, b0 in marks[name]]))
        queueing = float(np.median(host[name][-rounds:]))
        med, nbytes = float(np.median(us)), per_value * values
        out[name] = dict(us_median=round(med, 2), us_min=round(float(us.min()), 2), us_p10=round(float(np.percentile(us, 10)), 2),
                         us_p90=round(float(np.percentile(us, 90)), 2), bytes_per_step=nbytes, gb_per_s=round(nbytes / med / 1e3, 1),
                         share_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 3), launches_per_step=count_launches(opts[name][0]),
                         # the sample is device time only while the host queues it faster than the blocker runs
                         host_ms_per_sample=round(queueing, 2), blocker_ms=round(blocker, 2), host_ahead=queueing < blocker)
    return dict(tensors=len(shapes), values=values, rounds=rounds, steps_per_sample=per_sample, copies=copies, **out)


def train_step_ms(dev, kind, points, steps, warmup, group):
    """Mean wall ms per full training step (incr_bench.py's loop) with the given optimizer."""
    step = engine.OpenSegStep().to(dev)
    synthetic.fill_parameters_deterministic(step, seed=1)
    step.train()
    if kind == "fused_sgd":
        opt, sched = engine.FusedSGD(step.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4), None
    else:
        opt = engine.build_optimizer(dict(type="AdamW", lr=0.005, weight_decay=0.02), step)
        sched = engine.build_scheduler(dict(type="OneCycleLR", max_lr=0.005, pct_start=0.05, anneal_strategy="cos", div_factor=10.0,
                                            final_div_factor=1000.0), opt, warmup + steps)
    train = engine.TrainStep(step, opt, graph=True)
    batches = [synthetic.make_batch([points, points], first_scene_id=700 + 10 * i) for i in range(4)]
    loader = engine.GroupedGeometryLoader([batches[i % 4] for i in range(warmup + steps)], group=group, device=dev)
    t0, last = None, None
    for i, b in enumerate(loader):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        last = train(b)["loss"]
        if sched is not None:
            sched.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    res = dict(ms_per_step=round(ms, 3), captured=train.captured is not None, capture_error=train.capture_error, loss_last=float(last))
    del train, opt, step, loader
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--steps-per-sample", type=int, default=8)
    ap.add_argument("--copies", type=int, default=4, help="independent parameter sets each variant cycles through (working set above the Infinity Cache)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time the full 2-scene training step: FusedSGD vs FusedAdamW + OneCycleLR")
    ap.add_argument("--points", type=int, default=100000, help="--step: points per scene (two scenes per step)")
    ap.add_argument("--train-steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench.py measures on the GPU; there is no CPU fall-back"
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    res = dict(workload="optimizer_step", model="OpenSegStep(PointTransformer-Seg50) + PDF U-decoder", device=torch.cuda.get_device_name(dev),
               **optimizer_times(dev, args.rounds, args.steps_per_sample, args.copies, args.warmup))
    a, t, s = res["fused_adamw"], res["torch_adamw_fused"], res["fused_sgd"]
    res["fused_adamw_over_torch_fused"] = round(a["us_median"] / t["us_median"], 3)
    res["fused_adamw_over_fused_sgd"] = round(a["us_median"] / s["us_median"], 3)      # (expected near 28 / 20)
    if args.step:
        gc.collect()
        torch.cuda.empty_cache()
        res["train_step"] = dict(points=[args.points, args.points], steps=args.train_steps,
                                 **{k: train_step_ms(dev, k, args.points, args.train_steps, 4, 2) for k in ("fused_sgd", "fused_adamw_onecycle")})
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

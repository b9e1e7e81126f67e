#!/usr/bin/env python3
"""Device time of the Lovasz-softmax pass (losses.LovaszLoss on the device: csrc/lovasz.hip, forward + backward through autograd) against
the torch composition a user would otherwise run on the same device tensors (losses.lovasz_softmax_reference: boolean-mask row
selection, labels.unique(), one torch.sort + cumsum + dot per class, autograd backward).  Shape: 2 x 100,000 rows, 13 classes, 10 % of the
rows ignored (BASELINE config 2's head).  Prints ONE JSON line and writes it to profiles/lovasz_bench.json; exits non-zero when the fused
pass is slower than the composition (`within_bound`) or the two losses differ by more than 1e-4 relative.

How the time is taken: one process, every sample is forward + backward between two HIP events, the variants alternate inside every round;
reported per variant: median, min and the 10th / 90th percentile over the rounds after a warm-up.  `fused_abi` is the forward entry
alone (pdf_lovasz_forward on preallocated buffers).  `sort_share`: the share of the sort's kernels (csrc/tile_sort.h: k_ts_hist /
k_ts_scan_segments / k_ts_scatter) in the device time of the pass's kernels (k_lv_* and k_ts_*), from a torch.profiler trace of a few
extra calls (information only; "not measured" when the profiler reports no kernels).

``--step``: information only -- the captured config-2 training step (2 x 100k points, Seg50, 6 channels, 13 classes, the stand-in pseudo
mask) with CrossEntropyLoss + LovaszLoss in both criteria lists, and with CrossEntropyLoss alone, each in a child process of its own.
``--baseline-tree PATH``: a checkout of the parent commit with its library built: its CE-only step is timed the same way in the same run.
The children run one after the other; the first one that fails, aborts or runs out of time ends the sequence (what was collected is
written, the exit code is non-zero): nothing more is started on a device after a fault.

    python tools/lovasz_bench.py --rounds 30 --step --baseline-tree ../parent
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CE = dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)
LOVASZ = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)


def summary(us):
    import numpy as np

    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def pass_times(dev, rows, classes, ignored, rounds, warmup):
    import torch

    from pointcloudpdf_amd import _native, losses

    g = torch.Generator().manual_seed(0)
    logits = (2.0 * torch.randn(rows, classes, generator=g)).to(dev)
    labels = torch.randint(0, classes, (rows,), generator=g)
    labels[torch.randperm(rows, generator=g)[: int(round(ignored * rows))]] = -1
    labels = labels.to(dev)
    module = losses.LovaszLoss(mode="multiclass", ignore_index=-1)
    lib = _native.hip_backend().lib
    prob, dlog = torch.empty_like(logits), torch.empty_like(logits)
    out = torch.empty(2, device=dev)
    ws = torch.empty(int(lib.pdf_lovasz_workspace_bytes(rows, classes)), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(_native.raw_stream())
    kept = {}

    def fused():
        x = logits.detach().requires_grad_()
        loss = module(x, labels)
        loss.backward()
        kept["fused"] = (loss.detach(), x.grad)

    def composition():
        x = logits.detach().requires_grad_()
        loss = losses.lovasz_softmax_reference(x, labels, -1)
        loss.backward()
        kept["composition"] = (loss.detach(), x.grad)

    def fused_abi():
        rc = lib.pdf_lovasz_forward(rows, classes, logits.data_ptr(), labels.data_ptr(), -1, None, prob.data_ptr(), dlog.data_ptr(),
                                    out.data_ptr(), ws.data_ptr(), stream)
        assert rc == 0, rc

    variants = {"fused": fused, "composition": composition, "fused_abi": fused_abi}
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
    lf, lc = float(kept["fused"][0]), float(kept["composition"][0])
    gf, gc_ = kept["fused"][1], kept["composition"][1]
    res = dict(rows=rows, classes=classes, ignored_share=ignored, rounds=rounds, warmup=warmup, loss_fused=lf, loss_composition=lc,
               loss_rel_diff=abs(lf - lc) / abs(lc), grad_max_diff_over_max=float((gf - gc_).abs().max() / gc_.abs().max()),
               **{k: summary(v) for k, v in times.items()})
    res["fused_over_composition"] = round(res["fused"]["us_median"] / res["composition"]["us_median"], 4)
    res["sort_share"] = sort_share(fused_abi)
    # the bound: the fused pass is not slower than the composition it replaces
    res["within_bound"] = bool(res["fused_over_composition"] <= 1.0 and res["loss_rel_diff"] <= 1e-4)
    return res


def sort_share(run):
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(5):
                run()
            torch.cuda.synchronize()
        tot, sort, per = 0.0, 0.0, {}
        for ev in prof.key_averages():
            at = max(ev.key.find("k_lv_"), ev.key.find("k_ts_"))   # the pass's own kernels and the shared sort's
            if at < 0:
                continue
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            name = ev.key[at:].split("(")[0].split("<")[0]
            per[name] = round(per.get(name, 0.0) + t / 5, 2)
            tot += t
            if name in ("k_ts_hist", "k_ts_scan_segments", "k_ts_scatter"):
                sort += t
        if tot <= 0:
            return "not measured"
        return dict(share=round(sort / tot, 4), kernel_us_per_call=per)
    except Exception as e:   # noqa: BLE001 -- information only
        return f"not measured ({type(e).__name__})"


def step_child(tree, criteria, points, steps, warmup):
    """Runs in a child process: the captured config-2 step of the package under `tree`; prints one JSON line."""
    sys.path.insert(0, tree)
    import torch

    from pointcloudpdf_amd import engine, segmentor, synthetic

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    step = engine.OpenSegStep()
    crit = [CE, LOVASZ] if criteria == "ce+lovasz" else [CE]
    step.model.criteria = segmentor.build_criteria(crit)
    step.recognizer.criteria = segmentor.build_criteria(crit)
    step = step.to(dev)
    synthetic.fill_parameters_deterministic(step, seed=1)
    step.train()
    opt = engine.FusedSGD(step.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    train = engine.TrainStep(step, opt, graph=True)
    batches = [synthetic.make_batch([points, points], first_scene_id=50 + 5 * i) for i in range(3)]
    loader = engine.GroupedGeometryLoader([batches[i % 3] for i in range(warmup + steps)], group=2, device=dev, **step.prepass_plan)
    t0, last = None, None
    for i, b in enumerate(loader):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        last = train(b)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    print(json.dumps(dict(criteria=criteria, ms_per_step=round(ms, 3), captured=train.captured is not None,
                          one_graph=train.captured is not None and train.captured.graph2 is None, capture_error=train.capture_error,
                          loss_last=float(last["loss"].detach()), recognizer_loss_last=float(last["recognizer_loss"]))))


def run_child(tree, criteria, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", os.path.abspath(tree), criteria, "--points", str(args.points),
           "--train-steps", str(args.train_steps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    except subprocess.TimeoutExpired:
        return dict(criteria=criteria, returncode=124, error="the child did not finish within 420 s")
    if r.returncode != 0:
        return dict(criteria=criteria, returncode=r.returncode, error=(r.stderr or r.stdout)[-400:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000, help="rows per scene (the batch holds two scenes)")
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--ignored", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time the captured config-2 step with CE + Lovasz and with CE alone")
    ap.add_argument("--baseline-tree", default=None, help="checkout of the parent commit, library built: its CE-only step in the same run")
    ap.add_argument("--train-steps", type=int, default=16)
    ap.add_argument("--step-child", nargs=2, metavar=("TREE", "CRITERIA"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lovasz_bench.json"))
    args = ap.parse_args()
    if args.step_child:
        return step_child(args.step_child[0], args.step_child[1], args.points, args.train_steps, 6)
    sys.path.insert(0, ROOT)
    import torch

    assert torch.cuda.is_available(), "lovasz_bench.py measures on the GPU; there is no CPU fall-back"
    assert args.rounds >= 20, "at least 20 timed rounds per variant"
    dev = torch.device("cuda", 0)
    res = dict(workload="lovasz_softmax forward + backward", device=torch.cuda.get_device_name(dev),
               **pass_times(dev, 2 * args.points, args.classes, args.ignored, args.rounds, args.warmup))
    failed_child = None
    if args.step:
        # children one after the other (this process keeps its device context but queues nothing meanwhile)
        order = ([("parent_ce", args.baseline_tree, "ce")] if args.baseline_tree else []) + [("ce_lovasz", ROOT, "ce+lovasz"), ("ce", ROOT, "ce")]
        if args.baseline_tree:
            order.append(("parent_ce_again", args.baseline_tree, "ce"))
        res["train_step"] = dict(points=[args.points, args.points], steps=args.train_steps, model="Seg50 + U-decoder, 6 channels, 13 classes")
        for k, tree, crit in order:
            res["train_step"][k] = run_child(tree, crit, args)
            if "error" in res["train_step"][k]:   # a child that failed, aborted, faulted or hung: nothing more is started on the device
                failed_child = k
                break
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if failed_child is not None:
        sys.exit(f"--step: child `{failed_child}` ended with status {res['train_step'][failed_child]['returncode']}; the remaining "
                 "children were not started")
    if not res["within_bound"]:
        sys.exit(f"fused pass {res['fused_over_composition']} x the torch composition (bound 1.0 x), loss difference {res['loss_rel_diff']}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the criteria passes of csrc/criteria.hip (forward + backward through autograd) against the torch composition a user
would otherwise run on the same device tensors: nn.CrossEntropyLoss for the cross-entropy, losses.focal_loss_reference /
dice_loss_reference / binary_focal_loss_reference for the others.  Shape: 2 x 100,000 rows, 14 classes, 10 % of the rows ignored (the
recognizer's (C + 1)-way head of BASELINE config 2); the cross-entropy also at 200 classes.  Prints ONE JSON line and writes it to
profiles/criteria_bench.json; exits non-zero when a fused pass is slower than its composition (`within_bound`) or the two losses
differ by more than 1e-4 relative.

How the time is taken (as tools/lovasz_bench.py): one process, every sample is forward + backward between two HIP events, the two
variants of a pass alternate inside every round; reported per variant: median, min and the 10th / 90th percentile over the rounds after
a warm-up.

    python tools/criteria_bench.py --rounds 30
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(us):
    import numpy as np

    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def time_pair(fused, composition, x, target, rounds, warmup):
    import torch

    kept = {}

    def run(name, fn):
        a = x.detach().requires_grad_()
        loss = fn(a, target)
        loss.backward()
        kept[name] = (loss.detach(), a.grad)

    variants = {"fused": fused, "composition": composition}
    times = {k: [] for k in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, fn)
            e1.record()
            e1.synchronize()
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    torch.cuda.synchronize()
    lf, lc = float(kept["fused"][0]), float(kept["composition"][0])
    gf, gc_ = kept["fused"][1], kept["composition"][1]
    res = dict(loss_fused=lf, loss_composition=lc, loss_rel_diff=abs(lf - lc) / abs(lc),
               grad_max_diff_over_max=float((gf - gc_).abs().max() / gc_.abs().max()), **{k: summary(v) for k, v in times.items()})
    res["fused_over_composition"] = round(res["fused"]["us_median"] / res["composition"]["us_median"], 4)
    # the bound: the fused pass is not slower than the composition it replaces
    res["within_bound"] = bool(res["fused_over_composition"] <= 1.0 and res["loss_rel_diff"] <= 1e-4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000, help="rows per scene (the batch holds two scenes)")
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--wide-classes", type=int, default=200, help="class count of the second cross-entropy measurement")
    ap.add_argument("--ignored", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criteria_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    from pointcloudpdf_amd import losses, segmentor

    assert torch.cuda.is_available(), "criteria_bench.py measures on the GPU; there is no CPU fall-back"
    assert args.rounds >= 20, "at least 20 timed rounds per variant"
    dev = torch.device("cuda", 0)
    rows = 2 * args.points

    def rows_of(c, seed):
        g = torch.Generator().manual_seed(seed)
        x = 2.0 * torch.randn(rows, c, generator=g)
        t = torch.randint(0, c, (rows,), generator=g)
        t[torch.randperm(rows, generator=g)[: int(round(args.ignored * rows))]] = -1
        return x.to(dev), t.to(dev)

    def weights(c):
        return [0.5 + k / c for k in range(c)]

    res = dict(workload="criteria forward + backward", device=torch.cuda.get_device_name(dev), rows=rows, classes=args.classes,
               wide_classes=args.wide_classes, ignored_share=args.ignored, rounds=args.rounds, warmup=args.warmup, passes={})
    x, t = rows_of(args.classes, 0)
    for name, c, (xx, tt) in (("cross_entropy_weight_smoothing", args.classes, (x, t)),
                              ("cross_entropy_weight_smoothing_wide", args.wide_classes, rows_of(args.wide_classes, 1))):
        w = weights(c)
        torch_ce = torch.nn.CrossEntropyLoss(weight=torch.tensor(w, device=dev), ignore_index=-1, label_smoothing=0.1)
        res["passes"][name] = time_pair(segmentor.CrossEntropyLoss(weight=w, label_smoothing=0.1), torch_ce, xx, tt, args.rounds, args.warmup)
    res["passes"]["focal"] = time_pair(losses.FocalLoss(), lambda a, b: losses.focal_loss_reference(a, b), x, t, args.rounds, args.warmup)
    res["passes"]["dice"] = time_pair(losses.DiceLoss(), lambda a, b: losses.dice_loss_reference(a, b), x, t, args.rounds, args.warmup)
    g = torch.Generator().manual_seed(2)
    xb, tb = (2.0 * torch.randn(rows, generator=g)).to(dev), torch.randint(0, 2, (rows,), generator=g).float().to(dev)
    res["passes"]["binary_focal"] = time_pair(losses.BinaryFocalLoss(), lambda a, b: losses.binary_focal_loss_reference(a, b), xb, tb,
                                              args.rounds, args.warmup)
    res["within_bound"] = all(p["within_bound"] for p in res["passes"].values())
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not res["within_bound"]:
        bad = {k: p["fused_over_composition"] for k, p in res["passes"].items() if not p["within_bound"]}
        sys.exit(f"fused pass slower than its torch composition, or the losses differ: {bad}")


if __name__ == "__main__":
    main()

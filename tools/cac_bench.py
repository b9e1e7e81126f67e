#!/usr/bin/env python3
"""Time the CAC-v1m1 head on the device: the fused ops (csrc/cac.hip) against the ``*_torch`` compositions of pointcloudpdf_amd/cac.py.

    python tools/cac_bench.py --rounds 30            -> profiles/cac_bench.json

Work timed: the head only, as ``CACSegmentor.forward`` chains it in train mode -- ``seg_head``, both prototype passes, the three small
MLPs, both cosines, the distillation loss -- forward + backward, no backbone and no criteria (the loss of the run is the distillation loss
plus the means of the two logit tensors' squares, so that every branch carries a gradient).  2 x 100,000 rows, c = 48, K = 20 and
K = 200, conf_thresh = 0.75, detach_pre_logits = True.

Protocol: one process; HIP events around forward + backward; the two sides alternate; median of the rounds after 5 warm-up rounds, p10 /
p90 recorded; both sides start from the same device tensors and parameters, and their results are compared at this size (max-abs
difference relative to the tensor's max-abs).  The composition is given the scenes' ends on the host (``offset_host``), so it slices the
scenes as the reference does and reads nothing back either."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudpdf_amd import cac, synthetic  # noqa: E402

ROWS, C, THRESH, WARMUP = [100000, 100000], 48, 0.75, 5


class _Head(cac.CACSegmentor):
    """The head without a backbone (the registry's ``build_model`` is not asked for one)."""

    def __init__(self, k):
        torch.nn.Module.__init__(self)
        ref = torch.nn
        self.num_classes, self.cos_temp, self.conf_thresh, self.detach_pre_logits = k, 15, THRESH, True
        self.seg_head = cac._Linear(C, k)
        self.proj = ref.Sequential(ref.Linear(C * 2, C * 2, bias=False), ref.ReLU(inplace=True), ref.Linear(C * 2, C))
        self.apd_proj = ref.Sequential(ref.Linear(C * 2, C * 2, bias=False), ref.ReLU(inplace=True), ref.Linear(C * 2, C))
        self.feat_proj_layer = ref.Sequential(cac._Linear(C, C, bias=False), ref.BatchNorm1d(C), ref.ReLU(inplace=True), cac._Linear(C, C))


def step(head, feat, target, data):
    head.zero_grad(set_to_none=True)
    x = feat.detach().requires_grad_()
    logits = head.seg_head(x)
    refine = head.refine(x, logits, data)
    pred = head.adaptive_perspective(x, target)
    kl = cac.distill_loss(refine, pred.detach(), target)
    (kl + refine.square().mean() + pred.square().mean()).backward()
    return dict(refine=refine.detach(), pred=pred.detach(), kl=kl.detach(), g_feat=x.grad, g_seg_head=head.seg_head.weight.grad,
                g_proj=head.proj[0].weight.grad, g_apd=head.apd_proj[0].weight.grad, g_feat_proj=head.feat_proj_layer[0].weight.grad)


def measure(k, rounds):
    dev = "cuda"
    g = torch.Generator().manual_seed(k)
    n = sum(ROWS)
    feat = torch.randn(n, C, generator=g).to(dev)
    target = torch.randint(0, k, (n,), generator=g)
    target[torch.randperm(n, generator=g)[: n // 10]] = -1
    target = target.to(dev)
    ends = [int(v) for v in np.cumsum(ROWS)]
    data = dict(offset=torch.tensor(ends, dtype=torch.int32, device=dev), offset_host=ends)
    head = _Head(k)
    synthetic.fill_parameters_deterministic(head, seed=7)
    head.seg_head.weight.data.mul_(8.0)   # (sharper pre-logits: about half of the rows pass the threshold)
    head.to(dev).train()
    buffers = {name: v.clone() for name, v in head.feat_proj_layer[1].state_dict().items()}
    times, results = {"fused": [], "composition": []}, {}
    for r in range(WARMUP + rounds):
        for side in ("fused", "composition"):
            cac.FORCE_TORCH = side == "composition"
            head.feat_proj_layer[1].load_state_dict(buffers)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out = step(head, feat, target, data)
            e1.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[side].append(e0.elapsed_time(e1))
            results[side] = {key: v.clone() for key, v in out.items()}
    cac.FORCE_TORCH = False
    share = float((torch.softmax(head.seg_head(feat), 1).max(1)[0] >= THRESH).float().mean())
    stat = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
    diff = {key: float((results["fused"][key] - v).abs().max() / v.abs().max().clamp(min=1e-30)) for key, v in results["composition"].items()}
    return dict(classes=k, channels=C, rows=ROWS, conf_thresh=THRESH, rows_over_threshold=share, rounds=rounds, warmup=WARMUP,
                fused=stat(times["fused"]), composition=stat(times["composition"]),
                ratio=float(np.median(times["fused"]) / np.median(times["composition"])), max_rel_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cac_bench.json"))
    args = ap.parse_args()
    report = dict(device=torch.cuda.get_device_name(0), cases=[measure(k, args.rounds) for k in (20, 200)])
    for case in report["cases"]:
        print(json.dumps(case))
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

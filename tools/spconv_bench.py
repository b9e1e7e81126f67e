#!/usr/bin/env python3
"""Time the sparse-convolution passes (csrc/sparse_conv.hip) against the torch composition of pointcloudpdf_amd/sparse_conv.py.

    python tools/spconv_bench.py --rounds 30            -> profiles/spconv_bench.json

Workload: 2 ScanNet-shaped synthetic scenes (pointcloudpdf_amd/synthetic.py, 100,000 voxels each at 0.02 m), the five levels of
SpUNet-v1m1's pyramid over them, and per level the 3x3x3 SubM layer at the level's width; for information also the stem, the wide first
decoder convolution, a strided and an inverse layer, and the whole ``semseg-spunet-v1m1-0-base`` training step with the compositions
forced and not forced.

Protocol: one process; HIP events around forward + backward (gradients of input and weight); the two sides alternate; median of the
rounds after 5 warm-up rounds, p10 / p90 recorded.  Both sides read the same device tensors and the same tables; the composition's pair
lists are prebuilt outside the timed region, like the tables of the HIP side (spconv's "native" algorithm: gather, product, index_add
per offset).  ``required`` marks the rows the package promises not to be slower on (ratio <= 1.0): 3x3x3 SubM at levels 0-2."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudpdf_amd import engine, sparse_conv as spconv, sparse_unet, synthetic  # noqa: E402,F401

ROWS, WARMUP, GRID = [100000, 100000], 5, 0.02
# (name, kind, level, C_in, C_out, kernel size, required)
CASES = [("subm3 level 0 (dec.0)", "subm", 0, 96, 96, 3, True), ("subm3 level 1 (enc.0)", "subm", 1, 32, 32, 3, True),
         ("subm3 level 2 (enc.1)", "subm", 2, 64, 64, 3, True), ("subm3 level 3 (enc.2)", "subm", 3, 128, 128, 3, False),
         ("subm3 level 4 (enc.3)", "subm", 4, 256, 256, 3, False), ("subm3 level 0, 128 -> 96 (dec.0.block0.conv1)", "subm", 0, 128, 96, 3, False),
         ("stem 5x5x5, 6 -> 32", "subm", 0, 6, 32, 5, False), ("down 0 -> 1, 32 -> 32", "down", 0, 32, 32, 2, False),
         ("inverse 1 -> 0, 96 -> 96", "inverse", 0, 96, 96, 2, False)]


def batch(dev):
    b = synthetic.make_batch(ROWS, kind="scannet", device=dev, snap=True, grid_size=GRID)
    b["grid_coord"] = torch.round(b["coord"] / GRID).int()
    b["feat"] = b["feat"][:, 3:].contiguous()   # colour + normal: the recipe's in_channels = 6
    return b


def timed(fn, sides, rounds, setup):
    times = {s: [] for s in sides}
    for r in range(WARMUP + rounds):
        for side in sides:
            setup(side)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[side].append(e0.elapsed_time(e1))
    setup(sides[0])
    stat = lambda v: dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
    return {s: stat(v) for s, v in times.items()}


def force(side):
    spconv.FORCE_TORCH = side == "composition"


def measure_layer(geo, case, rounds, dev):
    name, kind, level, cin, cout, ks, required = case
    fn = dict(subm=spconv.subm_conv, down=spconv.down_conv, inverse=spconv.inverse_conv)[kind]
    rows_in = geo.levels[level + (kind == "inverse")]["n"]
    rows_out = geo.levels[level + (kind == "down")]["n"]
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = torch.randn(rows_in, cin, generator=g).to(dev).requires_grad_()
    w = (torch.randn(cout, ks, ks, ks, cin, generator=g) * 0.05).to(dev).requires_grad_()
    gy = torch.randn(rows_out, cout, generator=g).to(dev)

    def run():
        x.grad = w.grad = None
        fn(x, w, None, geo, level).backward(gy)

    res = timed(run, ("hip", "composition"), rounds, force)
    tbl = geo.subm(level, ks) if kind == "subm" else geo.steps[level].children
    return dict(name=name, kind=kind, level=level, rows_in=rows_in, rows_out=rows_out, c_in=cin, c_out=cout, kernel_size=ks,
                pairs=int((tbl >= 0).sum()), required=required, **res, ratio=res["hip"]["median_ms"] / res["composition"]["median_ms"])


def measure_step(b, rounds, dev):
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=20,
                                                                 channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2)),
                          criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]))
    torch.manual_seed(0)
    step = engine.build_seg_step(cfg).to(dev).train()
    train = engine.TrainStep(step, engine.FusedSGD(step.parameters(), lr=0.05, momentum=0.9, weight_decay=0.0001), graph=False)
    geo = step.model.backbone.make_geometry(b["grid_coord"], b["offset"])
    data = dict(grid_coord=b["grid_coord"], feat=b["feat"], offset=b["offset"], segment=b["segment"], spunet_geometry=geo)
    res = timed(lambda: train(data), ("hip", "composition"), rounds, force)
    return dict(name="semseg-spunet-v1m1-0-base step, geometry handed in", rows=ROWS, **res,
                ratio=res["hip"]["median_ms"] / res["composition"]["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--step-rounds", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spconv_bench.json"))
    args = ap.parse_args()
    dev = "cuda"
    b = batch(dev)
    indices = sparse_unet.SpUNetBase._indices(b["grid_coord"], b["offset"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spconv.SpGeometry.build(indices, 5, [(5, 3)] + [(3,)] * 4)   # (warm-up)
    e0.record()
    geo = spconv.SpGeometry.build(indices, 5, [(5, 3)] + [(3,)] * 4)
    e1.record()
    torch.cuda.synchronize()
    assert not geo.has_duplicates
    report = dict(device=torch.cuda.get_device_name(0), rows=ROWS, grid_size=GRID, levels=[lv["n"] for lv in geo.levels],
                  geometry_build_ms=e0.elapsed_time(e1), rounds=args.rounds, warmup=WARMUP, cases=[])
    for case in CASES:
        report["cases"].append(measure_layer(geo, case, args.rounds, dev))
        print(json.dumps(report["cases"][-1]), flush=True)
    report["step"] = measure_step(b, args.step_rounds, dev)
    print(json.dumps(report["step"]), flush=True)
    report["required_met"] = all(c["ratio"] <= 1.0 for c in report["cases"] if c["required"])
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time PT-v3m1's HIP passes (csrc/serial_attention.hip, csrc/serialization.hip) against the torch compositions of
pointcloudpdf_amd/point_transformer_v3.py.

    python tools/ptv3_bench.py --rounds 30            -> profiles/ptv3_bench.json

Workload: 2 ScanNet-shaped synthetic scenes (pointcloudpdf_amd/synthetic.py, 100,000 voxels each at 0.02 m).
  * the attention node, forward + backward, over level 0's z-order at (C, H, K) = (32, 2, 1024), (64, 4, 1024), (32, 2, 128), and over
    the first 12,500 rows at (512, 32, 1024), against the reference's non-flash branch (gather, reshape, two batched products, softmax,
    scatter) on the same rows and tables; peak device memory of each side;
  * serialization (four codes, orders, inverses) + one pooling partition against their compositions;
  * for information: the ``semseg-pt-v3m1-0-base`` backbone step (forward + backward + FusedAdamW), HIP against every composition forced.

Protocol: one process; HIP events around the timed region; the two sides alternate; median of the rounds after 5 warm-up rounds, p10 / p90
recorded.  ``required`` rows are the ones the package promises not to be slower on (ratio <= 1.0)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudpdf_amd import engine, point_transformer_v3 as v3, sparse_conv as spconv, synthetic  # noqa: E402

ROWS, WARMUP, GRID = [100000, 100000], 5, 0.02
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
# (C, H, K, rows or None = all)
ATTN = [(32, 2, 1024, None), (64, 4, 1024, None), (32, 2, 128, None), (512, 32, 1024, 12500)]


def batch(dev):
    b = synthetic.make_batch(ROWS, kind="scannet", device=dev, snap=True, grid_size=GRID)
    b["grid_coord"] = torch.round(b["coord"] / GRID).int()
    b["grid_coord"] = b["grid_coord"] - b["grid_coord"].min(0).values
    b["feat"] = b["feat"][:, 3:].contiguous()   # colour + normal: the recipe's in_channels = 6
    return b


def force(side):
    v3.FORCE_TORCH = spconv.FORCE_TORCH = side == "composition"


def timed(fn, rounds, sides=("hip", "composition")):
    times, peak = {s: [] for s in sides}, {}
    for r in range(WARMUP + rounds):
        for side in sides:
            force(side)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[side].append(e0.elapsed_time(e1))
                peak[side] = max(peak.get(side, 0), torch.cuda.max_memory_allocated() - base)
    force("hip")
    stat = lambda s: dict(median_ms=float(np.median(times[s])), p10_ms=float(np.percentile(times[s], 10)),
                          p90_ms=float(np.percentile(times[s], 90)), peak_bytes=int(peak[s]))
    res = {s: stat(s) for s in sides}
    res["ratio"] = res["hip"]["median_ms"] / res["composition"]["median_ms"]
    return res


class Level:
    """A geometry level cut down to what serial_attention reads: one order over the first scenes' rows."""

    def __init__(self, order, inverse, sizes, device):
        self.order, self.inverse, self.sizes, self.device, self._t = order.unsqueeze(0), inverse.unsqueeze(0), sizes, device, {}

    def patch(self, K):
        if K not in self._t:
            self._t[K] = v3.PatchTables(self.sizes, K, self.device)
        return self._t[K]


def measure_attention(b, case, rounds, dev):
    c, h, K, rows = case
    if rows is None:
        grid, offset = b["grid_coord"], b["offset"].long()
    else:
        grid, offset = b["grid_coord"][:rows].contiguous(), torch.tensor([rows], device=dev)
    n = grid.shape[0]
    batch_ = v3.offset2batch(offset, n)
    code = v3.serialize_codes(grid, batch_, int(grid.max()).bit_length(), ("z",))
    order, inverse = v3.order_and_inverse(code)
    level = Level(order[0], inverse[0], v3.offset2bincount(offset).tolist(), torch.device(dev))
    g = torch.Generator().manual_seed(c)
    qkv = torch.randn(n, 3 * c, generator=g).to(dev).requires_grad_()
    gout = torch.randn(n, c, generator=g).to(dev)
    scale = (c // h) ** -0.5

    def run():
        qkv.grad = None
        v3.serial_attention(qkv, level, 0, h, K, scale).backward(gout)

    return dict(name=f"attention C={c} H={h} K={K}", rows=n, c=c, heads=h, patch_size=K, required=True, **timed(run, rounds))


def measure_serialization(b, rounds):
    grid, offset = b["grid_coord"], b["offset"].long()
    batch_ = v3.offset2batch(offset, grid.shape[0])
    depth = int(grid.max()).bit_length()

    def run():
        code = v3.serialize_codes(grid, batch_, depth, ORDERS)
        order, _ = v3.order_and_inverse(code)
        v3.pool_partition(code[0], order[0], 3)

    return dict(name="serialization (4 orders) + pooling partition", rows=int(grid.shape[0]), depth=depth, required=True, **timed(run, rounds))


def measure_step(b, rounds, dev):
    cfg = dict(type="DefaultSegmentorV2", num_classes=20, backbone_out_channels=64,
               backbone=dict(type="PT-v3m1", in_channels=6, order=ORDERS, stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2),
                             enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(1024,) * 5,
                             dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16),
                             dec_patch_size=(1024,) * 4, drop_path=0.3, shuffle_orders=True, enable_rpe=False, enable_flash=True,
                             upcast_attention=False, upcast_softmax=False),
               criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)])
    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=cfg)).to(dev).train()
    opt = engine.build_optimizer(dict(type="AdamW", lr=0.006, weight_decay=0.05), step, [dict(keyword="block", lr=0.0006)])
    train = engine.TrainStep(step, opt, graph=False)
    geo = step.model.backbone.make_geometry(b["grid_coord"], b["offset"])
    data = dict(grid_coord=b["grid_coord"], coord=b["coord"], feat=b["feat"], offset=b["offset"], segment=b["segment"], ptv3_geometry=geo)
    return dict(name="semseg-pt-v3m1-0-base step, geometry handed in", rows=ROWS, levels=[lv.n for lv in geo.levels], required=False,
                **timed(lambda: train(data), rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ptv3_bench.json"))
    args = ap.parse_args()
    dev = "cuda"
    b = batch(dev)
    report = dict(device=torch.cuda.get_device_name(0), rows=ROWS, grid_size=GRID, rounds=args.rounds, warmup=WARMUP, cases=[])

    def save():
        report["required_met"] = all(c["ratio"] <= 1.0 for c in report["cases"] if c["required"])
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for case in ATTN:
        report["cases"].append(measure_attention(b, case, args.rounds, dev))
        print(json.dumps(report["cases"][-1]), flush=True)
        save()
    report["cases"].append(measure_serialization(b, args.rounds))
    print(json.dumps(report["cases"][-1]), flush=True)
    save()
    if args.step_rounds > 0:
        report["cases"].append(measure_step(b, args.step_rounds, dev))
        print(json.dumps(report["cases"][-1]), flush=True)
        save()


if __name__ == "__main__":
    main()

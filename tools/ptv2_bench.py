#!/usr/bin/env python3
"""Device time of the PT-v2m2 HIP passes (csrc/gva.hip, csrc/grid_pool.hip) against the torch compositions of
pointcloudpdf_amd/point_transformer_v2.py on the same device tensors.  Prints ONE JSON line and writes it to profiles/ptv2_bench.json;
exits non-zero when a HIP pass is slower than its composition (ratio > 1.0).

  1. GVA relation + attend, forward + backward: n = 200,000 with (c, groups, s) = (48, 6, 16), (96, 12, 16); n = 12,500 with (384, 48, 16);
     the recipes' options (pe_bias on, pe_multiplier off); the kNN table of synthetic scenes.
  2. Grid pooling + map unpooling, forward + backward: 2 x 100,000 points, width 96, cell 0.1 m (partition, pooled coordinates, segment
     max, row gather and their backwards).
  3. Information only (``--step``): the backbone of configs/s3dis/semseg-pt-v2m2-0-base.py on 2 x 100,000 synthetic points, forward +
     backward + FusedAdamW, ms per step with the HIP nodes and with the compositions forced.

How the time is taken (as tools/lovasz_bench.py): one process, every sample between two HIP events, the variants alternate inside every
round; reported per variant: median, min and the 10th / 90th percentile over the rounds after a warm-up.

    python tools/ptv2_bench.py --rounds 30 --step
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S3DIS_BACKBONE = dict(   # configs/s3dis/semseg-pt-v2m2-0-base.py
    in_channels=6, num_classes=13, patch_embed_depth=2, patch_embed_channels=48, patch_embed_groups=6, patch_embed_neighbours=16,
    enc_depths=(2, 6, 2), enc_channels=(96, 192, 384), enc_groups=(12, 24, 48), enc_neighbours=(16, 16, 16), dec_depths=(1, 1, 1),
    dec_channels=(48, 96, 192), dec_groups=(6, 12, 24), dec_neighbours=(16, 16, 16), grid_sizes=(0.1, 0.2, 0.4), attn_qkv_bias=True,
    pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.3, enable_checkpoint=False, unpool_backend="interp")


def summary(us):
    import numpy as np

    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def alternate(variants, rounds, warmup):
    import torch

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
    return {k: summary(v) for k, v in times.items()}


def ratio(res):
    res["hip_over_composition"] = round(res["hip"]["us_median"] / res["composition"]["us_median"], 4)
    return res


def gva_times(dev, n, c, groups, s, rounds, warmup):
    import torch

    from pointcloudpdf_amd import _native, point_transformer_v2 as ptv2, pointops, synthetic

    b = synthetic.make_batch([n // 2, n - n // 2], first_scene_id=70, device=dev)
    idx = pointops.knn_query(s, b["coord"], b["offset"])[0]
    _native.inverse_table(idx, n)
    g = torch.Generator().manual_seed(0)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    q, k, v, peb, wenc, wout = mk(n, c), mk(n, c), mk(n, c), mk(n, s, c), mk(c, groups) / c ** 0.5, mk(n, c)
    kept = {}

    def run(rel_fn, att_fn, tag):
        ins = [t.detach().requires_grad_() for t in (q, k, v, peb)]
        rel = rel_fn(ins[0], ins[1], idx, None, ins[3])
        out = att_fn(rel @ wenc, ins[2], ins[3], idx)   # (a plain product stands in for weight_encoding: the same in both variants)
        (out * wout).sum().backward()
        kept[tag] = (out.detach(), ins[2].grad)

    variants = {"hip": lambda: run(ptv2.gva_relation, ptv2.gva_attend, "hip"),
                "composition": lambda: run(ptv2.gva_relation_torch, ptv2.gva_attend_torch, "composition")}
    res = dict(n=n, c=c, groups=groups, s=s, **alternate(variants, rounds, warmup))
    res["out_max_diff_over_max"] = float((kept["hip"][0] - kept["composition"][0]).abs().max() / kept["composition"][0].abs().max())
    res["g_value_max_diff_over_max"] = float((kept["hip"][1] - kept["composition"][1]).abs().max() / kept["composition"][1].abs().max())
    return ratio(res)


def pool_times(dev, points, width, cell, rounds, warmup):
    import torch

    from pointcloudpdf_amd import point_transformer_v2 as ptv2, synthetic

    b = synthetic.make_batch([points, points], first_scene_id=80, device=dev)
    g = torch.Generator().manual_seed(1)
    feat = torch.randn(2 * points, width, generator=g).relu_().to(dev)
    wf = torch.randn(2 * points, width, generator=g).to(dev)
    kept = {}

    def run(part_fn, max_fn, unpool_fn, tag):
        x = feat.detach().requires_grad_()
        part = part_fn(b["coord"], b["offset"], cell)
        pooled = max_fn(x, part)
        fine = unpool_fn(pooled, part)
        (fine * wf).sum().backward()
        kept[tag] = (part.m, part.coord, x.grad)

    variants = {"hip": lambda: run(ptv2.grid_partition, ptv2.segment_max, ptv2.map_unpool, "hip"),
                "composition": lambda: run(ptv2.grid_partition_torch, lambda x, p: ptv2.segment_max_torch(x, p.idx_ptr, p.sorted),
                                           ptv2.map_unpool_torch, "composition")}
    res = dict(points=[points, points], width=width, cell=cell, **alternate(variants, rounds, warmup))
    res["clusters"] = kept["hip"][0]
    res["identical"] = bool(kept["hip"][0] == kept["composition"][0] and torch.equal(kept["hip"][1], kept["composition"][1])
                            and torch.equal(kept["hip"][2], kept["composition"][2]))
    return ratio(res)


def step_times(dev, points, rounds, warmup):
    import torch

    from pointcloudpdf_amd import optim, point_transformer_v2 as ptv2, synthetic

    b = synthetic.make_batch([points, points], first_scene_id=90, device=dev)
    model = ptv2.PointTransformerV2(**S3DIS_BACKBONE)
    synthetic.fill_parameters_deterministic(model, seed=3)
    model = model.to(dev).train()
    opt = optim.FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.05)
    data = dict(coord=b["coord"], feat=b["feat"], offset=b["offset"])

    def step(hip):
        ptv2.HIP_NODES = hip
        try:
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(data), b["segment"], ignore_index=-1)
            loss.backward()
            opt.step()
        finally:
            ptv2.HIP_NODES = True

    res = alternate({"hip": lambda: step(True), "composition": lambda: step(False)}, rounds, warmup)
    return dict(points=[points, points], model="configs/s3dis/semseg-pt-v2m2-0-base.py backbone + CrossEntropyLoss + FusedAdamW",
                ms_per_step_hip=round(res["hip"]["us_median"] / 1e3, 3), ms_per_step_composition=round(res["composition"]["us_median"] / 1e3, 3),
                hip=res["hip"], composition=res["composition"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=100000, help="points per scene of the pooling and step workloads (two scenes)")
    ap.add_argument("--step", action="store_true", help="also time the S3DIS recipe's backbone step (information only)")
    ap.add_argument("--step-rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptv2_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pointcloudpdf_amd  # noqa: F401  (before the first device call)
    import torch

    assert torch.cuda.is_available(), "ptv2_bench.py measures on the GPU; there is no CPU fall-back"
    dev = torch.device("cuda", 0)
    res = dict(workload="PT-v2m2 passes, forward + backward", device=torch.cuda.get_device_name(dev), rounds=args.rounds, warmup=args.warmup)
    res["gva"] = [gva_times(dev, n, c, g, s, args.rounds, args.warmup)
                  for n, c, g, s in ((2 * args.points, 48, 6, 16), (2 * args.points, 96, 12, 16), (args.points // 8, 384, 48, 16))]
    res["grid_pool"] = pool_times(dev, args.points, 96, 0.1, args.rounds, args.warmup)
    if args.step:
        res["train_step"] = step_times(dev, args.points, args.step_rounds, 3)
    ratios = [r["hip_over_composition"] for r in res["gva"]] + [res["grid_pool"]["hip_over_composition"]]
    res["within_bound"] = bool(max(ratios) <= 1.0 and res["grid_pool"]["identical"])
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not res["within_bound"]:
        sys.exit(f"a HIP pass is slower than its composition (ratios {ratios}) or the pooling results differ")


if __name__ == "__main__":
    main()

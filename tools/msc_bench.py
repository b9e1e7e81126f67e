#!/usr/bin/env python3
"""Device time of the two MSC-v1m1 loss nodes (csrc/scene_contrast.hip, forward + backward through autograd) against the torch
compositions they replace on the same device tensors -- the reference's own lines:

* ``infonce``: ``losses.matched_info_nce`` at the recipe's P = 8,192 pairs of C = 96 channels against
  ``losses.matched_info_nce_reference`` (gather, normalise, the (P, P) similarity matrix, cross-entropy);
* ``recon_color`` / ``recon_normal``: ``masked_scene_contrast.masked_reconstruction`` at 2 x 100,000 rows, 40 % masked, against
  ``masked_reconstruction_composition`` (boolean gathers, the head on the compacted rows).

Prints ONE JSON line and writes it to profiles/msc_bench.json; exits non-zero when a node is slower than its composition (bound: ratio of
the medians <= 1.0) or their losses differ by more than 1e-4 relative.

How the time is taken: one process, every sample is forward + backward between two HIP events, the variants alternate inside every round;
reported per variant: median, min and the 10th / 90th percentile over the rounds after a warm-up, and the peak of
``torch.cuda.max_memory_allocated`` over one call.

Information only (``--no-model`` skips it) -- one training step (forward, backward, SGD) of the ``pretrain-msc-v1m1-0-spunet-base`` model section at
2 scenes x ``--voxels`` voxels per view, with the two nodes and with their compositions (``masked_scene_contrast.FORCE_TORCH``).

    python tools/msc_bench.py --rounds 30
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL = dict(   # the `model` section of configs/scannet/pretrain-msc-v1m1-0-spunet-base.py
    type="MSC-v1m1",
    backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, base_channels=32, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                  layers=(2, 3, 4, 6, 2, 2, 2, 2)),
    backbone_in_channels=6, backbone_out_channels=96, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0.8, view2_mix_prob=0,
    matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4, contrast_weight=1, reconstruct_weight=1,
    reconstruct_color=True, reconstruct_normal=False)


def summary(us):
    import numpy as np

    a = np.sort(np.asarray(us))
    return dict(us_median=round(float(np.median(a)), 2), us_min=round(float(a[0]), 2), us_p10=round(float(np.percentile(a, 10)), 2),
                us_p90=round(float(np.percentile(a, 90)), 2), samples=len(a))


def alternate(variants, rounds, warmup):
    """variants: name -> callable that returns the loss.  -> (times in us per variant, last losses, peak bytes per variant)."""
    import torch

    times, last, peak = {k: [] for k in variants}, {}, {}
    for rnd in range(warmup + rounds):
        for name, run in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last[name] = run()
            e1.record()
            e1.synchronize()
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    for name, run in variants.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    return times, last, peak


def report(times, last, peak, extra):
    lf, lc = float(last["fused"]), float(last["composition"])
    res = dict(**extra, loss_fused=lf, loss_composition=lc, loss_rel_diff=abs(lf - lc) / abs(lc), **{k: summary(v) for k, v in times.items()},
               peak_bytes={k: v for k, v in peak.items()})
    res["fused_over_composition"] = round(res["fused"]["us_median"] / res["composition"]["us_median"], 4)
    res["within_bound"] = bool(res["fused_over_composition"] <= 1.0 and res["loss_rel_diff"] <= 1e-4)
    return res


def infonce_times(dev, pairs, channels, rounds, warmup):
    import torch

    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(0)
    rows = pairs + pairs // 8
    f1 = torch.randn(rows, channels, generator=g).to(dev)
    f2 = (0.7 * f1 + 0.5 * torch.randn(rows, channels, generator=g).to(dev)).contiguous()
    m0 = torch.randperm(rows, generator=g)[:pairs]
    m1 = m0.clone()
    m1[::50] = m1[1::50][: m1[::50].numel()]          # some view-2 rows are matched twice
    match = torch.stack([m0, m1], dim=1).to(dev)

    def variant(fn):
        def run():
            a, b = f1.detach().requires_grad_(), f2.detach().requires_grad_()
            loss = fn(a, b, match, 0.4)[0]
            loss.backward()
            return loss.detach()
        return run

    times, last, peak = alternate({"fused": variant(losses.matched_info_nce), "composition": variant(losses.matched_info_nce_reference)},
                                  rounds, warmup)
    return report(times, last, peak, dict(pairs=pairs, channels=channels, rows_per_view=rows, similarity_matrix_bytes=pairs * pairs * 4))


def recon_times(dev, kind, rows, channels, masked, rounds, warmup):
    import torch

    from pointcloudpdf_amd import masked_scene_contrast as msc

    g = torch.Generator().manual_seed(1)
    f1, f2 = torch.randn(rows, channels, generator=g).to(dev), torch.randn(rows, channels, generator=g).to(dev)
    m1, m2 = (torch.rand(rows, generator=g) < masked).to(dev), (torch.rand(rows, generator=g) < masked).to(dev)
    w, b = (0.1 * torch.randn(3, channels, generator=g)).to(dev), (0.1 * torch.randn(3, generator=g)).to(dev)
    t1, t2 = torch.randn(rows, 3, generator=g).to(dev), torch.randn(rows, 3, generator=g).to(dev)

    def variant(fn):
        def run():
            a, c, ww, bb = f1.detach().requires_grad_(), f2.detach().requires_grad_(), w.detach().requires_grad_(), b.detach().requires_grad_()
            loss = fn(kind, a, c, m1, m2, ww, bb, t1, t2)
            loss.backward()
            return loss.detach()
        return run

    times, last, peak = alternate({"fused": variant(msc.masked_reconstruction), "composition": variant(msc.masked_reconstruction_composition)},
                                  rounds, warmup)
    return report(times, last, peak, dict(kind=kind, rows_per_view=rows, channels=channels, masked_share=masked))


def model_step(dev, voxels, steps, warmup):
    """Information only: ms per training step of the recipe's model with the two nodes and with their compositions."""
    import numpy as np
    import torch

    from pointcloudpdf_amd import engine, masked_scene_contrast as msc

    rng = np.random.default_rng(3)
    side = int(np.ceil((voxels * 1.6) ** (1 / 3)))
    data, views = {}, {1: [], 2: []}
    for _ in range(2):
        cells = rng.permutation(side ** 3)[: int(voxels * 1.3)]
        grid = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1)
        for v in (1, 2):
            views[v].append(grid[np.sort(rng.permutation(grid.shape[0])[:voxels])])
    for v in (1, 2):
        grid = torch.from_numpy(np.concatenate(views[v]).astype(np.int32)).to(dev)
        origin = grid.float() * 0.02
        color = torch.sin(origin * 9 + v)
        data.update({f"view{v}_origin_coord": origin, f"view{v}_coord": origin.clone(), f"view{v}_grid_coord": grid, f"view{v}_color": color,
                     f"view{v}_feat": torch.cat([color, torch.cos(origin * 5)], dim=1),
                     f"view{v}_offset": torch.tensor(np.cumsum([x.shape[0] for x in views[v]]), dtype=torch.int32, device=dev)})
    out = dict(voxels_per_view=[voxels, voxels], steps=steps)
    for name, force in (("nodes", False), ("compositions", True)):
        torch.manual_seed(0)
        step = engine.build_seg_step(dict(model=MODEL)).to(dev)
        step.train()
        train = engine.TrainStep(step, engine.build_optimizer(dict(type="SGD", lr=0.001, momentum=0.9), step, None), graph=False)
        msc.FORCE_TORCH = force
        try:
            ms = []
            for i in range(warmup + steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                last = train(data)
                e1.record()
                e1.synchronize()
                if i >= warmup:
                    ms.append(e0.elapsed_time(e1))
        finally:
            msc.FORCE_TORCH = False
        out[name] = dict(ms_median=round(float(np.median(ms)), 3), ms_min=round(float(np.min(ms)), 3), loss_last=float(last["loss"].detach()),
                         pairs_note="matching_max_pair = 8192")
        del step, train
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--channels", type=int, default=96)
    ap.add_argument("--rows", type=int, default=100000, help="rows per view of the reconstruction measurement")
    ap.add_argument("--masked", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="skip the training step of the recipe's model (information only)")
    ap.add_argument("--voxels", type=int, default=100000)
    ap.add_argument("--train-steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msc_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    assert torch.cuda.is_available(), "msc_bench.py measures on the GPU; there is no CPU fall-back"
    assert args.rounds >= 20, "at least 20 timed rounds per variant"
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    res = dict(workload="MSC-v1m1 loss nodes, forward + backward", device=torch.cuda.get_device_name(dev), rounds=args.rounds, warmup=args.warmup,
               infonce=infonce_times(dev, args.pairs, args.channels, args.rounds, args.warmup),
               recon_color=recon_times(dev, "color", args.rows, args.channels, args.masked, args.rounds, args.warmup),
               recon_normal=recon_times(dev, "normal", args.rows, args.channels, args.masked, args.rounds, args.warmup))
    res["within_bound"] = bool(all(res[k]["within_bound"] for k in ("infonce", "recon_color", "recon_normal")))
    if not args.no_model:
        res["train_step"] = model_step(dev, args.voxels, args.train_steps, 3)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not res["within_bound"]:
        sys.exit("a node is slower than its composition (bound 1.0 x) or the losses differ: " +
                 ", ".join(f"{k} {res[k]['fused_over_composition']} x" for k in ("infonce", "recon_color", "recon_normal")))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""SHA-256 of what the slot-sum passes (csrc/slot_sum.h) compute on seeded inputs: one JSON line, equal between two trees that sum in
the same order.

    python tools/slot_sum_bits.py [--out FILE]

Per pass and row count: the loss, the saved unscaled buffer, the head words of `acc` and the input gradients.  Row counts: 1 (one partly
filled wave, one slot), 257 (two slots), 65,537 (257 slots: the finisher's lane loop takes a second trip), 300,001 (the 1,024-workgroup cap:
the forward grid-strides).  Only bytes the pass defines are hashed (the slots behind the used ones and the rows a pass skips are not).

The passes are driven through their autograd Functions (segmentor._FusedCE, losses._FusedDice, ...) and the saved buffer / `acc` are read
from the node's saved_tensors BY POSITION: the positions below track each Function's ctx.save_for_backward order and must follow it.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudpdf_amd import evaluator, incremental, losses, masked_scene_contrast, point_group, segmentor  # noqa: E402

ROWS = (1, 257, 65537, 300001)
C = 13
DEV = "cuda:0"


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rnd(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen, dtype=dtype).to(DEV)


def labels(gen, n, c, ignore=-1):
    t = torch.randint(0, c, (n,), generator=gen)
    t[torch.rand(n, generator=gen) < 0.1] = ignore
    return t.to(DEV)


def record(losses_, node, saved, acc, inputs, select=None):
    """losses_: the pass's outputs (the first one is differentiated); saved / acc: positions in the node's saved tensors."""
    st = node.saved_tensors
    out = {"loss": [sha(l) for l in losses_]}
    if saved is not None:
        out["saved"] = sha(st[saved] if select is None else st[saved][select])
    if acc is not None:
        out["acc"] = sha(st[acc][:4])
    grads = torch.autograd.grad(losses_[0].sum(), inputs, retain_graph=True)
    out["grad"] = [sha(g) for g in grads]
    return out


def row_passes(n, gen):
    res = {}
    x = rnd(gen, n, C).requires_grad_()
    t = labels(gen, n, C)
    l = segmentor._FusedCE.apply(x, t, -1)
    res["ce"] = record([l], l.grad_fn, 0, 1, [x])
    w = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    l = segmentor._FusedCEEx.apply(x, t, w, 0.1, "mean", -1)
    res["ce_ex"] = record([l], l.grad_fn, 0, 1, [x])
    l = losses._FusedFocal.apply(x, t, 0.5, 2.0, "mean", -1)
    res["focal"] = record([l], l.grad_fn, 0, 1, [x])
    l = losses._FusedDice.apply(x, t, 1.0, 2.0, -1)
    res["dice"] = record([l], l.grad_fn, 0, 2, [x])
    l = losses._FusedLovasz.apply(x, t, -1, None)
    res["lovasz"] = record([l], l.grad_fn, 0, None, [x])
    teacher = rnd(gen, n, C - 3)
    tl = labels(gen, n, C)
    tl[torch.rand(n, generator=gen).to(DEV) < 0.5] = -1   # half of the rows take the teacher's soft target
    l = incremental._FusedIncrKl.apply(x, teacher, tl, -1, 1.0 / 2.0, 1.0 / 3.0)
    res["incr_kl"] = record([l], l.grad_fn, 0, 1, [x])
    p = rnd(gen, n).requires_grad_()
    bt = (torch.rand(n, generator=gen) < 0.3).float().to(DEV)
    l = losses._FusedBinaryFocal.apply(p, bt, 0.5, 2.0, True, True)
    res["bfocal"] = record([l], l.grad_fn, 0, 1, [p])
    bias = rnd(gen, n, 3).requires_grad_()
    coord, inst = rnd(gen, n, 3), labels(gen, n, 30)
    for name, dt in (("pg_bias_f32", torch.float32), ("pg_bias_f64", torch.float64)):
        l1, l2 = point_group._BiasLosses.apply(bias, coord, rnd(gen, n, 3, dtype=dt), inst, -1)
        res[name] = {**record([l1, l2], l1.grad_fn, 0, 1, [bias]), "grad_cos": [sha(g) for g in torch.autograd.grad(l2, [bias])]}
    n1, cw = n // 2, 96
    f1, f2 = rnd(gen, n1, cw).requires_grad_(), rnd(gen, n - n1, cw).requires_grad_()
    m1, m2 = (torch.rand(n1, generator=gen) < 0.4).to(DEV), (torch.rand(n - n1, generator=gen) < 0.4).to(DEV)
    m2[-1] = True
    wt, b = rnd(gen, 3, cw).requires_grad_(), rnd(gen, 3).requires_grad_()
    t1, t2 = rnd(gen, n1, 3), rnd(gen, n - n1, 3)
    for kind, name in ((0, "msc_color"), (1, "msc_normal")):
        l = masked_scene_contrast._MaskedReconstruction.apply(kind, f1, f2, m1, m2, wt, b, t1, t2)
        res[name] = record([l], l.grad_fn, 5, 6, [f1, f2, wt, b], select=torch.cat([m1, m2]))   # (dpred: the masked rows are written)
    score = rnd(gen, n)
    hist, rec = evaluator.openset_metrics(x.detach(), score, labels(gen, n, C), C, [C - 1], -1)
    res["openset"] = {"hist": sha(hist), "record": sha(rec)}
    return res


def info_nce(p, c, gen):
    f1, f2 = rnd(gen, p + 50, c).requires_grad_(), rnd(gen, p + 20, c).requires_grad_()
    match = torch.stack([torch.randint(0, p + 50, (p,), generator=gen), torch.randint(0, p + 20, (p,), generator=gen)], 1).to(DEV)
    out = losses._FusedInfoNCE.apply(f1, f2, match, 0.4)
    return record(list(out), out[0].grad_fn, None, None, [f1, f2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {}
    for n in ROWS:
        gen = torch.Generator().manual_seed(1000 + n)
        for name, r in row_passes(n, gen).items():
            res[f"{name}/{n}"] = r
    for p, c in ((257, 96), (3000, 32)):
        res[f"info_nce/{p}x{c}"] = info_nce(p, c, torch.Generator().manual_seed(p))
    torch.cuda.synchronize()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

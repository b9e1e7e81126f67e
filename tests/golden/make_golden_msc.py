#!/usr/bin/env python3
"""Generate tests/golden/model_msc_ref.npz by running the REFERENCE's own ``MaskedSceneContrast``.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_msc.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py  -- MaskedSceneContrast, CPU tensors
over stand-ins for what the container lacks (msc_cases.py holds the ones the tests' restatement shares):
  * ``torch_geometric.nn.pool.voxel_grid``: the grid_cluster formula (msc_cases.voxel_grid);
  * ``timm.models.layers.trunc_normal_``: torch's;
  * ``pointops.knn_query``: brute force plus ``sqrt`` (msc_cases.knn_query);
  * ``pointcept.utils.comm.get_world_size``: 1; ``pointcept.models.utils.offset2batch``;
  * ``pointcept.models.builder`` with a registry holding msc_cases.TinyBackbone (per-point MLP + BatchNorm + the per-scene mean over
    ``offset``, so that view mixing is visible);
  * ``Tensor.cuda`` is the identity for the duration of a run (the reference calls ``.cuda()`` inside ``generate_cross_masks``).

Inputs: two scenes; per scene an origin cloud on a floor and a wall, two views that are different random subsets of it under different
rotations, ``origin_coord`` kept (so matches exist), feat = [color | normal].  Two runs (msc_cases.RUNS): A -- ``matching_max_pair``
below the matched count (the randperm cut fires), ``view1_mix_prob = 1``, both heads; B -- pairs below the cap, no mixing, color head only.
Every draw is recorded by wrapping the torch / random calls.  The float64 run keeps ``origin_coord`` in fp32 (geometry: masks and pairs
must be the fp32 run's), everything differentiable in double.

A view-1 point whose kNN row has a distance within 2e-5 of ``max_radius`` or two distances within 2e-6 of each other is left out of view 1.
The seed is stepped until, judged by the reference runs alone: no kNN distance lies within 1e-5 of ``max_radius``, no two of a query's
``max_k`` distances lie within 1e-6 of each other, the fp32 gradients lie within 1e-5 of the float64 ones (no ReLU kink), and run A has a
view-2 row that is matched twice."""
import copy
import importlib.util
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (where the reference tree lives)
import msc_cases as mc  # noqa: E402

REF = mg.REF
RADIUS_MARGIN, TIE_MARGIN, KINK_FREE = 1e-5, 1e-6, 1e-5
TERMS = ("loss", "nce_loss", "pos_sim", "neg_sim", "color_loss", "normal_loss")


def load_reference():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class _Registry:
        def __init__(self, *a, **k):
            self.classes = {}

        def register_module(self, name=None, **k):
            def deco(cls):
                self.classes[name or cls.__name__] = cls
                return cls
            return deco(name) if isinstance(name, type) else deco

        def build(self, cfg):
            cfg = dict(cfg)
            return self.classes[cfg.pop("type")](**cfg)

    models = _Registry()
    models.classes["MSC-test-MLP"] = mc.TinyBackbone
    for name in ("torch_geometric", "torch_geometric.nn", "timm", "timm.models", "pointcept", "pointcept.models", "pointcept.utils"):
        module(name)
    module("torch_geometric.nn.pool", voxel_grid=mc.voxel_grid)
    module("timm.models.layers", trunc_normal_=torch.nn.init.trunc_normal_)
    module("pointops", knn_query=mc.knn_query)
    module("pointcept.models.builder", MODELS=models, build_model=models.build)
    module("pointcept.models.utils", offset2batch=mc.offset2batch)
    module("pointcept.utils.comm", get_world_size=lambda: 1)
    spec = importlib.util.spec_from_file_location("ref_msc", os.path.join(REF, "pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_msc"] = mod
    spec.loader.exec_module(mod)
    return mod


def rotation(rng):
    a = rng.uniform(0, 2 * np.pi)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    views = {1: [], 2: []}
    for n_origin in (2000, 2100):
        floor = np.concatenate([rng.uniform(-0.35, 0.35, (n_origin * 2 // 3, 2)), np.zeros((n_origin * 2 // 3, 1))], 1)
        wall = np.stack([rng.uniform(-0.35, 0.35, n_origin // 3), np.full(n_origin // 3, 0.35), rng.uniform(0, 0.5, n_origin // 3)], 1)
        origin = np.concatenate([floor, wall]).astype(np.float32)
        origin[:, 0] -= 0.2 * (len(views[1]) % 2)            # the second scene reaches into negative cells further
        normal = np.concatenate([np.tile([0, 0, 1.0], (floor.shape[0], 1)), np.tile([0, -1.0, 0], (wall.shape[0], 1))]).astype(np.float32)
        normal = normal + 0.1 * rng.standard_normal(normal.shape).astype(np.float32)
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        color = (0.5 + 0.5 * np.sin(7 * origin + rng.uniform(0, 3, 3)) + 0.05 * rng.standard_normal(origin.shape)).astype(np.float32)
        pair = {}
        for v in (1, 2):
            keep = np.sort(rng.permutation(origin.shape[0])[:1300 + 17 * v + 5 * len(views[v])])
            rot = rotation(rng)
            pair[v] = dict(origin_coord=origin[keep], coord=origin[keep] @ rot.T, color=color[keep], normal=(normal[keep] @ rot.T).astype(np.float32))
        # a view-1 point whose own kNN row comes close to the radius or holds a near-tie is left out of view 1 (the other rows look into
        # view 2 and do not change): the two margins hold by construction, with a factor 2 to spare
        kw = mc.RUNS["a"]
        o1, o2 = torch.from_numpy(pair[1]["origin_coord"]), torch.from_numpy(pair[2]["origin_coord"])
        _, dist = mc.knn_query(kw["matching_max_k"], o2, torch.tensor([o2.shape[0]]), o1, torch.tensor([o1.shape[0]]))
        d = dist.double()
        good = ((d - kw["matching_max_radius"]).abs().min(1).values >= 2 * RADIUS_MARGIN) & ((d[:, 1:] - d[:, :-1]).abs().min(1).values >= 2 * TIE_MARGIN)
        pair[1] = {k: a[good.numpy()] for k, a in pair[1].items()}
        for v in (1, 2):
            views[v].append(pair[v])
    out = {}
    for v in (1, 2):
        for k in ("origin_coord", "coord", "color", "normal"):
            out[f"view{v}_{k}"] = np.concatenate([s[k] for s in views[v]]).astype(np.float32)
        out[f"view{v}_offset"] = np.cumsum([s["coord"].shape[0] for s in views[v]]).astype(np.int32)
    return out


def tensors(inputs, dtype):
    data = {}
    for k, v in inputs.items():
        t = torch.from_numpy(v)
        data[k] = t if k.endswith("offset") or k.endswith("origin_coord") else t.to(dtype)
    for v in (1, 2):
        data[f"view{v}_feat"] = torch.cat([data[f"view{v}_color"], data[f"view{v}_normal"]], dim=1)
    return data


def run(model, data, seed):
    """One train-mode forward + backward of the reference model under the given seeds, draws recorded."""
    m = copy.deepcopy(model).train()
    torch.manual_seed(seed)
    random.seed(seed)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    log = {}
    gen, match = m.generate_cross_masks, m.match_contrastive_pair

    def masks(*a, **k):
        log["mask1"], log["mask2"] = gen(*a, **k)
        return log["mask1"], log["mask2"]

    def pairs(*a, **k):
        log["match"] = match(*a, **k)
        return log["match"]

    m.generate_cross_masks, m.match_contrastive_pair = masks, pairs
    try:
        with mc.Recorder() as rec:
            out = m(dict(data))
    finally:
        torch.Tensor.cuda = cuda
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(out["loss"], [p for _, p in m.named_parameters()])
    return ({k: out[k].detach() for k in TERMS if k in out}, dict(zip(names, [g.detach() for g in grads])), rec.seq, log)


def knn_margins(data, kw):
    idx, dist = mc.knn_query(kw["matching_max_k"], data["view2_origin_coord"].float(), data["view2_offset"].int(),
                             data["view1_origin_coord"].float(), data["view1_offset"].int())
    d = dist.double()
    return float((d - kw["matching_max_radius"]).abs().min()), float((d[:, 1:] - d[:, :-1]).abs().min())


def main():
    ref = load_reference()
    seed = 0
    while True:
        inputs = build_inputs(300 + seed)
        data32, data64 = tensors(inputs, torch.float32), tensors(inputs, torch.float64)
        radius_margin, tie_margin = knn_margins(data32, mc.RUNS["a"])
        runs, ok = {}, radius_margin >= RADIUS_MARGIN and tie_margin >= TIE_MARGIN
        for name, kw in mc.RUNS.items():
            torch.manual_seed(seed)
            model = ref.MaskedSceneContrast(**kw)
            with torch.no_grad():   # (a zero-initialised head bias and a 0.02 token make the heads' gradients tiny: give them a size)
                for p in model.parameters():
                    if p.dim() == 1:
                        p.add_(0.1 * torch.randn_like(p))
            lo_t, lo_g, seq, log = run(model, data32, 1000 + seed)
            hi_t, hi_g, seq64, log64 = run(copy.deepcopy(model).double(), data64, 1000 + seed)
            assert torch.equal(log["mask1"], log64["mask1"]) and torch.equal(log["mask2"], log64["mask2"]) and torch.equal(log["match"], log64["match"])
            assert [n for n, _ in seq] == [n for n, _ in seq64]
            top = max(float(g.abs().max()) for g in hi_g.values())
            # (relative to the largest gradient element overall: the bias of the Linear in front of the BatchNorm has a gradient of exactly
            #  zero, and an activation that sits on a ReLU kink moves a whole row's contribution, orders of magnitude above rounding)
            kink = max(float((lo_g[k].double() - hi_g[k]).abs().max()) for k in hi_g) / top
            twice = int(torch.bincount(log["match"][:, 1]).max()) >= 2
            pairs = log["match"].shape[0]
            print(f"seed {seed} run {name}: {pairs} pairs, draws {[n for n, _ in seq]}, masked {int(log['mask1'].sum())} + {int(log['mask2'].sum())}, "
                  f"fp32 gradients {kink:.2e} off the float64 run, a row matched twice: {twice}", flush=True)
            ok = ok and kink <= KINK_FREE and (name != "a" or (twice and [n for n, _ in seq].count("randperm") == 2))
            ok = ok and (name != "b" or [n for n, _ in seq].count("randperm") == 1)
            runs[name] = (model, lo_t, lo_g, hi_t, hi_g, seq, log)
        print(f"seed {seed}: radius margin {radius_margin:.2e}, tie margin {tie_margin:.2e}", flush=True)
        if ok:
            break
        seed += 1
        assert seed < 16, "no admissible seed among 16"

    out = dict(seed=np.int64(seed), forward_seed=np.int64(1000 + seed), radius_margin=np.float64(radius_margin), tie_margin=np.float64(tie_margin))
    for k, v in inputs.items():
        out[f"in_{k}"] = v
    for name, (model, lo_t, lo_g, hi_t, hi_g, seq, log) in runs.items():
        sd = model.state_dict()
        out[f"{name}_keys"] = np.array(list(sd.keys()))
        for i, v in enumerate(sd.values()):
            out[f"{name}_weight_{i}"] = v.numpy()
        out[f"{name}_draw_names"] = np.array([n for n, _ in seq])
        for i, (n, v) in enumerate(seq):
            out[f"{name}_draw_{i}"] = np.float64(v) if n == "random" else v.numpy().astype(np.int32)
        out[f"{name}_mask1"], out[f"{name}_mask2"] = np.packbits(log["mask1"].numpy()), np.packbits(log["mask2"].numpy())
        out[f"{name}_match"] = log["match"].numpy().astype(np.int32)
        out[f"{name}_term_names"] = np.array(list(hi_t.keys()))
        out[f"{name}_terms"] = np.array([float(hi_t[k]) for k in hi_t])
        out[f"{name}_err_terms"] = np.array([abs(float(lo_t[k]) - float(hi_t[k])) for k in hi_t])
        out[f"{name}_grad_names"] = np.array(list(hi_g.keys()))
        for i, k in enumerate(hi_g):
            out[f"{name}_grad_{i}"] = hi_g[k].numpy()
            out[f"{name}_err_grad_{i}"] = np.float64((lo_g[k].double() - hi_g[k]).abs().max())
    path = os.path.join(HERE, "model_msc_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

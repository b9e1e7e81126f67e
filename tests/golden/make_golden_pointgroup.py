#!/usr/bin/env python3
"""Generate tests/golden/model_pointgroup_ref.npz by running the REFERENCE's own ``PointGroup``, ``InstanceParser`` and ``InsSegEvaluator``.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_pointgroup.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/point_group/point_group_v1m1_base.py  -- PointGroup, CPU tensors
  * pointcept/datasets/transform.py                        -- InstanceParser
  * pointcept/engines/hooks/evaluator.py                   -- InsSegEvaluator.associate_instances / evaluate_matches on a stub trainer
over stand-ins written HERE for what the container lacks:
  * ``pointgroup_ops``: ``ballquery_batch_p`` / ``bfs_cluster`` as the statement-by-statement Python form of
    libs/pointgroup_ops/src/bfs_cluster_kernel.cu:16-62 and bfs_cluster.cpp:53-137 (rows in row order instead of atomicAdd order);
  * ``pointcept.models.builder`` with a registry holding the small per-point MLP + BatchNorm backbone of pointgroup_cases.TinyBackbone, so
    the fixture pins the PointGroup wiring and not spconv again; ``pointcept.models.utils`` (offset2batch, batch2offset);
  * ``pointcept.utils.registry`` / ``comm`` / ``misc``, ``pointops`` and the hooks' ``default`` / ``builder``: names only.

The run: two scenes of about 1,500 points -- blobs of 40-400 points of four object classes, a floor and a wall of the two ignored classes,
some unlabelled points, two instances close enough to merge (APs below 1) -- through InstanceParser per scene, collated.  The reference model is trained with SGD on the CPU until eval mode
yields at least three proposals, a cluster dropped by cluster_min_points and one dropped by cluster_propose_points.  The seed is stepped
until, judged by the reference run alone: no in-scene pair of predicted centres lies within PAIR_MARGIN voxel of the radius, no softmax
top-two margin is below TOP2_MARGIN, and the fp32 gradients are within KINK_FREE of the float64 run's (no activation on a ReLU kink).
Stored: the inputs, the parser outputs, the weights, train-mode loss terms and float64 gradients with the reference run's own fp32 error,
eval-mode masks (bit-packed), classes and scores, the tables and clusters of the eval run, and the AP dict."""
import copy
import importlib.util
import os
import sys
import types
from collections import deque

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import make_golden as mg  # noqa: E402  (where the reference tree lives)
import pointgroup_cases as pc  # noqa: E402

REF = mg.REF
PAIR_MARGIN, TOP2_MARGIN, KINK_FREE = 1e-3, 1e-5, 1e-5
MIN_STEPS = 600   # (BatchNorm momentum 0.01: the running statistics the eval run uses have caught up by then, and the predicted
#                    centres of a blob have collapsed well inside the radius)
CLASS_NOISE = 0.45
NAMES = ["floor", "wall", "chair", "table", "sofa", "desk"]
LOG = {}


# ---- stand-in for pointgroup_ops ------------------------------------------------------------------------------------------------------
def ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive):
    xyz = coords.detach().numpy().astype(np.float32)
    n = xyz.shape[0]
    radius2 = np.float32(radius) * np.float32(radius)
    idx, start_len, cumsum = [], np.zeros((n, 2), np.int32), 0
    for pt_idx in range(n):
        o_x, o_y, o_z = xyz[pt_idx]
        start, end = int(batch_offsets[batch_idxs[pt_idx]]), int(batch_offsets[batch_idxs[pt_idx] + 1])
        x, y, z = xyz[start:end, 0], xyz[start:end, 1], xyz[start:end, 2]
        d2 = (o_x - x) * (o_x - x) + (o_y - y) * (o_y - y) + (o_z - z) * (o_z - z)
        cnt = 0
        for k in np.nonzero(d2 < radius2)[0]:
            if cnt < 1000:
                idx.append(start + int(k))
            else:
                break
            cnt += 1
        start_len[pt_idx] = (cumsum, cnt)
        cumsum += cnt
    LOG["idx"], LOG["start_len"] = np.array(idx, np.int32), start_len
    return torch.from_numpy(LOG["idx"].copy()), torch.from_numpy(start_len.copy())


def bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold):
    label, idxs, sl = semantic_label.numpy(), ball_query_idxs.numpy(), start_len.numpy()
    n = sl.shape[0]
    visited = np.zeros(n, np.int32)
    clusters, sizes = [], []
    for i in range(n):
        if visited[i] == 0:
            cc = [i]
            visited[i] = 1
            queue = deque([i])
            while queue:
                cur = queue.popleft()
                start, length = int(sl[cur, 0]), int(sl[cur, 1])
                label_cur = label[cur]
                for j in range(start, start + length):
                    idx_i = int(idxs[j])
                    if label[idx_i] != label_cur:
                        continue
                    if visited[idx_i] == 1:
                        continue
                    cc.append(idx_i)
                    visited[idx_i] = 1
                    queue.append(idx_i)
            sizes.append(len(cc))
            if len(cc) >= threshold:
                clusters.append(cc)
    offsets = np.zeros(len(clusters) + 1, np.int32)
    out = np.zeros((sum(len(c) for c in clusters), 2), np.int32)
    for i, cc in enumerate(clusters):
        offsets[i + 1] = offsets[i] + len(cc)
        out[offsets[i]:offsets[i + 1], 0] = i
        out[offsets[i]:offsets[i + 1], 1] = cc
    LOG["component_sizes"], LOG["cluster_idxs"], LOG["cluster_offsets"], LOG["labels"] = np.array(sizes), out, offsets, label.astype(np.int32)
    return torch.from_numpy(out.copy()), torch.from_numpy(offsets.copy())


# ---- the reference, imported in place ---------------------------------------------------------------------------------------------------
def load_reference():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    def load(modname, rel):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

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
    models.classes["PG-test-MLP"] = pc.TinyBackbone

    def offset2batch(offset):
        return torch.searchsorted(offset.long(), torch.arange(int(offset[-1])), right=True)

    def batch2offset(batch):
        return torch.cumsum(batch.bincount(), dim=0).long()

    for name in ("pointcept", "pointcept.models", "pointcept.utils", "pointcept.engines", "pointcept.engines.hooks"):
        module(name)
    module("pointgroup_ops", ballquery_batch_p=ballquery_batch_p, bfs_cluster=bfs_cluster)
    module("pointcept.models.builder", MODELS=models, build_model=models.build)
    module("pointcept.models.utils", offset2batch=offset2batch, batch2offset=batch2offset)
    module("pointcept.utils.registry", Registry=_Registry)
    module("pointcept.utils.comm")
    module("pointcept.utils.misc", aupr_and_auroc=None, intersection_and_union_gpu=None, is_pytorch_model=None, selected_mask=None)
    module("pointops")
    module("pointcept.engines.hooks.default", HookBase=type("HookBase", (), {}))
    module("pointcept.engines.hooks.builder", HOOKS=_Registry())
    model = load("ref_point_group", "pointcept/models/point_group/point_group_v1m1_base.py")
    transform = load("ref_transform_pg", "pointcept/datasets/transform.py")
    hooks = load("pointcept.engines.hooks.evaluator", "pointcept/engines/hooks/evaluator.py")
    return model, transform, hooks


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def raw_scene(rng, sizes, floor, wall, unlabelled, twins=()):
    coord, segment, instance, target = [], [], [], []
    centres = []
    for i, s in enumerate(sizes):
        while True:
            c = rng.uniform(0.5, 5.5, 3).astype(np.float32)
            if all(np.linalg.norm(c - o) > 1.2 for o in centres):
                break
        if i in dict(twins):   # 0.8 voxel from an earlier blob of the same class: the two instances come out as ONE proposal
            c = centres[dict(twins)[i]] + np.float32([0.04, 0, 0])
        centres.append(c)
        coord.append(c + rng.normal(0, 0.08, (s, 3)).astype(np.float32))
        segment.append(np.full(s, 2 + i % 4))
        instance.append(np.full(s, 5 + 3 * i))          # raw ids: arbitrary, not contiguous
        target.append(np.full(s, i))
    for cls, s, axis in ((0, floor, 2), (1, wall, 0)):
        p = rng.uniform(0, 6, (s, 3)).astype(np.float32)
        p[:, axis] = 0
        coord.append(p)
        segment.append(np.full(s, cls))
        instance.append(np.full(s, 100 + cls))          # an instance id on an ignored class: InstanceParser maps it to the ignore index
        target.append(np.full(s, -1))
    # unlabelled points that look like members of a blob (they end up inside proposals: void intersections)
    host = rng.integers(0, len(sizes), unlabelled)
    coord.append(np.stack(centres)[host] + rng.normal(0, 0.08, (unlabelled, 3)).astype(np.float32))
    segment.append(np.full(unlabelled, -1))
    instance.append(np.full(unlabelled, -1))
    target.append(host)
    order = rng.permutation(sum(len(c) for c in coord))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt)[order]
    return cat(coord, np.float32), cat(segment, np.int64), cat(instance, np.int64), cat(target, np.int64), np.stack(centres), np.array(sizes)


def features(rng, coord, segment, target, centres, sizes):
    """[10 x (offset to the blob's centre + noise) | noisy one-hot of the blob's class, the object classes noisier]; zeros / the ignored class on floor and wall."""
    n = coord.shape[0]
    feat = np.zeros((n, pc.FEAT), np.float32)
    on = target >= 0
    feat[on, :3] = 10 * ((centres[target[on]] - coord[on]) + rng.normal(0, 0.004, (int(on.sum()), 3)).astype(np.float32))
    cls = np.where(on, 2 + np.maximum(target, 0) % 4, segment)
    feat[np.arange(n), 3 + cls] = 1.0
    feat[:, 3:] += rng.normal(0, 0.05, (n, pc.NUM_CLASSES)).astype(np.float32)
    # the object classes are hard to tell apart (the cross-entropy of the trained model stays at a realistic 0.1 - 0.5, and some members of
    # a blob are predicted as another class: the label split of the clustering is exercised)
    feat[cls >= 2, 5:] += rng.normal(0, CLASS_NOISE, (int((cls >= 2).sum()), pc.NUM_CLASSES - 2)).astype(np.float32)
    return feat


def build_inputs(transform, seed):
    rng = np.random.default_rng(seed)
    parser = transform.InstanceParser(segment_ignore_index=pc.IGNORE, instance_ignore_index=-1)
    raw, parsed, feats = [], [], []
    for sizes, floor, wall, unl, twins in (([400, 260, 150, 120, 80, 45], 300, 110, 35, ()), ([330, 210, 170, 90, 60, 40, 130], 280, 120, 30, ((6, 2),))):
        coord, segment, instance, target, centres, sz = raw_scene(rng, sizes, floor, wall, unl, twins)
        raw.append((coord, segment, instance))
        parsed.append(parser(dict(coord=coord.copy(), segment=segment.copy(), instance=instance.copy())))
        feats.append(features(rng, coord, segment, target, centres, sz))
    return raw, parsed, np.concatenate(feats)


def collate(parsed, feat, dtype):
    sizes = [p["coord"].shape[0] for p in parsed]
    cat = lambda k: np.concatenate([p[k] for p in parsed])
    return dict(coord=torch.from_numpy(cat("coord")).to(dtype), feat=torch.from_numpy(feat).to(dtype),
                segment=torch.from_numpy(cat("segment")), instance=torch.from_numpy(cat("instance")),
                instance_centroid=torch.from_numpy(cat("instance_centroid")),       # float64, as ToTensor keeps it
                offset=torch.from_numpy(np.cumsum(sizes)).int())


def rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def train_outputs(model, data):
    m = copy.deepcopy(model).train()
    out = m(dict(data))
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(out["loss"], [p for _, p in m.named_parameters()])
    return {k: out[k].detach() for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss")}, dict(zip(names, [g.detach() for g in grads]))


def eval_outputs(model, data):
    m = copy.deepcopy(model).eval()
    with torch.no_grad():
        out = m(dict(data))
    return out, {k: np.copy(v) for k, v in LOG.items()}


def margins(model, data):
    """(smallest | distance - radius | over the in-scene pairs of predicted centres, smallest softmax top-two margin) of the eval run."""
    m = copy.deepcopy(model).eval()
    with torch.no_grad():
        feat = m.backbone(dict(data))
        centre = (data["coord"] + m.bias_head(feat)) / m.voxel_size
        prob = torch.softmax(m.seg_head(feat), -1)
    top2 = prob.topk(2, -1)[0]
    clustered = ~torch.isin(prob.argmax(-1), torch.tensor(m.segment_ignore_index))   # the rows that enter the ball table
    pair = float("inf")
    ends = data["offset"].tolist()
    for s, e in zip([0] + ends[:-1], ends):
        c = centre[s:e][clustered[s:e]].double()
        pair = min(pair, float((torch.cdist(c, c) - m.cluster_thresh).abs().min()))
    return pair, float((top2[:, 0] - top2[:, 1]).min())


def main():
    ref_model, transform, hooks = load_reference()
    seed = 0
    while True:
        raw, parsed, feat = build_inputs(transform, 100 + seed)
        data32, data64 = collate(parsed, feat, torch.float32), collate(parsed, feat, torch.float64)
        torch.manual_seed(seed)
        model = ref_model.PointGroup(**pc.MODEL_KW)
        opt = torch.optim.SGD(model.parameters(), lr=0.02, momentum=0.9)
        good, steps = False, 0
        while steps < 1200 and not (good and steps >= MIN_STEPS):
            model.train()
            for _ in range(25):
                opt.zero_grad()
                model(dict(data32))["loss"].backward()
                opt.step()
                steps += 1
            ev, log = eval_outputs(model, data32)
            sizes = log.get("component_sizes", np.zeros(0))
            kept = np.diff(log.get("cluster_offsets", np.zeros(1)))
            good = (len(ev["pred_scores"]) >= 3 and np.any(sizes < model.cluster_min_points)
                    and np.any(kept <= model.cluster_propose_points))
            print(f"seed {seed} step {steps}: {len(ev['pred_scores'])} proposals, {len(kept)} clusters of {len(sizes)} components, "
                  f"bias_l1_loss {float(ev['bias_l1_loss']):.4f}", flush=True)
        pair, top2 = margins(model, data32)
        lo_t, lo_g = train_outputs(model, data32)
        hi_model = copy.deepcopy(model).double()
        hi_t, hi_g = train_outputs(hi_model, data64)
        # (relative to the tensor's largest element, but no finer than 1e-3 of the largest gradient element overall: the bias of the
        #  Linear in front of a BatchNorm has a gradient of exactly zero)
        top = max(float(g.abs().max()) for g in hi_g.values())
        kink = max(float((lo_g[k].double() - hi_g[k]).abs().max()) / max(float(hi_g[k].abs().max()), 1e-3 * top) for k in hi_g)
        print(f"seed {seed}: pair margin {pair:.2e} voxel, top-two margin {top2:.2e}, fp32 gradients {kink:.2e} off the float64 run", flush=True)
        if good and pair >= PAIR_MARGIN and top2 >= TOP2_MARGIN and kink <= KINK_FREE:
            break
        seed += 1
        assert seed < 16, "no admissible seed among 16"
    ev64, _ = eval_outputs(hi_model, data64)
    assert torch.equal(ev64["pred_masks"], ev["pred_masks"]) and torch.equal(ev64["pred_classes"], ev["pred_classes"])

    # ---- the reference's evaluator on a stub trainer
    hook = hooks.InsSegEvaluator(segment_ignore_index=pc.IGNORE, instance_ignore_index=-1)
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(num_classes=pc.NUM_CLASSES, names=NAMES))
    hook.trainer = types.SimpleNamespace(cfg=cfg)
    hook.before_train()
    scenes, ends = [], data32["offset"].tolist()
    # (the hook evaluates one scene per batch: the collated eval run is cut per scene; a proposal never spans scenes)
    for s, e in zip([0] + ends[:-1], ends):
        inside = ev["pred_masks"][:, s:e].sum(1) > 0
        pred = dict(pred_masks=ev["pred_masks"][inside][:, s:e], pred_classes=ev["pred_classes"][inside], pred_scores=ev["pred_scores"][inside])
        gt, pr = hook.associate_instances(pred, data32["segment"][s:e], data32["instance"][s:e])
        scenes.append(dict(gt=gt, pred=pr))
    ap = hook.evaluate_matches(scenes)

    sd = model.state_dict()
    out = dict(seed=np.int64(seed), steps=np.int64(steps), keys=np.array(list(sd.keys())), names=np.array(NAMES), feat=feat,
               offset=data32["offset"].numpy(), pair_margin=np.float64(pair), top2_margin=np.float64(top2),
               grad_names=np.array(list(hi_g.keys())), loss_names=np.array(list(hi_t.keys())),
               train_terms=np.array([float(hi_t[k]) for k in hi_t]), err_train_terms=np.array([abs(float(lo_t[k]) - float(hi_t[k])) for k in hi_t]),
               eval_terms=np.array([float(ev64[k]) for k in hi_t]), err_eval_terms=np.array([abs(float(ev[k]) - float(ev64[k])) for k in hi_t]),
               pred_masks=np.packbits(ev["pred_masks"].numpy().astype(bool), axis=1), pred_classes=ev["pred_classes"].numpy(),
               pred_scores=ev64["pred_scores"].numpy(), err_pred_scores=(ev["pred_scores"].double() - ev64["pred_scores"]).abs().numpy(),
               table_idx=log["idx"], table_start_len=log["start_len"], table_labels=log["labels"], cluster_idxs=log["cluster_idxs"],
               cluster_offsets=log["cluster_offsets"], component_sizes=log["component_sizes"],
               ap_all=np.array([ap["all_ap"], ap["all_ap_50%"], ap["all_ap_25%"]]),
               ap_classes=np.array([[ap["classes"][n][k] for k in ("ap", "ap50%", "ap25%")] for n in hook.valid_class_names]),
               ap_class_names=np.array(hook.valid_class_names))
    for i, (k, v) in enumerate(sd.items()):
        out[f"weight_{i}"] = v.numpy()
    for i, k in enumerate(hi_g):
        out[f"grad_{i}"] = hi_g[k].numpy()
        out[f"err_grad_{i}"] = np.float64((lo_g[k].double() - hi_g[k]).abs().max())
    for s, ((coord, segment, instance), p) in enumerate(zip(raw, parsed)):
        out[f"raw_coord_{s}"], out[f"raw_segment_{s}"], out[f"raw_instance_{s}"] = coord, segment, instance
        out[f"instance_{s}"], out[f"centroid_{s}"], out[f"bbox_{s}"] = p["instance"], p["instance_centroid"], p["bbox"]
    path = os.path.join(HERE, "model_pointgroup_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(ev["pred_scores"]), "proposals; AP", out["ap_all"])
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

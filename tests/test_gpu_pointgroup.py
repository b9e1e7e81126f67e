"""GPU suite of PG-v1m1: the kernels of csrc/point_group.hip against the host restatement of pointcloudpdf_amd/pointgroup_ops (every
coordinate a multiple of 0.25 and radius 1.5, so every squared distance is exact in fp32 with or without contraction), the proposal stage
and the bias losses against their torch compositions evaluated in float64 (pointgroup_cases.bound), the intersection table against the
per-pair ``logical_and`` counts, and the model against the fixture of the reference's classes."""
import numpy as np
import pytest
import torch

import pointgroup_cases as pc
import test_pointgroup_cpu as cpu
from pointcloudpdf_amd import _native, data_path, engine, evaluator, point_group, pointgroup_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return np.load(pc.GOLDEN, allow_pickle=False)


def device_table(xyz, ends):
    b, off = pc.batch_vectors(ends)
    return pointgroup_ops.ballquery_batch_p(torch.from_numpy(xyz).to(DEV), torch.from_numpy(b).to(DEV), torch.from_numpy(off).to(DEV), pc.RADIUS, 300)


def host_table(xyz, ends):
    b, off = pc.batch_vectors(ends)
    return pointgroup_ops.ballquery_batch_p_host(xyz, b, off, pc.RADIUS)


def check_table(xyz, ends):
    """Rows bit-equal to the restatement, starts = the exclusive scan of the counts."""
    idx, start_len = device_table(xyz, ends)
    assert idx.dtype == torch.int32 and start_len.dtype == torch.int32 and idx.is_cuda and start_len.is_cuda
    want_idx, want_sl = host_table(xyz, ends)
    assert np.array_equal(start_len.cpu().numpy(), want_sl)
    assert np.array_equal(start_len[:, 0].cpu().numpy(), np.cumsum(want_sl[:, 1]) - want_sl[:, 1])
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    return idx, start_len


def device_clusters(label, idx, start_len, threshold):
    out, off = pointgroup_ops.bfs_cluster(torch.as_tensor(label, dtype=torch.int32).to(DEV), idx, start_len, threshold)
    assert out.dtype == torch.int32 and off.dtype == torch.int32 and out.is_cuda and out.dim() == 2 and out.shape[1] == 2
    return out.cpu().numpy(), off.cpu().numpy()


def check_clusters(label, idx, start_len, threshold):
    out, off = device_clusters(label, idx, start_len, threshold)
    want, want_off = pointgroup_ops.bfs_cluster_host(np.asarray(label), idx.cpu().numpy(), start_len.cpu().numpy(), threshold)
    assert pc.same_clusters(out, off, want, want_off)
    for c in range(len(off) - 1):
        assert np.all(np.diff(out[off[c]:off[c + 1], 1]) > 0)   # ascending index inside a cluster
    return out, off


def test_strict_radius():
    xyz, ends, rows = pc.scene_strict_radius()
    idx, start_len = check_table(xyz, ends)
    s, l = start_len[0].tolist()
    assert idx[s:s + l].tolist() == rows[0]        # 1.25 and 1.479 inside, exactly 1.5 outside
    assert start_len[8].tolist()[1] == 1           # the far point sees itself


def test_saturation_and_direction():
    xyz, ends = pc.scene_saturation()
    idx, start_len = check_table(xyz, ends)
    sl = start_len.cpu().numpy()
    saturated = np.nonzero(sl[:, 1] == 1000)[0]
    assert saturated.tolist() == list(range(1200)) + [1260]
    table = idx.cpu().numpy()
    for r in saturated:
        assert np.array_equal(table[sl[r, 0]:sl[r, 0] + 1000], np.arange(1000))
    out, off = check_clusters(np.zeros(len(xyz), np.int32), idx, start_len, 50)
    assert np.diff(off).tolist() == [1000, 60, 70]
    members = [set(out[off[c]:off[c + 1], 1].tolist()) for c in range(3)]
    assert members[0] == set(range(1000)) and members[1] == set(range(1200, 1260)) and members[2] == set(range(1261, 1331))
    clustered = set().union(*members)
    assert not clustered & set(range(1000, 1200)) and 1260 not in clustered and 1331 not in clustered


def test_label_split():
    xyz, ends, label = pc.scene_label_split()
    idx, start_len = check_table(xyz, ends)
    out, off = check_clusters(label, idx, start_len, 50)
    assert np.diff(off).tolist() == [60, 60]
    assert out[0, 1] == 0 and out[off[1], 1] == 1      # ordered by their smallest index
    assert set(label[out[:60, 1]]) == {5} and set(label[out[60:, 1]]) == {2}


def test_threshold_edges():
    xyz, ends, sizes = pc.scene_threshold_edges()
    idx, start_len = check_table(xyz, ends)
    label = np.full(len(xyz), 2, np.int32)
    out, off = check_clusters(label, idx, start_len, 50)
    assert np.diff(off).tolist() == [50, 100, 101]     # 49 dropped under >= 50
    prob = torch.zeros((len(xyz), 4), device=DEV)
    prob[:, 2] = 0.5
    res = _native.hip_backend().pg_proposals(torch.from_numpy(out).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(label).to(DEV), None, prob,
                                             100, want_masks=True)
    assert res["offsets"].tolist() == [0, 101] and res["classes"].tolist() == [2] and res["scores"].tolist() == [0.5]   # 100 dropped under > 100
    assert res["masks"].sum().item() == 101 and res["masks"][0, -101:].all()


def test_long_chain_converges_after_more_than_one_batch_of_rounds():
    xyz, ends = pc.scene_chain()
    idx, start_len = check_table(xyz, ends)
    label = torch.zeros(len(xyz), dtype=torch.int32, device=DEV)
    out, off, stats = _native.hip_backend().pg_cluster(label, idx, start_len, 50, with_stats=True)
    assert off.tolist() == [0, 3000] and out[:, 1].tolist() == list(range(3000)) and (out[:, 0] == 0).all()
    assert (stats["labels"] == 0).all()
    assert 4 < stats["rounds"] <= 3001, stats["rounds"]   # the first batch is 4 rounds; n + 1 is the bound


def test_empty_and_tiny():
    e = torch.zeros((0, 3), device=DEV)
    idx, start_len = pointgroup_ops.ballquery_batch_p(e, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), 1.5, 300)
    assert idx.shape == (0,) and start_len.shape == (0, 2) and idx.dtype == torch.int32 and start_len.dtype == torch.int32
    out, off = pointgroup_ops.bfs_cluster(torch.zeros(0, dtype=torch.int32, device=DEV), idx, start_len, 50)
    assert out.shape == (0, 2) and off.tolist() == [0] and out.dtype == torch.int32 and off.dtype == torch.int32
    # a one-point scene
    idx, start_len = check_table(np.zeros((1, 3), np.float32), [1])
    assert idx.tolist() == [0] and start_len.tolist() == [[0, 1]]
    out, off = device_clusters(np.zeros(1, np.int32), idx, start_len, 1)
    assert out.tolist() == [[0, 0]] and off.tolist() == [0, 1]
    out, off = device_clusters(np.zeros(1, np.int32), idx, start_len, 2)
    assert out.shape == (0, 2) and off.tolist() == [0]
    # every point ignored: the model's empty branch
    prob = torch.zeros((40, 3), device=DEV)
    prob[:, 0] = 1
    res = point_group.proposals(torch.zeros((40, 3), device=DEV), prob.argmax(1), prob, torch.tensor([40], device=DEV), (-1, 0, 1), 1.5, 50, 100)
    assert res["masks"].shape == (0, 40) and res["masks"].dtype == torch.int32 and res["scores"].shape == (0,) and res["classes"].shape == (0,)
    assert res["offsets"].tolist() == [0] and (res["proposal_of"] == -1).all()


def test_tables_are_bit_equal_to_the_restatement_and_reproducible():
    xyz, ends = pc.scene_random()
    idx, start_len = check_table(xyz, ends)
    assert int(start_len[:, 1].max()) == 1000 and int(start_len[:, 1].min()) >= 1    # saturated rows next to unsaturated ones
    idx2, start_len2 = device_table(xyz, ends)
    assert torch.equal(idx, idx2) and torch.equal(start_len, start_len2)
    rng = np.random.default_rng(5)
    label = rng.integers(2, 4, len(xyz)).astype(np.int32)
    a = check_clusters(label, idx, start_len, 5)
    b = device_clusters(label, idx, start_len, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_random_directed_graphs_cluster_like_the_bfs():
    rng = np.random.default_rng(8)
    for _ in range(20):
        label, idx, start_len = pc.random_graph(rng)
        check_clusters(label, torch.from_numpy(idx).to(DEV), torch.from_numpy(start_len).to(DEV), int(rng.integers(1, 4)))


def _proposal_inputs(seed=21, n=2600, k=5):
    rng = np.random.default_rng(seed)
    sizes = [30, 101, 100, 400, 260, 99, 150]
    members = rng.permutation(n)[:sum(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cluster_idxs = np.stack([np.repeat(np.arange(len(sizes)), sizes), members], 1).astype(np.int32)
    for c in range(len(sizes)):
        cluster_idxs[off[c]:off[c + 1], 1].sort()
    logits = torch.from_numpy(rng.normal(0, 2, (n, k)).astype(np.float32))
    segment_pred = torch.from_numpy(rng.integers(0, k, n))
    for c in range(len(sizes)):
        segment_pred[cluster_idxs[off[c]:off[c + 1], 1]] = c % k
    return torch.from_numpy(cluster_idxs), torch.from_numpy(off), segment_pred, logits


def test_proposal_scores_and_masks_equal_the_composition():
    cluster_idxs, off, segment_pred, logits = _proposal_inputs()
    prob32, prob64 = torch.softmax(logits, -1), torch.softmax(logits.double(), -1)
    s32, masks, classes = point_group.proposals_composition(cluster_idxs, off, segment_pred, prob32, 100)
    s64, _, _ = point_group.proposals_composition(cluster_idxs, off, segment_pred, prob32.double(), 100)   # the same fp32 values, summed in float64
    res = _native.hip_backend().pg_proposals(cluster_idxs.to(DEV), off.to(DEV), segment_pred.int().to(DEV), None, prob32.to(DEV), 100, want_masks=True)
    assert torch.equal(res["masks"].cpu(), masks) and torch.equal(res["classes"].cpu(), classes) and res["scores"].dtype == torch.float32
    assert res["offsets"].tolist() == [0, 101, 501, 761, 911]
    for p in range(len(s64)):
        e, b = pc.err(res["scores"][p], s64[p]), pc.bound(abs(float(s32[p]) - float(s64[p])), s64[p])
        assert e <= b, (p, e, b)
    of = res["proposal_of"].cpu()
    assert torch.equal(of >= 0, masks.sum(0) > 0) and torch.equal(of[of >= 0].long(), masks.argmax(0)[of >= 0])
    compact = _native.hip_backend().pg_proposals(cluster_idxs.to(DEV), off.to(DEV), segment_pred.int().to(DEV), None, prob32.to(DEV), 100)
    assert compact["masks"] is None and torch.equal(compact["scores"], res["scores"]) and torch.equal(compact["members"], res["members"])
    del prob64


def _bias_inputs(n, dtype, seed=31, all_masked=False):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, 3, generator=g)
    coord = torch.randn(n, 3, generator=g) * 3
    centroid = (coord + torch.randn(n, 3, generator=g) * 0.3).to(dtype)
    instance = torch.randint(-1, 6, (n,), generator=g)
    pred[min(5, n - 1)] = 0                      # a zero-norm bias_pred row
    pred[min(7, n - 1), 1] = (centroid - coord)[min(7, n - 1), 1].float()   # |pred - gt| on its kink in one coordinate
    if all_masked:
        instance[:] = -1
    return pred, coord, centroid, instance


def _bias_eval(fn, pred, coord, centroid, instance, weights=(1.0, 0.7)):
    p = pred.clone().requires_grad_()
    l1, cos = fn(p, coord, centroid, instance, -1)
    (weights[0] * l1 + weights[1] * cos).backward()
    return l1.detach(), cos.detach(), p.grad


@pytest.mark.parametrize("n", [1, 257, 70001])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_bias_loss_node_matches_the_float64_evaluation(n, dtype):
    """1 row; more than one workgroup; more rows than one sweep of the 1,024 workgroup slots covers in one pass."""
    pred, coord, centroid, instance = _bias_inputs(n, dtype)
    ref = _bias_eval(point_group.bias_losses_composition, pred.double(), coord.double(), centroid.double(), instance)
    own = _bias_eval(point_group.bias_losses_composition, pred, coord, centroid, instance)       # the reference's own precision
    dev = _bias_eval(point_group.bias_losses, *(t.to(DEV) for t in (pred, coord, centroid, instance)))
    assert dev[0].dtype == dtype and dev[1].dtype == dtype and dev[2].dtype == torch.float32     # torch's promotion
    again = _bias_eval(point_group.bias_losses, *(t.to(DEV) for t in (pred, coord, centroid, instance)))
    for a, b in zip(dev, again):
        assert torch.equal(a, b)
    for name, d, o, r in zip(("l1", "cosine", "grad"), dev, own, ref):
        e, b = pc.err(d, r), pc.bound(pc.err(o, r), r)
        print(f"{name} n={n} {dtype}: |error| {e:.3e}, the composition's own {pc.err(o, r):.3e}, bound {b:.3e}")
        assert e <= b, (name, e, b)
    assert torch.isfinite(dev[2]).all()                 # the zero-norm row included


def test_bias_loss_node_with_every_row_masked():
    pred, coord, centroid, instance = _bias_inputs(300, torch.float64, all_masked=True)
    l1, cos, grad = _bias_eval(point_group.bias_losses, *(t.to(DEV) for t in (pred, coord, centroid, instance)))
    assert float(l1) == 0.0 and float(cos) == 0.0 and not grad.any()      # 0 / (0 + 1e-8)


def test_bias_loss_node_records_without_memset_nodes():
    tensors = [t.to(DEV) for t in _bias_inputs(5000, torch.float64)]

    def run():
        return list(_bias_eval(point_group.bias_losses, *tensors))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [t.clone() for t in run()]
    s.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        static = run()
    census = engine.graph_node_census(g.raw_cuda_graph())
    assert census["kernel"] >= 3 and census["memset"] == 0, census
    for t in static:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)


def test_intersection_table_equals_the_per_pair_counts():
    rng = np.random.default_rng(41)
    n, m, p = 3000, 4100, 6
    of = rng.integers(-1, p, n).astype(np.int32)
    of[of == 4] = -1                                  # proposal 4 exists but owns no point
    index_map = rng.integers(0, n, m)
    instance = rng.integers(-1, 9, m) * 7
    segment = rng.integers(-1, 5, m)
    void_only = of[index_map] == 5                    # proposal 5 meets void points only
    segment[void_only] = 0
    ev = evaluator.InsSegEvaluator(5, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-7)
    for mapped in (True, False):
        seg, inst = (segment, instance) if mapped else (segment[:n], instance[:n])
        got = ev.intersection_table(torch.from_numpy(of).to(DEV), p, torch.from_numpy(seg).to(DEV), torch.from_numpy(inst).to(DEV),
                                    torch.from_numpy(index_map).to(DEV) if mapped else None)
        host = ev.intersection_table(torch.from_numpy(of), p, torch.from_numpy(seg), torch.from_numpy(inst),
                                     torch.from_numpy(index_map) if mapped else None)
        ids, _, counts, table, vert, voidc = got
        where = of[index_map] if mapped else of
        void_mask = np.isin(seg, (-1, 0, 1))
        for q in range(p):
            mask = where == q
            assert vert[q] == np.count_nonzero(mask) and voidc[q] == np.count_nonzero(np.logical_and(void_mask, mask))
            for gi, gid in enumerate(ids):
                assert table[q, gi] == np.count_nonzero(np.logical_and(inst == gid, mask))
        assert vert[4] == 0 and (not mapped or (vert[5] > 0 and voidc[5] == vert[5]))
        assert np.array_equal(counts, np.unique(inst, return_counts=True)[1])
        for a, b in zip(got, host):
            assert np.array_equal(a, b)


def test_model_on_the_fixture(golden):
    g = golden
    data = cpu.batch(g, DEV)
    cpu.check_train(g, cpu.build_model(g, DEV), data)
    model = cpu.build_model(g, DEV)
    assert list(model.state_dict().keys()) == [str(k) for k in g["keys"]]
    out = cpu.check_eval(g, model, data)              # masks and classes exact, every proposal
    # the compact proposals say what the masks say
    of = out["proposal_of"].cpu()
    assert torch.equal(of >= 0, out["pred_masks"].sum(0) > 0) and torch.equal(of[of >= 0].long(), out["pred_masks"].argmax(0)[of >= 0])
    assert out["proposal_offsets"].tolist() == np.concatenate([[0], np.cumsum(out["pred_masks"].sum(1).numpy())]).tolist()
    # and the evaluator reaches the reference's APs from them, on the device
    ev = evaluator.InsSegEvaluator(pc.NUM_CLASSES, [str(n) for n in g["names"]], segment_ignore_index=pc.IGNORE, instance_ignore_index=-1)
    cpu.scene_updates(g, ev, data, out)
    cpu.ap_check(g, ev.summary())
    # device instance_parser: ids, boxes and classes exact, the centroid within the rounding of the reference's own float32 sum
    for s in range(len(g["offset"])):
        raw = [torch.from_numpy(g[f"raw_{k}_{s}"]).to(DEV) for k in ("coord", "segment", "instance")]
        parsed = data_path.instance_parser(*raw, segment_ignore_index=pc.IGNORE, instance_ignore_index=-1)
        assert torch.equal(parsed["instance"].cpu(), torch.from_numpy(g[f"instance_{s}"]))
        assert np.array_equal(parsed["bbox"].cpu().numpy(), g[f"bbox_{s}"])                        # min / max / class: exact
        # the reference's mean is a row-by-row float32 sum of k <= 400 terms: off the exact mean by at most k 2^-24 max|x|, as ours is by one rounding
        want, k = g[f"centroid_{s}"], int(np.bincount(g[f"instance_{s}"][g[f"instance_{s}"] >= 0]).max())
        assert np.abs(parsed["instance_centroid"].cpu().numpy() - want).max() <= (k + 1) * 2.0 ** -24 * np.abs(g[f"raw_coord_{s}"]).max()


SCANNET_MODEL = dict(   # the `model` section of configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py
    type="PG-v1m1",
    backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0, channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2)),
    backbone_out_channels=96, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1,
    cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50)


def test_scannet_recipe_trains_and_evaluates_over_the_real_backbone():
    rng = np.random.default_rng(51)
    sizes = (1600, 1400)
    grids, segs, insts = [], [], []
    for n in sizes:
        cells = rng.permutation(24 ** 3)[:n]
        grid = np.stack([cells // 576, (cells // 24) % 24, cells % 24], 1)
        grids.append(grid)
        blob = (grid[:, 0] // 8) * 3 + grid[:, 1] // 8          # 9 slabs as instances
        segs.append(np.where(blob < 2, blob, 2 + blob % 5))      # two of them of the ignored classes
        insts.append(blob)
    grid = torch.from_numpy(np.concatenate(grids).astype(np.int32)).to(DEV)
    coord = grid.float() * 0.02
    segment, instance = torch.from_numpy(np.concatenate(segs)).to(DEV), torch.from_numpy(np.concatenate(insts)).to(DEV)
    offset = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=DEV)
    parsed = data_path.instance_parser(coord, segment, instance, offset=offset)
    batch = dict(coord=coord, grid_coord=grid, feat=torch.from_numpy(rng.uniform(-1, 1, (sum(sizes), 6)).astype(np.float32)).to(DEV), offset=offset,
                 segment=segment, instance=parsed["instance"], instance_centroid=parsed["instance_centroid"])
    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=SCANNET_MODEL)).to(DEV)
    step.train()
    out = step(batch)
    assert set(out) == {"loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"} and out["loss"].dtype == torch.float64
    out["loss"].backward()
    for name, p in step.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(step.model.bias_head[3].weight.grad.abs().max()) > 0
    step.eval()
    with torch.no_grad():
        ev = step(batch)
    n = sum(sizes)
    assert ev["pred_masks"].shape[1] == n and ev["pred_masks"].dtype == torch.int32 and ev["proposal_of"].shape == (n,)
    assert ev["pred_masks"].shape[0] == ev["pred_scores"].shape[0] == ev["pred_classes"].shape[0] == ev["proposal_offsets"].shape[0] - 1
    assert torch.isfinite(ev["loss"])


def test_model_empty_branch_on_the_device(golden):
    """Every predicted class ignored: the device branch returns the reference's empty outputs (torch.tensor([]) twice, a (0, N) int32 mask)."""
    model, data = cpu.build_model(golden, DEV).eval(), cpu.batch(golden, DEV)
    model.segment_ignore_index = tuple(range(-1, pc.NUM_CLASSES))
    with torch.no_grad():
        out = model(dict(data))
    n = data["coord"].shape[0]
    assert out["pred_masks"].shape == (0, n) and out["pred_masks"].dtype == torch.int32 and out["pred_masks"].device.type == "cpu"
    for key in ("pred_scores", "pred_classes"):
        assert out[key].shape == (0,) and out[key].dtype == torch.float32 and out[key].device.type == "cpu"
    assert out["proposal_offsets"].tolist() == [0] and out["proposal_members"].shape == (0,) and (out["proposal_of"] == -1).all()
    ev = evaluator.InsSegEvaluator(pc.NUM_CLASSES, segment_ignore_index=pc.IGNORE)
    ev.update(out, dict(segment=data["segment"], instance=data["instance"]))
    assert ev.summary()["all_ap"] == 0.0          # instances, no proposal


def test_evaluator_carries_proposals_to_the_original_cloud(golden):
    """``update`` with ``origin_coord``: every original point takes the proposal of its nearest evaluated point (pointops.knn_query, k = 1).
    The original cloud holds every evaluated point of the first scene twice, the copy nudged by far less than the point spacing and given
    labels of its own; the same records must come out of the host path fed with the brute-force nearest neighbour."""
    g = golden
    data = cpu.batch(g, DEV)
    model = cpu.build_model(g, DEV).eval()
    with torch.no_grad():
        out = model(dict(data))
    e = int(g["offset"][0])
    rng = np.random.default_rng(61)
    coord = data["coord"][:e]
    origin = torch.cat([coord, coord + torch.from_numpy(rng.uniform(-1e-4, 1e-4, (e, 3)).astype(np.float32)).to(DEV)])
    seg = torch.cat([data["segment"][:e], data["segment"][:e]])
    inst = torch.cat([data["instance"][:e], torch.where(data["instance"][:e] >= 0, data["instance"][:e] + 50, data["instance"][:e])])
    pred = dict(pred_classes=out["pred_classes"], pred_scores=out["pred_scores"], proposal_of=out["proposal_of"][:e])
    ev = evaluator.InsSegEvaluator(pc.NUM_CLASSES, segment_ignore_index=pc.IGNORE)
    ev.update(pred, dict(coord=coord, offset=torch.tensor([e], device=DEV), segment=data["segment"][:e], instance=data["instance"][:e],
                         origin_coord=origin, origin_offset=torch.tensor([2 * e], device=DEV), origin_segment=seg, origin_instance=inst))
    nearest = torch.cdist(origin.double().cpu(), coord.double().cpu()).argmin(1)
    assert torch.equal(nearest, torch.arange(e).repeat(2))          # (the nudge never changes the nearest point)
    host = evaluator.InsSegEvaluator(pc.NUM_CLASSES, segment_ignore_index=pc.IGNORE)
    want = host.associate_instances(dict(pred, proposal_of=out["proposal_of"][:e].cpu()), seg.cpu(), inst.cpu(), nearest)
    got = ev.scenes[0]
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    base = host.associate_instances(dict(pred, proposal_of=out["proposal_of"][:e].cpu()), data["segment"][:e].cpu(), data["instance"][:e].cpu())
    assert np.array_equal(got["pr_size"], 2 * base["pr_size"]) and np.array_equal(got["pr_void"], 2 * base["pr_void"])
    assert got["inter"].sum() > 0 and len(got["gt_size"]) == 2 * len(np.unique(g["instance_0"][g["instance_0"] >= 0]))

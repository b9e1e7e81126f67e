"""GPU suite of the precise tester with a StratifiedTransformer: the per-scene window keys and bounds of csrc/window_edges.hip against
their torch composition, the grouped pre-pass and the look-ahead with one origin per fragment, batched fragments against single ones and
against tests/golden/tester_st_ref.npz (the reference's own classes, make_golden_st_tester.py), and OpenSegTester end to end."""
import os

import numpy as np
import pytest
import torch

import st_tester_common as C
from helpers import assert_close

pytestmark = pytest.mark.gpu

SIZES = [1500, 1, 2049]   # a one-point scene, a scene one past a 2,048 boundary
S3DIS_ST_TEST = dict(   # configs/s3dis/openseg-st-v1m1-0-origin-msp.py (the section the config keeps as a comment), two aug_transform lists
    type="S3DISDataset", split="Area_5", data_root="data/s3dis",
    transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
    test_mode=True, unknown_label=[5, 9],
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="test", keys=("coord", "color"), return_grid_coord=True),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=("coord", "color"))],
        aug_transform=[[dict(type="RandomScale", scale=[0.9, 0.9])], [dict(type="RandomScale", scale=[1, 1]), dict(type="RandomFlip", p=1)]]))


@pytest.fixture(scope="module")
def be():
    from pointcloudpdf_amd import _native

    assert torch.cuda.is_available()
    return _native.hip_backend()   # raises if libpdfops.so is missing: no fallback


@pytest.fixture(scope="module")
def model(be):
    return C.tiny_model("cuda")


@pytest.fixture(scope="module")
def host_tables(oracle_backend):
    """Per level (0, 1): the 3-scene batch and its scene-origin tables from the torch composition on host tensors."""
    from pointcloudpdf_amd import _native

    prev = _native._set_backend_for_testing(oracle_backend)
    try:
        cpu = C.tiny_model("cpu").backbone
        out = {}
        for level in (0, 1):
            layer = cpu.layers[level]
            xyz, offset, ends = C.three_scenes(SIZES, layer.window_size, seed=3 + level)
            ds, _ = C.key_subset(ends)
            out[level] = dict(xyz=xyz, offset=offset, ends=ends, ds=ds, tables=layer.window_tables(xyz, offset, ds, origin="scene"))
        return out
    finally:
        _native._set_backend_for_testing(prev)


@pytest.mark.parametrize("level", [0, 1])
def test_scene_keys_kernel_builds_the_tables_of_the_torch_composition(be, model, host_tables, level):
    from pointcloudpdf_amd import stratified

    h = host_tables[level]
    layer = model.backbone.layers[level]
    assert layer.window_size == (0.16, 0.32)[level]
    xyz, offset, ds = h["xyz"].cuda(), h["offset"].cuda(), h["ds"].cuda()
    got = layer.window_tables(xyz, offset, ds, origin="scene")
    lo, hi = be.scene_bounds(xyz, offset)
    ws = torch.tensor([layer.window_size] * 3)
    for parity in (0, 1):
        assert C.tables_equal(C.restrict(got[parity], 0, xyz.shape[0]), C.restrict(h["tables"][parity], 0, xyz.shape[0])), (level, parity)
        assert got[parity][3] == h["tables"][parity][3]
        keys = be.window_keys(xyz, offset, lo, hi, layer.window_size, parity, per_scene=True)
        want = stratified.window_keys_scene(h["xyz"], h["offset"], ws, parity)
        for name, a, b in zip(("kf", "kc", "wk"), keys, want):
            assert torch.equal(a.cpu(), b), (level, parity, name)
    with pytest.raises(ValueError, match="per_scene"):
        be.window_keys(xyz, offset, lo[0], hi[0], layer.window_size, 0, per_scene=True)


def test_scene_bounds_kernel_is_exact(be, host_tables):
    for level in (0, 1):
        h = host_tables[level]
        lo, hi = be.scene_bounds(h["xyz"].cuda(), h["offset"].cuda())
        assert lo.shape == hi.shape == (3, 3) and lo.dtype == torch.float32
        for s, (a, z) in enumerate(zip([0] + h["ends"][:-1], h["ends"])):
            mn, mx = torch.aminmax(h["xyz"][a:z], dim=0)
            assert torch.equal(lo[s].cpu(), mn) and torch.equal(hi[s].cpu(), mx), (level, s)
    # rows that are no multiple of the workgroup's stride, a scene shorter than one wave, an empty scene
    g = torch.Generator().manual_seed(9)
    xyz = (torch.randn(5000, 3, generator=g) * 3).cuda()
    ends = [769, 769, 800, 5000]
    lo, hi = be.scene_bounds(xyz, torch.tensor(ends, dtype=torch.int32, device="cuda"))
    for s, (a, z) in enumerate(zip([0] + ends[:-1], ends)):
        if z > a:
            mn, mx = torch.aminmax(xyz[a:z], dim=0)
            assert torch.equal(lo[s], mn) and torch.equal(hi[s], mx), s
        else:
            assert not lo[s].any() and not hi[s].any()


def _same_geometry(got, alone):
    assert set(got.samples) == set(alone.samples) and set(got.windows) == set(alone.windows) == {0, 1, 2, 3}
    for k in alone.samples:
        assert torch.equal(got.samples[k][0], alone.samples[k][0]) and torch.equal(got.samples[k][1], alone.samples[k][1]), k
    for lv in alone.windows:
        for parity, tab in alone.windows[lv].items():
            for x, y in zip(tab, got.windows[lv][parity]):
                assert torch.equal(x, y) if torch.is_tensor(x) else x == y, (lv, parity)
    assert set(got.neighbors) == set(alone.neighbors) == {("ball",)} | {(kind, l) for kind in ("td", "up") for l in range(3)}
    for k, v in alone.neighbors.items():
        for x, y in zip(v if isinstance(v, tuple) else (v,), got.neighbors[k] if isinstance(v, tuple) else (got.neighbors[k],)):
            assert torch.equal(x, y), k


def test_scene_origin_group_prepass_is_the_per_batch_prepass(model):
    from pointcloudpdf_amd import stratified, synthetic

    bb = model.backbone
    batches = [synthetic.make_batch(sz, first_scene_id=80 + 7 * i, device="cuda") for i, sz in enumerate([[900, 700], [1200], [300, 410, 250]])]
    for b in batches:   # (every synthetic scene starts at 0: move scene s by 0.37 s level-0 windows in x / y, so that the origins differ)
        for s, (a, z) in enumerate(zip([0] + b["offset_host"][:-1], b["offset_host"])):
            b["coord"][a:z, :2] += 0.37 * s * 0.16
    geoms = [bb.make_geometry(b["coord"], b["offset"], b["offset_host"], window_origin="scene") for b in batches]
    stratified.StratifiedGeometry.precompute_group(geoms, bb.layers_by_level())
    pf = stratified.StratifiedPrefetcher(bb, window_origin="scene")
    try:
        tickets = pf.submit_group(batches)
        coupled = False
        for b, g, t in zip(batches, geoms, tickets):
            alone = bb.make_geometry(b["coord"], b["offset"], b["offset_host"], window_origin="scene").precompute(bb.layers_by_level())
            threaded = pf.get(t)
            torch.cuda.synchronize()
            assert g.window_origin == threaded.window_origin == "scene"
            _same_geometry(g, alone)
            _same_geometry(threaded, alone)
            default = bb.make_geometry(b["coord"], b["offset"], b["offset_host"]).precompute(bb.layers_by_level())
            coupled = coupled or not torch.equal(default.windows[0][0][1], alone.windows[0][0][1])
        assert coupled   # (the batch origin gives other tables for at least one multi-scene batch: the argument is not ignored)
    finally:
        pf.close()


@pytest.fixture(scope="module")
def gpu_runs(model, golden_dir):
    ref = C.load_ref(golden_dir)
    scene = C.ref_scene(ref)
    with torch.no_grad():
        return dict(ref=ref, inline=C.run_scene_tester(model, scene, "cuda", 1, group=0), ahead=C.run_scene_tester(model, scene, "cuda", 1, group=2),
                    three=C.run_scene_tester(model, scene, "cuda", 3))


def test_look_ahead_votes_are_the_inline_votes(gpu_runs):
    a, b = gpu_runs["inline"], gpu_runs["ahead"]
    assert len(a["logits"]) == len(b["logits"]) == 3
    assert all(g is not None and g.window_origin == "scene" and len(g.windows) == 4 for g in a["geometry"] + b["geometry"])
    assert torch.equal(a["votes"], b["votes"]) and torch.equal(a["pred"], b["pred"]) and torch.equal(a["score"], b["score"])
    for x, y in zip(a["logits"], b["logits"]):
        assert torch.equal(x, y)


def test_batched_fragments_vote_like_single_fragments_on_gpu(gpu_runs):
    one, three, ref = gpu_runs["inline"], gpu_runs["three"], gpu_runs["ref"]
    assert len(three["logits"]) == 1 and three["geometry"][0] is not None
    C.check_votes_agree(three["votes"], one["votes"])
    for tag, run in (("one", one), ("three", three)):
        logits = torch.cat(run["logits"]).reshape(3, -1, C.K)
        index = torch.cat([b[0] for b in run["batches"]]).reshape(3, -1)
        for f in range(3):
            assert np.array_equal(index[f].cpu().numpy(), ref[f"frag{f}/index"].astype(np.int64)), (tag, f)
            assert_close(logits[f], ref[f"frag{f}/logits"], 1e-4, f"{tag}: logits of fragment {f}")
        assert_close(run["votes"], ref["votes"], 1e-4, f"{tag}: votes")
        C.check_votes_agree(run["votes"], torch.from_numpy(ref["votes"]))


def test_openseg_tester_runs_the_st_recipe_end_to_end(be, golden_dir, tmp_path):
    from pointcloudpdf_amd import engine
    from pointcloudpdf_amd.testing import IncrSegTester, OpenSegTester

    torch.manual_seed(0)
    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).cuda()
    cfg = dict(data=dict(num_classes=13, ignore_index=-1, test=S3DIS_ST_TEST), unknown_label=[5, 9], fragments_per_batch=3, group=2)
    scene = C.ref_scene(C.load_ref(golden_dir))
    tester = OpenSegTester(step, cfg)
    try:
        assert tester.scene_tester.st_backbone is step.model.backbone
        out = tester.test([scene], save_path=str(tmp_path))
        for k in ("mIoU", "mAcc", "allAcc", "aupr", "auroc", "all_aupr", "all_auroc"):
            assert np.isfinite(out[k]), (k, out[k])
        assert np.isfinite(out["iou_class"]).all() and np.isfinite(out["acc_class"]).all()
        pred, score = tester.scene_tester.run(scene)
        saved = np.load(os.path.join(str(tmp_path), "result", "golden_st_pred.npy"))
        assert np.array_equal(saved, pred.cpu().numpy()) and saved.shape[0] == scene["coord"].shape[0]
        assert score is not None and bool(torch.isfinite(score).all())
    finally:
        tester.close()
    with pytest.raises(NotImplementedError, match="PointTransformer-V1 only"):
        IncrSegTester(step.model, dict(data=dict(num_classes=13, test=S3DIS_ST_TEST), incr_label_remap={12: 12}))

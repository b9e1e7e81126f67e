"""CPU suite of the precise tester (pointcloudpdf_amd/testing.py: TestPipeline / SceneTester / OpenSegTester / IncrSegTester) on host
tensors -- the torch-op composition of the device steps -- against tests/golden/tester_ref.npz (the reference's own GridSample(mode="test"),
aug ops and post_transform on one small scene; make_golden_tester.py), plus the C ABI's argument validation of the three fragment entries."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from helpers import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 13
AUGS = [[dict(type="RandomScale", scale=[1, 1])], [dict(type="RandomScale", scale=[0.9, 0.9])],
        [dict(type="RandomScale", scale=[1.1, 1.1]), dict(type="RandomFlip", p=1)]]
# must match tests/golden/make_golden_tester.py: CASES
CASES = {
    "f32_center": dict(dtype=np.float32, normal=False, transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
                       post=dict(type="CenterShift", apply_z=False), keys=("coord", "color"), feat_keys=("coord", "color")),
    "f32_positive": dict(dtype=np.float32, normal=True, transform=[dict(type="PositiveShift"), dict(type="NormalizeColor", mode="zeroOne")],
                         post=dict(type="PositiveShift"), keys=("coord", "color", "normal"), feat_keys=("coord", "color", "normal")),
    "f64_center": dict(dtype=np.float64, normal=False, transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
                       post=dict(type="CenterShift", apply_z=False), keys=("coord", "color"), feat_keys=("coord", "color")),
}

# ---- the `test` sections of the reference's PDF configs, copied as literal dicts (settings only) -----------------------------------
S3DIS_INCRSEG_TEST = dict(   # configs/s3dis/incrseg-pt-v1-0-pointpdf-v1m1-base.py
    type="S3DISDataset", split="Area_5", data_root="data/s3dis",
    transform=[dict(type="PositiveShift"), dict(type="NormalizeColor", mode="zeroOne")],
    test_mode=True,
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="test", keys=("coord", "color"), return_grid_coord=True),
        crop=None,
        post_transform=[dict(type="PositiveShift"), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=("coord", "color"))],
        aug_transform=[[dict(type="RandomScale", scale=[1, 1])]]))
S3DIS_OPENSEG_TEST = dict(   # configs/s3dis/openseg-pt-v1-0-pointpdf-v1m1-base.py (the section the config keeps as a comment)
    type="S3DISDataset", split="Area_5", data_root="data/s3dis",
    transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
    test_mode=True, unknown_label=[5, 9],
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="test", keys=("coord", "color"), return_grid_coord=True),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=("coord", "color"))],
        aug_transform=[[dict(type="RandomScale", scale=[s, s])] for s in (0.9, 0.95, 1, 1.05, 1.1)]
        + [[dict(type="RandomScale", scale=[s, s]), dict(type="RandomFlip", p=1)] for s in (0.9, 0.95, 1, 1.05, 1.1)]))
_ROT = [dict(type="RandomRotateTargetAngle", angle=[a], axis="z", center=[0, 0, 0], p=1) for a in (0, 1 / 2, 1, 3 / 2)]
SCANNET_OPENSEG_TEST = dict(   # configs/scannet/openseg-pt-v1-0-pointpdf-v1m1-base.py (kept as a comment there as well)
    type="ScanNetDataset", split="val", data_root="data/scannet",
    transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
    test_mode=True,
    test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=0.02, hash_type="fnv", mode="test", keys=("coord", "color", "normal")),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "index"), feat_keys=("coord", "color", "normal"))],
        aug_transform=[[r] for r in _ROT] + [[r, dict(type="RandomScale", scale=[s, s])] for s in (0.95, 1.05) for r in _ROT]))


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(os.path.join(golden_dir, "tester_ref.npz"))


def case_cfg(case, grid_size):
    return dict(transform=case["transform"], test_mode=True, test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=grid_size, hash_type="fnv", mode="test", keys=case["keys"], return_grid_coord=True),
        crop=None, post_transform=[case["post"], dict(type="ToTensor"),
                                   dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=case["feat_keys"])],
        aug_transform=AUGS))


def case_scene(ref, case):
    scene = dict(coord=ref["scene/coord"].astype(case["dtype"]), color=ref["scene/color"], segment=ref["scene/segment"], name="golden")
    if case["normal"]:
        scene["normal"] = ref["scene/normal"]
    return scene


def fragment_digest(index, coord, feat, grid_coord):
    h = hashlib.sha256()
    for t, dt in ((index, torch.int64), (coord, torch.float32), (feat, torch.float32), (grid_coord, torch.int64)):
        assert t.dtype == dt
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def table_rows(aug, frag, rows):
    """tests/golden/make_golden_tester.py: logit_rows."""
    return (np.arange(rows, dtype=np.int64) * 2654435761 + frag * 40503 + aug * 97) % 1024


def check_fragments(ref, tag, batches):
    """Every fragment of every batch against the fixture: shapes, per-fragment digests (index / grid_coord / coord / feat exact), and
    the one fragment the fixture stores in full compared array by array (so that a mismatch says where)."""
    seen = {}
    for batch in batches:
        fr = batch["fragment"]
        v = batch["index"].shape[0] // fr["g"]
        assert batch["offset"].tolist() == [(k + 1) * v for k in range(fr["g"])] == batch["offset_host"]
        for k in range(fr["g"]):
            a, f, rows = fr["aug"], fr["f0"] + k, slice(k * v, (k + 1) * v)
            cmax, want_v = (int(x) for x in ref[f"{tag}/aug{a}/shape"])
            assert v == want_v and f < cmax
            if f"{tag}/aug{a}/index" in ref.files:
                assert np.array_equal(batch["index"][rows].cpu().numpy(), ref[f"{tag}/aug{a}/index"][f].astype(np.int64)), (tag, a, f, "index")
            if a == 2 and f == cmax - 1 and f"{tag}/sample/feat" in ref.files:
                assert np.array_equal(batch["index"][rows].cpu().numpy(), ref[f"{tag}/sample/index"].astype(np.int64))
                assert np.array_equal(batch["grid_coord"][rows].cpu().numpy(), ref[f"{tag}/sample/grid_coord"].astype(np.int64))
                assert np.array_equal(batch["feat"][rows].cpu().numpy(), ref[f"{tag}/sample/feat"]), (tag, "feat")
                assert np.array_equal(batch["coord"][rows].cpu().numpy(), ref[f"{tag}/sample/feat"][:, :3]), (tag, "coord")
            got = fragment_digest(batch["index"][rows], batch["coord"][rows], batch["feat"][rows], batch["grid_coord"][rows])
            assert np.array_equal(got, ref[f"{tag}/aug{a}/digest"][f]), (tag, a, f, "digest of index | coord | feat | grid_coord")
            seen[(a, f)] = True
    assert len(seen) == sum(int(ref[f"{tag}/aug{a}/shape"][0]) for a in range(len(AUGS)))   # every fragment, once


@pytest.mark.parametrize("tag,g", [("f32_center", 4), ("f32_center", 1), ("f32_positive", 5), ("f64_center", 3)])
def test_fragments_match_the_reference_pipeline(ref, tag, g):
    from pointcloudpdf_amd.testing import TestPipeline

    pipe = TestPipeline(case_cfg(CASES[tag], float(ref["grid_size"])))
    st = pipe.prepare(case_scene(ref, CASES[tag]), "cpu")
    assert st["coord"].dtype == (torch.float64 if tag == "f64_center" else torch.float32)
    check_fragments(ref, tag, pipe.batches(st, g))


def test_votes_pred_and_score_match_the_restated_tester(ref):
    from pointcloudpdf_amd.testing import SceneTester, TestPipeline

    logit_table, score_table = torch.from_numpy(ref["logit_table"]), torch.from_numpy(ref["score_table"])

    def forward(batch):
        fr = batch["fragment"]
        v = batch["index"].shape[0] // fr["g"]
        sel = torch.from_numpy(np.concatenate([table_rows(fr["aug"], fr["f0"] + k, v) for k in range(fr["g"])]))
        return logit_table[sel], score_table[sel]

    pipe = TestPipeline(case_cfg(CASES["f32_center"], float(ref["grid_size"])))
    tester = SceneTester(forward, K, pipe, fragments_per_batch=4, device="cpu")
    pred, score, votes = tester.run(case_scene(ref, CASES["f32_center"]), return_votes=True)
    assert_close(votes, ref["votes"], 1e-6, "votes")
    assert_close(score, ref["score"], 1e-6, "score")
    top2 = np.sort(ref["votes"], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-5                           # arg-max is demanded wherever the fixture's margin exceeds 1e-5
    assert (~clear).mean() <= 1e-3
    assert np.array_equal(pred.numpy()[clear], ref["pred"].astype(np.int64)[clear])
    # a forward that returns no score -> score None, same votes
    pred2, score2 = SceneTester(lambda b: (forward(b)[0], None), K, pipe, fragments_per_batch=16, device="cpu").run(case_scene(ref, CASES["f32_center"]))
    assert score2 is None and np.array_equal(pred2.numpy()[clear], ref["pred"].astype(np.int64)[clear])


def test_scene_level_grid_sample_returns_inverse(ref):
    """transform = [Copy, GridSample(train, return_inverse)]: the fragments come from the sub-sampled scene, predictions return on the full one."""
    from pointcloudpdf_amd.testing import SceneTester, TestPipeline

    cfg = case_cfg(CASES["f32_center"], 0.08)
    cfg["transform"] = [dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor"),
                        dict(type="Copy", keys_dict=dict(segment="origin_segment")),
                        dict(type="GridSample", grid_size=0.05, hash_type="fnv", mode="train", return_inverse=True, keys=("coord", "color", "segment"))]
    pipe = TestPipeline(cfg, generator=torch.Generator().manual_seed(3))
    scene = case_scene(ref, CASES["f32_center"])
    st = pipe.prepare(scene, "cpu")
    n, m = scene["coord"].shape[0], st["coord"].shape[0]
    assert m < n and st["inverse"].shape == (n,) and int(st["inverse"].max()) == m - 1 and st["origin_segment"].shape == (n,)
    assert st["segment"].shape == (m,) and st["color"].shape == (m, 3)
    kept = torch.unique(st["inverse"])
    assert kept.numel() == m                                            # every kept voxel is some point's voxel
    # the prediction of a point is the prediction of its voxel's kept point: label the fragments by their own point id modulo K
    onehot = lambda b: (torch.nn.functional.one_hot(b["index"] % K, K).float() * 20.0, None)
    pred, score = SceneTester(onehot, K, pipe, fragments_per_batch=3, device="cpu").run(scene)
    assert score is None and pred.shape == (n,)
    assert torch.equal(pred, (torch.arange(m) % K)[st["inverse"]])


def test_pipeline_accepts_the_reference_test_sections_and_refuses_what_it_cannot_run():
    import copy

    from pointcloudpdf_amd.testing import TestPipeline

    p = TestPipeline(S3DIS_INCRSEG_TEST)
    assert len(p.augs) == 1 and p.grid_size == 0.04 and p.feat_keys == ["coord", "color"] and p.return_grid_coord
    p = TestPipeline(S3DIS_OPENSEG_TEST)
    assert len(p.augs) == 10 and [len(a) for a in p.augs] == [1] * 5 + [2] * 5
    p = TestPipeline(SCANNET_OPENSEG_TEST)
    assert len(p.augs) == 12 and p.feat_keys == ["coord", "color", "normal"] and not p.return_grid_coord
    bad = copy.deepcopy(S3DIS_OPENSEG_TEST)
    bad["test_cfg"]["crop"] = dict(type="SphereCrop", point_max=100000, mode="all")
    with pytest.raises(NotImplementedError, match="sphere_crop"):
        TestPipeline(bad)
    bad = copy.deepcopy(S3DIS_OPENSEG_TEST)
    bad["test_cfg"]["aug_transform"][1] = [dict(type="RandomScale", scale=[0.9, 1.1])]
    with pytest.raises(ValueError, match="RandomScale"):
        TestPipeline(bad)
    bad = copy.deepcopy(S3DIS_OPENSEG_TEST)
    bad["test_cfg"]["aug_transform"][5][1] = dict(type="RandomFlip", p=0.5)
    with pytest.raises(ValueError, match="RandomFlip"):
        TestPipeline(bad)
    bad = copy.deepcopy(SCANNET_OPENSEG_TEST)
    bad["test_cfg"]["aug_transform"][0] = [dict(type="RandomRotateTargetAngle", angle=[0, 1 / 2], axis="z", center=[0, 0, 0], p=1)]
    with pytest.raises(ValueError, match="RandomRotateTargetAngle"):
        TestPipeline(bad)


def test_scannet_section_runs_and_rotations_permute_the_axes(ref):
    """RandomRotateTargetAngle by 0, 1/2, 1, 3/2 turns about the origin: fragments exist for every list and |coord| is preserved."""
    from pointcloudpdf_amd.testing import TestPipeline

    cfg = dict(SCANNET_OPENSEG_TEST, test_cfg=dict(SCANNET_OPENSEG_TEST["test_cfg"], voxelize=dict(SCANNET_OPENSEG_TEST["test_cfg"]["voxelize"], grid_size=0.08)))
    pipe = TestPipeline(cfg)
    st = pipe.prepare(case_scene(ref, CASES["f32_positive"]), "cpu")
    base = st["coord"].double()
    for a, ops in enumerate(pipe.augs[:4]):
        coord, normal = pipe.augmented(st, ops)
        assert coord.dtype == torch.float64 and normal.dtype == torch.float64      # np.dot with the float64 matrix
        quarter = [lambda c: c, lambda c: torch.stack([-c[:, 1], c[:, 0], c[:, 2]], 1), lambda c: torch.stack([-c[:, 0], -c[:, 1], c[:, 2]], 1),
                   lambda c: torch.stack([c[:, 1], -c[:, 0], c[:, 2]], 1)][a]
        assert torch.allclose(coord, quarter(base), atol=1e-12, rtol=0)
    batch = next(iter(pipe.batches(st, 2)))
    assert batch["feat"].shape[1] == 9 and "grid_coord" not in batch and batch["coord"].dtype == torch.float32


# ---- tester summaries against the formulas of engines/test.py restated with numpy ----------------------------------------------------

def hist(pred, seg, k, ignore=-1):
    """utils/misc.py:41-52 (intersection_and_union on host arrays)."""
    pred, seg = pred.copy(), seg.copy()
    pred[seg == ignore] = ignore
    inter = pred[pred == seg]
    ai = np.histogram(inter, bins=np.arange(k + 1))[0].astype(np.float64)
    ao = np.histogram(pred, bins=np.arange(k + 1))[0].astype(np.float64)
    at = np.histogram(seg, bins=np.arange(k + 1))[0].astype(np.float64)
    return ai, ao + at - ai, at


def two_scenes(ref, tmp_path, with_score):
    """The fixture scene twice (second copy: labels and predictions rolled), with their predictions stored as the result files the testers reuse."""
    case = CASES["f32_center"]
    a = case_scene(ref, case)
    b = dict(a, name="golden_b", segment=np.roll(ref["scene/segment"], 17))
    preds = {"golden": ref["pred"].astype(np.int64), "golden_b": np.roll(ref["pred"].astype(np.int64), 5)}
    scores = {"golden": ref["score"], "golden_b": np.roll(ref["score"], 3)}
    os.makedirs(tmp_path / "result")
    for name in preds:
        np.save(tmp_path / "result" / f"{name}_pred.npy", preds[name])
        if with_score:
            np.save(tmp_path / "result" / f"{name}_score.npy", scores[name])
    return [a, b], preds, scores


class NeverCalled(torch.nn.Module):
    def forward(self, d):
        raise AssertionError("stored results must be reused (engines/test.py:195-204)")


def test_openseg_tester_summary(ref, tmp_path):
    from pointcloudpdf_amd.recognizer import MaxProbability
    from pointcloudpdf_amd.testing import OpenSegTester

    scenes, preds, scores = two_scenes(ref, tmp_path, True)
    unknown = [5, 9]
    cfg = dict(data=dict(num_classes=K, ignore_index=-1, test=case_cfg(CASES["f32_center"], 0.08)), unknown_label=unknown, device="cpu")
    out = OpenSegTester((NeverCalled(), MaxProbability("msp")), cfg).test(scenes, save_path=str(tmp_path))
    known = np.ones(K, dtype=bool)
    known[unknown] = False
    I, U, T = np.zeros(K), np.zeros(K), np.zeros(K)
    for s in scenes:
        i, u, t = hist(preds[s["name"]], s["segment"], K)
        I, U, T = I + i, U + u, T + t
        got = out["scenes"][s["name"]]
        cls = (u != 0) & known
        assert abs(got["mIoU"] - np.mean((i / (u + 1e-10))[cls])) < 1e-9 and abs(got["allAcc"] - sum(i[cls]) / (sum(t[cls]) + 1e-10)) < 1e-9
        assert abs(got["running_mIoU"] - np.mean(I[cls] / (U[cls] + 1e-10))) < 1e-9
    assert abs(out["mIoU"] - np.mean((I / (U + 1e-10))[known])) < 1e-9
    assert abs(out["mAcc"] - np.mean((I / (T + 1e-10))[known])) < 1e-9
    assert abs(out["allAcc"] - sum(I[known]) / (sum(T[known]) + 1e-10)) < 1e-9
    assert np.allclose(out["iou_class"], I / (U + 1e-10), atol=1e-9, rtol=0)

    def aupr_auroc(score, seg):
        """utils/misc.py:70-87 with the step-wise / trapezoidal sums written out (no sklearn here)."""
        keep = seg != -1
        score, pos = score[keep].astype(np.float64), np.isin(seg[keep], unknown)
        order = np.argsort(-score, kind="stable")
        s, y = score[order], pos[order].astype(np.float64)
        tp, fp = np.cumsum(y), np.cumsum(1 - y)
        last = np.r_[s[1:] != s[:-1], True]
        tp, fp = tp[last], fp[last]
        rec, prec = tp / pos.sum(), tp / (tp + fp)
        aupr = np.sum(np.diff(np.r_[0.0, rec]) * prec)
        tpr, fpr = np.r_[0.0, tp / pos.sum()], np.r_[0.0, fp / (~pos).sum()]
        return aupr, np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2)

    pairs = [aupr_auroc(scores[s["name"]], s["segment"]) for s in scenes]
    assert abs(out["aupr"] - np.mean([p[0] for p in pairs])) < 1e-9 and abs(out["auroc"] - np.mean([p[1] for p in pairs])) < 1e-9
    a, r = aupr_auroc(np.concatenate([scores[s["name"]] for s in scenes]), np.concatenate([s["segment"] for s in scenes]))
    assert abs(out["all_aupr"] - a) < 1e-9 and abs(out["all_auroc"] - r) < 1e-9


def test_incrseg_tester_summary(ref, tmp_path):
    from pointcloudpdf_amd.testing import IncrSegTester

    scenes, preds, _ = two_scenes(ref, tmp_path, False)
    remap = {5: 13, 9: 14}
    for name in preds:   # predictions of a 15-class head: some points of the remapped classes found, some not
        p = preds[name]
        p[(p == 5) & (np.arange(p.size) % 2 == 0)] = 13
        p[(p == 9) & (np.arange(p.size) % 3 != 0)] = 14
        np.save(tmp_path / "result" / f"{name}_pred.npy", p)
    cfg = dict(data=dict(num_classes=K, ignore_index=-1, test=case_cfg(CASES["f32_center"], 0.08)), incr_label_remap=remap,
               incr_label_select=[5, 9], device="cpu")
    out = IncrSegTester(NeverCalled(), cfg).test(scenes, save_path=str(tmp_path))
    kc, b = K + 2, K
    known = np.ones(b, dtype=bool)
    known[[5, 9]] = False
    idx = [13, 14]
    rm = np.ones(kc, dtype=bool)
    rm[[5, 9]] = False                                   # ~selected(old + new ids) | selected(new ids)
    I, U, T = np.zeros(kc), np.zeros(kc), np.zeros(kc)
    for s in scenes:
        seg = s["segment"].copy()
        for old, new in remap.items():
            seg[s["segment"] == old] = new
        i, u, t = hist(preds[s["name"]], seg, kc)
        I, U, T = I + i, U + u, T + t
        got, mask = out["scenes"][s["name"]], u != 0
        assert abs(got["mIoU_known"] - np.mean((i / (u + 1e-10))[:b][mask[:b] & known])) < 1e-9
        assert abs(got["mIoU_incr"] - np.mean((i / (u + 1e-10))[np.array(idx)[mask[b:]]])) < 1e-9
        assert abs(got["allAcc_remap"] - sum(i[mask & rm]) / (sum(t[mask & rm]) + 1e-10)) < 1e-9
        assert abs(got["running_mAcc_incr"] - np.mean(I[idx] / (T[idx] + 1e-10))) < 1e-9
    iou, acc = I / (U + 1e-10), I / (T + 1e-10)
    want = dict(mIoU_known=np.mean(iou[:b][known]), mAcc_known=np.mean(acc[:b][known]), allAcc_known=sum(I[:b][known]) / (sum(T[:b][known]) + 1e-10),
                mIoU_incr=np.mean(iou[idx]), mAcc_incr=np.mean(acc[idx]), allAcc_incr=sum(I[idx]) / (sum(T[idx]) + 1e-10),
                mIoU_remap=np.mean(iou[rm]), mAcc_remap=np.mean(acc[rm]), allAcc_remap=sum(I[rm]) / (sum(T[rm]) + 1e-10))
    for key, v in want.items():
        assert abs(out[key] - v) < 1e-9, key
    assert T[5] == 0 and T[9] == 0 and T[13] > 0 and T[14] > 0          # the labels were remapped


def test_results_are_written_then_reused(ref, tmp_path):
    """Without stored files the tester votes and writes {name}_pred.npy / {name}_score.npy; a second run reads them back."""
    from pointcloudpdf_amd.recognizer import MaxProbability
    from pointcloudpdf_amd.testing import OpenSegTester

    logit_table = torch.from_numpy(ref["logit_table"])

    class TableModel(torch.nn.Module):
        def forward(self, d):
            return dict(seg_logits=logit_table[(torch.arange(d["coord"].shape[0]) * 7) % 1024])

    cfg = dict(data=dict(num_classes=K, ignore_index=-1, test=case_cfg(CASES["f32_center"], 0.08)), unknown_label=[5, 9], device="cpu",
               fragments_per_batch=8)
    scene = case_scene(ref, CASES["f32_center"])
    first = OpenSegTester((TableModel(), MaxProbability("msp")), cfg).test([scene], save_path=str(tmp_path))
    assert os.path.isfile(tmp_path / "result" / "golden_pred.npy") and os.path.isfile(tmp_path / "result" / "golden_score.npy")
    again = OpenSegTester((NeverCalled(), MaxProbability("msp")), cfg).test([scene], save_path=str(tmp_path))
    assert first["mIoU"] == again["mIoU"] and first["aupr"] == again["aupr"] and 0 <= first["auroc"] <= 1


# ---- C ABI: the three fragment entries validate before any launch (no GPU needed) ----------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    L, I, P = ctypes.c_long, ctypes.c_int, ctypes.c_void_p
    lib.pdf_fragment_bounds.argtypes = [L, L, I, I, I] + [P] * 7
    lib.pdf_fragment_gather.argtypes = [L, L, I, I, I] + [P] * 5 + [I] + [P] * 9
    lib.pdf_fragment_vote.argtypes = [L, L, I, I, I] + [P] * 10
    lib.pdf_fragment_bounds_ws_doubles.restype = L
    lib.pdf_fragment_bounds_ws_doubles.argtypes = [I]
    return lib


def test_fragment_entries_validate_before_any_launch(lib):
    buf = (ctypes.c_double * 64)()      # stands in for every pointer: nothing is dereferenced before the checks
    p = ctypes.cast(buf, ctypes.c_void_p)
    segs = (ctypes.c_void_p * 4)(None, p.value, None, None)
    w = (ctypes.c_int * 4)(3, 3, 0, 0)
    BAD, OK = -1, 0

    def bounds(n=8, v=4, f0=0, g=2, f64=0, coord=p, order=p, vstart=p, count=p, ws=p, out=p):
        return lib.pdf_fragment_bounds(n, v, f0, g, f64, coord, order, vstart, count, ws, out, None)

    def gather(n=8, v=4, f0=0, g=2, f64=0, coord=p, order=p, vstart=p, count=p, shift=p, nseg=2, src=segs, sw=w, grid=p, index=p,
               oc=p, of=p, og=p, oo=p):
        return lib.pdf_fragment_gather(n, v, f0, g, f64, coord, order, vstart, count, shift, nseg, src, sw, grid, index, oc, of, og, oo, None)

    def vote(n=8, v=4, f0=0, g=2, c=13, logits=p, score=p, order=p, vstart=p, count=p, voxel_of=p, pred=p, ssum=p, scnt=p):
        return lib.pdf_fragment_vote(n, v, f0, g, c, logits, score, order, vstart, count, voxel_of, pred, ssum, scnt, None)

    for fn in (bounds, gather, vote):
        assert fn(v=0) == OK and fn(n=0, v=0) == OK                       # an empty scene is a no-op ...
        assert fn(v=0, g=0) == BAD and fn(v=0, order=None) == BAD         # ... after the checks
        for kw in (dict(n=-1), dict(v=-1), dict(v=9), dict(f0=-1), dict(g=0), dict(g=-3), dict(order=None), dict(vstart=None), dict(count=None)):
            assert fn(**kw) == BAD, (fn.__name__, kw)
    for kw in (dict(coord=None), dict(ws=None), dict(out=None), dict(f64=2)):
        assert bounds(**kw) == BAD, kw
    for kw in (dict(coord=None), dict(shift=None), dict(index=None), dict(oc=None), dict(of=None), dict(oo=None), dict(f64=-1), dict(nseg=0),
               dict(nseg=5), dict(src=None), dict(sw=None), dict(grid=None), dict(og=None), dict(g=257),
               dict(n=2 ** 31, v=2 ** 30, g=2),                          # offset is int32: g v must fit
               dict(sw=(ctypes.c_int * 4)(4, 3, 0, 0)),                  # the coordinate segment is 3 wide
               dict(sw=(ctypes.c_int * 4)(3, 5, 0, 0)), dict(sw=(ctypes.c_int * 4)(3, 0, 0, 0))):
        assert gather(**kw) == BAD, kw
    assert gather(v=0, grid=None, og=None) == OK                          # grid_coord is optional (both or neither)
    for kw in (dict(c=0), dict(logits=None), dict(voxel_of=None), dict(pred=None), dict(ssum=None), dict(scnt=None)):
        assert vote(**kw) == BAD, kw
    assert vote(v=0, score=None, ssum=None, scnt=None) == OK              # score may be NULL (then the sums are not needed)
    assert lib.pdf_fragment_bounds_ws_doubles(4) >= 4 * 6 and lib.pdf_fragment_bounds_ws_doubles(0) == 0


def test_backend_methods_refuse_host_tensors_and_bad_shapes():
    """No quiet fall-back: the HIP backend's fragment methods raise on host tensors; shapes / dtypes are checked before the call."""
    from pointcloudpdf_amd import _native
    from pointcloudpdf_amd.testing import _table

    coord = torch.rand(50, 3)
    t = _table(coord, 0.2)
    be = _native.HipBackend.__new__(_native.HipBackend)     # (no library call is reached)
    with pytest.raises(ValueError, match="g >= 1"):
        be._fragment_table(t, 0, 0, coord)
    with pytest.raises(TypeError, match="float32 or float64"):
        be._fragment_table(t, 0, 1, coord.half())
    with pytest.raises(ValueError, match="coord"):
        be._fragment_table(t, 0, 1, coord[:10])
    with pytest.raises(TypeError, match="order"):
        be._fragment_table(dict(t, order=t["order"].int()), 0, 1, coord)
    with pytest.raises(_native.PdfOpsError):
        _native.backend_for(coord)

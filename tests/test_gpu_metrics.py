"""GPU suite: the open-set metrics pass of csrc/openset_metrics.hip -- through the C ABI against the reference's own results
(tests/golden/ops_metrics_ref.npz: histograms exact, AUPR / AUROC within 1e-9 of sklearn's), against the torch composition on the same
device tensors, under capture and replay, and inside the evaluators and the testers."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from test_metrics_cpu import TOL, load_cases, same_area

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import _native

    return _native.hip_backend().lib


def run_abi(lib, k, target, ignore, logits=None, pred=None, score=None, unknown=None):
    """One call of pdf_openset_metrics on the current stream -> hist (3, k) int64, record (4) float64 (device tensors).  The outputs and
    the workspace start from a pattern that is no valid result: every element has to be written, nothing may depend on a zeroed byte."""
    from pointcloudpdf_amd import _native

    n = target.shape[0]
    c = logits.shape[1] if logits is not None else 0
    hist = torch.full((3, k), -7, dtype=torch.int64, device=target.device)
    record = torch.full((4,), -7.0, dtype=torch.float64, device=target.device)
    ws = torch.full((int(lib.pdf_openset_metrics_workspace_bytes(n, c)),), 0xA5, dtype=torch.uint8, device=target.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.pdf_openset_metrics(n, c, ptr(logits), ptr(pred), ptr(score), target.data_ptr(), ignore, ptr(unknown), k, hist.data_ptr(),
                                 record.data_ptr(), ws.data_ptr(), ctypes.c_void_p(_native.raw_stream()))
    assert rc == 0, rc
    return hist, record


def unknown_bytes(mod):
    m = torch.zeros(mod.K, dtype=torch.uint8)
    m[list(mod.UNKNOWN)] = 1
    return m.cuda()


# csrc/tile_sort.h: TILE = 2048 keys per sort tile, SCAN_CHUNK = 1024 words per workgroup of the first scan level, 256 lanes in
# the second: "deep_scan" (2048 * 1024 + 1 rows) is the first size at which a lane of the second level owns more than one chunk;
# every case above 4 tiles (1024 / 256 digits) runs both levels.
def test_every_fixture_case_through_the_c_abi(cases, lib):
    mod, golden = cases
    unknown = unknown_bytes(mod)
    worst = 0.0
    for name in mod.CASES:
        pred, score, target = (torch.from_numpy(a).cuda() for a in mod.make_case(name))
        hist, rec = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=score, unknown=unknown)
        hist, rec, want = hist.cpu().numpy(), rec.cpu().numpy(), golden[f"{name}_record"]
        print(name, rec, want)
        assert np.array_equal(hist, golden[f"{name}_hist"]), name
        assert rec[2] == want[2] and rec[3] == want[3], name
        assert same_area(rec[0], want[0]) and same_area(rec[1], want[1]), (name, rec, want)
        if not math.isnan(want[1]):
            worst = max(worst, abs(rec[0] - want[0]), abs(rec[1] - want[1]))
    print(f"max |area - sklearn| over the fixture: {worst:.3e}")
    none = golden["no_pos_record"]
    assert math.isnan(none[0]) and none[2] == 0 and math.isnan(golden["no_neg_record"][1]) and golden["all_ignored_hist"].sum() == 0


def test_logits_form_equals_the_pred_form(cases, lib):
    mod, _ = cases
    _, score, target = (torch.from_numpy(a).cuda() for a in mod.make_case("n3tiles1"))
    n = target.shape[0]
    g = torch.Generator(device="cuda").manual_seed(5)
    logits = torch.randn(n, mod.K, device="cuda", generator=g)
    logits[::7, 3] = logits[::7].max(1)[0]          # tied maxima: the lowest index wins
    logits[::11, 12] = logits[::11].max(1)[0]
    logits[5, 8] = float("nan")                     # a NaN is maximal
    logits[6, 2] = float("nan"); logits[6, 10] = float("nan")
    logits[7, 0] = float("inf")
    target[5:8] = torch.tensor([8, 2, 0], device="cuda")
    pred = logits.max(1)[1]
    assert int(pred[5]) == 8 and int(pred[6]) == 2
    unknown = unknown_bytes(mod)
    h1, r1 = run_abi(lib, mod.K, target, mod.IGNORE, logits=logits, score=score, unknown=unknown)
    h2, r2 = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=score, unknown=unknown)
    assert torch.equal(h1, h2) and torch.equal(r1, r2)
    for c in (1, 2, 70):                            # other widths
        x = torch.randn(300, c, device="cuda", generator=g)
        t = torch.randint(0, max(c, 2), (300,), device="cuda", generator=g)
        h1, _ = run_abi(lib, max(c, 2), t, -1, logits=x)
        h2, _ = run_abi(lib, max(c, 2), t, -1, pred=x.max(1)[1])
        assert torch.equal(h1, h2), c


def test_nan_score_and_missing_score(cases, lib):
    mod, golden = cases
    pred, score, target = (torch.from_numpy(a).cuda() for a in mod.make_case("n2049"))
    unknown = unknown_bytes(mod)
    row = int(torch.nonzero(target != mod.IGNORE)[3])
    bad = score.clone()
    bad[row] = float("nan")
    hist, rec = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=bad, unknown=unknown)
    want = golden["n2049_record"]
    assert math.isnan(rec[0]) and math.isnan(rec[1]) and rec[2] == want[2] and rec[3] == want[3]
    assert np.array_equal(hist.cpu().numpy(), golden["n2049_hist"])
    ign = score.clone()
    ign[int(torch.nonzero(target == mod.IGNORE)[0])] = float("nan")     # on an ignored row a NaN means nothing
    _, rec = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=ign, unknown=unknown)
    assert same_area(float(rec[0]), want[0]) and same_area(float(rec[1]), want[1])
    hist, rec = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred)
    assert np.array_equal(hist.cpu().numpy(), golden["n2049_hist"])
    assert math.isnan(rec[0]) and math.isnan(rec[1]) and rec[2] == 0 and rec[3] == 0


def test_ten_evaluations_are_bit_identical(cases, lib):
    mod, _ = cases
    pred, score, target = (torch.from_numpy(a).cuda() for a in mod.make_case("thousandths"))
    unknown = unknown_bytes(mod)
    first = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=score, unknown=unknown)
    for _ in range(9):
        again = run_abi(lib, mod.K, target, mod.IGNORE, pred=pred, score=score, unknown=unknown)
        assert torch.equal(again[0], first[0]) and again[1].view(torch.int64).equal(first[1].view(torch.int64))


def test_four_million_rows_against_the_composition():
    """Counts exact, areas within 1e-9 of ``aupr_and_auroc`` on the same device tensors; the expected difference is the composition's own
    double-sum rounding (~1e-12).  Observed on an MI355X: |aupr difference| 5.6e-17, |auroc difference| 1.1e-16 (the test prints both)."""
    from pointcloudpdf_amd import evaluator

    n, k = 4_000_000, 13
    g = torch.Generator(device="cuda").manual_seed(9)
    target = torch.randint(0, k, (n,), device="cuda", generator=g)
    target[torch.rand(n, device="cuda", generator=g) < 0.08] = -1
    pos = torch.isin(target, torch.tensor([5, 9], device="cuda"))
    score = torch.randn(n, device="cuda", generator=g) + 0.8 * pos          # mixed sign; float32 normals at 4M rows hold ties
    pred = torch.where(torch.rand(n, device="cuda", generator=g) < 0.7, target.clamp(min=0), torch.randint(0, k, (n,), device="cuda", generator=g))
    hist, rec = evaluator.openset_metrics(pred, score, target, k, [5, 9], -1)
    i, u, t = evaluator.intersection_and_union(pred, target, k, -1)
    assert torch.equal(hist, torch.stack([i, u, t]).long())
    aupr, auroc = evaluator.aupr_and_auroc(score, target, [5, 9], -1)
    rec = rec.cpu().numpy()
    valid = target != -1
    assert rec[2] == int((pos & valid).sum()) and rec[3] == int((~pos & valid).sum())
    print(f"4M rows: |aupr - composition| {abs(rec[0] - aupr):.3e}, |auroc - composition| {abs(rec[1] - auroc):.3e}")
    assert abs(rec[0] - aupr) <= TOL and abs(rec[1] - auroc) <= TOL


def test_capture_and_replay(cases):
    """The call recorded into a graph on one stream (a host read would raise during the capture), no memset node in it, two replays with
    other contents of the static inputs and other device work in between: each equals the eager call bit for bit."""
    from pointcloudpdf_amd import engine, evaluator

    mod, _ = cases
    data = [tuple(torch.from_numpy(a).cuda() for a in mod.make_case(name)) for name in ("eighths", "mixed_sign", "outside")]
    g0 = torch.Generator(device="cuda").manual_seed(3)
    logit_sets = [torch.randn(5000, mod.K, device="cuda", generator=g0) for _ in data]
    evaluator.unknown_mask(mod.K, mod.UNKNOWN, "cuda")          # uploaded eagerly, as the evaluators do when they are constructed
    logits, score, target = logit_sets[0].clone(), data[0][1].clone(), data[0][2].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=s):
        hist, rec = evaluator.openset_metrics(logits, score, target, mod.K, mod.UNKNOWN, mod.IGNORE)
    census = engine.graph_node_census(graph.raw_cuda_graph())
    assert census["kernel"] >= 20 and census["memset"] == 0 and census["memcpy"] == 0, census
    for j in (1, 2):
        logits.copy_(logit_sets[j]); score.copy_(data[j][1]); target.copy_(data[j][2])
        junk = torch.randn(1 << 20, device="cuda").sort()[0]   # other device work (and other users of the allocator) in between
        graph.replay()
        torch.cuda.synchronize()
        want_h, want_r = evaluator.openset_metrics(logit_sets[j], data[j][1], data[j][2], mod.K, mod.UNKNOWN, mod.IGNORE)
        assert torch.equal(hist, want_h) and rec.view(torch.int64).equal(want_r.view(torch.int64)), j
        assert rec[2] > 0 and not math.isnan(float(rec[0]))
        del junk


def test_missing_mask_inside_a_capture_is_an_error(monkeypatch):
    from pointcloudpdf_amd import evaluator

    x, t = torch.zeros(4, 31, device="cuda"), torch.zeros(4, dtype=torch.long, device="cuda")
    with monkeypatch.context() as m:   # (no capture is begun: the refusal comes before any device work)
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="before the capture"):
            evaluator.openset_metrics(x, x[:, 0].contiguous(), t, 31, [30], -1)


def test_deferred_evaluator_over_device_batches():
    from pointcloudpdf_amd import evaluator
    from test_metrics_cpu import _batches

    eager = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=False)
    deferred = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1)          # device tensors: deferred by default
    for logits, score, seg, loss in _batches(6, n=3000):
        eager.update(logits, score, seg, loss=float(loss))
        deferred.update(logits.cuda(), score.cuda(), seg.cuda(), loss=loss.cuda())
    assert deferred.hist.is_cuda and deferred.hist.dtype == torch.int64 and len(deferred._records) == 6 and deferred._aupr == []
    a, d = eager.summary(), deferred.summary()
    assert len(deferred.aupr) == 5                                                         # one batch without unknown points
    for key in ("mIoU", "mAcc", "allAcc"):
        assert a[key] == d[key], key
    for key in ("aupr", "auroc"):
        assert abs(a[key] - d[key]) <= TOL, (key, a[key], d[key])
    assert abs(a["loss"] - d["loss"]) <= 1e-7
    incr_args = (5, {3: 5, 4: 6}, [3, 4], -1)
    ie, idf = evaluator.IncrSegEvaluator(*incr_args, deferred=False), evaluator.IncrSegEvaluator(*incr_args)
    g = torch.Generator().manual_seed(8)
    for _ in range(3):
        logits, seg = torch.randn(2500, 7, generator=g), torch.randint(-1, 7, (2500,), generator=g)
        ie.update(logits, seg)
        idf.update(logits.cuda(), seg.cuda())
    a, d = ie.summary(), idf.summary()
    assert all(a[key] == d[key] for key in a if isinstance(a[key], float) and key != "loss")


# ---- the testers ---------------------------------------------------------------------------------------------------------------------

def host_figures(result_dir, name, segment, k, unknown, ignore=-1):
    """The parent commit's host formulas on the tester's own result files."""
    from pointcloudpdf_amd import evaluator

    pred = torch.from_numpy(np.load(os.path.join(result_dir, f"{name}_pred.npy")))
    seg = torch.from_numpy(np.asarray(segment)).long()
    i, u, t = (x.double().numpy() for x in evaluator.intersection_and_union(pred, seg, k, ignore))
    score_path = os.path.join(result_dir, f"{name}_score.npy")
    score = torch.from_numpy(np.load(score_path)) if os.path.isfile(score_path) else None
    pair = evaluator.aupr_and_auroc(score, seg, unknown, ignore) if score is not None else (None, None)
    return i, u, t, pair, score, seg


def two_scenes(golden_dir):
    from test_tester_cpu import CASES, case_scene

    ref = np.load(os.path.join(golden_dir, "tester_ref.npz"))
    first = case_scene(ref, CASES["f32_center"])
    seg = np.asarray(first["segment"]).copy()
    second = dict(first, name="second", segment=np.where(np.arange(seg.shape[0]) % 5 == 0, -1, np.roll(seg, 17)))
    return [first, second]


def test_openseg_tester_takes_its_metrics_from_the_device(golden_dir, tmp_path):
    from pointcloudpdf_amd import recognizer, synthetic, testing
    from pointcloudpdf_amd.registry import MODELS
    from test_gpu_tester import K, make_cfg

    seg = MODELS.build(dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg26", in_channels=6, num_classes=K))).cuda().eval()
    synthetic.fill_parameters_deterministic(seg, seed=5)
    scenes = two_scenes(golden_dir)
    tester = testing.OpenSegTester((seg, recognizer.MaxProbability("max_logits")), make_cfg(2))
    res = tester.test(scenes, save_path=str(tmp_path))
    result_dir = str(tmp_path / "result")
    isum, scores, segs, auprs = np.zeros(K), [], [], []
    for scene in scenes:
        i, u, t, (aupr, auroc), score, s = host_figures(result_dir, scene["name"], scene["segment"], K, [5, 9])
        rec = res["scenes"][scene["name"]]
        assert np.array_equal(rec["intersection"], i) and np.array_equal(rec["union"], u) and np.array_equal(rec["target"], t)
        assert aupr is not None and abs(rec["aupr"] - aupr) <= TOL and abs(rec["auroc"] - auroc) <= TOL, (rec["aupr"], aupr, rec["auroc"], auroc)
        isum += i; scores.append(score); segs.append(s); auprs.append(aupr)
    from pointcloudpdf_amd import evaluator

    assert np.array_equal(res["intersection"], isum) and abs(res["aupr"] - np.mean(auprs)) <= TOL
    a, r = evaluator.aupr_and_auroc(torch.cat(scores), torch.cat(segs), [5, 9], -1)
    assert abs(res["all_aupr"] - a) <= TOL and abs(res["all_auroc"] - r) <= TOL, (res["all_aupr"], a, res["all_auroc"], r)
    assert (torch.cat(scores) < 0).any()                                                    # max_logits scores are negative logits
    calls = []
    tester.scene_tester.forward_fn = lambda batch: calls.append(1)                          # a second run reuses the saved result files
    again = tester.test(scenes, save_path=str(tmp_path))
    assert not calls
    for key in ("mIoU", "mAcc", "allAcc", "aupr", "auroc", "all_aupr", "all_auroc"):
        assert again[key] == res[key], key
    assert all(again["scenes"][n]["aupr"] == res["scenes"][n]["aupr"] for n in res["scenes"])


def test_incrseg_tester_takes_its_histograms_from_the_device(golden_dir, tmp_path):
    from pointcloudpdf_amd import data_path, engine, synthetic, testing
    from test_gpu_tester import make_cfg

    step = engine.IncrSegStep(backbone="PointTransformer-Seg26").cuda()
    synthetic.fill_parameters_deterministic(step.teacher, seed=1)
    synthetic.fill_parameters_deterministic(step.student, seed=2)
    scenes = two_scenes(golden_dir)[:1]
    remap = {5: 13, 9: 14}
    tester = testing.IncrSegTester(step, make_cfg(2, incr_label_remap=remap, incr_label_select=[5, 9]))
    res = tester.test(scenes, save_path=str(tmp_path))
    labels = data_path.remap_label(torch.from_numpy(np.asarray(scenes[0]["segment"])).long(), remap, ignore_index=-1)[0]
    i, u, t, _, _, _ = host_figures(str(tmp_path / "result"), scenes[0]["name"], labels.numpy(), 15, [])
    rec = res["scenes"][scenes[0]["name"]]
    assert np.array_equal(rec["intersection"], i) and np.array_equal(rec["union"], u) and np.array_equal(rec["target"], t)
    assert np.array_equal(res["intersection"], i) and np.array_equal(res["union"], u) and np.array_equal(res["target"], t)
    b, k, idx, r = tester.base_num_classes, tester.mask_known, tester.incr_label_idx, tester.mask_incr_remap
    iou, acc = i / (u + 1e-10), i / (t + 1e-10)
    for tag, sel in (("known", lambda x: x[:b][k]), ("incr", lambda x: x[idx]), ("remap", lambda x: x[r])):   # the three class sets
        assert res[f"mIoU_{tag}"] == float(np.mean(sel(iou))) and res[f"mAcc_{tag}"] == float(np.mean(sel(acc))), tag
        assert res[f"allAcc_{tag}"] == float(sum(sel(i)) / (sum(sel(t)) + 1e-10)), tag
    again = tester.test(scenes, save_path=str(tmp_path))
    assert all(again[f"mIoU_{tag}"] == res[f"mIoU_{tag}"] for tag in ("known", "incr", "remap"))

"""CPU suite: ``evaluator.openset_metrics`` on host tensors (the composition of ``intersection_and_union`` + ``aupr_and_auroc``) against the
reference's own results (tests/golden/ops_metrics_ref.npz, written by make_golden_metrics.py), and the deferred mode of the two
evaluators against their eager mode."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from pointcloudpdf_amd import evaluator

TOL = 1e-9   # tests/test_datapath.py::check_metrics


def load_cases(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_metrics", os.path.join(golden_dir, "make_golden_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)   # (the reference tree is only touched by its main())
    return mod, np.load(os.path.join(golden_dir, "ops_metrics_ref.npz"))


def same_area(got, want, tol=TOL):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= tol


@pytest.fixture(scope="module")
def cases(golden_dir):
    return load_cases(golden_dir)


def test_fixture_lists_every_case(cases):
    mod, golden = cases
    assert sorted(mod.CASES) == list(golden["cases"])
    assert (int(golden["num_classes"]), tuple(golden["unknown"]), int(golden["ignore_index"])) == (mod.K, mod.UNKNOWN, mod.IGNORE)
    assert mod.DEEP == 2048 * 1024 + 1


def test_openset_metrics_on_cpu_tensors_matches_the_reference(cases):
    mod, golden = cases
    for name in mod.CASES:
        pred, score, target = (torch.from_numpy(a) for a in mod.make_case(name))
        hist, rec = evaluator.openset_metrics(pred, score, target, mod.K, mod.UNKNOWN, mod.IGNORE)
        assert hist.dtype == torch.int64 and hist.shape == (3, mod.K) and rec.dtype == torch.float64 and rec.shape == (4,)
        assert np.array_equal(hist.numpy(), golden[f"{name}_hist"]), name
        want = golden[f"{name}_record"]
        assert rec[2] == want[2] and rec[3] == want[3], name
        assert same_area(float(rec[0]), want[0]) and same_area(float(rec[1]), want[1]), (name, rec, want)


def test_logits_form_nan_score_and_no_score_on_cpu(cases):
    mod, _ = cases
    pred, score, target = (torch.from_numpy(a) for a in mod.make_case("n2049"))
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(pred.shape[0], mod.K, generator=g)
    logits[::7, 3] = logits[::7].max(1)[0]     # tied maxima
    logits[5, 8] = float("nan")
    h_logits, r_logits = evaluator.openset_metrics(logits, score, target, mod.K, mod.UNKNOWN, mod.IGNORE)
    h_pred, r_pred = evaluator.openset_metrics(logits.max(1)[1], score, target, mod.K, mod.UNKNOWN, mod.IGNORE)
    assert torch.equal(h_logits, h_pred) and torch.equal(r_logits, r_pred)
    bad = score.clone()
    bad[int(torch.nonzero(target != mod.IGNORE)[0])] = float("nan")
    _, rec = evaluator.openset_metrics(pred, bad, target, mod.K, mod.UNKNOWN, mod.IGNORE)
    assert math.isnan(rec[0]) and math.isnan(rec[1]) and rec[2] > 0 and rec[3] > 0
    hist, rec = evaluator.openset_metrics(pred, None, target, mod.K, (), mod.IGNORE)
    assert torch.equal(hist, evaluator.openset_metrics(pred, score, target, mod.K, mod.UNKNOWN, mod.IGNORE)[0])
    assert math.isnan(rec[0]) and math.isnan(rec[1]) and rec[2] == 0 and rec[3] == 0


def _batches(count=6, n=700, k=6, without_unknown=(2,)):
    for b in range(count):
        g = torch.Generator().manual_seed(300 + b)
        logits, score, seg = torch.randn(n, k, generator=g), torch.rand(n, generator=g), torch.randint(0, k, (n,), generator=g)
        seg[torch.rand(n, generator=g) < 0.1] = -1
        if b in without_unknown:
            seg[seg == 4] = 0
        yield logits, score, seg, torch.rand((), generator=g)


def test_deferred_evaluator_equals_the_eager_one():
    eager = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1)
    deferred = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=True)
    for b, (logits, score, seg, loss) in enumerate(_batches()):
        eager.update(logits, score, seg, loss=float(loss))
        deferred.update(logits, score, seg, loss=loss)          # a tensor: kept as one
        assert len(deferred._records) == b + 1 and len(deferred._loss_t) == b + 1 and deferred._aupr == []   # nothing read yet
        assert torch.equal(deferred.hist.double(), eager.hist)
    assert deferred.hist.dtype == torch.int64
    a, d = eager.summary(), deferred.summary()
    assert len(eager.aupr) == 5 and deferred.aupr == eager.aupr and deferred.auroc == eager.auroc       # batch 2 holds no unknown point
    assert deferred.losses == pytest.approx(eager.losses, rel=0, abs=1e-7) and len(deferred.losses) == 6
    for key in ("mIoU", "mAcc", "allAcc", "aupr", "auroc"):
        assert a[key] == d[key], key
    assert abs(a["loss"] - d["loss"]) <= 1e-7
    assert np.array_equal(a["iou_class"], d["iou_class"]) and np.array_equal(a["acc_class"], d["acc_class"])


def test_list_attributes_flush_pending_records():
    ev = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1, deferred=True)
    batches = list(_batches(3, without_unknown=(1,)))
    ev.update(*batches[0][:3], loss=batches[0][3])
    assert len(ev.aupr) == 1 and ev._records == []              # reading the attribute flushed
    assert len(ev.auroc) == 1 and len(ev.losses) == 1
    ev.update(*batches[1][:3])                                  # no unknown point: dropped at the flush
    ev.update(*batches[2][:3], loss=0.25)                       # a python float keeps its place in the list
    assert len(ev.auroc) == 2 and ev.losses == [pytest.approx(float(batches[0][3])), 0.25]
    ev.reset()
    assert ev.aupr == [] and ev.auroc == [] and ev.losses == [] and ev.hist is None


def test_default_mode_on_cpu_tensors_is_the_eager_path():
    ev = evaluator.OpenSegEvaluator(6, unknown_label=[4], ignore_index=-1)
    logits, score, seg, _ = next(_batches(1))
    ev.update(logits, score, seg, loss=1.5)
    assert ev._records == [] and ev.hist.dtype == torch.float64 and len(ev._aupr) == 1 and ev._losses == [1.5]
    pair = evaluator.aupr_and_auroc(score, seg, [4], -1)
    assert (ev.aupr[0], ev.auroc[0]) == pair


def test_incr_evaluator_summaries_are_unchanged_by_the_deferred_mode():
    args = (5, {3: 5, 4: 6}, [3, 4], -1)
    eager, deferred = evaluator.IncrSegEvaluator(*args), evaluator.IncrSegEvaluator(*args, deferred=True)
    for b in range(4):
        g = torch.Generator().manual_seed(400 + b)
        logits, seg = torch.randn(600, 7, generator=g), torch.randint(0, 7, (600,), generator=g)
        seg[torch.rand(600, generator=g) < 0.1] = -1
        loss = torch.rand((), generator=g)
        eager.update(logits, seg, loss=float(loss))
        deferred.update(logits, seg, loss=loss)
        # what IncrSegEvaluator.update computed before there was a deferred mode
        i, u, t = evaluator.intersection_and_union(logits.max(1)[1], seg, 7, -1)
        assert torch.equal(eager.hist, torch.stack([i, u, t]).double() + (0 if b == 0 else prev))
        prev = eager.hist.clone()
    a, d = eager.summary(), deferred.summary()
    assert set(a) == set(d)
    for key, v in a.items():
        if isinstance(v, dict):
            assert all(v[s] == d[key][s] for s in v), key
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, d[key]), key
        else:
            assert v == pytest.approx(d[key], rel=0, abs=1e-7 if key == "loss" else 0), key


def test_bad_arguments_are_refused_before_any_launch():
    """Pure validation: no GPU is touched (the pointers are host buffers that no kernel ever sees)."""
    import ctypes

    from pointcloudpdf_amd import _native, build

    lib = ctypes.CDLL(build.build_library())
    be = _native.HipBackend(lib)   # binds the prototypes (no GPU call)
    assert be.lib.pdf_openset_metrics_workspace_bytes(0, 13) == 0 and be.lib.pdf_openset_metrics_workspace_bytes(2 ** 31 - 1, 13) == 0
    small, big = be.lib.pdf_openset_metrics_workspace_bytes(1, 13), be.lib.pdf_openset_metrics_workspace_bytes(2 ** 31 - 2, 13)
    assert 0 < small < big and be.lib.pdf_openset_metrics_workspace_bytes(2049, 0) > 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = be.lib.pdf_openset_metrics
    ok = dict(n=4, c=13, logits=p, pred=None, score=p, target=p, ignore=-1, unknown=p, k=13, hist=p, record=p, ws=p, stream=None)
    for change in (dict(n=0), dict(n=2 ** 31 - 1), dict(k=0), dict(pred=p), dict(logits=None), dict(c=0), dict(target=None), dict(hist=None),
                   dict(record=None), dict(ws=None)):
        assert f(*dict(ok, **change).values()) == -1, change
    assert f(*dict(ok, k=1025).values()) == -3      # PDF_ERR_UNSUPPORTED: more classes than the histogram's LDS counters

"""CPU suite of the incremental stage (pointcloudpdf_amd/incremental.py): the learner on the oracle backend against the reference's own
classes (tests/golden/model_incr_ref.npz, made by tests/golden/make_golden_incr.py), the device label transforms, the loss's torch
composition, checkpoint adaptation and the incremental evaluator."""
import os

import numpy as np
import pytest
import torch

import helpers

SIZES, GRID = [2048, 1600], 0.25
REMAP = {5: 13, 9: 14}
CASES = {"train": (True, 1.0, 1.0), "temp": (True, 2.0, 0.5), "eval": (False, 1.0, 1.0)}
GRADS = ["cls.0.weight", "cls.1.weight", "cls.3.weight", "cls.3.bias", "dec1.0.linear1.0.weight", "dec1.1.linear1.weight",
         "dec1.1.transformer.linear_q.weight", "dec2.0.linear1.0.weight", "dec2.1.linear3.weight", "dec3.0.linear1.0.weight",
         "dec4.0.linear1.0.weight", "enc1.0.linear.weight"]
TOL = 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "model_incr_ref.npz"))


def build_learner(device="cpu", tp=1.0, tt=1.0):
    from pointcloudpdf_amd import incremental, segmentor  # noqa: F401  (registers the classes)
    from pointcloudpdf_amd import synthetic
    from pointcloudpdf_amd.registry import INCREMENTALLEARNER, MODELS

    ce = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]
    teacher = MODELS.build(dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg50", in_channels=6, num_classes=13), criteria=ce))
    synthetic.fill_parameters_deterministic(teacher, seed=1)
    learner = INCREMENTALLEARNER.build(dict(type="PointPdf-incr-v1m1", eval_criteria=ce,
                                            backbone=dict(type="PointTransformer-Seg50", in_channels=6, num_classes=15)))
    synthetic.fill_parameters_deterministic(learner.incr_backbone, seed=2)
    learner.criteria = incremental.IncrDistillKlLoss(tp, tt)
    teacher.requires_grad_(False)
    learner.inject_teacher_model(teacher)
    return learner.to(device), teacher.to(device)


def run_learner(case, golden, device="cpu"):
    """The learner on the fixture's batch -> (output dict, student logits, teacher logits, learner)."""
    from pointcloudpdf_amd import synthetic

    train, tp, tt = CASES[case]
    learner, teacher = build_learner(device, tp, tt)
    learner.train(train)
    teacher.eval()
    batch = synthetic.make_batch(SIZES, first_scene_id=100, grid_size=GRID, device=device, unknown=())
    d = dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"], offset_host=batch["offset_host"],
             segment=torch.from_numpy(golden["segment"]).to(device), segment_incr=torch.from_numpy(golden["segment_incr"]).to(device),
             segment_incr_remap=torch.from_numpy(golden["segment_incr_remap"]).to(device))
    seen = {}
    hs = [learner.incr_backbone.register_forward_hook(lambda m, i, o: seen.__setitem__("student", o.detach())),
          teacher.backbone.register_forward_hook(lambda m, i, o: seen.__setitem__("teacher", o.detach()))]
    out = learner(d)
    for h in hs:
        h.remove()
    if train:
        out["loss"].backward()
    return out, seen.get("student"), seen.get("teacher"), learner


@pytest.mark.parametrize("case", list(CASES))
def test_learner_matches_reference_class(use_oracle, golden, case):
    out, student, teacher, learner = run_learner(case, golden)
    assert sorted(out.keys()) == list(golden[f"{case}_keys"])
    helpers.assert_close(out["loss"], golden[f"{case}_loss"], TOL, f"{case} loss")
    if "seg_logits" in out:
        helpers.assert_close(helpers.thin(out["seg_logits"].detach().numpy()), golden[f"{case}_seg_logits"], TOL, f"{case} seg_logits")
    if CASES[case][0]:
        helpers.assert_close(helpers.thin(student.numpy()), golden[f"{case}_student_logits"], TOL, f"{case} student logits")
        helpers.assert_close(helpers.thin(teacher.numpy()), golden[f"{case}_teacher_logits"], TOL, f"{case} teacher logits")
        named = dict(learner.incr_backbone.named_parameters())
        for k in GRADS:
            g = named[k].grad.numpy()
            g = g[:helpers.GRAD_ROWS] if g.ndim >= 2 else g
            helpers.assert_close(g, golden[f"{case}_grad_{k}"], 1e-4, f"{case} grad {k}")
        assert all(p.grad is None for p in learner.teacher_model.parameters())


def test_label_transforms_match_reference(golden):
    from pointcloudpdf_amd import data_path

    seg = torch.from_numpy(golden["segment"])
    known = data_path.mask_label(seg, [5, 9])
    remap, incr = data_path.remap_label(seg, REMAP)
    assert torch.equal(known, torch.from_numpy(golden["segment_known"]))
    assert torch.equal(remap, torch.from_numpy(golden["segment_incr_remap"]))
    assert torch.equal(incr, torch.from_numpy(golden["segment_incr"]))
    remap, incr = data_path.remap_label(seg, REMAP, remap_select=[5])
    assert torch.equal(remap, torch.from_numpy(golden["sel_segment_incr_remap"]))
    assert torch.equal(incr, torch.from_numpy(golden["sel_segment_incr"]))
    assert torch.equal(seg, torch.from_numpy(golden["segment"])), "the transforms must not modify their input"
    # labels above every key keep their identity / become ignored (no table sized by segment.max())
    far = torch.tensor([0, 5, 9, 12, 40, -1])
    r, i = data_path.remap_label(far, REMAP)
    assert r.tolist() == [0, 13, 14, 12, 40, -1] and i.tolist() == [-1, 13, 14, -1, -1, -1]
    assert data_path.mask_label(far, [5, 9]).tolist() == [0, -1, -1, 12, 40, -1]


@pytest.mark.parametrize("tp,tt", [(1.0, 1.0), (2.0, 0.5)])
def test_loss_composition_matches_closed_form(tp, tt):
    from pointcloudpdf_amd import incremental

    g = torch.Generator().manual_seed(3)
    n, cs, ct = 500, 15, 13
    pred = torch.randn(n, cs, dtype=torch.float64, generator=g, requires_grad=True)
    teacher = torch.randn(n, ct, dtype=torch.float64, generator=g)
    lab = torch.full((n,), -1, dtype=torch.long)
    lab[::7] = 13
    lab[3::11] = 2
    loss = incremental.IncrDistillKlLoss(tp, tt, loss_weight=0.5)(pred, teacher, lab)
    loss.backward()
    t = torch.zeros(n, cs, dtype=torch.float64)
    t[:, :ct] = torch.softmax(teacher / tt, 1)
    for r in range(n):
        if lab[r] != -1:
            t[r] = 0
            t[r, lab[r]] = 1
    logp = torch.log_softmax(pred.detach() / tp, 1)
    want = 0.5 * float((torch.xlogy(t, t) - t * logp).sum() / n)
    assert abs(float(loss) - want) <= 1e-12 * abs(want)
    p = torch.softmax(pred.detach() / tp, 1)
    dgrad = 0.5 * (p * t.sum(1, keepdim=True) - t) / (tp * n)
    assert float((pred.grad - dgrad).abs().max()) <= 1e-14


def test_state_dict_holds_only_the_student():
    learner, teacher = build_learner()
    sd = learner.state_dict()
    assert sd and all(k.startswith("incr_backbone.") for k in sd)
    assert set(sd) == {"incr_backbone." + k for k in learner.incr_backbone.state_dict()}
    assert learner.need_teacher_model and learner.teacher_model is teacher and learner.teacher_model_hooks is None


def test_weight_adaptation():
    from pointcloudpdf_amd import incremental, synthetic

    learner, teacher = build_learner()
    base = {k: v.clone() for k, v in teacher.state_dict().items()}
    for k in base:   # a base checkpoint distinct from the teacher's current weights
        if base[k].is_floating_point():
            base[k] = base[k] + 0.25
    head = learner.incr_backbone.cls[3].weight.detach().clone()
    trimmed = incremental.trim_base_weight_head(base, learner)
    assert set(trimmed) == set(learner.state_dict())   # every tensor kept: the 13 -> 15 head partially
    w = trimmed["incr_backbone.cls.3.weight"]
    assert w.shape == (15, 32)
    assert torch.equal(w[:13], base["backbone.cls.3.weight"]) and torch.equal(w[13:], head[13:])
    assert torch.equal(trimmed["incr_backbone.cls.3.bias"][:13], base["backbone.cls.3.bias"])
    missing, unexpected = incremental.load_incremental_weight(learner, trimmed, base)
    assert not unexpected and not missing
    for k, v in base.items():
        assert torch.equal(teacher.state_dict()[k], v), k
    assert torch.equal(learner.incr_backbone.cls[3].weight, w)
    assert torch.equal(learner.incr_backbone.enc1[0].linear.weight, base["backbone.enc1.0.linear.weight"])
    # reserve_matched: equal shapes only -- the grown head is left out, and the result loads
    synthetic.fill_parameters_deterministic(learner.incr_backbone, seed=2)
    kept = incremental.reserve_matched(base, learner.state_dict())
    assert "incr_backbone.cls.3.weight" not in kept and "incr_backbone.cls.3.bias" not in kept
    assert "incr_backbone.enc1.0.linear.weight" in kept and len(kept) == len(learner.state_dict()) - 2
    missing, unexpected = incremental.load_incremental_weight(learner, kept, base)
    assert not unexpected and sorted(missing) == ["incr_backbone.cls.3.bias", "incr_backbone.cls.3.weight"]
    # a DDP-style "module." prefix is dropped as the reference's replace_key does
    assert set(incremental.reserve_matched({"module." + k: v for k, v in base.items()}, learner)) == set(kept)


def _incr_metric_numpy(inter, union, target, base, remap, select):
    """engines/hooks/evaluator.py:237-261, 377-405 restated with numpy."""
    k = base + len(remap)
    sel = lambda labels, n: np.isin(np.arange(n), labels)   # noqa: E731  (selected_mask)
    mask_known = ~sel(list(remap), base)
    idx = [remap[s] for s in select if s in remap]
    mask_remap = ~sel(list(remap) + list(remap.values()), k) | sel(idx, k)
    iou, acc = inter / (union + 1e-10), inter / (target + 1e-10)
    return dict(mIoU_known=iou[:base][mask_known].mean(), mAcc_known=acc[:base][mask_known].mean(),
                Acc_known=inter[:base][mask_known].sum() / (target[:base][mask_known] + 1e-10).sum(),
                mIoU_incr=iou[idx].mean(), mAcc_incr=acc[idx].mean(), Acc_incr=inter[idx].sum() / (target[idx].sum() + 1e-10),
                mIoU_remap=iou[mask_remap].mean(), mAcc_remap=acc[mask_remap].mean(),
                Acc_remap=inter[mask_remap].sum() / (target[mask_remap].sum() + 1e-10)), mask_known, mask_remap, idx


@pytest.mark.parametrize("select", [[5, 9], [9]])
def test_incr_evaluator_matches_numpy_restatement(select):
    from pointcloudpdf_amd.evaluator import IncrSegEvaluator

    rng = np.random.RandomState(7)
    ev = IncrSegEvaluator(13, REMAP, select, ignore_index=-1)
    inter, union, target = np.zeros(15), np.zeros(15), np.zeros(15)
    for _ in range(3):
        n = 4000
        logits = torch.from_numpy(rng.randn(n, 15).astype(np.float32))
        lab = torch.from_numpy(rng.randint(-1, 15, n))
        ev.update(logits, lab, loss=torch.tensor(0.5))
        pred, t = logits.argmax(1).numpy(), lab.numpy()
        v = t != -1
        for c in range(15):
            inter[c] += np.sum((pred[v] == c) & (t[v] == c))
            union[c] += np.sum(pred[v] == c) + np.sum(t[v] == c) - np.sum((pred[v] == c) & (t[v] == c))
            target[c] += np.sum(t[v] == c)
    want, mask_known, mask_remap, idx = _incr_metric_numpy(inter, union, target, 13, REMAP, select)
    assert np.array_equal(ev.mask_known, mask_known) and np.array_equal(ev.mask_incr_remap, mask_remap) and ev.incr_label_idx == idx
    got = ev.summary()
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    assert got["loss"] == 0.5 and got["known"]["mIoU"] == got["mIoU_known"]

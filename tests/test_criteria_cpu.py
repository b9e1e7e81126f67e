"""CPU suite: the criteria beyond the plain cross-entropy -- ``segmentor.CrossEntropyLoss`` in full, ``losses.FocalLoss`` / ``DiceLoss`` /
``BinaryFocalLoss``: registry and config building, the torch compositions against the reference's own results
(tests/golden/ops_criteria_ref.npz), and this package's choices where the reference is silent or broken (all rows ignored, the Dice
quirks, reduction="sum").  Tolerance rule: criteria_cases.py."""
import numpy as np
import pytest
import torch

import criteria_cases as cc

CASES = cc.case_ids()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return cc.load(golden_dir)


def crit_cfg(c):
    return [dict(type="CrossEntropyLoss", weight=[0.5 + k / c for k in range(c)], label_smoothing=0.1, loss_weight=1.0, ignore_index=-1),
            dict(type="FocalLoss", gamma=2.0, alpha=0.5, loss_weight=1.0, ignore_index=-1),
            dict(type="DiceLoss", smooth=1, exponent=2, loss_weight=1.0, ignore_index=-1)]


def test_registry_builds_every_class_from_a_config_dict():
    from pointcloudpdf_amd import losses, segmentor
    from pointcloudpdf_amd.registry import LOSSES

    f = LOSSES.build(dict(type="FocalLoss", gamma=1.5, alpha=[0.25, 0.75], reduction="sum", loss_weight=2.0, ignore_index=255))
    assert isinstance(f, losses.FocalLoss) and (f.gamma, f.alpha, f.reduction, f.loss_weight, f.ignore_index) == (1.5, [0.25, 0.75], "sum", 2.0, 255)
    d = LOSSES.build(dict(type="DiceLoss", smooth=0.5, exponent=3))
    assert isinstance(d, losses.DiceLoss) and (d.smooth, d.exponent, d.loss_weight, d.ignore_index) == (0.5, 3, 1.0, -1)
    b = LOSSES.build(dict(type="BinaryFocalLoss", alpha=0.25, logits=False, reduce=False))
    assert isinstance(b, losses.BinaryFocalLoss) and (b.gamma, b.alpha, b.logits, b.reduce, b.loss_weight) == (2.0, 0.25, False, False, 1.0)
    ce = LOSSES.build(dict(type="CrossEntropyLoss", weight=[1.0, 2.0], label_smoothing=0.1, reduction="sum"))
    assert isinstance(ce, segmentor.CrossEntropyLoss) and ce.loss.reduction == "sum" and ce.loss.label_smoothing == 0.1
    crit = segmentor.build_criteria(crit_cfg(5))
    assert [type(c).__name__ for c in crit.criteria] == ["CrossEntropyLoss", "FocalLoss", "DiceLoss"]
    x, y = torch.randn(40, 5), torch.randint(-1, 5, (40,))
    assert torch.equal(crit(x, y), crit.criteria[0](x, y) + crit.criteria[1](x, y) + crit.criteria[2](x, y))


def test_class_weights_stay_out_of_the_state_dict_and_legacy_arguments_map_to_a_reduction():
    from pointcloudpdf_amd import segmentor

    ce = segmentor.CrossEntropyLoss(weight=[1.0, 2.0, 0.5])
    assert ce.state_dict() == {} and torch.equal(ce.loss.weight, torch.tensor([1.0, 2.0, 0.5]))
    assert dict(ce.loss.named_buffers()).keys() == {"weight"}
    with pytest.warns(UserWarning):
        assert segmentor.CrossEntropyLoss(size_average=False).loss.reduction == "sum"
        assert segmentor.CrossEntropyLoss(reduce=False).loss.reduction == "none"


@pytest.mark.parametrize("kind,name", CASES, ids=[n for _, n in CASES])
def test_composition_reproduces_the_reference(golden, kind, name):
    x, target, kw, ref_loss, ref_grad = cc.case(golden, name)
    loss64, grad64 = cc.truth(kind, kw, x, target)
    loss, grad = cc.loss_and_grad(cc.build(kind, kw), x, target)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == tuple(np.shape(ref_loss))
    e_loss, e_ref = cc.err(loss, loss64), cc.err(ref_loss, loss64)
    g_loss, g_ref = cc.err(grad, grad64), cc.err(ref_grad, grad64)
    print(f"{name}: loss error {e_loss:.3e} (reference {e_ref:.3e}), gradient error {g_loss:.3e} (reference {g_ref:.3e})")
    assert e_loss <= cc.bound(e_ref, loss64), (e_loss, e_ref)
    assert g_loss <= cc.bound(g_ref, grad64), (g_loss, g_ref)
    if kind == "ce":   # the same torch call: bit for bit
        assert np.array_equal(loss.numpy(), ref_loss) and np.array_equal(grad.numpy(), ref_grad)


def test_focal_sum_equals_its_float64_restatement():
    """reduction="sum" cannot run in the reference (``Tensor.total``); it is the sum of the terms that "mean" averages."""
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(5)
    x, t = 2.0 * torch.randn(257, 13, generator=g), torch.randint(-1, 13, (257,), generator=g)
    alpha = [0.2 + 0.05 * k for k in range(13)]
    total, mean = losses.FocalLoss(alpha=alpha, reduction="sum"), losses.FocalLoss(alpha=alpha)
    n_valid = int((t != -1).sum())
    assert 0 < n_valid < 257
    want = mean(x.double(), t) * (n_valid * 13)
    assert abs(float(total(x.double(), t)) - float(want)) <= 1e-12 * float(want)
    assert abs(float(total(x, t)) - float(want)) <= cc.FLOOR_ULP * cc.ULP * float(want)


def test_all_rows_ignored():
    from pointcloudpdf_amd import losses, segmentor

    x = torch.randn(9, 4, requires_grad=True)
    t = torch.full((9,), -1)
    for crit in (losses.FocalLoss(), losses.FocalLoss(reduction="sum"), losses.DiceLoss()):
        out = crit(x, t)
        assert isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 0.0   # (the reference's FocalLoss: a python float)
        (g,) = torch.autograd.grad(out, x)
        assert torch.count_nonzero(g) == 0
    assert torch.isnan(segmentor.CrossEntropyLoss(weight=[1.0, 2.0, 3.0, 4.0])(x, t))   # torch's rule for "mean"
    assert float(segmentor.CrossEntropyLoss(reduction="sum")(x, t)) == 0.0


def test_bad_labels():
    from pointcloudpdf_amd import losses

    x = torch.randn(9, 4)
    t = torch.tensor([0, 1, 2, 3, -1, 4, 0, 1, 2])
    assert torch.isnan(losses.FocalLoss()(x, t))
    # Dice clamps (the reference's behaviour): label 4 counts as class 3, label -7 as class 0
    d = losses.DiceLoss()
    t2 = t.clone()
    t2[5] = 3
    assert torch.equal(d(x, t), d(x, t2))
    t[0], t2[0] = -7, 0
    assert torch.equal(d(x, t), d(x, t2))


def test_dice_ignored_class_is_skipped_and_the_divisor_stays_c():
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(6)
    x, t = torch.randn(50, 4, generator=g).double(), torch.randint(0, 4, (50,), generator=g)
    p = torch.softmax(x[t != 2], 1)
    y = torch.nn.functional.one_hot(t[t != 2], 4).double()
    terms = 1 - (2 * (p * y).sum(0) + 1) / ((p * p + y).sum(0) + 1)
    want = (terms[0] + terms[1] + terms[3]) / 4       # class 2 left out, divided by 4 all the same
    assert abs(float(losses.DiceLoss(ignore_index=2)(x, t)) - float(want)) <= 1e-14


def test_constructor_assertions():
    from pointcloudpdf_amd import losses

    for bad in (dict(reduction="none"), dict(alpha=1), dict(gamma=2), dict(loss_weight=1), dict(ignore_index=None)):
        with pytest.raises(AssertionError):
            losses.FocalLoss(**bad)
    for bad in (0, 1, 1.5):
        with pytest.raises(AssertionError):
            losses.BinaryFocalLoss(alpha=bad)


def test_higher_dimensional_input_is_flattened_like_the_reference():
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(8)
    x, t = torch.randn(2, 5, 7, generator=g), torch.randint(-1, 5, (2, 7), generator=g)
    flat = x.transpose(0, 1).reshape(5, -1).transpose(0, 1)
    for crit in (losses.FocalLoss(), losses.DiceLoss()):
        assert torch.equal(crit(x, t), crit(flat, t.reshape(-1)))


def test_step_from_a_config_with_the_new_criteria_runs_on_the_cpu(use_oracle):
    from pointcloudpdf_amd import engine, synthetic

    pas = dict(condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100, slide_window=True)
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg26", in_channels=9, num_classes=20), criteria=crit_cfg(20)),
               recognizer=dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=crit_cfg(21), loss_weight=0.04,
                               step_loss_weight=False, num_classes=20, start_epoch=0, kp_ball_radius=0.1, kp_max_neighbor=64,
                               adaptive_radius=False, **pas))
    step = engine.build_open_seg_step(cfg)
    names = ["CrossEntropyLoss", "FocalLoss", "DiceLoss"]
    assert [type(c).__name__ for c in step.model.criteria.criteria] == names
    assert [type(c).__name__ for c in step.recognizer.criteria.criteria] == names
    assert not [k for k in step.state_dict() if "criteria" in k]
    synthetic.fill_parameters_deterministic(step, seed=4)
    step.train()
    batch = synthetic.make_batch([2048, 1600], first_scene_id=20, kind="scannet", unknown=(4, 7, 14, 16))
    np.random.seed(0)
    torch.manual_seed(0)
    out = step(batch)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]).item() and float(out["recognizer_loss"]) > 0
    logits = step.hooks["backbone"]["forward_output"].detach()
    parts = [c(logits, batch["segment"]) for c in step.model.criteria.criteria]
    assert all(float(p) > 0 for p in parts)
    assert torch.allclose(out["model_loss"].detach(), parts[0] + parts[1] + parts[2], rtol=1e-6, atol=0)
    grads = [p.grad for p in step.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


def test_integration_registers_the_classes_into_a_pointcept_registry(monkeypatch):
    import sys
    import types

    from pointcloudpdf_amd import integration, losses, segmentor

    class Registry:
        def __init__(self):
            self.modules = {}

        def register_module(self, name=None, force=False, module=None):
            assert force or name not in self.modules
            self.modules[name] = module

    reg = Registry()
    for nm in ["pointcept", "pointcept.models", "pointcept.models.losses", "pointcept.models.losses.builder"]:
        m = types.ModuleType(nm)
        m.__path__ = []
        monkeypatch.setitem(sys.modules, nm, m)
    sys.modules["pointcept.models.losses.builder"].LOSSES = reg
    integration.register_criteria_into_pointcept(cross_entropy=False)
    new = {"FocalLoss": losses.FocalLoss, "DiceLoss": losses.DiceLoss, "BinaryFocalLoss": losses.BinaryFocalLoss}
    assert reg.modules == new
    integration.register_criteria_into_pointcept()
    assert reg.modules == dict(new, CrossEntropyLoss=segmentor.CrossEntropyLoss)

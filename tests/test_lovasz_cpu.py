"""CPU suite: ``losses.LovaszLoss`` -- registry and config building, the torch restatement against the reference's own results
(tests/golden/ops_lovasz_ref.npz, written by make_golden_lovasz.py), and this package's choices where the reference leaves the result open
(ties, all rows ignored, per_image)."""
import os

import numpy as np
import pytest
import torch

LOVASZ = dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)
CE_LOVASZ = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1), LOVASZ]
PARITY = 1e-4   # of the tensor's largest magnitude: the project's parity bar


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ops_lovasz_ref.npz"))


def rel_err(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def test_registry_builds_the_reference_config_entry():
    import pointcloudpdf_amd  # noqa: F401
    from pointcloudpdf_amd import losses, segmentor
    from pointcloudpdf_amd.registry import LOSSES

    loss = LOSSES.build(dict(LOVASZ))
    assert isinstance(loss, losses.LovaszLoss) and (loss.mode, loss.ignore_index, loss.loss_weight, loss.class_seen) == ("multiclass", -1, 1.0, None)
    crit = segmentor.build_criteria(CE_LOVASZ)
    assert [type(c).__name__ for c in crit.criteria] == ["CrossEntropyLoss", "LovaszLoss"]
    x, y = torch.randn(40, 5), torch.randint(0, 5, (40,))
    assert torch.equal(crit(x, y), crit.criteria[0](x, y) + crit.criteria[1](x, y))


def test_step_from_a_config_with_both_criteria_runs_on_the_cpu(use_oracle):
    from pointcloudpdf_amd import engine, synthetic

    pas = dict(condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100, slide_window=True)
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg26", in_channels=9, num_classes=20), criteria=CE_LOVASZ),
               recognizer=dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=CE_LOVASZ, loss_weight=0.04,
                               step_loss_weight=False, num_classes=20, start_epoch=0, kp_ball_radius=0.1, kp_max_neighbor=64,
                               adaptive_radius=False, **pas))
    step = engine.build_open_seg_step(cfg)
    assert [type(c).__name__ for c in step.model.criteria.criteria] == ["CrossEntropyLoss", "LovaszLoss"]
    assert [type(c).__name__ for c in step.recognizer.criteria.criteria] == ["CrossEntropyLoss", "LovaszLoss"]
    synthetic.fill_parameters_deterministic(step, seed=4)
    step.train()
    batch = synthetic.make_batch([2048, 1600], first_scene_id=20, kind="scannet", unknown=(4, 7, 14, 16))
    np.random.seed(0)
    torch.manual_seed(0)
    out = step(batch)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]).item() and float(out["recognizer_loss"]) > 0
    # the Lovasz term is there: the model's loss is the sum of the two criteria on the logits the hook kept
    logits = step.hooks["backbone"]["forward_output"].detach()
    ce, lov = step.model.criteria.criteria
    assert torch.allclose(out["model_loss"].detach(), ce(logits, batch["segment"]) + lov(logits, batch["segment"]), rtol=1e-6, atol=0)
    assert float(lov(logits, batch["segment"])) > 0
    grads = [p.grad for p in step.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


def test_multiclass_equals_the_reference(golden):
    from pointcloudpdf_amd import losses

    for name in golden["multiclass_cases"].tolist():
        seen = golden[f"{name}_class_seen"].tolist() or None
        loss = losses.LovaszLoss(mode="multiclass", class_seen=seen, ignore_index=int(golden["ignore_index"]))
        x = torch.from_numpy(golden[f"{name}_logits"]).requires_grad_()
        out = loss(x, torch.from_numpy(golden[f"{name}_labels"]))
        out.backward()
        assert out.dim() == 0 and out.dtype == torch.float32
        e_loss, e_grad = rel_err(out.detach().numpy(), golden[f"{name}_loss"]), rel_err(x.grad.numpy(), golden[f"{name}_grad"])
        print(name, "loss", e_loss, "grad", e_grad)
        assert e_loss <= PARITY and e_grad <= PARITY, (name, e_loss, e_grad)


def test_hinge_modes_equal_the_reference(golden):
    from pointcloudpdf_amd import losses

    for name in golden["hinge_cases"].tolist():
        loss = losses.LovaszLoss(mode=str(golden[f"{name}_mode"]), ignore_index=int(golden["ignore_index"]))
        x = torch.from_numpy(golden[f"{name}_logits"]).requires_grad_()
        out = loss(x, torch.from_numpy(golden[f"{name}_labels"]))
        out.backward()
        e_loss, e_grad = rel_err(out.detach().numpy(), golden[f"{name}_loss"]), rel_err(x.grad.numpy(), golden[f"{name}_grad"])
        print(name, "loss", e_loss, "grad", e_grad)
        assert e_loss <= PARITY and e_grad <= PARITY, (name, e_loss, e_grad)


def test_loss_weight_and_float64():
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(90, 6, generator=g), torch.randint(0, 6, (90,), generator=g)
    one = losses.LovaszLoss(mode="multiclass", ignore_index=-1)(x, y)
    assert torch.equal(losses.LovaszLoss(mode="multiclass", ignore_index=-1, loss_weight=0.25)(x, y), one * 0.25)
    d = losses.lovasz_softmax_reference(x, y, -1, dtype=torch.float64)
    assert d.dtype == torch.float64 and abs(float(d) - float(one)) <= 1e-6 * float(d)
    # given probabilities: the same loss
    p = torch.softmax(x, 1)
    assert torch.allclose(losses.lovasz_softmax_reference(None, y, -1, probas=p), one, rtol=1e-6, atol=0)


def test_ties_loss_is_invariant_under_row_permutation():
    """Duplicated rows give equal errors: the loss does not depend on their order (the subgradient does -- the stable order is this
    package's choice)."""
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(6)
    base = 2.0 * torch.randn(40, 7, generator=g)
    x = base.repeat(5, 1)                                   # every row five times
    y = torch.randint(0, 7, (40,), generator=g).repeat(5)   # ... with its label: equal errors in every class
    loss = losses.LovaszLoss(mode="multiclass", ignore_index=-1)
    want = float(loss(x, y))
    for seed in range(4):
        perm = torch.randperm(200, generator=torch.Generator().manual_seed(seed))
        got = float(loss(x[perm], y[perm]))
        assert abs(got - want) <= 1e-6 * abs(want), (seed, got, want)


def hand_dprob(p, y, earlier_row_first):
    """d loss / d P of the module docstring's definition, written out with numpy: per class the rows ordered by descending error, equal
    errors by ascending (``earlier_row_first``) or descending row index; rank i gets sign(p - fg) * (J_i - J_{i-1}) / #classes."""
    n, c = p.shape
    out = np.zeros((n, c))
    classes = sorted(set(y.tolist()))
    rows = np.arange(n)
    for k in classes:
        fg = (y == k).astype(np.float64)
        e = np.abs(fg - p[:, k].astype(np.float64))
        order = np.lexsort((rows if earlier_row_first else -rows, -e))     # last key first: -e, then the row index
        f = fg[order]
        g, seen, pos = f.sum(), np.cumsum(f), np.arange(1, n + 1)
        jac = 1.0 - (g - seen) / (g + pos - seen)
        step = np.diff(jac, prepend=0.0)
        out[order, k] = np.sign(p[order, k] - f) * step / len(classes)
    return out


def test_tied_errors_take_their_ranks_in_row_order():
    """This package's choice on ties: among equal errors the EARLIER row takes the earlier rank.  Rows r and r + 30 carry the same
    probabilities and the same label, so in every class their errors are equal and their ranks adjacent; the Jaccard step differs from one
    rank to the next, so the two rows get different gradients and the tie rule decides which row gets which."""
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(8)
    p = torch.softmax(2.0 * torch.randn(30, 5, generator=g), 1).repeat(2, 1)
    y = torch.randint(0, 5, (30,), generator=g).repeat(2)
    leaf = p.clone().requires_grad_()
    losses.lovasz_softmax_reference(None, y, -1, probas=leaf, dtype=torch.float64).backward()
    got = leaf.grad.double().numpy()
    stable, reverse = hand_dprob(p.numpy(), y.numpy(), True), hand_dprob(p.numpy(), y.numpy(), False)
    scale = np.abs(stable).max()
    assert np.abs(got - stable).max() <= 1e-6 * scale, np.abs(got - stable).max() / scale
    # the rule matters here: the other order of the ties is a different gradient, far outside that bound ...
    assert np.abs(reverse - stable).max() > 1e-2 * scale
    # ... and of every background pair that still has foreground behind it (I > 0) the earlier row holds the earlier rank, where the
    # Jaccard step I / (U (U - 1)) is the larger one (same I, U one less); a foreground pair shares its step 1 / U
    pairs = [(r, k) for r in range(30) for k in range(5) if k != int(y[r]) and got[r, k] != 0.0]
    assert len(pairs) >= 30 and all(abs(got[r, k]) > abs(got[r + 30, k]) for r, k in pairs)
    assert all(got[r, int(y[r])] == got[r + 30, int(y[r])] for r in range(30))
    # the module (fp32, from logits) makes the same choice
    x = torch.log(p).clone().requires_grad_()
    losses.LovaszLoss(mode="multiclass", ignore_index=-1)(x, y).backward()
    pd = p.double().numpy()
    want = pd * (stable - (stable * pd).sum(1, keepdims=True))
    assert np.abs(x.grad.double().numpy() - want).max() <= PARITY * np.abs(want).max()


def test_all_rows_ignored_is_a_scalar_zero_with_zero_gradient():
    from pointcloudpdf_amd import losses

    x = torch.randn(12, 4, requires_grad=True)
    out = losses.LovaszLoss(mode="multiclass", ignore_index=-1)(x, torch.full((12,), -1))
    out.backward()
    assert out.dim() == 0 and float(out.detach()) == 0.0 and x.grad is not None and not x.grad.any()
    h = torch.randn(9, requires_grad=True)
    out = losses.LovaszLoss(mode="binary", ignore_index=-1)(h, torch.full((9,), -1))
    out.backward()
    assert out.dim() == 0 and float(out.detach()) == 0.0 and not h.grad.any()


def test_bad_label_is_nan_and_bad_arguments_raise():
    from pointcloudpdf_amd import losses

    x = torch.randn(12, 4)
    y = torch.randint(0, 4, (12,))
    y[3] = 4
    assert torch.isnan(losses.LovaszLoss(mode="multiclass", ignore_index=-1)(x, y))
    with pytest.raises(NotImplementedError):
        losses.LovaszLoss(mode="multiclass", per_image=True)
    with pytest.raises(ValueError):
        losses.LovaszLoss(mode="softmax")


def test_integration_registers_the_loss_into_a_pointcept_registry(monkeypatch):
    import sys
    import types

    from pointcloudpdf_amd import integration, losses

    class Registry:
        def __init__(self):
            self.modules = {}

        def register_module(self, name=None, force=False, module=None):
            assert force or name not in self.modules
            self.modules[name] = module

    reg = Registry()
    names = ["pointcept", "pointcept.models", "pointcept.models.losses", "pointcept.models.losses.builder"]
    for nm in names:
        m = types.ModuleType(nm)
        m.__path__ = []
        monkeypatch.setitem(sys.modules, nm, m)
    sys.modules["pointcept.models.losses.builder"].LOSSES = reg
    integration.register_losses_into_pointcept()
    assert reg.modules == {"LovaszLoss": losses.LovaszLoss}

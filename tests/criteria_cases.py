"""Shared by test_criteria_cpu.py and test_gpu_criteria.py: the fixture's cases (tests/golden/ops_criteria_ref.npz, written by
make_golden_criteria.py from the reference's own classes), the module and the torch composition of a case, and the tolerance rule.

Tolerance (nothing measured goes into it): for every case the same formula is evaluated in float64; the result under test may be off by
at most 2x the error of the reference's own fp32 result -- the fixture's value, or the fp32 composition where no fixture exists -- and
never has to be closer than FLOOR_ULP fp32 ulps of the largest magnitude of the result (a loss or a gradient element goes through an
exp, a log, a quotient and a final rounding, one ulp each; test_gpu_optim.py uses the same rule with its own floor)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ULP = 2.0 ** -23
FLOOR_ULP = 4
KINDS = {"ce": "CrossEntropyLoss", "focal": "FocalLoss", "dice": "DiceLoss", "bfocal": "BinaryFocalLoss"}


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "ops_criteria_ref.npz"))


def case_ids(golden_dir=os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
    g = load(golden_dir)
    return [(kind, str(name)) for kind in KINDS for name in g[f"{kind}_cases"]]


def case(golden, name):
    """-> inputs (fp32), target, constructor arguments, the reference's loss and gradient (numpy)."""
    kw = json.loads(str(golden[f"{name}_kwargs"]))
    return (torch.from_numpy(golden[f"{name}_logits"]), torch.from_numpy(golden[f"{name}_labels"]), kw,
            golden[f"{name}_loss"], golden[f"{name}_grad"])


def build(kind, kw):
    import pointcloudpdf_amd  # noqa: F401
    from pointcloudpdf_amd import segmentor  # noqa: F401  (fills LOSSES)
    from pointcloudpdf_amd.registry import LOSSES

    return LOSSES.build(dict(type=KINDS[kind], **kw))


def composition(kind, kw, x, target):
    """The torch composition of the package (CE: torch's own function) in x's dtype, on x's device, loss_weight applied."""
    from pointcloudpdf_amd import losses

    kw = dict(kw)
    lw = kw.pop("loss_weight", 1.0)
    if kind == "ce":
        w = kw.get("weight")
        w = None if w is None else torch.tensor(w, dtype=x.dtype, device=x.device)
        return F.cross_entropy(x, target, weight=w, ignore_index=kw.get("ignore_index", -1), reduction=kw.get("reduction", "mean"),
                               label_smoothing=kw.get("label_smoothing", 0.0)) * lw
    if kind == "focal":
        return losses.focal_loss_reference(x, target, kw.get("gamma", 2.0), kw.get("alpha", 0.5), kw.get("reduction", "mean"),
                                           kw.get("ignore_index", -1)) * lw
    if kind == "dice":
        return losses.dice_loss_reference(x, target, kw.get("smooth", 1), kw.get("exponent", 2), kw.get("ignore_index", -1)) * lw
    return losses.binary_focal_loss_reference(x, target.to(x.dtype), kw.get("gamma", 2.0), kw.get("alpha", 0.5), kw.get("logits", True),
                                              kw.get("reduce", True)) * lw


def loss_and_grad(fn, x, target):
    """fn(x, target) -> (loss, d sum(loss) / d x), both detached."""
    x = x.detach().clone().requires_grad_()
    out = fn(x, target)
    (out if out.dim() == 0 else out.sum()).backward()
    return out.detach(), x.grad.detach()


def truth(kind, kw, x, target):
    """The float64 evaluation of the case's formula (on x's device)."""
    t64 = target.double() if target.is_floating_point() else target
    return loss_and_grad(lambda a, b: composition(kind, kw, a, b), x.double(), t64)


def err(value, ref64):
    value = torch.as_tensor(value)
    return float((value.double().cpu() - ref64.cpu()).abs().max())


def bound(theirs, ref64):
    return max(2.0 * theirs, FLOOR_ULP * ULP * float(ref64.abs().max()))

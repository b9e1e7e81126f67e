#!/usr/bin/env python3
"""Generate tests/golden/ops_criteria_ref.npz by running the REFERENCE's own criteria.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_criteria.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/losses/misc.py -- CrossEntropyLoss, FocalLoss, DiceLoss, BinaryFocalLoss, over a stub ``builder`` module whose
    ``LOSSES.register_module()`` is the identity (as make_golden_lovasz.py).  The reference's CrossEntropyLoss constructor calls
    ``.cuda()`` on its weight tensor; the build container has no GPU, so that call is a no-op while the object is constructed.
Cases: logits ``2 * randn`` in fp32, one seed per case, CPU.  Stored per case: the inputs, the constructor arguments (as a JSON
string), the reference's fp32 loss and its fp32 input gradient (of the sum, where the result is elementwise).  The file has to stay
small, so 65 classes come with 63 rows and 1500 rows with 2 classes.  ``FocalLoss(reduction="sum")`` and ``SmoothCELoss`` are absent: the
reference raises AttributeError (``Tensor.total``) on every call of either.  An all-ignored FocalLoss returns the python float 0.0
without a graph: stored as loss 0 with a zero gradient.
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (where the reference tree lives)

REF = mg.REF
IGNORE = -1

# name: (N, C, share of ignored rows (1.0: all), seed, constructor arguments)
CE = {
    "ce_n1_c2_weight": (1, 2, 0.0, 101, dict(weight=[0.5, 2.0])),
    "ce_n2_c13_smooth": (2, 13, 0.0, 102, dict(label_smoothing=0.1)),
    "ce_n63_c14_weight_smooth": (63, 14, 0.1, 103, dict(weight="ramp", label_smoothing=0.1)),
    "ce_n257_c13_weight": (257, 13, 0.1, 104, dict(weight="ramp")),
    "ce_n63_c65_plain": (63, 65, 0.0, 105, dict()),
    "ce_n63_c65_weight_smooth": (63, 65, 0.1, 106, dict(weight="ramp", label_smoothing=0.2)),
    "ce_n1500_c2_sum": (1500, 2, 0.1, 107, dict(weight="ramp", reduction="sum")),
    "ce_n257_c14_none": (257, 14, 0.1, 108, dict(weight="ramp", label_smoothing=0.1, reduction="none")),
    "ce_n63_c2_smooth_sum": (63, 2, 0.0, 109, dict(label_smoothing=0.3, reduction="sum")),
    "ce_n63_c13_all_ignored_sum": (63, 13, 1.0, 110, dict(weight="ramp", label_smoothing=0.1, reduction="sum")),
}
FOCAL = {
    "focal_n1_c2": (1, 2, 0.0, 201, dict()),
    "focal_n2_c13_list": (2, 13, 0.0, 202, dict(alpha="ramp")),
    "focal_n63_c14": (63, 14, 0.1, 203, dict(gamma=1.5, alpha=0.25)),
    "focal_n257_c13_list": (257, 13, 0.1, 204, dict(alpha="ramp", gamma=2.0)),
    "focal_n63_c65": (63, 65, 0.0, 205, dict()),
    "focal_n1500_c2": (1500, 2, 0.1, 206, dict(gamma=3.0, alpha=0.75, loss_weight=0.5)),
    "focal_n63_c13_all_ignored": (63, 13, 1.0, 207, dict()),
}
# (absent: classes that no label takes)
DICE = {
    "dice_n1_c2": (1, 2, 0.0, 301, dict(), ()),
    "dice_n2_c13": (2, 13, 0.0, 302, dict(smooth=1, exponent=2), ()),
    "dice_n63_c14_e3": (63, 14, 0.1, 303, dict(smooth=0.5, exponent=3), ()),
    "dice_n257_c13_absent": (257, 13, 0.0, 304, dict(smooth=1, exponent=2), (5,)),
    "dice_n257_c14_ignore_inside": (257, 14, 0.0, 305, dict(smooth=1, exponent=2, ignore_index=3), ()),
    "dice_n63_c65": (63, 65, 0.1, 306, dict(smooth=0.5, exponent=3, loss_weight=2.0), ()),
    "dice_n1500_c2": (1500, 2, 0.1, 307, dict(), ()),
    "dice_n63_c13_all_ignored": (63, 13, 1.0, 308, dict(), ()),
}
# name: (N, soft targets, seed, constructor arguments)
BFOCAL = {
    "bfocal_n1_hard": (1, False, 401, dict()),
    "bfocal_n63_soft": (63, True, 402, dict(gamma=1.5, alpha=0.25)),
    "bfocal_n257_hard_elementwise": (257, False, 403, dict(reduce=False)),
    "bfocal_n1500_soft_prob": (1500, True, 404, dict(logits=False)),
    "bfocal_n257_hard_prob_elementwise": (257, False, 405, dict(logits=False, reduce=False, gamma=3.0, alpha=0.75)),
    "bfocal_n1500_hard": (1500, False, 406, dict(loss_weight=0.5)),
}


def load_reference():
    pkg = types.ModuleType("ref_losses")
    pkg.__path__ = []
    builder = types.ModuleType("ref_losses.builder")

    class _Registry:
        @staticmethod
        def register_module(*a, **k):
            return lambda cls: cls

    builder.LOSSES = _Registry()
    sys.modules["ref_losses"], sys.modules["ref_losses.builder"] = pkg, builder
    spec = importlib.util.spec_from_file_location("ref_losses.misc", os.path.join(REF, "pointcept/models/losses/misc.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_losses.misc"] = mod
    spec.loader.exec_module(mod)
    return mod


def ramp(c):
    """Class vector 'ramp': c values in (0.2, 0.9), none equal."""
    return [round(0.2 + 0.7 * (k + 0.5) / c, 4) for k in range(c)]


def resolve(kw, c):
    return {k: (ramp(c) if isinstance(v, str) and v == "ramp" else v) for k, v in kw.items()}


def make_rows(n, c, ignored, seed, absent=(), ignore=IGNORE):
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(n, c, generator=g)
    present = torch.tensor([k for k in range(c) if k not in absent])
    labels = present[torch.randint(0, len(present), (n,), generator=g)]
    if ignored >= 1.0:
        labels[:] = ignore
    elif ignored > 0:
        labels[torch.randperm(n, generator=g)[: max(1, int(round(ignored * n)))]] = ignore
    return logits, labels


def run(module, x0, target):
    x = x0.clone().requires_grad_()
    loss = module(x, target)
    if not isinstance(loss, torch.Tensor):   # FocalLoss with every row ignored: the python float 0.0
        return np.float32(loss), np.zeros(tuple(x0.shape), dtype=np.float32)
    (loss if loss.dim() == 0 else loss.sum()).backward()   # elementwise results: the gradient of their sum
    return loss.detach().numpy(), x.grad.numpy()


def main():
    ref = load_reference()
    out = {"ignore_index": np.int64(IGNORE)}
    for kind, cases in (("ce", CE), ("focal", FOCAL), ("dice", DICE), ("bfocal", BFOCAL)):
        out[f"{kind}_cases"] = np.array(sorted(cases))

    def store(name, kw, logits, labels, loss, grad):
        out[f"{name}_logits"], out[f"{name}_labels"] = logits.numpy(), labels.numpy()
        out[f"{name}_kwargs"] = np.array(json.dumps(kw))
        out[f"{name}_loss"], out[f"{name}_grad"] = loss, grad
        print(name, "loss", float(np.asarray(loss).reshape(-1)[0]), "max |grad|", float(np.abs(grad).max()))

    for name, (n, c, ignored, seed, kw) in CE.items():
        kw = resolve(kw, c)
        logits, labels = make_rows(n, c, ignored, seed)
        cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self   # (no GPU here: the constructor's weight.cuda() keeps the CPU tensor)
        try:
            module = ref.CrossEntropyLoss(ignore_index=IGNORE, **kw)
        finally:
            torch.Tensor.cuda = cuda
        store(name, kw, logits, labels, *run(module, logits, labels))
    for name, (n, c, ignored, seed, kw) in FOCAL.items():
        kw = resolve(kw, c)
        logits, labels = make_rows(n, c, ignored, seed)
        store(name, kw, logits, labels, *run(ref.FocalLoss(ignore_index=IGNORE, **kw), logits, labels))
    for name, (n, c, ignored, seed, kw, absent) in DICE.items():
        kw = dict(kw)
        ignore = kw.setdefault("ignore_index", IGNORE)
        logits, labels = make_rows(n, c, ignored, seed, absent, ignore=ignore)
        store(name, kw, logits, labels, *run(ref.DiceLoss(**kw), logits, labels))
    for name, (n, soft, seed, kw) in BFOCAL.items():
        g = torch.Generator().manual_seed(seed)
        pred = 2.0 * torch.randn(n, generator=g)
        if not kw.get("logits", True):
            pred = torch.sigmoid(pred)
        target = torch.rand(n, generator=g) if soft else torch.randint(0, 2, (n,), generator=g).float()
        store(name, kw, pred, target, *run(ref.BinaryFocalLoss(**kw), pred, target))
    path = os.path.join(HERE, "ops_criteria_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

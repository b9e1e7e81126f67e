#!/usr/bin/env python3
"""Generate tests/golden/ops_lovasz_ref.npz by running the REFERENCE's own ``LovaszLoss``.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_lovasz.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/losses/lovasz.py -- LovaszLoss, over a stub ``builder`` module whose ``LOSSES.register_module()`` is the identity
    (the real one imports the registry machinery of the whole package).
Cases: logits ``2 * randn`` in fp32, one seed per case, CPU.  Stored per case: logits, labels, the reference's fp32 loss and its fp32
logits gradient, plus the constructor arguments.  The script asserts that no multiclass case holds two equal errors inside a class:
the reference's ``torch.sort(descending=True)`` is unstable, so its gradient is only defined without ties (large cases have ties --
465 at 70,000 rows with this recipe -- and stay out of the fixture).
"""
import importlib.util
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

# name: (N, C, absent classes, share of ignored rows, class_seen, seed)
MULTICLASS = {
    "n1_c3": (1, 3, (), 0.0, None, 11),
    "n2_c2": (2, 2, (), 0.0, None, 12),
    "n63_c5": (63, 5, (), 0.0, None, 13),
    "n257_c13_absent": (257, 13, (5, 9), 0.0, None, 14),
    "n1500_c14": (1500, 14, (), 0.0, None, 15),
    "n2500_c20_absent": (2500, 20, (17,), 0.0, None, 19),   # (seeds 16-18 hold equal errors: the assertion below)
    "n257_c13_ignored": (257, 13, (), 0.1, None, 17),
    "n257_c13_seen": (257, 13, (), 0.1, (0, 2, 3, 7, 12), 18),
}
# name: (mode, shape, share of ignored elements, seed)
HINGE = {
    "hinge_binary": ("binary", (300,), 0.0, 21),
    "hinge_multilabel_ignored": ("multilabel", (200, 4), 0.1, 22),
}
IGNORE = -1


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
    spec = importlib.util.spec_from_file_location("ref_losses.lovasz", os.path.join(REF, "pointcept/models/losses/lovasz.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_losses.lovasz"] = mod
    spec.loader.exec_module(mod)
    return mod


def make_multiclass(n, c, absent, ignored, seed):
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(n, c, generator=g)
    present = torch.tensor([k for k in range(c) if k not in absent])
    labels = present[torch.randint(0, len(present), (n,), generator=g)]
    if ignored > 0:
        labels[torch.randperm(n, generator=g)[: max(1, int(round(ignored * n)))]] = IGNORE
    return logits, labels


def count_ties(logits, labels):
    p = torch.softmax(logits, 1)[labels != IGNORE]
    lab = labels[labels != IGNORE]
    ties = 0
    for c in lab.unique().tolist():
        e = ((lab == c).float() - p[:, c]).abs()
        ties += e.numel() - e.unique().numel()
    return ties


def main():
    ref = load_reference()
    out = {"multiclass_cases": np.array(sorted(MULTICLASS)), "hinge_cases": np.array(sorted(HINGE)), "ignore_index": np.int64(IGNORE)}
    for name, (n, c, absent, ignored, seen, seed) in MULTICLASS.items():
        logits, labels = make_multiclass(n, c, absent, ignored, seed)
        assert count_ties(logits, labels) == 0, (name, "equal errors inside a class: the reference's gradient is undefined")
        x = logits.clone().requires_grad_()
        loss = ref.LovaszLoss(mode="multiclass", class_seen=None if seen is None else list(seen), ignore_index=IGNORE)(x, labels)
        loss.backward()
        out[f"{name}_logits"], out[f"{name}_labels"] = logits.numpy(), labels.numpy()
        out[f"{name}_loss"], out[f"{name}_grad"] = loss.detach().numpy(), x.grad.numpy()
        out[f"{name}_class_seen"] = np.array([] if seen is None else seen, dtype=np.int64)
        print(name, "loss", float(loss.detach()), "max |grad|", float(x.grad.abs().max()))
    for name, (mode, shape, ignored, seed) in HINGE.items():
        g = torch.Generator().manual_seed(seed)
        logits = 2.0 * torch.randn(*shape, generator=g)
        labels = torch.randint(0, 2, shape, generator=g)
        if ignored > 0:
            labels.view(-1)[torch.randperm(labels.numel(), generator=g)[: int(round(ignored * labels.numel()))]] = IGNORE
        x = logits.clone().requires_grad_()
        loss = ref.LovaszLoss(mode=mode, ignore_index=IGNORE)(x, labels)
        loss.backward()
        out[f"{name}_mode"] = np.array(mode)
        out[f"{name}_logits"], out[f"{name}_labels"] = logits.numpy(), labels.numpy()
        out[f"{name}_loss"], out[f"{name}_grad"] = loss.detach().numpy(), x.grad.numpy()
        print(name, "loss", float(loss.detach()), "max |grad|", float(x.grad.abs().max()))
    path = os.path.join(HERE, "ops_lovasz_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

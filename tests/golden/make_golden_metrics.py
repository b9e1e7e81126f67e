#!/usr/bin/env python3
"""Generate tests/golden/ops_metrics_ref.npz by running the REFERENCE's own evaluation helpers.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_metrics.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/utils/misc.py -- ``aupr_and_auroc`` (with its sklearn calls) and ``intersection_and_union_gpu``.
Every case is rebuilt from its seed by ``make_case`` below (NumPy's RandomState streams are stable), which the tests import too: the
fixture stores the case table's expected histograms, AUPR / AUROC and positive / negative counts only.

Where the reference cannot be asked as is:
  * +-inf scores: sklearn refuses non-finite scores.  The areas depend on the ORDER of the scores and their ties alone, so the reference
    is given +-FLT_MAX in their place (the case holds no other score of that size).
  * no negative row: ``roc_auc_score`` raises.  Expected AUROC = NaN, AUPR = sklearn's ``average_precision_score`` on the same input.
  * no positive row / every row ignored: the reference returns (None, None) -> stored as NaN with n_pos = 0.
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np  # noqa: E402

K = 13
UNKNOWN = (5, 9)
IGNORE = -1
TILE, SCAN_CHUNK, RADIX = 2048, 1024, 256      # csrc/tile_sort.h: keys per sort tile, words per first-level scan workgroup, digits
# The (digit, tile) scan has one word per digit and tile: its second level (one workgroup, 256 lanes) gives a lane more than one chunk once
# there are more than 256 chunks, i.e. more than 256 * SCAN_CHUNK / RADIX = 1024 tiles = 2,097,152 rows.
DEEP = TILE * (256 * SCAN_CHUNK // RADIX) + 1

# name: (rows, kind, seed)
CASES = {
    "n1": (1, "plain", 101), "n2": (2, "plain", 102), "n63": (63, "plain", 103), "n64": (64, "plain", 104), "n65": (65, "plain", 105),
    "n2047": (2047, "plain", 106), "n2048": (2048, "plain", 107), "n2049": (2049, "plain", 108), "n3tiles1": (3 * TILE + 1, "plain", 109),
    "equal": (5000, "equal", 110), "distinct": (5000, "distinct", 111), "eighths": (5000, "eighths", 112),
    "thousandths": (300000, "thousandths", 113),
    "mixed_sign": (5000, "mixed", 114), "zeros": (5000, "zeros", 115), "inf": (5000, "inf", 116),
    "no_pos": (5000, "no_pos", 117), "no_neg": (5000, "no_neg", 118), "all_ignored": (5000, "all_ignored", 119),
    "outside": (5000, "outside", 120),
    "deep_scan": (DEEP, "thousandths", 121),
}


def make_case(name):
    """-> pred (n) int64, score (n) float32, target (n) int64 of one case."""
    n, kind, seed = CASES[name]
    rng = np.random.RandomState(seed)
    target = rng.randint(0, K, n).astype(np.int64)
    if kind == "no_pos":
        target[np.isin(target, UNKNOWN)] = 4
    elif kind == "no_neg":
        target = np.asarray(UNKNOWN, dtype=np.int64)[rng.randint(0, len(UNKNOWN), n)]
    pos = np.isin(target, UNKNOWN)
    score = (rng.rand(n) + 0.5 * pos).astype(np.float32)
    pred = np.where(rng.rand(n) < 0.7, target, rng.randint(0, K, n)).astype(np.int64)
    if kind == "equal":
        score[:] = 0.5
    elif kind == "distinct":
        score = (np.argsort(np.argsort(rng.rand(n) + 0.5 * pos, kind="stable"), kind="stable") / np.float64(n)).astype(np.float32)   # ranks
        assert np.unique(score).size == n
    elif kind == "eighths":
        score = (np.round(score * 8) / 8).astype(np.float32)
    elif kind == "thousandths":
        score = (np.round(score * 1000) / 1000).astype(np.float32)
    elif kind == "mixed":
        score = (score - np.float32(0.7)).astype(np.float32)
    elif kind == "zeros":
        score = np.asarray([-0.0, 0.0, -1.0, 1.0, -0.0, 0.0], dtype=np.float32)[rng.randint(0, 6, n)]
        score[pos & (rng.rand(n) < 0.3)] = 1.0
    elif kind == "inf":
        score = (score - np.float32(0.7)).astype(np.float32)
        r = rng.rand(n)
        score[r < 0.05] = np.inf
        score[r > 0.95] = -np.inf
    elif kind == "outside":
        r = rng.rand(n)
        target[r < 0.05] = rng.randint(K, K + 3, int((r < 0.05).sum()))
        target[(r >= 0.05) & (r < 0.08)] = -3
        q = rng.rand(n)
        pred[q < 0.05] = K + 1
        pred[(q >= 0.05) & (q < 0.08)] = -2
        pred[(q >= 0.08) & (q < 0.10)] = target[(q >= 0.08) & (q < 0.10)]   # (an out-of-range hit is no intersection)
    if kind == "all_ignored":
        target[:] = IGNORE
    elif n > 1:
        target[rng.rand(n) < 0.08] = IGNORE
    return pred, score, target


def load_reference():
    import make_golden as mg  # (where the reference tree lives)

    spec = importlib.util.spec_from_file_location("ref_misc", os.path.join(mg.REF, "pointcept/utils/misc.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_misc"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, HERE)
    import sklearn.metrics
    import torch

    misc = load_reference()
    out = {"cases": np.array(sorted(CASES)), "num_classes": np.int64(K), "unknown": np.array(UNKNOWN, dtype=np.int64), "ignore_index": np.int64(IGNORE)}
    fmax = np.finfo(np.float32).max
    for name in CASES:
        pred, score, target = make_case(name)
        i, u, t = misc.intersection_and_union_gpu(torch.from_numpy(pred).float(), torch.from_numpy(target).float(), K, IGNORE)
        out[f"{name}_hist"] = np.stack([i.numpy(), u.numpy(), t.numpy()]).astype(np.int64)
        valid = target != IGNORE
        n_pos = int(np.isin(target[valid], UNKNOWN).sum())
        n_neg = int(valid.sum()) - n_pos
        finite = score.copy()
        if np.isinf(score).any():
            assert np.abs(score[np.isfinite(score)]).max() < 1e30
            finite[score == np.inf], finite[score == -np.inf] = fmax, -fmax
        if n_pos and not n_neg:
            y = np.isin(target[valid], UNKNOWN).astype(np.int64)
            aupr, auroc = sklearn.metrics.average_precision_score(y, finite[valid]), None
        else:
            aupr, auroc = misc.aupr_and_auroc(finite.copy(), target.copy(), list(UNKNOWN), IGNORE)
            assert (aupr is None) == (n_pos == 0)
        out[f"{name}_record"] = np.array([np.nan if aupr is None else aupr, np.nan if auroc is None else auroc, n_pos, n_neg], dtype=np.float64)
        print(name, pred.shape[0], out[f"{name}_record"])
    path = os.path.join(HERE, "ops_metrics_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

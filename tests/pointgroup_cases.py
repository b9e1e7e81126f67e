"""Shared by test_pointgroup_cpu.py, test_gpu_pointgroup.py and golden/make_golden_pointgroup.py: the fixture's model arguments and
stand-in backbone, the hand-built scenes of the kernel tests, and the tolerance rule.

Tolerance (nothing measured goes into it; the rule of criteria_cases.bound / the CAC tests): a float result may be off its float64
evaluation by at most 2x the error of the reference's own fp32 result against that evaluation, and never has to be closer than FLOOR_ULP
fp32 ulps of the largest magnitude of the result.  FLOOR_ULP = 24: a loss term is a sum of ~10^3 rows that each went through a norm, two
quotients and a product (the floor of the issue that introduced the suite)."""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_pointgroup_ref.npz")
ULP = 2.0 ** -23
FLOOR_ULP = 24
RADIUS = 1.5

NUM_CLASSES = 6
IGNORE = (-1, 0, 1)
FEAT = 3 + NUM_CLASSES
WIDTH = 32
MODEL_KW = dict(backbone=dict(type="PG-test-MLP", in_channels=FEAT, out_channels=WIDTH), backbone_out_channels=WIDTH,
                semantic_num_classes=NUM_CLASSES, semantic_ignore_index=-1, segment_ignore_index=IGNORE, instance_ignore_index=-1,
                cluster_thresh=RADIUS, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50, voxel_size=0.05)


class TinyBackbone(nn.Module):
    """The fixture's backbone: a per-point MLP with a BatchNorm over ``data_dict["feat"]`` (the fixture pins PointGroup's wiring, not a
    sparse U-Net again)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin1 = nn.Linear(in_channels, out_channels)
        self.bn = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        self.lin2 = nn.Linear(out_channels, out_channels)

    def forward(self, data_dict):
        return self.lin2(torch.relu(self.bn(self.lin1(data_dict["feat"]))))


def bound(theirs, ref64):
    ref64 = torch.as_tensor(ref64)
    return max(2.0 * float(theirs), FLOOR_ULP * ULP * float(ref64.abs().max()) if ref64.numel() else 0.0)


def err(value, ref64):
    value, ref64 = torch.as_tensor(value).double().cpu(), torch.as_tensor(ref64).double()
    return float((value - ref64).abs().max()) if ref64.numel() else 0.0


# ---- hand-built scenes of the kernel tests: every coordinate a multiple of 0.25, radius 1.5 -> every squared distance exact in fp32 ----
def quarter(rng, n, lo, hi):
    return rng.integers(int(lo * 4), int(hi * 4) + 1, (n, 3)).astype(np.float32) / 4


def scene_strict_radius():
    """Point 0 at the origin; neighbours at distance exactly 1.5 (axis: 1.5; and (1, 1, 0.5): 1 + 1 + 0.25 = 2.25) are outside, the ones
    at 1.25 (and at sqrt(2.1875) = 1.479) inside."""
    xyz = np.array([[0, 0, 0], [1.5, 0, 0], [0, -1.5, 0], [1, 1, 0.5], [1.25, 0, 0], [0, 0, -1.25], [1, 1, 0.25], [0.75, 0.75, 0.75],
                    [40, 40, 40]], np.float32)
    return xyz, [9], {0: [0, 4, 5, 6, 7]}


def scene_saturation():
    """Scene 1: 1,200 points inside one ball, 60 far away, one late point inside the first ball.  Scene 2: 70 coincident points and one at
    distance exactly 1.5, over the coordinates of scene 1."""
    rng = np.random.default_rng(11)
    ball = rng.integers(-1, 2, (1200, 3)).astype(np.float32) / 4      # all within 0.25 * sqrt(3) * 2 < 1.5 of each other
    far = np.float32([200, 200, 200]) + rng.integers(-1, 2, (60, 3)).astype(np.float32) / 4
    late = np.zeros((1, 3), np.float32)
    second = np.concatenate([np.zeros((70, 3), np.float32), np.float32([[0, 1.5, 0]])])
    xyz = np.concatenate([ball, far, late, second])
    return xyz, [1261, 1332]


def scene_label_split():
    rng = np.random.default_rng(12)
    xyz = rng.integers(-1, 2, (120, 3)).astype(np.float32) / 4
    label = (np.arange(120) % 2 == 0).astype(np.int32) * 3 + 2      # 5, 2, 5, 2, ...: the first cluster is the class of point 0
    return xyz, [120], label


def scene_threshold_edges():
    """Coincident groups of 49, 50, 100 and 101 points, far apart."""
    sizes = [49, 50, 100, 101]
    xyz = np.concatenate([np.full((s, 3), 30.0 * i, np.float32) for i, s in enumerate(sizes)])
    return xyz, [int(sum(sizes))], sizes


def scene_chain(n=3000, seed=13):
    """n points on a line at spacing 1.0 (a point sees its two neighbours: 1.0 < 1.5 < 2.0), indices shuffled along it: the worst case of
    the label propagation, one cluster."""
    rng = np.random.default_rng(seed)
    pos = rng.permutation(n).astype(np.float32)
    xyz = np.stack([pos, np.zeros(n, np.float32), np.zeros(n, np.float32)], 1)
    return xyz, [n]


def scene_random(seed=14, sizes=(700, 1, 0, 650)):
    """Mixed densities: sparse points, a dense knot of 1,100+ candidates around some rows (saturated rows next to unsaturated ones), a
    one-point scene and an empty scene in the middle."""
    rng = np.random.default_rng(seed)
    parts = []
    for s in sizes:
        if s > 100:
            knot = 1150 if len(parts) == 0 else 0
            parts.append(np.concatenate([quarter(rng, s - 0, -6, 6), rng.integers(-2, 3, (knot, 3)).astype(np.float32) / 4 + 20]))
        else:
            parts.append(quarter(rng, s, -3, 3))
    ends = np.cumsum([p.shape[0] for p in parts]).tolist()
    xyz = np.concatenate(parts).astype(np.float32)
    return xyz, ends


def batch_vectors(ends):
    ends = np.asarray(ends, np.int64)
    sizes = np.diff(ends, prepend=0)
    return np.repeat(np.arange(len(ends)), sizes).astype(np.int32), np.concatenate([[0], ends]).astype(np.int32)


def random_graph(rng, n=None):
    """A random directed graph with labels in CSR form (rows anywhere in the table, as the reference's atomicAdd leaves them)."""
    n = int(rng.integers(1, 70)) if n is None else n
    lens = np.minimum(rng.integers(0, 6, n), n)
    order = rng.permutation(n)
    start = np.zeros(n, np.int64)
    start[order] = np.cumsum(lens[order]) - lens[order]
    idx = np.zeros(int(lens.sum()), np.int32)
    for r in range(n):
        idx[start[r]:start[r] + lens[r]] = rng.choice(n, lens[r], replace=False)
    label = rng.integers(0, 3, n).astype(np.int32)
    return label, idx, np.stack([start, lens], 1).astype(np.int32)


def same_clusters(a_idx, a_off, b_idx, b_off):
    """Same clusters in the same order; the order of the members inside a cluster is free."""
    a_idx, a_off, b_idx, b_off = (np.asarray(v) for v in (a_idx, a_off, b_idx, b_off))
    if not np.array_equal(a_off, b_off) or a_idx.shape != b_idx.shape:
        return False
    for c in range(len(a_off) - 1):
        sl = slice(a_off[c], a_off[c + 1])
        if not (np.all(a_idx[sl, 0] == c) and np.all(b_idx[sl, 0] == c) and np.array_equal(np.sort(a_idx[sl, 1]), np.sort(b_idx[sl, 1]))):
            return False
    return True

"""Drop-in for the reference's ``libs/pointgroup_ops`` (functions/functions.py): ``ballquery_batch_p`` and ``bfs_cluster``.

Device tensors run the kernels of csrc/point_group.hip and return device tensors.  CPU tensors (the reference model hands
``bfs_cluster`` ``.cpu()`` copies) run the host restatement below: the two reference functions statement by statement in NumPy, which is
also the oracle of the tests.

Two documented differences, neither visible downstream:

* ``start_len[:, 0]`` is the exclusive scan of the row lengths in row order (the reference's starts come from an ``atomicAdd`` and are
  in no particular order); ``meanActive`` only sized the reference's allocation and is ignored.
* On the device the members of a cluster come in ascending index, on the host in the reference's BFS order.  The clusters, their order
  and their offsets are the same ("PointGroup"); nothing downstream reads the order inside a cluster -- ``proposals_pred`` is
  a mask and ``instance_pred`` reads the label of any one member.
"""
from collections import deque

import numpy as np
import torch

from .. import _native

__all__ = ["ballquery_batch_p", "bfs_cluster"]

ROW_CAP = 1000   # bfs_cluster_kernel.cu:22 (int idx_temp[1000]): a row is cut after its first 1,000 hits


# ---- host restatement ----------------------------------------------------------------------------------------------------------------
def ballquery_batch_p_host(coords, batch_idxs, batch_offsets, radius):
    """bfs_cluster_kernel.cu:16-62 for every row: the points k of the row's scene in ascending k with d2 < radius * radius in fp32 (every
    product and sum rounded, as written), the first 1,000 of them.  -> (idx (total) int32, start_len (n, 2) int32)."""
    xyz = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 3)
    batch_idxs = np.asarray(batch_idxs).astype(np.int64)
    batch_offsets = np.asarray(batch_offsets).astype(np.int64)
    n = xyz.shape[0]
    radius2 = np.float32(radius) * np.float32(radius)
    rows, start_len, run = [], np.zeros((n, 2), np.int32), 0
    for p in range(n):
        start, end = batch_offsets[batch_idxs[p]], batch_offsets[batch_idxs[p] + 1]
        d = xyz[p] - xyz[start:end]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        hit = (np.nonzero(d2 < radius2)[0][:ROW_CAP] + start).astype(np.int32)
        rows.append(hit)
        start_len[p] = (run, hit.shape[0])
        run += hit.shape[0]
    if run >= 2 ** 31:
        raise OverflowError("ballquery_batch_p: the table does not fit int32 starts")
    return (np.concatenate(rows) if rows else np.zeros(0, np.int32)), start_len


def bfs_cluster_host(semantic_label, ball_query_idxs, start_len, threshold):
    """bfs_cluster.cpp:53-137: for i ascending, a BFS from every unvisited i along the rows' out-edges to unvisited targets of equal
    label; kept with >= threshold points; clusters in the order found, members in BFS order.
    -> (cluster_idxs (s, 2) int32, cluster_offsets (c + 1) int32)."""
    label = np.asarray(semantic_label).astype(np.int64)
    idx = np.asarray(ball_query_idxs).astype(np.int64)
    start_len = np.asarray(start_len).astype(np.int64).reshape(-1, 2)
    n = start_len.shape[0]
    visited = np.zeros(n, bool)
    clusters = []
    for i in range(n):
        if visited[i]:
            continue
        cc, queue = [i], deque([i])
        visited[i] = True
        while queue:
            cur = queue.popleft()
            start, length = start_len[cur]
            nb = idx[start:start + length]
            nb = nb[(label[nb] == label[cur]) & ~visited[nb]]
            _, first = np.unique(nb, return_index=True)   # (a target listed twice is visited at its first mention)
            nb = nb[np.sort(first)]
            visited[nb] = True
            cc.extend(nb.tolist())
            queue.extend(nb.tolist())
        if len(cc) >= threshold:
            clusters.append(cc)
    offsets = np.zeros(len(clusters) + 1, np.int32)
    offsets[1:] = np.cumsum([len(c) for c in clusters])
    out = np.zeros((int(offsets[-1]), 2), np.int32)
    for c, cc in enumerate(clusters):
        out[offsets[c]:offsets[c + 1], 0] = c
        out[offsets[c]:offsets[c + 1], 1] = cc
    return out, offsets


def min_label_clusters(semantic_label, ball_query_idxs, start_len, threshold):
    """The closed form the kernel computes: L = the least fixed point of L(v) = min(v, min over equal-label edges u -> v of L(u)), i.e.
    L(w) = the smallest index that reaches w; clusters = the classes of L with >= threshold members in ascending root index, members in
    ascending index.  Same partition and cluster order as ``bfs_cluster_host`` (tests/test_pointgroup_cpu.py; DESIGN.md: proof)."""
    label = np.asarray(semantic_label).astype(np.int64)
    idx = np.asarray(ball_query_idxs).astype(np.int64)
    start_len = np.asarray(start_len).astype(np.int64).reshape(-1, 2)
    n = start_len.shape[0]
    src = np.repeat(np.arange(n), start_len[:, 1])
    pos = np.arange(src.shape[0]) - np.repeat(np.cumsum(start_len[:, 1]) - start_len[:, 1], start_len[:, 1]) + np.repeat(start_len[:, 0], start_len[:, 1])
    dst = idx[pos]
    same = label[src] == label[dst]
    src, dst = src[same], dst[same]
    L = np.arange(n)
    rounds = 0
    while True:
        rounds += 1
        new = L.copy()
        np.minimum.at(new, dst, L[src])
        new = np.minimum(new, new[new])
        if np.array_equal(new, L):
            break
        L = new
    size = np.bincount(L, minlength=n)
    roots = np.nonzero((L == np.arange(n)) & (size >= threshold))[0]
    rank = np.full(n, -1)
    rank[roots] = np.arange(roots.shape[0])
    member = np.nonzero(rank[L] >= 0)[0] if n else np.zeros(0, np.int64)
    order = np.argsort(rank[L[member]], kind="stable")
    out = np.stack([rank[L[member]][order], member[order]], 1).astype(np.int32).reshape(-1, 2)
    offsets = np.zeros(roots.shape[0] + 1, np.int32)
    offsets[1:] = np.cumsum(size[roots])
    return out, offsets, rounds


# ---- the two public names --------------------------------------------------------------------------------------------------------------
def ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive=None):
    """coords (n, 3) float, batch_idxs (n) int, batch_offsets (B + 1) int -> (idx (nActive) int32, start_len (n, 2) int32).  The points
    of a scene are contiguous (batch_offsets), as upstream."""
    if coords.device.type == "cpu":
        idx, start_len = ballquery_batch_p_host(coords.detach().numpy(), batch_idxs.numpy(), batch_offsets.numpy(), radius)
        return torch.from_numpy(idx), torch.from_numpy(start_len)
    _native.require_current_device(coords, batch_offsets)
    coords = coords.detach().float().contiguous()
    offset = batch_offsets[1:].to(torch.int32).contiguous()
    return _native.backend_for(coords).pg_ball_table(coords, offset, float(radius))


def bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold):
    """semantic_label (N) int, ball_query_idxs (nActive) int, start_len (N, 2) int -> (cluster_idxs (sumNPoint, 2) int32 = [cluster id,
    point], cluster_offsets (nCluster + 1) int32), on the device of the arguments."""
    if start_len.device.type == "cpu":
        out, offsets = bfs_cluster_host(semantic_label.numpy(), ball_query_idxs.numpy(), start_len.numpy(), int(threshold))
        return torch.from_numpy(out), torch.from_numpy(offsets)
    _native.require_current_device(start_len)
    be = _native.backend_for(start_len)
    return be.pg_cluster(semantic_label.to(torch.int32).contiguous(), ball_query_idxs.to(torch.int32).contiguous(),
                         start_len.to(torch.int32).contiguous(), int(threshold))

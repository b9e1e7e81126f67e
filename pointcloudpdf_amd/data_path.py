"""Data contract either side of the hot path, on the device (second half): ``SphereCrop`` and the offset
collate -- pointcept/datasets/transform.py:929-1025 and pointcept/datasets/utils.py:15-56.

With GridSample (voxelize.py) this closes the per-batch input pipeline voxelise -> crop -> collate without leaving the GPU: at
9 M points/s per GPU the numpy pipeline upstream (argsort of every scene per sample) cannot feed eight GPUs from one host.

* ``sphere_crop`` crops a whole batch of scenes in one pass: squared distances to the scene's centre point, one stable device sort
  by (scene, distance), the first ``point_max`` rows of every scene kept.  Upstream's ``np.argsort`` is unstable, so WHICH of
  several equidistant points survives at the cut is undefined there; everything else (the kept set, the ascending-distance order
  of the kept points, "random" / "center" centre choice, scenes at or below ``point_max`` left untouched) is reproduced.
* ``collate_fn`` / ``point_collate_fn`` are upstream's recursion (tensors concatenated, every key containing "offset" turned into
  cumulative ends, Mix3D merge of neighbouring scenes).
* ``mask_label`` / ``remap_label`` are ``MaskLabel`` / ``RemapLabel`` (transform.py:1145-1206) of the incremental stage on device
  label tensors: lookup-table gathers, no host read (the table is sized by the remapped keys, not by ``segment.max()``).
Plumbing on torch device ops; the arithmetic is a three-term fp32 sum per point -- nothing here is worth a hand-written kernel.
"""
import random
from collections.abc import Mapping, Sequence

import torch

_CROP_KEYS = ("coord", "origin_coord", "grid_coord", "color", "normal", "segment", "instance", "displacement", "strength")


def sphere_crop(data, offset, point_max=80000, sample_rate=None, mode="random", generator=None, centers=None):
    """data: dict of (N, ...) device tensors with "coord" (N, 3); offset (B,) cumulative ends (host list or tensor).
    -> (cropped dict, new offset int32 tensor, kept row indices int64).  ``mode``: "random" | "center" (transform.py:995-1000);
    ``centers`` (B,) row indices override the choice (tests)."""
    coord = data["coord"]
    dev = coord.device
    ends = [int(v) for v in (offset.tolist() if isinstance(offset, torch.Tensor) else offset)]
    starts = [0] + ends[:-1]
    sizes = [e - s for s, e in zip(starts, ends)]
    limits = [int(sample_rate * n) if sample_rate is not None else int(point_max) for n in sizes]
    if centers is None:
        if mode == "center":
            centers = [s + n // 2 for s, n in zip(starts, sizes)]
        elif mode == "random":
            centers = [s + int(torch.randint(n, (1,), generator=generator).item()) for s, n in zip(starts, sizes)]
        else:
            raise NotImplementedError(f"sphere_crop: mode {mode!r} (the sliding 'all' mode of the test pipeline is not a per-batch op)")
    sizes_t = torch.tensor(sizes, device=dev)
    scene = torch.repeat_interleave(torch.arange(len(sizes), device=dev), sizes_t, output_size=coord.shape[0])
    c = coord[torch.tensor(centers, device=dev)][scene]
    d2 = torch.sum(torch.square(coord - c), 1)                                   # np.sum(np.square(coord - center), 1)
    crop = torch.tensor([n > lim for n, lim in zip(sizes, limits)], device=dev)[scene]
    rows = torch.arange(coord.shape[0], device=dev)
    # scenes that are cropped: ascending distance (stable: ties by row); scenes at or below the limit: untouched, original order
    key = torch.where(crop, d2, torch.zeros_like(d2))
    order = torch.argsort(key, stable=True)
    order = order[torch.argsort(scene[order], stable=True)]
    start_t = torch.tensor(starts, device=dev)[scene[order]]
    rank = torch.arange(coord.shape[0], device=dev) - start_t
    keep = rank < torch.tensor(limits, device=dev)[scene[order]]
    kept = order[keep]
    # untouched scenes keep their original order (argsort of the all-zero key is the identity under a stable sort)
    out = {k: (v[kept] if (k in _CROP_KEYS and isinstance(v, torch.Tensor)) else v) for k, v in data.items()}
    new_sizes = [min(n, lim) for n, lim in zip(sizes, limits)]
    new_offset = torch.cumsum(torch.tensor(new_sizes, device=dev), 0).int()
    return out, new_offset, kept


def collate_fn(batch):
    """pointcept/datasets/utils.py:15-41: tensors are concatenated; a list sample gets its length appended and the last column
    becomes the cumulative offset; a dict is collated key by key and every key containing "offset" is accumulated."""
    if not isinstance(batch, Sequence):
        raise TypeError(f"{type(batch)} is not supported.")
    if isinstance(batch[0], torch.Tensor):
        return torch.cat(list(batch))
    if isinstance(batch[0], str):
        return list(batch)
    if isinstance(batch[0], Sequence):
        for data in batch:
            data.append(torch.tensor([data[0].shape[0]], device=data[0].device))
        batch = [collate_fn(samples) for samples in zip(*batch)]
        batch[-1] = torch.cumsum(batch[-1], dim=0).int()
        return batch
    if isinstance(batch[0], Mapping):
        out = {key: collate_fn([d[key] for d in batch]) for key in batch[0]}
        for key in out.keys():
            if "offset" in key:
                out[key] = torch.cumsum(out[key], dim=0)
        return out
    from torch.utils.data.dataloader import default_collate

    return default_collate(batch)


def point_collate_fn(batch, mix_prob=0):
    """pointcept/datasets/utils.py:44-56 (Mix3D: neighbouring scenes merged pairwise with probability ``mix_prob``)."""
    assert isinstance(batch[0], Mapping)
    batch = collate_fn(batch)
    if "offset" in batch.keys():
        if random.random() < mix_prob:
            batch["offset_ori"] = batch["offset"].clone()
            batch["offset"] = torch.cat([batch["offset"][1:-1:2], batch["offset"][-1].unsqueeze(0)], dim=0)
    return batch


def _lookup(segment, table, outside):
    """table[segment] where 0 <= segment < len(table), ``outside`` (a tensor like ``segment`` or a scalar) elsewhere."""
    table = table.to(segment.device, non_blocking=True)
    inside = (segment >= 0) & (segment < table.numel())
    return torch.where(inside, table[segment.clamp(0, table.numel() - 1)], outside)


def mask_label(segment, mask_label=None, mask_to=-1):
    """transform.py:1145-1158 -> ``segment_known``: the labels in ``mask_label`` become ``mask_to``; ``segment`` itself is untouched."""
    if mask_label is None:
        return segment.clone()
    labels = [int(v) for v in mask_label]
    if not labels:
        return segment.clone()
    hit = [False] * (max(labels) + 1)
    for v in labels:
        if v >= 0:
            hit[v] = True
    masked = _lookup(segment, torch.tensor(hit), torch.zeros((), dtype=torch.bool, device=segment.device))
    return torch.where(masked, torch.full_like(segment, mask_to), segment)


def remap_label(segment, remap_dict, remap_select=None, ignore_index=-1):
    """transform.py:1161-1206 -> (``segment_incr_remap``, ``segment_incr``).  ``segment_incr_remap``: every key of ``remap_dict`` replaced by
    its new label, every other label kept; ``segment_incr``: the new label on the remapped points, ``ignore_index`` everywhere else (the
    distillation target's "labelled" rows).  With ``remap_select``, only the selected keys are remapped; the unselected keys become
    ``ignore_index`` in both outputs (:1177-1191).  Labels outside [0, max key] take the identity / ``ignore_index`` entries as well; the
    reference's numpy table would wrap a negative label around to its last entry (no S3DIS label is negative)."""
    keys = [int(k) for k in remap_dict]
    size = max(keys) + 1
    remap, inc = list(range(size)), [ignore_index] * size
    if remap_select is not None:
        selected = set(int(k) for k in remap_select)
        for k in keys:
            new = int(remap_dict[k]) if k in selected else ignore_index
            remap[k] = inc[k] = new
    else:
        for k in keys:
            remap[k] = inc[k] = int(remap_dict[k])
    segment_incr_remap = _lookup(segment, torch.tensor(remap, dtype=segment.dtype), segment)
    segment_incr = _lookup(segment, torch.tensor(inc, dtype=segment.dtype), torch.full_like(segment, ignore_index))
    return segment_incr_remap, segment_incr


def instance_parser(coord, segment, instance, offset=None, segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1):
    """``InstanceParser`` (transform.py:1098-1141) on tensors of any device, for one scene (``offset=None``) or a collated batch (``offset``:
    cumulative ends; every scene is parsed on its own, as upstream parses before it collates).
    -> dict(instance (n) like the input: ids of the kept instances renumbered 0.. per scene in ascending id, ``instance_ignore_index``
    on rows of an ignored class; instance_centroid (n, 3) float64: the instance's mean coordinate -- a float32 mean stored into float64,
    as NumPy does -- or the ignore index; bbox (instances, 8) float64: centre, size, 0, class shifted down by the ignored class ids below it).
    The inputs are not modified (upstream overwrites ``instance`` in place).  Plumbing on torch ops with one host read (the instance count);
    min / max are exact on any device, the mean is NumPy's row-by-row float32 sum on CPU tensors (bit-equal) and a float64 prefix sum rounded
    to float32 on the device (order-independent up to that rounding, no float atomics)."""
    n, dev = coord.shape[0], coord.device
    rows = torch.arange(n, device=dev)
    scene = torch.zeros(n, dtype=torch.long, device=dev) if offset is None else torch.searchsorted(offset.to(dev).long(), rows, right=True)
    ignored = torch.as_tensor(list(segment_ignore_index), device=dev, dtype=segment.dtype)
    mask = ~torch.isin(segment, ignored)
    instance = torch.where(mask, instance, torch.full_like(instance, instance_ignore_index))
    centroid = torch.full((n, 3), float(instance_ignore_index), dtype=torch.float64, device=dev)
    kept = instance[mask].long()
    if kept.numel() == 0:
        return dict(instance=instance, instance_centroid=centroid, bbox=torch.zeros((0, 8), dtype=torch.float64, device=dev))
    lo = kept.min()
    span = kept.max() - lo + 1
    uniq, inverse = torch.unique(scene[mask] * span + (kept - lo), return_inverse=True)   # ascending (scene, id)
    num = uniq.shape[0]
    scene_of = uniq // span
    first = torch.searchsorted(scene_of, torch.arange(int(scene.max()) + 1, device=dev))
    instance = instance.clone()
    instance[mask] = (inverse - first[scene_of[inverse]]).to(instance.dtype)
    gid = torch.full((n,), -1, dtype=torch.long, device=dev)
    gid[mask] = inverse
    xyz = coord[mask]
    idx3 = inverse.unsqueeze(1).expand(-1, 3)
    bmin = torch.zeros((num, 3), dtype=coord.dtype, device=dev).scatter_reduce_(0, idx3, xyz, "amin", include_self=False)
    bmax = torch.zeros((num, 3), dtype=coord.dtype, device=dev).scatter_reduce_(0, idx3, xyz, "amax", include_self=False)
    count = torch.bincount(inverse, minlength=num)
    if dev.type == "cpu":
        import numpy as np

        total = np.zeros((num, 3), xyz.numpy().dtype)
        np.add.at(total, inverse.numpy(), xyz.numpy())          # row by row in the array's own precision: coord_.mean(0)
        mean = torch.from_numpy(total / count.numpy()[:, None].astype(total.dtype))
    else:
        order = torch.argsort(inverse, stable=True)
        run = torch.cat([torch.zeros((1, 3), dtype=torch.float64, device=dev), torch.cumsum(xyz[order].double(), 0)])
        ends = torch.cumsum(count, 0)
        mean = ((run[ends] - run[ends - count]) / count.unsqueeze(1)).to(coord.dtype)
    centroid[mask] = mean[inverse].double()
    head = torch.full((num,), n, dtype=torch.long, device=dev).scatter_reduce_(0, inverse, rows[mask], "amin", include_self=True)
    cls = segment[head].to(coord.dtype)
    vacancy = torch.as_tensor([float(v) for v in segment_ignore_index if v >= 0], dtype=coord.dtype, device=dev)
    cls = cls - (cls.unsqueeze(1) > vacancy.unsqueeze(0)).sum(1).to(coord.dtype)
    bbox = torch.cat([(bmax + bmin) / 2, bmax - bmin, torch.zeros((num, 1), dtype=coord.dtype, device=dev), cls.unsqueeze(1)], 1).double()
    return dict(instance=instance, instance_centroid=centroid, bbox=bbox)

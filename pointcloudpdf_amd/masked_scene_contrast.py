"""MSC-v1m1 -- pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py (``MaskedSceneContrast``): masked scene
contrast pre-training (Wu et al., CVPR 2023), the ``pretrain-msc-v1m1-*`` recipes over ``SpUNet-v1m1``.

Same constructor arguments and defaults, the same ``state_dict`` keys (``backbone.*``, ``mask_token``, ``color_head.*``,
``normal_head.*``; a head is absent when its flag is off), the same input dict (``view{1,2}_{origin_coord,coord,feat,offset}`` plus the
optional ``grid_coord`` / ``color`` / ``normal``) and the same returned dict (``loss, nce_loss, pos_sim, neg_sim`` and ``color_loss`` /
``normal_loss``).

What differs is how the three stages outside the backbone run:

* cross masks (``cross_masks``): the patch id of a point is ``stratified._voxel_grid``'s formula (``start=0``, cell size 1) over
  ``floor(origin_coord / mask_grid_size)`` of both views, its rank among the distinct ids selects the patch's tag.  No
  (patch_num, patch_max_point) map, no ``counts.max()``; one host read (the patch count, which sizes the reference's ``randperm``);
* pair matching (``match_pairs``): from the (N1, max_k) kNN table directly, without the (N, k, 2) index tensor;
* the contrastive loss is ``losses.matched_info_nce`` and every reconstruction head one node of csrc/scene_contrast.hip
  (``masked_reconstruction``): no (P, P) matrix, no boolean gather, no compacted copy.

Random draws are made in the reference's order through ``model.draws`` (``Draws``: torch / ``random`` exactly as upstream, so a CPU run
under the same seeds reproduces a reference run); ``RecordedDraws`` replays recorded ones where the device generator differs.
``make_geometry(data_dict)`` makes the two view-mixing draws and builds both views' SpUNet geometry ahead of the forward
(``data_dict["msc_geometry"]``, good for one forward); without it the forward does the same inline, with bit-identical outputs.
With more than one rank the three ``all_reduce`` calls and the division stay as upstream writes them."""
import random

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _native, dense, losses, stratified
from .dense import _amp_bwd, _amp_fwd
from .registry import MODELS, build_model

FORCE_TORCH = False   # the torch composition of the two loss stages on the device as well (the tests' and the tool's yardstick)


# ---- draws -----------------------------------------------------------------------------------------------------------------------------
class Draws:
    """The reference's calls, as it makes them."""

    def randperm(self, n):
        return torch.randperm(n)

    def random(self):
        return random.random()

    def randint(self, high, shape, device):
        return torch.randint(high, shape, device=device)


class RecordedDraws:
    """The draws of a recorded reference run: ``seq`` is a list of (name, value) with name in randperm / random / randint, replayed per
    name in the recorded order (tests/golden/make_golden_msc.py records them)."""

    def __init__(self, seq):
        self.queues = {}
        for name, value in seq:
            self.queues.setdefault(name, []).append(value)

    def _next(self, name):
        if not self.queues.get(name):
            raise RuntimeError(f"recorded draws exhausted at {name}")
        return self.queues[name].pop(0)

    def randperm(self, n):
        v = torch.as_tensor(self._next("randperm")).long()
        if v.numel() != n:
            raise RuntimeError(f"recorded randperm has {v.numel()} entries, the model asks for {n}")
        return v

    def random(self):
        return float(self._next("random"))

    def randint(self, high, shape, device):
        v = torch.as_tensor(self._next("randint")).long()
        if tuple(v.shape) != tuple(shape) or (v.numel() and int(v.max()) >= high):
            raise RuntimeError(f"recorded randint does not fit randint({high}, {tuple(shape)})")
        return v.to(device)


# ---- cross masks -------------------------------------------------------------------------------------------------------------------------
def _batch_of(offset, n):
    return torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)   # offset2batch without a host read


def cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, mask_grid_size, mask_rate, draws):
    """``generate_cross_masks`` (:69-141) -> (view1_point_mask, view2_point_mask), bool.  The patch id depends on the cell and the scene
    alone, so the union needs no per-scene interleaving: the ids of [view1, view2] are the ids of the reference's union, row for row."""
    assert mask_rate <= 0.5
    n1, n2 = view1_origin_coord.shape[0], view2_origin_coord.shape[0]
    cell = torch.floor(torch.cat([view1_origin_coord, view2_origin_coord]).div(mask_grid_size))
    batch = torch.cat([_batch_of(view1_offset, n1), _batch_of(view2_offset, n2)])
    ids = stratified._voxel_grid(cell, batch, cell.new_ones(3), start=cell.new_zeros(3))
    unique, rank = torch.unique(ids, sorted=True, return_inverse=True)
    patch_num = unique.shape[0]                                   # (the one host read: it sizes the permutation)
    tag = torch.zeros(patch_num, dtype=torch.int32, device=cell.device)
    perm = draws.randperm(patch_num).to(cell.device)
    m = int(patch_num * mask_rate)
    tag[perm[0:m]] = 1
    tag[perm[m:2 * m]] = 2
    point_tag = tag[rank]
    return point_tag[:n1] == 1, point_tag[n1:] == 2


# ---- pair matching -----------------------------------------------------------------------------------------------------------------------
def _knn_host(k, xyz, offset, new_xyz, new_offset):
    """pointops.knn_query for host tensors: brute force per scene -> idx (m, k) int32 (-1 where the scene is short), dist (m, k)."""
    m = new_xyz.shape[0]
    idx = torch.full((m, k), -1, dtype=torch.int32)
    dst = torch.full((m, k), 1e10, dtype=torch.float32)
    s0 = q0 = 0
    for s1, q1 in zip(offset.tolist(), new_offset.tolist()):
        if q1 > q0 and s1 > s0:
            d2 = ((new_xyz[q0:q1, None, :] - xyz[None, s0:s1, :]) ** 2).sum(-1)
            kk = min(k, s1 - s0)
            val, arg = torch.topk(d2, kk, dim=1, largest=False, sorted=True)
            idx[q0:q1, :kk] = (arg + s0).int()
            dst[q0:q1, :kk] = torch.sqrt(val)
        s0, q0 = s1, q1
    return idx, dst


def match_pairs(view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius, max_pair, draws):
    """``match_contrastive_pair`` (:143-172) -> match_index (P, 2) int64 = (row of view 1, row of view 2), queries ascending: every
    view-1 row with c >= 1 neighbours closer than ``max_radius`` keeps the one at position c - 1 - (draw % c) of its valid neighbours
    in ascending-k order; more than ``max_pair`` pairs are cut to a ``randperm`` subset, in the permutation's order."""
    from . import pointops

    knn = pointops.knn_query if view1_coord.is_cuda else _knn_host
    index, distance = knn(max_k, view2_coord.float().contiguous(), view2_offset.int(), view1_coord.float().contiguous(), view1_offset.int())
    valid = distance.reshape(-1, max_k) < max_radius
    index = index.reshape(-1, max_k)
    count_all = valid.sum(dim=1)
    query = torch.nonzero(count_all > 0).view(-1)                 # (host read: the number of queries with a match)
    count = count_all[query]
    draw = draws.randint(int(count.max()), count.shape, count.device)   # (host read: the reference's count.max())
    keep = count - 1 - draw % count
    order = torch.cumsum(valid[query], dim=1) - 1                  # position of a neighbour among the query's valid ones
    column = (valid[query] & (order == keep.unsqueeze(1))).to(torch.uint8).argmax(dim=1)
    match = torch.stack([query, index[query, column].long()], dim=1)
    if match.shape[0] > max_pair:
        match = match[draws.randperm(match.shape[0])[:max_pair].to(match.device)]
    return match.contiguous()


# ---- reconstruction heads ---------------------------------------------------------------------------------------------------------------
def masked_reconstruction_composition(kind, view1_feat, view2_feat, view1_mask, view2_mask, weight, bias, view1_target, view2_target):
    """The reference's lines (:279-284 color, :293-305 normal): boolean gathers, the 3-wide head on the compacted rows, the loss."""
    pred1 = nn.functional.linear(view1_feat[view1_mask], weight, bias)
    pred2 = nn.functional.linear(view2_feat[view2_mask], weight, bias)
    if kind == "color":
        total = torch.sum((pred1 - view1_target[view1_mask]) ** 2) + torch.sum((pred2 - view2_target[view2_mask]) ** 2)
    else:
        pred1 = pred1 / (torch.norm(pred1, p=2, dim=1, keepdim=True) + 1e-10)
        pred2 = pred2 / (torch.norm(pred2, p=2, dim=1, keepdim=True) + 1e-10)
        total = torch.sum(pred1 * view1_target[view1_mask]) + torch.sum(pred2 * view2_target[view2_mask])
    return total / (pred1.shape[0] + pred2.shape[0])


class _MaskedReconstruction(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, kind, feat1, feat2, mask1, mask2, weight, bias, target1, target2):
        be = _native.hip_backend()
        feat1, feat2, mask1, mask2, weight = feat1.contiguous(), feat2.contiguous(), mask1.contiguous(), mask2.contiguous(), weight.contiguous()
        loss, dpred, acc = be.msc_recon_forward(kind, feat1, feat2, mask1, mask2, weight, bias.contiguous(), target1.contiguous(),
                                                target2.contiguous())
        ctx.save_for_backward(feat1, feat2, mask1, mask2, weight, dpred, acc)
        return loss[0]

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        feat1, feat2, mask1, mask2, weight, dpred, acc = ctx.saved_tensors
        g1, g2, gw, gb = _native.hip_backend().msc_recon_backward(feat1, feat2, mask1, mask2, weight, dpred, acc,
                                                                  gy.contiguous().float().reshape(1))
        return None, g1, g2, None, None, gw, gb, None, None


def masked_reconstruction(kind, view1_feat, view2_feat, view1_mask, view2_mask, weight, bias, view1_target, view2_target):
    """One reconstruction head (``kind`` "color": squared error; "normal": the cosine form with + 1e-10) over the masked rows of both
    views -> the 0-dim loss.  fp32 device tensors with C a multiple of 32 up to 256 run as one node of csrc/scene_contrast.hip; anything
    else takes the composition."""
    if kind not in ("color", "normal"):
        raise ValueError(f"masked_reconstruction: kind {kind!r}")
    tensors = (view1_feat, view2_feat, weight, bias, view1_target, view2_target)
    fused = (not FORCE_TORCH and all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and view1_mask.dtype == torch.bool
             and view2_mask.dtype == torch.bool and _native.hip_backend().msc_recon_supported(weight.shape[1]))
    if not fused:
        return masked_reconstruction_composition(kind, view1_feat, view2_feat, view1_mask, view2_mask, weight, bias, view1_target, view2_target)
    _native.require_current_device(view1_feat, view2_feat, view1_mask, view2_mask, weight, bias, view1_target, view2_target)
    return _MaskedReconstruction.apply(int(kind == "normal"), view1_feat, view2_feat, view1_mask, view2_mask, weight, bias, view1_target,
                                       view2_target)


def _world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@MODELS.register_module("MSC-v1m1")
class MaskedSceneContrast(nn.Module):
    def __init__(self, backbone, backbone_in_channels, backbone_out_channels, mask_grid_size=0.1, mask_rate=0.4, view1_mix_prob=0,
                 view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4, contrast_weight=1,
                 reconstruct_weight=1, reconstruct_color=True, reconstruct_normal=True):
        super().__init__()
        self.backbone = build_model(backbone)
        self.mask_grid_size = mask_grid_size
        self.mask_rate = mask_rate
        self.view1_mix_prob = view1_mix_prob
        self.view2_mix_prob = view2_mix_prob
        self.matching_max_k = matching_max_k
        self.matching_max_radius = matching_max_radius
        self.matching_max_pair = matching_max_pair
        self.nce_t = nce_t
        self.contrast_weight = contrast_weight
        self.reconstruct_weight = reconstruct_weight
        self.reconstruct_color = reconstruct_color
        self.reconstruct_normal = reconstruct_normal

        self.mask_token = nn.Parameter(torch.zeros(1, backbone_in_channels))
        nn.init.trunc_normal_(self.mask_token, mean=0.0, std=0.02, a=-2.0, b=2.0)   # timm's trunc_normal_ defaults
        self.color_head = nn.Linear(backbone_out_channels, 3) if reconstruct_color else None
        self.normal_head = nn.Linear(backbone_out_channels, 3) if reconstruct_normal else None
        self.draws = Draws()

    @torch.no_grad()
    def generate_cross_masks(self, view1_origin_coord, view1_offset, view2_origin_coord, view2_offset):
        return cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, self.mask_grid_size, self.mask_rate, self.draws)

    @torch.no_grad()
    def match_contrastive_pair(self, view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius):
        return match_pairs(view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius, self.matching_max_pair, self.draws)

    def compute_contrastive_loss(self, view1_feat, view1_offset, view2_feat, view2_offset, match_index):
        assert view1_offset.shape == view2_offset.shape
        if FORCE_TORCH:
            loss, pos_sim, neg_sim = losses.matched_info_nce_reference(view1_feat, view2_feat, match_index, self.nce_t)
        else:
            loss, pos_sim, neg_sim = losses.matched_info_nce(view1_feat, view2_feat, match_index, self.nce_t)
        if _world_size() > 1:
            dist.all_reduce(loss)
            dist.all_reduce(pos_sim)
            dist.all_reduce(neg_sim)
        return loss / _world_size(), pos_sim / _world_size(), neg_sim / _world_size()

    @staticmethod
    def _mixed(offset):
        return torch.cat([offset[1:-1:2], offset[-1].unsqueeze(0)], dim=0)

    @torch.no_grad()
    def make_geometry(self, data_dict):
        """The two view-mixing draws and, for a backbone that has one, the geometry of both views under the offsets the backbone will see
        -> ``data_dict["msc_geometry"]``, good for ONE forward."""
        out = {}
        for view, prob in (("view1", self.view1_mix_prob), ("view2", self.view2_mix_prob)):
            offset = data_dict[f"{view}_offset"].int()
            if self.draws.random() < prob:
                offset = self._mixed(offset)
            geometry = None
            if hasattr(self.backbone, "make_geometry") and f"{view}_grid_coord" in data_dict:
                geometry = self.backbone.make_geometry(data_dict[f"{view}_grid_coord"], offset)
            out[view] = (offset, geometry)
        return out

    @dense.fp32_path
    def forward(self, data_dict):
        view1_origin_coord = data_dict["view1_origin_coord"]
        view1_coord = data_dict["view1_coord"]
        view1_feat = data_dict["view1_feat"]
        view1_offset = data_dict["view1_offset"].int()

        view2_origin_coord = data_dict["view2_origin_coord"]
        view2_coord = data_dict["view2_coord"]
        view2_feat = data_dict["view2_feat"]
        view2_offset = data_dict["view2_offset"].int()

        # the masks come from the un-augmented coordinates of both views
        view1_point_mask, view2_point_mask = self.generate_cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset)

        view1_weight = view1_point_mask.unsqueeze(-1).type_as(self.mask_token)
        view1_feat = view1_feat * (1 - view1_weight) + self.mask_token.expand(view1_coord.shape[0], -1) * view1_weight
        view2_weight = view2_point_mask.unsqueeze(-1).type_as(self.mask_token)
        view2_feat = view2_feat * (1 - view2_weight) + self.mask_token.expand(view2_coord.shape[0], -1) * view2_weight

        view1_data_dict = dict(origin_coord=view1_origin_coord, coord=view1_coord, feat=view1_feat, offset=view1_offset)
        view2_data_dict = dict(origin_coord=view2_origin_coord, coord=view2_coord, feat=view2_feat, offset=view2_offset)
        # a sparse-convolution backbone reads its sites from grid_coord
        if "view1_grid_coord" in data_dict.keys():
            view1_data_dict["grid_coord"] = data_dict["view1_grid_coord"]
        if "view2_grid_coord" in data_dict.keys():
            view2_data_dict["grid_coord"] = data_dict["view2_grid_coord"]

        # view mixing changes only the offsets the backbone sees
        geometry = data_dict.get("msc_geometry")
        if geometry is None:
            geometry = self.make_geometry(data_dict)
        for view_dict, (offset, tables) in ((view1_data_dict, geometry["view1"]), (view2_data_dict, geometry["view2"])):
            view_dict["offset"] = offset
            if tables is not None:
                view_dict["spunet_geometry"] = tables

        view1_feat = self.backbone(view1_data_dict).contiguous()
        view2_feat = self.backbone(view2_data_dict).contiguous()
        match_index = self.match_contrastive_pair(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset,
                                                  max_k=self.matching_max_k, max_radius=self.matching_max_radius)
        nce_loss, pos_sim, neg_sim = self.compute_contrastive_loss(view1_feat, view1_offset, view2_feat, view2_offset, match_index)
        loss = nce_loss * self.contrast_weight
        result_dict = dict(nce_loss=nce_loss, pos_sim=pos_sim, neg_sim=neg_sim)

        if self.color_head is not None:
            assert "view1_color" in data_dict.keys()
            assert "view2_color" in data_dict.keys()
            color_loss = masked_reconstruction("color", view1_feat, view2_feat, view1_point_mask, view2_point_mask, self.color_head.weight,
                                               self.color_head.bias, data_dict["view1_color"], data_dict["view2_color"])
            loss = loss + color_loss * self.reconstruct_weight
            result_dict["color_loss"] = color_loss

        if self.normal_head is not None:
            assert "view1_normal" in data_dict.keys()
            assert "view2_normal" in data_dict.keys()
            normal_loss = masked_reconstruction("normal", view1_feat, view2_feat, view1_point_mask, view2_point_mask, self.normal_head.weight,
                                                self.normal_head.bias, data_dict["view1_normal"], data_dict["view2_normal"])
            loss = loss + normal_loss * self.reconstruct_weight
            result_dict["normal_loss"] = normal_loss

        result_dict["loss"] = loss
        return result_dict

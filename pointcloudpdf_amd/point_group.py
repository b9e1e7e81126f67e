"""PG-v1m1 -- pointcept/models/point_group/point_group_v1m1_base.py (``PointGroup``): instance segmentation by clustering shifted points.

Same constructor arguments, submodule names and ``state_dict`` keys (``backbone``, ``bias_head.{0,1,3}``, ``seg_head``;
``BatchNorm1d(eps=1e-3, momentum=0.01)``) and the same returned dicts: train ``loss, seg_loss, bias_l1_loss, bias_cosine_loss``; eval
additionally ``pred_scores, pred_masks, pred_classes`` on the CPU with the reference's dtypes, its empty cases included.

On the device
* the two bias losses are ONE autograd node over csrc/point_group.hip (``bias_losses``): capturable, bit-reproducible, float32 or float64
  centroids with torch's promotion (the reference's ``instance_centroid`` arrives as float64);
* the eval branch stays on the device up to the three final copies: ball table, clustering and proposal stage are kernels (``proposals``);
  the reference copies the table to the host, clusters there, builds the (nProposal, N) mask on the CPU and scores in a Python loop;
* the compact proposals come back under additional keys -- ``proposal_offsets`` (P + 1), ``proposal_members`` (row indices, proposal by
  proposal), ``proposal_of`` (N: the row's proposal or -1; clusters are disjoint) -- which ``evaluator.InsSegEvaluator`` consumes
  without densifying.

16-bit ``bias_pred`` (autocast) and host tensors take the torch composition (``FORCE_TORCH = True`` forces it: the tests' reference)."""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native, dense, pointgroup_ops
from .registry import MODELS, build_model
from .segmentor import CrossEntropyLoss

FORCE_TORCH = False


# ---- bias losses -----------------------------------------------------------------------------------------------------------------------
def bias_losses_composition(bias_pred, coord, instance_centroid, instance, instance_ignore_index=-1):
    """The two bias terms of the reference (its lines 74-86) as a torch composition -> (bias_l1_loss, bias_cosine_loss): over the rows of a
    kept instance, the mean L1 distance between the predicted and the true offset to the instance's centroid, and the mean negative cosine
    of the two offsets; both means divide by (kept rows + 1e-8).  torch's promotion decides the dtypes, as it does upstream."""
    kept = (instance != instance_ignore_index).to(torch.float32)
    rows = kept.sum() + 1e-8
    offset_true = instance_centroid - coord

    def direction(v):
        return v / (v.norm(p=2, dim=1, keepdim=True) + 1e-8)

    l1 = (bias_pred - offset_true).abs().sum(dim=-1)
    cosine = (direction(bias_pred) * direction(offset_true)).sum(dim=-1)
    return (l1 * kept).sum() / rows, (-cosine * kept).sum() / rows


class _BiasLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bias_pred, coord, centroid, instance, ignore):
        be = _native.hip_backend()
        loss, d, acc = be.pg_bias_loss_forward(bias_pred.contiguous(), coord.contiguous(), centroid.contiguous(), instance.contiguous(), ignore)
        ctx.save_for_backward(d, acc)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_l1, g_cos):
        d, acc = ctx.saved_tensors
        return _native.hip_backend().pg_bias_loss_backward(d, acc, torch.stack([g_l1, g_cos])), None, None, None, None


def bias_losses(bias_pred, coord, instance_centroid, instance, instance_ignore_index=-1):
    """-> (bias_l1_loss, bias_cosine_loss), 0-dim, float64 with a float64 centroid (torch's promotion), float32 otherwise."""
    if (FORCE_TORCH or not bias_pred.is_cuda or bias_pred.dtype != torch.float32 or coord.dtype != torch.float32
            or instance_centroid.dtype not in (torch.float32, torch.float64)):
        return bias_losses_composition(bias_pred, coord, instance_centroid, instance, instance_ignore_index)
    _native.require_current_device(bias_pred, coord, instance_centroid, instance)
    return _BiasLosses.apply(bias_pred, coord, instance_centroid, instance.long(), int(instance_ignore_index))


# ---- proposals ---------------------------------------------------------------------------------------------------------------------------
def proposals_composition(cluster_idxs, cluster_offsets, segment_pred, prob, propose_points):
    """The proposal stage as a torch composition on the host (what the reference's lines 140-170 compute; ``cluster_idxs[:, 1]`` are rows of
    ``prob``) -> (pred_scores, pred_masks, pred_classes): clusters of more than ``propose_points`` rows, the class of the cluster's first
    listed member, the mean probability of that class over the members in ascending row order, an int32 (P, N) mask.  Without a proposal
    scores and classes are ``torch.tensor([])``, as upstream."""
    member = cluster_idxs.cpu().long().reshape(-1, 2)[:, 1]
    ends = cluster_offsets.cpu().long()
    segment_pred, prob = segment_pred.cpu(), prob.cpu()
    big = torch.nonzero(ends[1:] - ends[:-1] > propose_points).view(-1).tolist()
    masks = torch.zeros((len(big), prob.shape[0]), dtype=torch.int32)
    scores, classes = [], []
    for p, c in enumerate(big):
        rows = member[ends[c]:ends[c + 1]].sort().values
        cls = segment_pred[member[ends[c]]]
        masks[p, rows] = 1
        classes.append(cls)
        scores.append(prob[rows, cls].mean())
    if not big:
        return torch.tensor([]), masks, torch.tensor([])
    return torch.stack(scores), masks, torch.stack(classes)


def _kept_rows(segment_pred, ignore_index):
    keep = torch.ones_like(segment_pred, dtype=torch.bool)
    for index in ignore_index:
        keep &= segment_pred != index
    return keep


def _kept_scene_ends(keep, offset):
    """Scene boundaries [0, e_1, ..] among the kept rows: the kept rows in front of every boundary of ``offset``."""
    before = torch.cat([keep.new_zeros(1, dtype=torch.long), torch.cumsum(keep, 0)])
    return torch.cat([before[:1], before[offset.long().to(keep.device)]])


def host_clusters(center_pred, segment_pred, offset, ignore_index, radius, min_points):
    """Ball table and clusters of the kept rows through the host restatement of pointgroup_ops -> (cluster_idxs in the rows of the batch,
    cluster_offsets), CPU int32; the members of a cluster in the reference's BFS order."""
    keep = _kept_rows(segment_pred, ignore_index).cpu()
    rows = keep.nonzero().view(-1)
    if rows.numel() == 0:
        return torch.zeros((0, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    bounds = _kept_scene_ends(keep, offset.cpu())
    scene = torch.searchsorted(bounds[1:].contiguous(), torch.arange(rows.numel()), right=True)
    idx, start_len = pointgroup_ops.ballquery_batch_p(center_pred.cpu()[rows], scene.int(), bounds.int(), radius)
    clusters, ends = pointgroup_ops.bfs_cluster(segment_pred.cpu()[rows].int(), idx, start_len, min_points)
    clusters[:, 1] = rows[clusters[:, 1].long()].int()
    return clusters, ends


def proposals(center_pred, segment_pred, prob, offset, ignore_index, radius, min_points, propose_points, want_masks=True):
    """The eval branch of the reference (lines 101-170) on device tensors: rows whose predicted class is not ignored are clustered per scene
    (ball table of ``radius`` over ``center_pred``, equal-label min-label propagation, clusters of >= ``min_points``), the clusters with more
    than ``propose_points`` rows become proposals.  -> dict(offsets, members, proposal_of, classes, scores, masks), all on the device."""
    be = _native.backend_for(center_pred)
    n, dev = center_pred.shape[0], center_pred.device
    keep = _kept_rows(segment_pred, ignore_index)
    object_idxs = keep.nonzero().view(-1)                       # (the one data-dependent size ahead of the table: a host read)
    label = segment_pred[object_idxs].to(torch.int32).contiguous()
    if object_idxs.numel() == 0:
        cluster_idxs = torch.zeros((0, 2), dtype=torch.int32, device=dev)
        cluster_offsets = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        ends = _kept_scene_ends(keep, offset)[1:].to(torch.int32).contiguous()
        idx, start_len = be.pg_ball_table(center_pred[object_idxs].float().contiguous(), ends, float(radius))
        cluster_idxs, cluster_offsets = be.pg_cluster(label, idx, start_len, int(min_points))
    return be.pg_proposals(cluster_idxs, cluster_offsets, label, object_idxs, prob.contiguous(), int(propose_points), want_masks=want_masks)


@MODELS.register_module("PG-v1m1")
class PointGroup(nn.Module):
    def __init__(self, backbone, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=(-1, 0, 1),
                 instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50,
                 voxel_size=0.02):
        super().__init__()
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        self.semantic_num_classes = semantic_num_classes
        self.segment_ignore_index = segment_ignore_index
        self.semantic_ignore_index = semantic_ignore_index
        self.instance_ignore_index = instance_ignore_index
        self.cluster_thresh = cluster_thresh
        self.cluster_closed_points = cluster_closed_points   # (sized the reference's table allocation: unused by the CSR table)
        self.cluster_propose_points = cluster_propose_points
        self.cluster_min_points = cluster_min_points
        self.voxel_size = voxel_size
        self.backbone = build_model(backbone)
        self.bias_head = nn.Sequential(nn.Linear(backbone_out_channels, backbone_out_channels), norm_fn(backbone_out_channels), nn.ReLU(),
                                       nn.Linear(backbone_out_channels, 3))
        self.seg_head = nn.Linear(backbone_out_channels, semantic_num_classes)
        self.ce_criteria = CrossEntropyLoss(ignore_index=semantic_ignore_index)

    def _bias_head(self, feat):
        lin, bn, _, out = self.bias_head
        if not feat.is_cuda:
            return self.bias_head(feat)
        if dense.linbn_ok(lin, bn, feat):
            return dense.linear(out, dense.linear_bn_act(lin, bn, feat, True))
        return dense.linear(out, dense.bn_act(bn, dense.linear(lin, feat), relu=True))

    @dense.fp32_path
    def forward(self, data_dict):
        coord, offset = data_dict["coord"], data_dict["offset"]
        feat = self.backbone(data_dict).contiguous()
        bias_pred = self._bias_head(feat)
        logit_pred = dense.linear(self.seg_head, feat)

        seg_loss = self.ce_criteria(logit_pred, data_dict["segment"])
        bias_l1_loss, bias_cosine_loss = bias_losses(bias_pred, coord, data_dict["instance_centroid"], data_dict["instance"],
                                                     self.instance_ignore_index)
        out = dict(loss=seg_loss + bias_l1_loss + bias_cosine_loss, seg_loss=seg_loss, bias_l1_loss=bias_l1_loss,
                   bias_cosine_loss=bias_cosine_loss)
        if self.training:
            return out

        center_pred = (coord + bias_pred.detach()) / self.voxel_size      # shifted points, in voxels
        prob = F.softmax(logit_pred.detach().float(), dim=-1)
        segment_pred = prob.argmax(dim=1)
        if coord.is_cuda and not FORCE_TORCH:
            found = proposals(center_pred, segment_pred, prob, offset, self.segment_ignore_index, self.cluster_thresh, self.cluster_min_points,
                              self.cluster_propose_points, want_masks=data_dict.get("pointgroup_dense_masks", True))
            some = found["classes"].shape[0] > 0
            out.update(proposal_offsets=found["offsets"], proposal_members=found["members"], proposal_of=found["proposal_of"],
                       # the reference's three outputs, its empty case included: torch.tensor([]) twice next to a (0, N) int32 mask
                       pred_scores=found["scores"].cpu() if some else torch.tensor([]),
                       pred_classes=found["classes"].cpu() if some else torch.tensor([]),
                       pred_masks=found["masks"].cpu() if found["masks"] is not None else None)
            return out
        # host tensors (or the forced composition): the NumPy restatement of pointgroup_ops, then the torch composition
        clusters, ends = host_clusters(center_pred, segment_pred, offset, self.segment_ignore_index, self.cluster_thresh, self.cluster_min_points)
        out["pred_scores"], out["pred_masks"], out["pred_classes"] = proposals_composition(clusters, ends, segment_pred, prob,
                                                                                            self.cluster_propose_points)
        return out

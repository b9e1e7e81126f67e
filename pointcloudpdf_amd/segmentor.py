"""Segmentor wrapper and losses of the hot path -- pointcept/models/default.py:39-62,
pointcept/models/losses/builder.py:13-27, pointcept/models/losses/misc.py:14-39 (contract only: dict in, dict out)."""
import torch
import torch.nn as nn

from . import dense
from .dense import _amp_bwd, _amp_fwd   # (custom nodes keep fp32 tensors under autocast: dense.py)
from .registry import LOSSES, MODELS, build_model


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    """losses/misc.py:14-39 (ignore_index defaults to -1: unknown classes are relabelled -1 by the trainer).

    On the device, fp32 (N, C) logits against int64 labels never leave the HIP library: the plain configuration (no weight, no smoothing,
    mean, C <= 64) is ``_FusedCE`` (csrc/loss.hip), every other one -- class weights, label smoothing, sum / none, C > 64 --
    ``_FusedCEEx`` (csrc/criteria.hip).  Anything else (CPU, other dtypes, probability targets, > 2-D input) is ``nn.CrossEntropyLoss``.
    The class weights are a NON-persistent buffer of ``self.loss`` (never in a state_dict); ``Criteria`` is not a module, so nothing
    moves them with the model: they are uploaded once per device by the first EAGER forward there, never inside a capture."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0,
                 loss_weight=1.0, ignore_index=-1):
        super().__init__()
        self.loss_weight = loss_weight
        w = torch.tensor(weight) if weight is not None else None
        # (the legacy size_average / reduce arguments end up in .reduction as their string: torch's own mapping)
        self.loss = nn.CrossEntropyLoss(weight=w, size_average=size_average, ignore_index=ignore_index, reduce=reduce,
                                        reduction=reduction, label_smoothing=label_smoothing)
        if w is not None:
            del self.loss._buffers["weight"]
            self.loss.register_buffer("weight", w, persistent=False)
        self._weights = {}   # device -> fp32 weights there (losses._upload_once)

    def _weight_on(self, device):
        w = self.loss.weight
        if w is None or (w.device == device and w.dtype == torch.float32):
            return w
        return losses._upload_once(self._weights, (str(device),), lambda: w.detach().to(device=device, dtype=torch.float32).contiguous(),
                                   "CrossEntropyLoss(weight=...): the class weights")

    def forward(self, pred, target):
        l = self.loss
        if (pred.is_cuda and pred.dim() == 2 and pred.dtype == torch.float32 and pred.shape[1] <= 64 and target.dtype == torch.int64
                and l.weight is None and l.label_smoothing == 0.0 and l.reduction == "mean"):
            return _FusedCE.apply(pred.contiguous(), target.contiguous(), int(l.ignore_index)) * self.loss_weight
        if (pred.is_cuda and pred.dim() == 2 and pred.dtype == torch.float32 and target.dtype == torch.int64 and target.dim() == 1
                and pred.shape[0] > 0 and pred.shape[1] > 0 and l.reduction in ("mean", "sum", "none")):
            w = self._weight_on(pred.device)
            if w is not None and w.shape != (pred.shape[1],):
                raise ValueError(f"CrossEntropyLoss: {w.shape[0]} class weights for {pred.shape[1]} classes")
            return _FusedCEEx.apply(pred.contiguous(), target.contiguous(), w, float(l.label_smoothing), l.reduction,
                                    int(l.ignore_index)) * self.loss_weight
        if l.weight is not None and l.weight.device != pred.device:
            return nn.functional.cross_entropy(pred, target, weight=self._weight_on(pred.device), ignore_index=l.ignore_index,
                                               reduction=l.reduction, label_smoothing=l.label_smoothing) * self.loss_weight
        return l(pred, target) * self.loss_weight


class _FusedCEEx(torch.autograd.Function):
    """nn.CrossEntropyLoss in full (class weights, label smoothing, mean / sum / none, any class count) over (N, C) fp32 logits as one
    pass per direction (csrc/criteria.hip: pdf_ce_ex_forward / pdf_ce_ex_backward)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, weight, label_smoothing, reduction, ignore):
        from . import _native

        loss, dlogits, acc = _native.hip_backend().ce_ex_forward(pred, target, weight, label_smoothing, reduction, ignore)
        ctx.save_for_backward(dlogits, acc)
        ctx.reduction = reduction
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        dlogits, acc = ctx.saved_tensors   # only read: the node may be differentiated again (retain_graph)
        return _native.hip_backend().ce_ex_backward(dlogits, acc, gy.contiguous().float(), ctx.reduction), None, None, None, None, None


class _FusedCE(torch.autograd.Function):
    """nn.CrossEntropyLoss(mean, ignore_index) over (N, C <= 64) fp32 logits as one HIP kernel per direction (csrc/loss.hip)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, ignore):
        from . import _native

        be = _native.hip_backend()
        n, c = pred.shape
        grad = torch.empty_like(pred)
        # [sum, count, mean, -] + the per-workgroup partial sums (added in a fixed order: csrc/loss.hip)
        acc = torch.empty((int(be.lib.pdf_ce_workspace_floats()),), dtype=torch.float32, device=pred.device)
        _native.require_current_device(pred, target)
        be._launch("ce_forward", n, c, pred.data_ptr(), target.data_ptr(), ignore, grad.data_ptr(), acc.data_ptr(), acc.data_ptr() + 8)
        ctx.save_for_backward(grad, acc)
        return acc[2]

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        dlogits, acc = ctx.saved_tensors
        n, c = dlogits.shape
        gy = gy.contiguous().float()
        out = torch.empty_like(dlogits)   # the saved buffer stays untouched: the node may be differentiated again (retain_graph)
        _native.require_current_device(dlogits, gy)
        _native.hip_backend()._launch("ce_backward", n, c, dlogits.data_ptr(), acc.data_ptr(), gy.data_ptr(), out.data_ptr())
        return out, None, None


from . import losses  # noqa: E402,F401  (registers LovaszLoss, FocalLoss, DiceLoss, BinaryFocalLoss: LOSSES is complete once this module is imported)


class Criteria:
    """losses/builder.py:13-27: sum of the configured losses; an empty list returns the prediction itself."""

    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else []
        self.criteria = [LOSSES.build(cfg=c) for c in self.cfg]

    def __call__(self, pred, target):
        if len(self.criteria) == 0:
            return pred
        loss = 0
        for c in self.criteria:
            loss = loss + c(pred, target)
        return loss


def build_criteria(cfg):
    return Criteria(cfg)


@MODELS.register_module()
class DefaultSegmentor(nn.Module):
    """default.py:39-62: train -> {loss}; eval with labels -> {loss, seg_logits}; test -> {seg_logits}."""

    def __init__(self, backbone=None, criteria=None):
        super().__init__()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)

    @dense.fp32_path   # (the loss as well: fp32 tensors, reduced-precision product operands only -- dense.fp32_path)
    def forward(self, input_dict):
        if "condition" in input_dict.keys():
            input_dict["condition"] = input_dict["condition"][0]
        seg_logits = self.backbone(input_dict)
        if self.training:
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]))
        if "segment" in input_dict.keys():
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)


@MODELS.register_module()
class DefaultSegmentorV2(nn.Module):
    """default.py:65-97: a backbone that returns a ``Point`` (PT-v3m1) and a Linear head over its features."""

    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None):
        super().__init__()
        self.seg_head = nn.Linear(backbone_out_channels, num_classes) if num_classes > 0 else nn.Identity()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)

    @dense.fp32_path
    def forward(self, input_dict):
        from .point_transformer_v3 import Point, _apply

        point = Point(input_dict)
        point = self.backbone(point)
        seg_logits = _apply(self.seg_head, point.feat)
        if self.training:
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]))
        if "segment" in input_dict.keys():
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)

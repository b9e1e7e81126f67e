"""Second PDF stage, incremental learning -- pointcept/incrLearners/ours/pointpdf_incr_v1m1_base.py:13-87 (``PointPdfIncrV1``,
``IncrDistillKlLoss``) and the checkpoint adaptation of ``IncrSegCheckpointLoader`` (engines/hooks/misc.py:590-740).

A student network with a head widened by the newly discovered classes learns from the frozen base model (the teacher): on the rows
that carry a new-class label (``segment_incr != -1``) the target is that label, everywhere else the teacher's softmax padded with
zeros; the loss is ``kl_div(log_softmax(student), target, "batchmean")``.

* ``IncrDistillKlLoss`` runs as ONE HIP launch per direction on the device (csrc/incr_distill.hip): the reference's target assembly
  (a boolean-mask assignment = a nonzero with a host sync, a ``.cuda()`` copy, a concatenation, ~10 kernels) cannot be recorded
  into the captured training step.  Off the device it is a torch composition without the host copy (oracle / CPU runs).
* ``PointPdfIncrV1`` keeps the reference's surface (``need_teacher_model``, ``inject_teacher_model``, ``teacher_model_hooks``,
  ``state_dict`` = the student's keys only).  Without a hook tap it reads the teacher's logits from its backbone directly: the
  reference runs ``teacher_model(input_dict)`` and discards the cross-entropy it computes.  Teacher and student read the same
  ``input_dict`` -- the same ``pdf_geometry`` -- so every coordinate-only table (FPS, kNN, inverse tables) is built once per batch.
* ``trim_base_weight_head`` / ``reserve_matched`` / ``load_incremental_weight``: the loader hook's methods as plain functions over
  state dicts.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dense
from .dense import _amp_bwd, _amp_fwd   # (custom nodes keep fp32 tensors under autocast: dense.py)
from .registry import INCREMENTALLEARNER, build_model
from .segmentor import build_criteria

MAX_FUSED_CLASSES = 64   # csrc/incr_distill.hip: one lane per row, the row in registers


class _FusedIncrKl(torch.autograd.Function):
    """IncrDistillKlLoss over (N, Cs <= 64) fp32 student logits and (N, Ct <= Cs) teacher logits as one HIP kernel per direction."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, teacher, labels, ignore, inv_tp, inv_tt):
        from . import _native

        be = _native.hip_backend()
        n, cs = pred.shape
        ct = teacher.shape[1]
        grad = torch.empty_like(pred)
        # [sum, 1 / (T_p N), loss, -] + the per-workgroup partial sums (added in a fixed order: csrc/incr_distill.hip)
        acc = torch.empty((int(be.lib.pdf_incr_kl_workspace_floats()),), dtype=torch.float32, device=pred.device)
        _native.require_current_device(pred, teacher, labels)
        be._launch("incr_kl_forward", n, cs, ct, pred.data_ptr(), teacher.data_ptr(), labels.data_ptr(), ignore, inv_tp, inv_tt,
                   grad.data_ptr(), acc.data_ptr(), acc.data_ptr() + 8)
        ctx.save_for_backward(grad, acc)
        return acc[2]

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        dgrad, acc = ctx.saved_tensors
        n, cs = dgrad.shape
        gy = gy.contiguous().float()
        out = torch.empty_like(dgrad)   # the saved buffer stays untouched: the node may be differentiated again (retain_graph)
        _native.require_current_device(dgrad, gy)
        _native.hip_backend()._launch("incr_kl_backward", n, cs, dgrad.data_ptr(), acc.data_ptr(), gy.data_ptr(), out.data_ptr())
        return out, None, None, None, None, None


def incr_kl_reference(pred, target, segment_incr, pred_temp=1.0, target_temp=1.0, ignore_index=-1):
    """The loss as a torch composition (pointpdf_incr_v1m1_base.py:69-86) without the host copy and the boolean-mask assignment:
    the onehot rows are selected with ``torch.where``.  Used off the device and by the tests."""
    logp = F.log_softmax(pred / pred_temp, dim=1)
    n, cs = logp.shape
    soft = torch.softmax(target.to(logp.dtype) / target_temp, dim=1)
    t = F.pad(soft, (0, cs - soft.shape[1]))
    valid = segment_incr != ignore_index
    onehot = F.one_hot(torch.where(valid, segment_incr, torch.zeros_like(segment_incr)), cs).to(t.dtype)
    t = torch.where(valid.unsqueeze(1), onehot, t)
    return F.kl_div(logp, t, reduction="batchmean")


class IncrDistillKlLoss(nn.Module):
    """pointpdf_incr_v1m1_base.py:62-87.  ``ignore_index``: the label of the rows that take the teacher's distribution (the reference
    hard-codes -1)."""

    def __init__(self, pred_temp=1.0, target_temp=1.0, loss_weight=1.0, ignore_index=-1):
        super().__init__()
        self.pred_temp = pred_temp
        self.target_temp = target_temp
        self.loss_weight = loss_weight
        self.ignore_index = ignore_index

    def forward(self, pred, target, segment_incr):
        if (pred.is_cuda and pred.dim() == 2 and target.dim() == 2 and pred.dtype == torch.float32 and pred.shape[1] <= MAX_FUSED_CLASSES
                and target.shape[1] <= pred.shape[1] and segment_incr.dtype == torch.int64):
            loss = _FusedIncrKl.apply(pred.contiguous(), target.detach().float().contiguous(), segment_incr.contiguous(),
                                      int(self.ignore_index), 1.0 / float(self.pred_temp), 1.0 / float(self.target_temp))
        else:
            loss = incr_kl_reference(pred, target, segment_incr, self.pred_temp, self.target_temp, self.ignore_index)
        return loss * self.loss_weight


def _unwrap(model):
    return model.module if isinstance(model, (nn.parallel.DataParallel, nn.parallel.DistributedDataParallel)) else model


@INCREMENTALLEARNER.register_module("PointPdf-incr-v1m1")
class PointPdfIncrV1(nn.Module):
    """pointpdf_incr_v1m1_base.py:13-59: train -> {loss} (distillation from the injected teacher); eval with ``segment`` -> {loss,
    seg_logits} with the loss on ``segment_incr_remap``; test -> {seg_logits}."""

    def __init__(self, backbone=None, eval_criteria=None):
        super().__init__()
        self.need_teacher_model = True
        self.incr_backbone = build_model(backbone)
        self.criteria = IncrDistillKlLoss()
        self.eval_criteria = build_criteria(eval_criteria)
        self.teacher_model = None
        self.teacher_model_hooks = None

    @dense.fp32_path
    def forward(self, input_dict):
        seg_logits = self.incr_backbone(input_dict)
        if self.training:
            teacher_seg_logits = self.get_teacher_output(input_dict)
            return dict(loss=self.criteria(seg_logits, teacher_seg_logits, input_dict["segment_incr"]))
        if "segment" in input_dict:
            return dict(loss=self.eval_criteria(seg_logits, input_dict["segment_incr_remap"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)

    def get_teacher_output(self, input_dict):
        """The teacher's logits under no_grad.  With a hook tap (``teacher_model_hooks``, registered and active as in the reference's
        trainer) the teacher's full forward runs and the tap's ``backbone`` output is read; without one, the teacher's backbone runs alone."""
        assert self.teacher_model is not None, "Teacher model is not set."
        teacher = _unwrap(self.teacher_model)
        with torch.no_grad():
            if self.teacher_model_hooks is not None:
                self.teacher_model(input_dict)
                return self.teacher_model_hooks["backbone"]["forward_output"]
            if hasattr(teacher, "backbone"):
                return teacher.backbone(input_dict)
            return self.teacher_model({k: v for k, v in input_dict.items() if k != "segment"})["seg_logits"]

    def inject_teacher_model(self, model):
        if not isinstance(model, nn.Module):
            raise TypeError("model must be a pytorch model")
        self.teacher_model = model

    def state_dict(self, destination=None, prefix="", keep_vars=False):
        """Only the student's weights, under ``incr_backbone.`` (what IncrSegCheckpointSaver writes)."""
        return self.incr_backbone.state_dict(destination=destination, prefix=prefix + "incr_backbone.", keep_vars=keep_vars)


# ---- checkpoint adaptation (engines/hooks/misc.py:576-588, 666-724) ----

def replace_key(state_dict, keyword, replacement):
    """``CheckpointLoader.replace_key`` at world size 1: a leading ``module.`` dropped, ``keyword`` replaced in every key."""
    out = {}
    for key, value in state_dict.items():
        if key.startswith("module."):
            key = key[len("module."):]
        if keyword and keyword in key:
            key = key.replace(keyword, replacement)
        out[key] = value
    return out


def _model_state(target):
    return target.state_dict() if isinstance(target, nn.Module) else target


def trim_base_weight_head(weight, target):
    """Base-model weights -> the incremental learner's: ``backbone`` renamed ``incr_backbone``; equal shapes kept; a tensor that is smaller
    in its leading dimension only (the classifier head, 13 -> 15 rows) is copied into the leading rows of the learner's own tensor (the
    new rows keep the learner's values); every other key skipped.  ``target``: the learner or its ``state_dict()``."""
    model_state = _model_state(target)
    out = {}
    for k, v in replace_key(weight, "backbone", "incr_backbone").items():
        if k not in model_state:
            continue
        cur = model_state[k]
        if v.shape == cur.shape:
            out[k] = v
        elif v.dim() == cur.dim() and v.shape[1:] == cur.shape[1:] and v.shape[0] <= cur.shape[0]:
            new = cur.detach().clone()
            new[: v.shape[0]] = v.to(device=new.device, dtype=new.dtype)
            out[k] = new
    return out


def reserve_matched(weight, target):
    """Base-model weights -> the learner's keys (``backbone`` renamed ``incr_backbone``) whose shapes match; everything else dropped.
    The reference's method (misc.py:708-724, marked "TODO debug") builds this filtered dict and then returns the UNFILTERED one, which
    ``load_state_dict`` refuses with a size mismatch as soon as the head grew; this returns the filtered dict, as evidently intended."""
    model_state = _model_state(target)
    return {k: v for k, v in replace_key(weight, "backbone", "incr_backbone").items() if k in model_state and v.shape == model_state[k].shape}


def load_incremental_weight(learner, incr_weight, base_weight=None, strict=False):
    """misc.py:666-682: ``incr_weight`` (learner keys) plus the base model's weights under ``teacher_model.backbone.*`` into ONE
    ``load_state_dict`` of the learner (its teacher must be injected).  Returns torch's (missing, unexpected) report."""
    merged = dict(incr_weight)
    if getattr(_unwrap(learner), "need_teacher_model", False) and base_weight:
        merged.update(replace_key(base_weight, "backbone", "teacher_model.backbone"))
    return learner.load_state_dict(merged, strict=strict)

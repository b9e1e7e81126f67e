"""Criteria beyond the plain cross-entropy: the Lovasz loss (below) and FocalLoss / DiceLoss / BinaryFocalLoss (second half of this file).

Lovasz loss -- pointcept/models/losses/lovasz.py (``LovaszLoss``; Berman et al., "The Lovasz-Softmax loss", CVPR 2018), the second
criterion of the reference's segmentation recipes: ``dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)``.

``mode="multiclass"`` over (N, C) logits and (N,) int64 labels, the form every point-cloud config uses:

    P = softmax(logits, 1); rows with label == ignore_index are dropped;
    for every class c among the kept labels (ascending; with ``class_seen`` only the classes of that list):
        fg = (label == c), e = |fg - P[:, c]|, sorted descending with fg alongside;
        G = sum fg, F_i = inclusive prefix count of fg, J_i = 1 - (G - F_i) / (G + (i + 1) - F_i);
        loss_c = sum_i e_i (J_i - J_{i-1})                                   (J_{-1} = 0)
    loss = loss_weight * (sum_c loss_c, ascending class order) / (number of such classes)

On the device (fp32 logits, C <= 64) it runs as one pass of the HIP library (csrc/lovasz.hip): a batched stable radix sort of C segments
of N keys and fixed-order sums, nothing read back to the host, no torch sort or reduction -- so the loss can sit inside the captured
training step, where the reference's ``labels.unique()`` / ``fg.sum() == 0`` (host reads) and per-class ``torch.sort`` cannot.

Choices of this package where the reference leaves the result open:

* ties: equal errors keep ascending row order (a stable descending sort).  The loss does not depend on the order of ties; the
  subgradient does, and ``torch.sort(descending=True)`` leaves it undefined;
* all rows ignored: the loss is a scalar 0 with a zero gradient (the reference returns an empty (0, C) tensor);
* a label that is neither ``ignore_index`` nor in [0, C) makes the loss NaN, as the fused cross-entropy does;
* J_i - J_{i-1} is formed from the integer counts in double and rounded once (the reference differences fp32 quotients, which loses
  ~1e-3 of the largest gradient to cancellation at 10^5 rows); loss_c is accumulated in double.

``mode="binary"`` / ``"multilabel"`` (the hinge form, over the whole batch) are a plain torch composition and NOT capturable: they read
sizes back to the host.  ``per_image=True`` raises: the reference zips over the rows of its (N, C) input there, which has no meaning for
point clouds.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .dense import _amp_bwd, _amp_fwd   # (custom nodes keep fp32 tensors under autocast: dense.py)
from .registry import LOSSES

MAX_FUSED_CLASSES = 64   # csrc/lovasz.hip: one lane per row, the row in registers
_NO_IGNORE = -(2 ** 63)  # ignore_index=None: a value no class id takes


def _jaccard_steps(fg_sorted, dtype):
    """J_i - J_{i-1} along a sorted 0/1 foreground column, from the counts in double, rounded once to ``dtype``."""
    fg = fg_sorted.to(torch.float64)
    total = fg.sum()
    seen = fg.cumsum(0)
    pos = torch.arange(1, fg.shape[0] + 1, dtype=torch.float64, device=fg.device)
    jac = 1.0 - (total - seen) / (total + pos - seen)
    return torch.diff(jac, prepend=jac.new_zeros(1)).to(dtype)


def lovasz_softmax_reference(logits, labels, ignore_index=None, class_seen=None, stable=True, probas=None, dtype=None):
    """The multiclass loss of the module docstring as a torch composition (loss_weight 1): the path off the device, and the independent
    side of the tests.  Works in any float dtype (``dtype``: compute in that one).  With ``probas=`` the softmax is skipped; the sort
    ORDER is then taken from the errors evaluated in the given tensor's own dtype (what a kernel working on those values sees), the sums
    run in ``dtype``.  ``stable=False`` sorts like the reference (ties in an undefined order).  Reads sizes back: not capturable."""
    if probas is None:
        p_key = torch.softmax(logits if dtype is None else logits.to(dtype), dim=1)
        zero = logits.sum() * 0.0
    else:
        p_key = probas
        zero = probas.sum() * 0.0
    p = p_key if dtype is None else p_key.to(dtype)
    zero = zero.to(p.dtype)
    ncls = p.shape[1]
    keep = torch.ones_like(labels, dtype=torch.bool) if ignore_index is None else labels != ignore_index
    p, p_key, lab = p[keep], p_key[keep], labels[keep]
    if lab.numel() == 0:
        return zero
    if bool(((lab < 0) | (lab >= ncls)).any()):
        return zero + float("nan")
    total, count = zero.to(torch.float64), 0
    for c in lab.unique().tolist():
        if class_seen is not None and c not in class_seen:
            continue
        fg = lab == c
        order = torch.sort((fg.to(p_key.dtype) - p_key[:, c]).abs().detach(), dim=0, descending=True, stable=stable)[1]
        err = (fg.to(p.dtype) - p[:, c]).abs()[order]
        total = total + torch.dot(err.to(torch.float64), _jaccard_steps(fg[order], p.dtype).to(torch.float64))
        count += 1
    if count == 0:
        return zero
    return (total / count).to(p.dtype)


def lovasz_hinge_reference(logits, labels, ignore_index=None):
    """The binary / multilabel form over the whole batch (lovasz.py:36-86 with per_image=False): hinge errors 1 - logit * sign, sorted
    descending, relu(errors) . (J_i - J_{i-1}).  Only ignored elements: a zero that still reaches the logits."""
    x, y = logits.reshape(-1), labels.reshape(-1)
    if ignore_index is not None:
        keep = y != ignore_index
        x, y = x[keep], y[keep]
    if y.numel() == 0:
        return logits.sum() * 0.0
    err = 1.0 - x * (2.0 * y.to(x.dtype) - 1.0)
    err, order = torch.sort(err, dim=0, descending=True, stable=True)
    return torch.dot(torch.relu(err), _jaccard_steps(y[order], x.dtype))


class _FusedLovasz(torch.autograd.Function):
    """Multiclass Lovasz-softmax over (N, C <= 64) fp32 logits as one pass of csrc/lovasz.hip.  The forward leaves the finished logits
    gradient behind; the backward is one scaled copy that only reads it."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, ignore, class_mask):
        from . import _native

        be = _native.hip_backend()
        n, c = pred.shape
        prob = torch.empty_like(pred)
        dlogits = torch.empty_like(pred)
        out = torch.empty((2,), dtype=torch.float32, device=pred.device)   # [loss, number of classes averaged]
        # every byte is written before it is read (csrc/lovasz.hip): nothing to zero, no memset node in a captured step
        ws = torch.empty((int(be.lib.pdf_lovasz_workspace_bytes(n, c)),), dtype=torch.uint8, device=pred.device)
        _native.require_current_device(pred, target)
        be._launch("lovasz_forward", n, c, pred.data_ptr(), target.data_ptr(), ignore,
                   class_mask.data_ptr() if class_mask is not None else None, prob.data_ptr(), dlogits.data_ptr(),
                   out.data_ptr(), ws.data_ptr())
        ctx.save_for_backward(dlogits)
        return out[0]

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        (dlogits,) = ctx.saved_tensors
        n, c = dlogits.shape
        gy = gy.contiguous().float()
        out = torch.empty_like(dlogits)   # the saved buffer stays untouched: the node may be differentiated again (retain_graph)
        _native.require_current_device(dlogits, gy)
        _native.hip_backend()._launch("lovasz_backward", n, c, dlogits.data_ptr(), gy.data_ptr(), 1.0, out.data_ptr())
        return out, None, None, None


@LOSSES.register_module()
class LovaszLoss(nn.Module):
    """lovasz.py:210-257 (the reference's constructor).  See the module docstring for the definition and this package's choices."""

    def __init__(self, mode, class_seen=None, per_image=False, ignore_index=None, loss_weight=1.0):
        super().__init__()
        if mode not in ("binary", "multiclass", "multilabel"):
            raise ValueError(f"LovaszLoss: unknown mode {mode!r}")
        if per_image:
            raise NotImplementedError("LovaszLoss(per_image=True): the reference zips over the rows of its (N, C) input there, which has "
                                      "no meaning for point clouds; use per_image=False (the whole batch)")
        self.mode = mode
        self.class_seen = None if class_seen is None else [int(c) for c in class_seen]
        self.per_image = per_image
        self.ignore_index = ignore_index
        self.loss_weight = loss_weight
        self._masks = {}   # (device, C) -> uint8 (C): class_seen as the kernel reads it (see _class_mask)

    def _class_mask(self, device, c):
        """``class_seen`` as C bytes on ``device``, uploaded once per (device, C).  The upload is a host-to-device copy, which must not
        be recorded into a stream capture: the first call for a pair has to be an eager one (``engine.CapturedStep`` / ``TrainStep``
        run eager warm-up passes before they capture; a hand-made capture needs one eager forward first).  Inside a capture a missing
        mask is an error, never a silent copy."""
        if self.class_seen is None:
            return None
        key = (str(device), c)
        if key not in self._masks:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"LovaszLoss(class_seen=...): the class mask for {c} classes on {device} has not been uploaded yet and "
                                   "the stream is capturing; run one eager forward on this device before the capture")
            m = torch.zeros(c, dtype=torch.uint8)
            m[[k for k in self.class_seen if 0 <= k < c]] = 1
            self._masks[key] = m.to(device)
        return self._masks[key]

    def forward(self, y_pred, y_true):
        if self.mode != "multiclass":
            return lovasz_hinge_reference(y_pred, y_true, self.ignore_index) * self.loss_weight
        if (y_pred.is_cuda and y_pred.dim() == 2 and y_pred.dtype == torch.float32 and y_pred.shape[1] <= MAX_FUSED_CLASSES
                and y_true.dtype == torch.int64 and y_true.dim() == 1):
            ignore = _NO_IGNORE if self.ignore_index is None else int(self.ignore_index)
            loss = _FusedLovasz.apply(y_pred.contiguous(), y_true.contiguous(), ignore, self._class_mask(y_pred.device, y_pred.shape[1]))
        else:
            loss = lovasz_softmax_reference(y_pred, y_true, self.ignore_index, self.class_seen)
        return loss * self.loss_weight


# ---------------------------------------------------------------------------------------------------------------------------------------
# FocalLoss, DiceLoss, BinaryFocalLoss -- pointcept/models/losses/misc.py:60-223, with the reference's constructors (and its assertions
# on argument types).  On the device (fp32 logits, int64 labels) each runs as one capturable pass of csrc/criteria.hip; everywhere else as
# the ``*_reference`` composition below, which is also the independent side of the tests.  The reference selects rows with a boolean mask
# (``pred[valid_mask]``) and branches on ``len(target) == 0``: both read the device back, so its forwards cannot sit in a captured step.
# The compositions use ``where`` and counts instead, and add their sums in float64 when the input is float32 (the kernels do the same);
# everything elementwise stays in the input's dtype.
#
# Choices of this package where the reference is silent or broken:
#
# * FocalLoss with every row ignored: a scalar 0 tensor with a zero gradient (the reference returns the python float 0.0, a host branch);
# * FocalLoss(reduction="sum"): the reference calls ``Tensor.total`` there and raises AttributeError on every call; built to the evident
#   formula (the sum of the terms the mean averages);
# * FocalLoss with a label that is neither ``ignore_index`` nor a class id: NaN, as the fused cross-entropy (the reference's one_hot raises);
# * DiceLoss keeps the reference's two quirks: labels are CLAMPED into [0, C - 1], not refused, and class ``i == ignore_index`` is left out
#   of the sum while the divisor stays C (with the default -1 nothing is left out); rows whose label equals ignore_index are dropped;
# * SmoothCELoss is not provided: the reference's forward raises AttributeError on every call (``Tensor.total``), no config can use it;
#   ``CrossEntropyLoss(label_smoothing=...)`` covers the intent.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _acc_dtype(t):
    return torch.float64 if t.dtype == torch.float32 else t.dtype


def _rows_2d(pred, target):
    """misc.py:133-143: (B, C, d1, ...) -> (N, C), the target flattened."""
    if pred.dim() != 2:
        pred = pred.transpose(0, 1)
        pred = pred.reshape(pred.size(0), -1).transpose(0, 1)
    target = target.reshape(-1)
    assert pred.size(0) == target.size(0), "The shape of pred doesn't match the shape of target"
    return pred.contiguous(), target.contiguous()


def focal_loss_reference(pred, target, gamma=2.0, alpha=0.5, reduction="mean", ignore_index=-1):
    """FocalLoss (loss_weight 1) over (N, C) logits without mask indexing or host branches.  ``alpha``: float, list or (C) tensor."""
    c = pred.shape[1]
    valid = target != ignore_index
    bad = valid & ((target < 0) | (target >= c))
    t = F.one_hot(target.clamp(0, c - 1), num_classes=c).to(pred.dtype)
    if isinstance(alpha, (list, tuple)):
        alpha = pred.new_tensor(alpha)
    elif isinstance(alpha, torch.Tensor):
        alpha = alpha.to(pred.dtype)
    sig = pred.sigmoid()
    one_minus_pt = (1 - sig) * t + sig * (1 - t)
    focal_weight = (alpha * t + (1 - alpha) * (1 - t)) * one_minus_pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, t, reduction="none") * focal_weight
    loss = torch.where(valid[:, None], loss, torch.zeros_like(loss))
    total = loss.to(_acc_dtype(pred)).sum()
    if reduction == "mean":
        count = valid.sum() * c
        total = torch.where(count > 0, total / count.clamp(min=1), torch.zeros_like(total))
    elif reduction != "sum":
        raise ValueError(f"FocalLoss: reduction {reduction!r}")
    total = torch.where(bad.any(), torch.full_like(total, float("nan")), total)
    return total.to(pred.dtype)


def dice_loss_reference(pred, target, smooth=1, exponent=2, ignore_index=-1):
    """DiceLoss (loss_weight 1) over (N, C) logits: labels clamped, class ``ignore_index`` skipped with the divisor left at C."""
    c = pred.shape[1]
    valid = (target != ignore_index)[:, None]
    p = F.softmax(pred, dim=1)
    y = F.one_hot(target.clamp(0, c - 1), num_classes=c).to(p.dtype)
    zero = torch.zeros_like(p)
    acc = _acc_dtype(p)
    inter = torch.where(valid, p * y, zero).to(acc).sum(0)
    mass = torch.where(valid, p.pow(exponent) + y, zero).to(acc).sum(0)   # y is 0 / 1: y ** exponent == y
    term = 1 - (2 * inter + smooth) / (mass + smooth)
    keep = torch.arange(c, device=pred.device) != ignore_index
    return (torch.where(keep, term, torch.zeros_like(term)).sum() / c).to(p.dtype)


def binary_focal_loss_reference(pred, target, gamma=2.0, alpha=0.5, logits=True, reduce=True):
    """BinaryFocalLoss (loss_weight 1), elementwise over float targets; ``reduce`` -> the mean."""
    target = target.to(pred.dtype)
    if logits:
        bce = F.binary_cross_entropy_with_logits(pred, target, reduction="none")
    else:
        bce = F.binary_cross_entropy(pred, target, reduction="none")
    pt = torch.exp(-bce)
    focal = (alpha * target + (1 - alpha) * (1 - target)) * (1 - pt) ** gamma * bce
    if reduce:
        focal = (focal.to(_acc_dtype(pred)).sum() / focal.numel()).to(pred.dtype)
    return focal


def _upload_once(cache, key, make, what):
    """A small host constant as a device tensor, uploaded once per key.  The upload is a host-to-device copy, which must not be recorded
    into a stream capture: the first call has to be an eager one (``LovaszLoss._class_mask``)."""
    if key not in cache:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} has not been uploaded to {key[0]} yet and the stream is capturing; run one eager forward on this "
                               "device before the capture")
        cache[key] = make()
    return cache[key]


class _FusedFocal(torch.autograd.Function):
    """FocalLoss over (N, C) fp32 logits as one pass of csrc/criteria.hip; the backward is a scaled copy that only reads the saved buffer."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, alpha, gamma, reduction, ignore):
        from . import _native

        loss, dlogits, acc = _native.hip_backend().focal_forward(pred, target, alpha, gamma, reduction, ignore)
        ctx.save_for_backward(dlogits, acc)
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        dlogits, acc = ctx.saved_tensors
        return _native.hip_backend().focal_backward(dlogits, acc, gy.contiguous().float()), None, None, None, None, None


class _FusedDice(torch.autograd.Function):
    """DiceLoss over (N, C) fp32 logits: softmax + column sums + class terms forward, a second row pass backward (csrc/criteria.hip)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, smooth, exponent, ignore):
        from . import _native

        loss, prob, acc = _native.hip_backend().dice_forward(pred, target, smooth, exponent, ignore)
        ctx.save_for_backward(prob, target, acc)
        ctx.cfg = (exponent, ignore)
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        prob, target, acc = ctx.saved_tensors
        exponent, ignore = ctx.cfg
        return _native.hip_backend().dice_backward(prob, target, ignore, exponent, acc, gy.contiguous().float()), None, None, None, None


class _FusedBinaryFocal(torch.autograd.Function):
    """BinaryFocalLoss over flat fp32 predictions and float targets as one elementwise pass (csrc/criteria.hip); gradient with respect to
    the prediction only."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, target, alpha, gamma, logits, reduce):
        from . import _native

        loss, dpred, acc = _native.hip_backend().bfocal_forward(pred, target, alpha, gamma, logits, reduce)
        ctx.save_for_backward(dpred, acc)
        ctx.reduce = reduce
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        from . import _native

        dpred, acc = ctx.saved_tensors
        return _native.hip_backend().bfocal_backward(dpred, acc, gy.contiguous().float(), ctx.reduce), None, None, None, None, None


def _fused_rows(pred, target):
    return pred.is_cuda and pred.dim() == 2 and pred.dtype == torch.float32 and target.dtype == torch.int64 and pred.shape[0] > 0


@LOSSES.register_module()
class BinaryFocalLoss(nn.Module):
    """misc.py:60-93.  pred (N) -- or any shape, flattened -- against float targets of the same shape (probabilities allowed)."""

    def __init__(self, gamma=2.0, alpha=0.5, logits=True, reduce=True, loss_weight=1.0):
        super().__init__()
        assert 0 < alpha < 1
        self.gamma = gamma
        self.alpha = alpha
        self.logits = logits
        self.reduce = reduce
        self.loss_weight = loss_weight

    def forward(self, pred, target, **kwargs):
        if pred.is_cuda and pred.dtype == torch.float32 and pred.numel() > 0 and target.shape == pred.shape:
            loss = _FusedBinaryFocal.apply(pred.contiguous().view(-1), target.to(torch.float32).contiguous().view(-1), float(self.alpha),
                                           float(self.gamma), bool(self.logits), bool(self.reduce))
            if not self.reduce:
                loss = loss.view(pred.shape)
        else:
            loss = binary_focal_loss_reference(pred, target, self.gamma, self.alpha, self.logits, self.reduce)
        return loss * self.loss_weight


@LOSSES.register_module()
class FocalLoss(nn.Module):
    """misc.py:97-172.  See the notes above for the all-ignored case, reduction="sum" and bad labels."""

    def __init__(self, gamma=2.0, alpha=0.5, reduction="mean", loss_weight=1.0, ignore_index=-1):
        super().__init__()
        assert reduction in ("mean", "sum"), "AssertionError: reduction should be 'mean' or 'sum'"
        assert isinstance(alpha, (float, list)), "AssertionError: alpha should be of type float"
        assert isinstance(gamma, float), "AssertionError: gamma should be of type float"
        assert isinstance(loss_weight, float), "AssertionError: loss_weight should be of type float"
        assert isinstance(ignore_index, int), "ignore_index must be of type int"
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.ignore_index = ignore_index
        self._alpha = {}   # (device, C) -> the alpha list as (C) fp32 on the device (_upload_once)

    def forward(self, pred, target, **kwargs):
        pred, target = _rows_2d(pred, target)
        if _fused_rows(pred, target):
            alpha = self.alpha
            if isinstance(alpha, list):
                c = pred.shape[1]
                if len(alpha) != c:
                    raise ValueError(f"FocalLoss: alpha lists {len(alpha)} classes, the prediction has {c}")
                alpha = _upload_once(self._alpha, (str(pred.device), c), lambda: torch.tensor(self.alpha, dtype=torch.float32).to(pred.device),
                                     "FocalLoss(alpha=[...]): the class vector")
            loss = _FusedFocal.apply(pred, target, alpha, self.gamma, self.reduction, self.ignore_index)
        else:
            loss = focal_loss_reference(pred, target, self.gamma, self.alpha, self.reduction, self.ignore_index)
        return self.loss_weight * loss


@LOSSES.register_module()
class DiceLoss(nn.Module):
    """misc.py:176-223 (V-Net's Dice loss over the softmax), with the reference's clamp and ignored-class quirks (notes above)."""

    def __init__(self, smooth=1, exponent=2, loss_weight=1.0, ignore_index=-1):
        super().__init__()
        self.smooth = smooth
        self.exponent = exponent
        self.loss_weight = loss_weight
        self.ignore_index = ignore_index

    def forward(self, pred, target, **kwargs):
        pred, target = _rows_2d(pred, target)
        if _fused_rows(pred, target) and self.exponent > 0:
            loss = _FusedDice.apply(pred, target.long(), float(self.smooth), float(self.exponent), int(self.ignore_index))
        else:
            loss = dice_loss_reference(pred, target.long(), self.smooth, self.exponent, self.ignore_index)
        return self.loss_weight * loss


# ---- matched-pair InfoNCE (MSC-v1m1) -------------------------------------------------------------------------------------------------
def matched_info_nce_reference(feat1, feat2, match_index, temperature):
    """The reference's ``compute_contrastive_loss`` (masked_scene_contrast_v1m1_base.py:179-193) as it is written: gather, normalise,
    the (P, P) similarity matrix, cross-entropy against the diagonal -> (loss, pos_sim, neg_sim)."""
    a = feat1[match_index[:, 0]]
    b = feat2[match_index[:, 1]]
    a = a / (torch.norm(a, p=2, dim=1, keepdim=True) + 1e-7)
    b = b / (torch.norm(b, p=2, dim=1, keepdim=True) + 1e-7)
    sim = torch.mm(a, b.transpose(1, 0))
    with torch.no_grad():
        pos_sim = torch.diagonal(sim).mean()
        neg_sim = sim.mean(dim=-1).mean() - pos_sim / match_index.shape[0]
    labels = torch.arange(sim.shape[0], device=a.device).long()
    loss = F.cross_entropy(torch.div(sim, temperature), labels, reduction="mean")
    return loss, pos_sim, neg_sim


class _FusedInfoNCE(torch.autograd.Function):
    """csrc/scene_contrast.hip: the similarity tiles are formed on the matrix cores and folded into running row statistics; the backward
    recomputes them.  No (P, P) array in either direction, no atomics: two evaluations are bit-identical."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, feat1, feat2, match_index, temperature):
        from . import _native

        feat1, feat2, match_index = feat1.contiguous(), feat2.contiguous(), match_index.contiguous()
        out, saved = _native.hip_backend().msc_nce_forward(feat1, feat2, match_index, temperature)
        ctx.save_for_backward(feat1, feat2, match_index, saved)
        ctx.temperature = float(temperature)
        loss, pos_sim, neg_sim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(pos_sim, neg_sim)
        return loss, pos_sim, neg_sim

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy, _gpos, _gneg):
        from . import _native

        feat1, feat2, match_index, saved = ctx.saved_tensors
        g1, g2 = _native.hip_backend().msc_nce_backward(feat1, feat2, match_index, ctx.temperature, saved, gy.contiguous().float().reshape(1))
        return g1, g2, None, None


def matched_info_nce(feat1, feat2, match_index, temperature):
    """InfoNCE over the matched rows of two views -> (loss, pos_sim, neg_sim), 0-dim; ``pos_sim`` / ``neg_sim`` carry no gradient.
    fp32 device tensors with C a multiple of 32 up to 256 and at least one pair run as one node of the HIP library; anything else takes
    ``matched_info_nce_reference``."""
    from . import _native

    fused = (feat1.is_cuda and feat1.dtype == torch.float32 and feat2.dtype == torch.float32 and feat1.dim() == 2 and feat2.dim() == 2
             and feat1.shape[1] == feat2.shape[1] and match_index.dtype == torch.int64 and match_index.shape[0] >= 1
             and _native.hip_backend().msc_nce_supported(feat1.shape[1]))
    if not fused:
        return matched_info_nce_reference(feat1, feat2, match_index, temperature)
    _native.require_current_device(feat1, feat2, match_index)
    return _FusedInfoNCE.apply(feat1, feat2, match_index, float(temperature))

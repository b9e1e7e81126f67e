"""Lovasz loss -- pointcept/models/losses/lovasz.py (``LovaszLoss``; Berman et al., "The Lovasz-Softmax loss", CVPR 2018), the second
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
        import ctypes
        from . import _native

        be = _native.hip_backend()
        n, c = pred.shape
        prob = torch.empty_like(pred)
        dlogits = torch.empty_like(pred)
        out = torch.empty((2,), dtype=torch.float32, device=pred.device)   # [loss, number of classes averaged]
        # every byte is written before it is read (csrc/lovasz.hip): nothing to zero, no memset node in a captured step
        ws = torch.empty((int(be.lib.pdf_lovasz_workspace_bytes(n, c)),), dtype=torch.uint8, device=pred.device)
        _native.require_current_device(pred, target)
        s = ctypes.c_void_p(_native.raw_stream())
        rc = be.lib.pdf_lovasz_forward(n, c, pred.data_ptr(), target.data_ptr(), ignore,
                                       class_mask.data_ptr() if class_mask is not None else None, prob.data_ptr(), dlogits.data_ptr(),
                                       out.data_ptr(), ws.data_ptr(), s)
        if rc != 0:
            raise RuntimeError(f"pdf_lovasz_forward failed with status {rc}")
        ctx.save_for_backward(dlogits)
        return out[0]

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        import ctypes
        from . import _native

        (dlogits,) = ctx.saved_tensors
        n, c = dlogits.shape
        gy = gy.contiguous().float()
        out = torch.empty_like(dlogits)   # the saved buffer stays untouched: the node may be differentiated again (retain_graph)
        _native.require_current_device(dlogits, gy)
        s = ctypes.c_void_p(_native.raw_stream())
        rc = _native.hip_backend().lib.pdf_lovasz_backward(n, c, dlogits.data_ptr(), gy.data_ptr(), 1.0, out.data_ptr(), s)
        if rc != 0:
            raise RuntimeError(f"pdf_lovasz_backward failed with status {rc}")
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

"""Open-world evaluation metrics on the device (second half): the histogram IoU of
pointcept/utils/misc.py:55-67 (``intersection_and_union_gpu``), the known-class summary of ``OpenSegEvaluator.eval``
(engines/hooks/evaluator.py:77-86) and its per-batch AUPR / AUROC bookkeeping (:196-216, utils/misc.py:70-87).

The class histograms are exact integer counts (``torch.bincount`` instead of three ``torch.histc`` calls over float copies) kept
on the device; across ranks they are summed with one all-reduce of a (3, K) tensor instead of three.  AUPR / AUROC are computed on
the device too (sort by score + cumulative sums: the step-wise precision-recall sum and the trapezoidal ROC area with ties grouped,
i.e. what sklearn.metrics.average_precision_score / roc_auc_score compute); upstream hands the scores to sklearn on the host.

``openset_metrics`` is all of it in one call: on device tensors one capturable pass of the HIP library (csrc/openset_metrics.hip) that
reads nothing back, on CPU tensors the composition of the two functions below, which stay the CPU path and the yardstick.  The evaluators
use it in their deferred mode and the testers for every scene.
"""
import numpy as np
import torch


def intersection_and_union(output, target, k, ignore_index=-1):
    """-> (area_intersection, area_union, area_target), float32 (k,) on the inputs' device.  utils/misc.py:55-67; ``output`` is NOT
    modified (upstream overwrites ignored positions in place)."""
    output, target = output.reshape(-1), target.reshape(-1)
    valid = target != ignore_index
    o, t = output[valid].long(), target[valid].long()
    in_range = (o >= 0) & (o < k)
    area_output = torch.bincount(o[in_range], minlength=k)[:k]
    tr = (t >= 0) & (t < k)
    area_target = torch.bincount(t[tr], minlength=k)[:k]
    hit = (o == t) & in_range
    area_intersection = torch.bincount(o[hit], minlength=k)[:k]
    area_union = area_output + area_target - area_intersection
    return area_intersection.float(), area_union.float(), area_target.float()


def aupr_and_auroc(score, target, unknown_label, ignore_index=-1):
    """utils/misc.py:70-87 on the device: positives = points of the unknown classes, ignored points dropped; (None, None) when the
    batch holds no unknown point.  Returns python floats."""
    score, target = score.reshape(-1).double(), target.reshape(-1)
    valid = target != ignore_index
    score, target = score[valid], target[valid]
    pos = torch.isin(target, torch.as_tensor(list(unknown_label), device=target.device))
    n_pos = int(pos.sum())
    if n_pos == 0:
        return None, None
    n_neg = pos.numel() - n_pos
    order = torch.argsort(score, descending=True, stable=True)
    s, y = score[order], pos[order].double()
    tp, fp = torch.cumsum(y, 0), torch.cumsum(1.0 - y, 0)
    last = torch.ones_like(s, dtype=torch.bool)      # one operating point per DISTINCT score (ties share a threshold)
    last[:-1] = s[1:] != s[:-1]
    tp, fp = tp[last], fp[last]
    recall, precision = tp / n_pos, tp / (tp + fp)
    aupr = float(torch.sum(torch.diff(recall, prepend=recall.new_zeros(1)) * precision))
    if n_neg == 0:
        return aupr, float("nan")
    tpr, fpr = torch.cat([tp.new_zeros(1), tp / n_pos]), torch.cat([fp.new_zeros(1), fp / n_neg])
    auroc = float(torch.trapezoid(tpr, fpr))
    return aupr, auroc


MAX_FUSED_CLASSES = 1024   # csrc/openset_metrics.hip: 3 K + 3 LDS counters per workgroup
_MASKS = {}                # (device, K, unknown ids) -> uint8 (K): the unknown classes as the kernel reads them (see unknown_mask)


def unknown_mask(num_classes, unknown_label, device):
    """``unknown_label`` as K bytes on ``device`` (1 = the class id counts as positive), uploaded once per (device, K, ids).  The upload is
    a host-to-device copy, which must not be recorded into a stream capture: the evaluators and testers make it when they are constructed,
    a bare ``openset_metrics`` call on its first eager call.  Inside a capture a missing mask is an error, never a silent copy."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    ids = tuple(sorted({int(v) for v in unknown_label if 0 <= int(v) < num_classes}))
    key = (str(device), int(num_classes), ids)
    if key not in _MASKS:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"openset_metrics: the unknown-class mask for {num_classes} classes on {device} has not been uploaded yet and "
                               "the stream is capturing; call evaluator.unknown_mask(...) (or run one eager call) before the capture")
        m = torch.zeros(int(num_classes), dtype=torch.uint8)
        m[list(ids)] = 1
        _MASKS[key] = m.to(device)
    return _MASKS[key]


def _fusable(x, score, target, num_classes):
    return (x.is_cuda and target.is_cuda and target.dtype == torch.int64 and target.dim() == 1 and 1 <= num_classes <= MAX_FUSED_CLASSES
            and ((x.dim() == 2 and x.dtype == torch.float32) or (x.dim() == 1 and x.dtype == torch.int64))
            and x.shape[0] == target.shape[0] and 1 <= x.shape[0] < 2 ** 31 - 1
            and (score is None or (score.is_cuda and score.dtype == torch.float32 and score.numel() == target.shape[0])))


@torch.no_grad()
def openset_metrics(seg_logits_or_pred, score, target, num_classes, unknown_label, ignore_index=-1):
    """The metrics of one batch / scene in one call -> (hist (3, K) int64: intersection | union | target, record (4,) float64: aupr, auroc,
    n_pos, n_neg) on the inputs' device.  ``seg_logits_or_pred``: (n, C) logits (prediction = ``max(1)[1]``) or (n) predictions;
    ``score`` (n) or None (record = NaN, NaN, 0, 0); ``unknown_label``: class ids, or the tensor ``unknown_mask`` returned.

    Device tensors -- float32 logits / scores, int64 predictions / labels, K <= 1024, fewer than 2^31 - 1 rows -- take the fused pass
    (csrc/openset_metrics.hip: no host read, capturable, bit-reproducible).  CPU tensors and anything else take the composition of
    ``intersection_and_union`` + ``aupr_and_auroc``.  Both: aupr = auroc = NaN when no kept row is positive (the reference's ``None``) or a
    kept row's score is NaN (the reference raises), auroc = NaN without a negative row."""
    x, k = seg_logits_or_pred, int(num_classes)
    target = target.reshape(-1)
    if score is not None:
        score = score.reshape(-1)
    if _fusable(x, score, target, k):
        from . import _native

        mask = None
        if score is not None:
            mask = unknown_label if isinstance(unknown_label, torch.Tensor) else unknown_mask(k, unknown_label, x.device)
        logits, pred = (x.contiguous(), None) if x.dim() == 2 else (None, x.contiguous())
        return _native.hip_backend().openset_metrics(logits, pred, None if score is None else score.contiguous(), target.contiguous(),
                                                     int(ignore_index), mask, k)
    if isinstance(unknown_label, torch.Tensor):
        unknown_label = torch.nonzero(unknown_label.reshape(-1)).reshape(-1).tolist()
    pred = x.max(1)[1] if x.dim() == 2 else x.reshape(-1)
    i, u, t = intersection_and_union(pred, target, k, ignore_index)
    hist = torch.stack([i, u, t]).double().round().long()   # (bincount results: exact)
    nan = float("nan")
    rec = [nan, nan, 0.0, 0.0]
    if score is not None:
        valid = target != ignore_index
        pos = torch.isin(target[valid], torch.as_tensor([int(v) for v in unknown_label], dtype=target.dtype, device=target.device))
        n_pos = int(pos.sum())
        rec[2], rec[3] = float(n_pos), float(pos.numel() - n_pos)
        if n_pos and not bool(torch.isnan(score[valid]).any()):
            rec[0], rec[1] = aupr_and_auroc(score, target, unknown_label, ignore_index)
    return hist, torch.tensor(rec, dtype=torch.float64, device=target.device)


def _is_multi():
    return torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1


class _Deferred:
    """Bookkeeping the two evaluators share in deferred mode: the running (3, K) int64 histogram, the batches' records and losses as
    tensors wherever they were computed; nothing is read until ``summary()`` (or one of the list attributes) asks -- then ONE host read
    of everything pending."""

    def _reset_deferred(self):
        self.hist = None          # (3, K): float64 (eager updates) or int64 (deferred updates); intersection | union | target
        self._aupr, self._auroc, self._losses = [], [], []
        self._records, self._loss_t = [], []

    def _wants_deferred(self, x):
        return x.is_cuda if self.deferred is None else bool(self.deferred)

    def _add_hist(self, h):
        if _is_multi():
            torch.distributed.all_reduce(h)
        self.hist = h if self.hist is None else self.hist + h.to(self.hist.dtype)

    def _add_loss(self, loss, deferred):
        if loss is None:
            return
        if deferred and isinstance(loss, torch.Tensor):
            self._loss_t.append(loss.detach().reshape(-1)[:1].double())
        else:
            self._flush()         # (keeps the order of the list)
            self._losses.append(float(loss))

    def _flush(self, with_hist=False):
        """-> the histogram as a (3, K) float64 host array when asked for.  One device-to-host copy for all that is pending."""
        parts = [r.reshape(-1) for r in self._records] + self._loss_t
        nr, nl = sum(r.numel() for r in self._records), len(self._loss_t)
        hist = None
        if with_hist and self.hist is not None:
            parts = [self.hist.reshape(-1).double().to(parts[0].device) if parts else self.hist.reshape(-1).double()] + parts
        if not parts:
            return None
        flat = torch.cat(parts).cpu().numpy()
        if with_hist and self.hist is not None:
            nh = self.hist.numel()
            hist, flat = flat[:nh].reshape(3, -1), flat[nh:]
        for a, r, n_pos, _ in flat[:nr].reshape(-1, 4):
            if n_pos > 0:         # a batch without unknown points: the reference's None
                self._aupr.append(float(a)); self._auroc.append(float(r))
        self._losses.extend(float(v) for v in flat[nr:nr + nl])
        self._records, self._loss_t = [], []
        return hist

    @property
    def losses(self):
        self._flush()
        return self._losses


class OpenSegEvaluator(_Deferred):
    """Accumulates what ``OpenSegEvaluator.eval`` logs (engines/hooks/evaluator.py:39-158): class histograms over the validation
    batches, mIoU / mAcc / allAcc over the KNOWN classes, mean AUPR / AUROC over the batches that contain unknown points.

    ``deferred``: True = an update is one ``openset_metrics`` call whose histogram is added on the device and whose record (and loss, when
    it is a tensor) is kept as a tensor -- no host read, so an update can follow a captured forward; ``summary()`` reads everything at
    once.  False = every update reads its figures back (the path for CPU tensors).  None = deferred exactly when the update's tensors
    live on a device.  ``aupr`` / ``auroc`` / ``losses`` are lists in both modes (reading them flushes what is pending)."""

    def __init__(self, num_classes, unknown_label, ignore_index=-1, deferred=None):
        self.num_classes, self.unknown_label, self.ignore_index = num_classes, list(unknown_label), ignore_index
        self.deferred = deferred
        self.mask_known = np.ones(num_classes, dtype=bool)
        self.mask_known[self.unknown_label] = False   # ~selected_mask(unknown_label, num_classes)
        if deferred is not False and torch.cuda.is_available():
            unknown_mask(num_classes, self.unknown_label, "cuda")   # uploaded now: an update may run inside a capture
        self.reset()

    def reset(self):
        self._reset_deferred()

    @property
    def aupr(self):
        self._flush()
        return self._aupr

    @property
    def auroc(self):
        self._flush()
        return self._auroc

    @torch.no_grad()
    def update(self, seg_logits, score, segment_oracle, loss=None):
        """One validation batch: predictions = arg-max of the logits, ``segment_oracle`` = the labels incl. the unknown classes."""
        if self._wants_deferred(seg_logits):
            h, rec = openset_metrics(seg_logits, score, segment_oracle, self.num_classes, self.unknown_label, self.ignore_index)
            self._add_hist(h)
            if _is_multi():   # every rank's record of this batch, as `recognition_metric` gathers the pairs (hooks/evaluator.py:199-221)
                gathered = [torch.empty_like(rec) for _ in range(torch.distributed.get_world_size())]
                torch.distributed.all_gather(gathered, rec)
                rec = torch.stack(gathered)
            self._records.append(rec)
            self._add_loss(loss, True)
            return
        pred = seg_logits.max(1)[1]
        i, u, t = intersection_and_union(pred, segment_oracle, self.num_classes, self.ignore_index)
        self._add_hist(torch.stack([i, u, t]).double())
        pairs = [aupr_and_auroc(score, segment_oracle, self.unknown_label, self.ignore_index)]
        if _is_multi():   # every rank's pair of this batch, None included, as `recognition_metric` gathers them (hooks/evaluator.py:199-221)
            gathered = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(gathered, pairs[0])
            pairs = gathered
        self._flush()
        for a, r in pairs:
            if a is not None:
                self._aupr.append(a); self._auroc.append(r)
        self._add_loss(loss, False)

    def summary(self):
        inter, union, target = self._flush(with_hist=True)
        iou_class, acc_class = inter / (union + 1e-10), inter / (target + 1e-10)
        k = self.mask_known
        return dict(mIoU=float(np.mean(iou_class[k])), mAcc=float(np.mean(acc_class[k])),
                    allAcc=float(inter[k].sum() / (target[k].sum() + 1e-10)), iou_class=iou_class, acc_class=acc_class,
                    aupr=float(np.mean(self._aupr)) if self._aupr else float("nan"),
                    auroc=float(np.mean(self._auroc)) if self._auroc else float("nan"),
                    loss=float(np.mean(self._losses)) if self._losses else float("nan"))


def _selected(labels, k):
    """utils/misc.py:184-187 (``selected_mask``)."""
    m = np.zeros(k, dtype=bool)
    m[list(labels)] = True
    return m


class IncrSegEvaluator(_Deferred):
    """What ``IncrSegEvaluator.eval`` logs for the incremental stage (engines/hooks/evaluator.py:233-405): class histograms of the
    incremental learner's arg-max against ``segment_incr_remap`` over K = base + len(remap) classes, summarised over three class sets:
    ``known`` (the base classes that were not remapped), ``incr`` (the new ids of the selected remapped classes) and ``remap`` (all classes
    except the old and new ids of the remapped ones, plus the selected new ids) -- the masks of :237-261 and :377-405."""

    def __init__(self, base_num_classes, incr_label_remap, incr_label_select=None, ignore_index=-1, deferred=None):
        self.deferred = deferred   # as OpenSegEvaluator: None = deferred exactly when an update's tensors live on a device
        remap = {int(k): int(v) for k, v in incr_label_remap.items()}
        select = list(remap) if incr_label_select is None else [int(k) for k in incr_label_select]
        self.base_num_classes, self.ignore_index = int(base_num_classes), ignore_index
        self.num_classes = self.base_num_classes + len(remap)
        self.mask_known = ~_selected(list(remap), self.base_num_classes)
        self.incr_label_idx = [remap[k] for k in select if k in remap]
        self.mask_incr_remap = ~_selected(list(remap) + list(remap.values()), self.num_classes) | _selected(self.incr_label_idx, self.num_classes)
        self.map_reverse = {v: k for k, v in remap.items()}
        self.reset()

    def reset(self):
        self._reset_deferred()

    @torch.no_grad()
    def update(self, seg_logits, segment_incr_remap, loss=None):
        deferred = self._wants_deferred(seg_logits)
        if deferred:
            h, _ = openset_metrics(seg_logits, None, segment_incr_remap, self.num_classes, (), self.ignore_index)
        else:
            pred = seg_logits.max(1)[1]
            i, u, t = intersection_and_union(pred, segment_incr_remap, self.num_classes, self.ignore_index)
            h = torch.stack([i, u, t]).double()
        self._add_hist(h)
        self._add_loss(loss, deferred)

    def metrics(self, intersection, union, target):
        """``incr_segmentation_metric`` (:377-405) over host arrays -> (iou_class, acc_class, known, incr, remap)."""
        iou_class = intersection / (union + 1e-10)
        acc_class = intersection / (target + 1e-10)
        b, k, idx, r = self.base_num_classes, self.mask_known, self.incr_label_idx, self.mask_incr_remap
        known = {"mIoU": np.mean(iou_class[:b][k]), "mAcc": np.mean(acc_class[:b][k]),
                 "Acc": sum(intersection[:b][k]) / sum(target[:b][k] + 1e-10)}
        incr = {"mIoU": np.mean(iou_class[idx]), "mAcc": np.mean(acc_class[idx]), "Acc": sum(intersection[idx]) / (sum(target[idx]) + 1e-10)}
        remap = {"mIoU": np.mean(iou_class[r]), "mAcc": np.mean(acc_class[r]), "Acc": sum(intersection[r]) / (sum(target[r]) + 1e-10)}
        return iou_class, acc_class, known, incr, remap

    def summary(self):
        inter, union, target = self._flush(with_hist=True)
        iou_class, acc_class, known, incr, remap = self.metrics(inter, union, target)
        out = dict(iou_class=iou_class, acc_class=acc_class, known=known, incr=incr, remap=remap,
                   loss=float(np.mean(self._losses)) if self._losses else float("nan"))
        for name, m in (("known", known), ("incr", incr), ("remap", remap)):
            for key, v in m.items():
                out[f"{key}_{name}"] = float(v)
        return out

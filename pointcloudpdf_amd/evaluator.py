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


class InsSegEvaluator:
    """What ``InsSegEvaluator`` logs (engines/hooks/evaluator.py:592-968): ``associate_instances`` per scene, ``evaluate_matches`` over the
    scenes -> ``all_ap``, ``all_ap_50%``, ``all_ap_25%`` and per-class ``ap / ap50% / ap25%`` (ScanNet's instance benchmark: overlaps
    0.5 .. 0.9 and 0.25, regions of at least 100 points).

    The association never builds a mask: proposals arrive compact -- ``proposal_of`` (N): the row's proposal or -1, what ``PG-v1m1`` returns
    next to the reference's keys; a dense ``pred_masks`` of DISJOINT masks is converted -- and every count of the reference's per-pair
    ``logical_and`` passes (intersection with each ground-truth instance, ``vert_count``, ``void_intersection``) comes from ONE pass over the
    points into a (proposals, instance ids) integer table (csrc/point_group.hip on device tensors, ``bincount`` on the host).  A scene record
    is seven small arrays; the AP curves are float64 NumPy over them on the host (a few hundred numbers), pinned against the reference
    hook's results to 1e-12 by the fixture.  ``update(...)`` per scene, ``summary()`` at the end; the records (``self.scenes``) are gathered
    across ranks by the caller."""

    def __init__(self, num_classes, names=None, segment_ignore_index=(-1,), instance_ignore_index=-1):
        self.num_classes = int(num_classes)
        self.names = [str(i) for i in range(self.num_classes)] if names is None else list(names)
        self.segment_ignore_index = tuple(segment_ignore_index)
        self.instance_ignore_index = instance_ignore_index
        self.valid_class_names = [self.names[i] for i in range(self.num_classes) if i not in self.segment_ignore_index]
        self.overlaps = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
        self.min_region_sizes = 100
        self.reset()

    def reset(self):
        self.scenes, self.losses = [], []

    # -- counts ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _proposal_of(pred):
        if pred.get("proposal_of") is not None:
            return pred["proposal_of"].to(torch.int32)
        hit = pred["pred_masks"].ne(0)
        if hit.shape[0] == 0:
            return torch.full((hit.shape[1],), -1, dtype=torch.int32, device=hit.device)
        if int(hit.sum(0).max()) > 1:
            raise ValueError("InsSegEvaluator: overlapping pred_masks have no compact form; pass disjoint masks or `proposal_of`")
        of = hit.to(torch.int8).argmax(0).to(torch.int32)
        return torch.where(hit.any(0), of, torch.full_like(of, -1))

    def intersection_table(self, proposal_of, num_proposals, segment, instance, index_map=None):
        """-> (instance_ids (G), segment_ids (G), gt counts (G), table (P, G), vert_count (P), void_intersection (P)) as host arrays;
        ``index_map`` (M): evaluated point j reads ``proposal_of[index_map[j]]`` (the 1-NN map to the original cloud)."""
        dev = segment.device
        ignored = torch.as_tensor(list(self.segment_ignore_index), device=dev, dtype=segment.dtype)
        void = torch.isin(segment, ignored)
        ids, inverse, counts = torch.unique(instance, return_inverse=True, return_counts=True)
        rows = torch.arange(instance.shape[0], device=dev)
        first = torch.full((ids.shape[0],), instance.shape[0], dtype=torch.long, device=dev).scatter_reduce_(0, inverse, rows, "amin")
        segment_ids = segment[first]
        g, p = int(ids.shape[0]), int(num_proposals)
        if proposal_of.is_cuda:
            from . import _native

            table, vert, voidc = _native.hip_backend().pg_intersections(
                proposal_of.contiguous(), p, inverse.to(torch.int32).contiguous(), g, void.contiguous(),
                None if index_map is None else index_map.long().contiguous())
        else:
            of = (proposal_of if index_map is None else proposal_of[index_map.long()]).long()
            inside = of >= 0
            table = torch.bincount(of[inside] * g + inverse[inside], minlength=p * g).reshape(p, g)
            vert = torch.bincount(of[inside], minlength=p)
            voidc = torch.bincount(of[inside & void], minlength=p)
        return tuple(t.cpu().numpy() for t in (ids, segment_ids, counts, table, vert, voidc))

    def associate_instances(self, pred, segment, instance, index_map=None):
        """The scene record the AP needs, as arrays (what the reference hook keeps as nested dicts with a mask per proposal):
        ``gt_class / gt_size`` of the ground-truth instances that count (id not the ignore id, class not ignored; ascending id),
        ``pr_class / pr_score / pr_size / pr_void`` of the proposals that count (class not ignored, at least ``min_region_sizes`` points;
        in proposal order) and ``inter`` (proposals, instances): the shared point counts."""
        classes = np.asarray(pred["pred_classes"].cpu()).astype(np.int64).reshape(-1)
        scores = np.asarray(pred["pred_scores"].cpu()).astype(np.float64).reshape(-1)
        of = self._proposal_of(pred).to(segment.device)
        ids, segment_ids, counts, table, vert, voidc = self.intersection_table(of, classes.shape[0], segment, instance, index_map)
        ignored = np.asarray(self.segment_ignore_index)
        gt_keep = (ids != self.instance_ignore_index) & ~np.isin(segment_ids, ignored)
        pr_keep = ~np.isin(classes, ignored) & (vert >= self.min_region_sizes)
        return dict(gt_class=segment_ids[gt_keep].astype(np.int64), gt_size=counts[gt_keep].astype(np.int64),
                    pr_class=classes[pr_keep], pr_score=scores[pr_keep], pr_size=vert[pr_keep].astype(np.int64),
                    pr_void=voidc[pr_keep].astype(np.int64), inter=table[pr_keep][:, gt_keep].astype(np.int64))

    @torch.no_grad()
    def update(self, output_dict, input_dict):
        """One validation scene: the model's eval output and its input (``segment``, ``instance``; with ``origin_coord`` the proposals are
        carried to the original cloud through ``pointops.knn_query(1, ...)`` and scored against ``origin_segment`` / ``origin_instance``)."""
        segment, instance, index_map = input_dict["segment"], input_dict["instance"], None
        if "origin_coord" in input_dict:
            from . import pointops

            idx, _ = pointops.knn_query(1, input_dict["coord"].float(), input_dict["offset"].int(), input_dict["origin_coord"].float(),
                                        input_dict["origin_offset"].int())
            index_map = idx.flatten().long()
            segment, instance = input_dict["origin_segment"], input_dict["origin_instance"]
        self.scenes.append(self.associate_instances(output_dict, segment, instance, index_map))
        if output_dict.get("loss") is not None:
            self.losses.append(float(output_dict["loss"]))

    # -- average precision (float64 on the host) ---------------------------------------------------------------------------------------
    def _scene_records(self, scene, cls, threshold):
        """One scene, one class, one overlap threshold -> (scores of the true positives, scores of the false positives, missed instances,
        has an instance that counts, has a proposal).  Rules of the ScanNet benchmark as the reference hook applies them: instances in
        order, each takes the first free proposal whose IoU exceeds the threshold and keeps the best score among all free ones that do
        (the others are false positives); a proposal that exceeds the threshold with no instance of its class is a false positive unless
        more than ``threshold`` of it lies on ignored ground (void points and instances below ``min_region_sizes``)."""
        g, p = scene["gt_class"] == cls, scene["pr_class"] == cls
        inter = scene["inter"][p][:, g]
        gsize, psize, score = scene["gt_size"][g], scene["pr_size"][p], scene["pr_score"][p]
        iou = inter / np.maximum(gsize[None, :] + psize[:, None] - inter, 1)
        over = (inter > 0) & (iou > threshold)
        big = gsize >= self.min_region_sizes
        taken = np.zeros(psize.shape[0], bool)
        hits, false_alarms, missed = [], [], 0
        for j in np.nonzero(big)[0]:
            free = np.nonzero(over[:, j] & ~taken)[0]
            if free.size == 0:
                missed += 1
                continue
            taken[free[0]] = True
            ranked = np.sort(score[free])
            hits.append(ranked[-1])
            false_alarms.extend(ranked[:-1])
        lonely = ~over.any(1)
        on_ignored = scene["pr_void"][p] + inter[:, ~big].sum(1)
        false_alarms.extend(score[lonely & (on_ignored / np.maximum(psize, 1) <= threshold)])
        return hits, false_alarms, missed, bool(big.any()), bool(p.any())

    @staticmethod
    def _average_precision(hits, false_alarms, missed):
        """Area under the precision-recall curve with one operating point per distinct score and the benchmark's half-step widths."""
        score = np.concatenate([np.asarray(hits, float), np.asarray(false_alarms, float)])
        truth = np.concatenate([np.ones(len(hits)), np.zeros(len(false_alarms))])
        order = np.argsort(score, kind="stable")
        score, truth = score[order], truth[order]
        _, first = np.unique(score, return_index=True)              # operating point k keeps the records from first[k] on
        below = np.concatenate([[0.0], np.cumsum(truth)])[first]    # true records under the point
        tp = truth.sum() - below
        kept = score.shape[0] - first
        precision = np.append(tp / np.maximum(kept, 1), 1.0)
        recall = np.append(tp / np.maximum(tp + below + missed, 1), 0.0)
        padded = np.concatenate([recall[:1], recall, [0.0]])
        return float(np.dot(precision, 0.5 * (padded[:-2] - padded[2:])))

    def evaluate_matches(self, scenes):
        """Scene records -> the hook's dict: ``all_ap`` (mean over classes and the overlaps 0.5 .. 0.9), ``all_ap_50%``, ``all_ap_25%``,
        ``classes[name]`` = ``ap / ap50% / ap25%``.  A class without instances is NaN (left out of the means), one with instances but no
        proposal 0."""
        class_ids = [i for i in range(self.num_classes) if i not in self.segment_ignore_index]
        table = np.full((len(class_ids), len(self.overlaps)), np.nan)
        for ci, cls in enumerate(class_ids):
            for ti, threshold in enumerate(self.overlaps):
                parts = [self._scene_records(scene, cls, threshold) for scene in scenes]
                has_gt, has_pred = any(r[3] for r in parts), any(r[4] for r in parts)
                if has_gt and has_pred:
                    table[ci, ti] = self._average_precision([v for r in parts for v in r[0]], [v for r in parts for v in r[1]],
                                                            sum(r[2] for r in parts))
                elif has_gt:
                    table[ci, ti] = 0.0
        is25, is50 = np.isclose(self.overlaps, 0.25), np.isclose(self.overlaps, 0.5)
        out = {"all_ap": np.nanmean(table[:, ~is25]), "all_ap_50%": np.nanmean(table[:, is50]), "all_ap_25%": np.nanmean(table[:, is25]),
               "classes": {}}
        for ci, name in enumerate(self.valid_class_names):
            out["classes"][name] = {"ap": np.mean(table[ci, ~is25]), "ap50%": np.mean(table[ci, is50]), "ap25%": np.mean(table[ci, is25])}
        return out

    def summary(self):
        out = self.evaluate_matches(self.scenes)
        out["loss"] = float(np.mean(self.losses)) if self.losses else float("nan")
        return out

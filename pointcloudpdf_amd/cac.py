"""Context-aware classifier -- pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py (``CACSegmentor``,
registered as ``"CAC-v1m1"``; Tian et al., "Learning Context-aware Classifier for Semantic Segmentation", AAAI 2023): the head of the
``semseg-cac-v1m1-*`` recipes over any backbone built with ``num_classes=0``.

With ``F = backbone(data)`` (N, c), ``W = seg_head.weight`` (K, c), ``L = seg_head(F)``:

    soft prototypes, per scene s:   w_nk = softmax(L_n)_k [max_k softmax(L_n) >= conf_thresh],  A_k = sum_{n in s} w_nk,
                                    proto_s[k] = sum_{n in s} w_nk F_n / (A_k + 1e-7);
                                    refine_s = cos(feat_proj_layer(F_s), proj(cat[proto_s, W])) * cos_temp
    label prototypes, whole batch:  row y = sum_{t_n = y} F_n / (count_y + 1e-4) for the classes among the labels, W.detach()[y] elsewhere;
                                    cac_pred = cos(feat_proj_layer(F), apd_proj(cat[., W])) * cos_temp                  (train only)
    distillation loss:              l_n = -sum_k log_softmax(refine)_nk (0.5 softmax(cac_pred)_nk + 0.5 onehot_nk),
                                    e_n = -sum_k sm_nk log(sm_nk + 1e-4), per class y among the labels: sum_{t=y} l e / (sum_{t=y} e + 1e-4),
                                    loss = their sum / (#classes + 1e-4)

The four ops below are autograd nodes over csrc/cac.hip for fp32 device tensors in the fused class (``pdf_cac_supported(K, c)``: c a
multiple of 4 up to 64, K <= 256 -- it contains (20, 48), (13, 48), (13, 24), (200, 48)): segmented, fixed-order sums without atomics,
nothing read back to the host, so the head sits inside a captured step and is bit-reproducible.  Every op has a ``*_torch`` composition
that restates the reference's arithmetic without host reads (``unique`` becomes counts, boolean indexing becomes ``where``): it serves
host tensors and every other shape or dtype, and is the independent side of the tests and of tools/cac_bench.py.

Where the reference reads the device (a Python loop over ``offset[i]``, two ``target.unique()``, ``torch.zeros(..).cuda()`` scatters) this
module does not; the only scene sizes the head needs on the host are the row slices of the train-mode ``feat_proj_layer`` calls (its
BatchNorm sees one scene at a time), taken from ``data_dict["offset_host"]`` when present, else from ONE read of ``offset``.

Choices of this package where the reference leaves the result open:

* all rows ignored: the distillation loss is a scalar 0 with a zero gradient (the reference: the same value, through a host branch);
* a label that is neither -1 nor in [0, K) makes the distillation loss NaN, as the fused criteria do (the reference's scatter raises);
  the label prototypes skip such rows;
* ``eps > 0`` in the distillation loss runs as the composition (no reference recipe sets it).

Not provided: open-set scoring over CAC (``engine.build_open_seg_step`` refuses the model: its ``backbone`` hook would hand features,
not logits, to ``MaxProbability``).  The ``*-spunet`` CAC recipes build over sparse_unet.py's SpUNet-v1m1."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import dense
from .dense import _amp_bwd, _amp_fwd   # (custom nodes keep fp32 tensors under autocast: dense.py)
from .registry import MODELS, build_model
from .segmentor import build_criteria
from .stratified import _Linear

FORCE_TORCH = False   # module-wide switch: every op takes its composition (tools/cac_bench.py's other side; tests compare both)


def _scene_ids(offset, n):
    """Scene of every row from the scenes' ends, on the device."""
    return torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)


def _bounds(offset_host):
    ends = [int(v) for v in offset_host]
    return list(zip([0] + ends[:-1], ends))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Compositions
# ---------------------------------------------------------------------------------------------------------------------------------------
def _masked_softmax(logits, conf_thresh):
    p = F.softmax(logits, 1)
    if conf_thresh > 0:
        p = p * (p.max(1)[0] >= conf_thresh).to(p.dtype).unsqueeze(1)   # (:111-115: the mask is a constant of the graph)
    return p


def soft_prototypes_torch(feat, logits, offset, conf_thresh=0.0, offset_host=None):
    """(B, K, c) soft prototypes (post_refine_proto_batch :130-141).  With ``offset_host`` (the scenes' ends as Python ints) the scenes are
    sliced as the reference slices them; without, the scene sums are products with the scenes' one-hot matrix: no host read either way."""
    p = _masked_softmax(logits, conf_thresh)
    if offset_host is not None:
        out = []
        for a, b in _bounds(offset_host):
            ps = p[a:b].permute(1, 0)
            out.append((ps / (ps.sum(-1).unsqueeze(-1) + 1e-7)) @ feat[a:b])
        return torch.stack(out)
    n, k = p.shape
    b = offset.shape[0]
    sid = _scene_ids(offset, n)
    scene = F.one_hot(sid, b).to(p.dtype)                       # (n, B)
    mass = scene.t() @ p                                        # (B, K)
    w = p / (mass[sid] + 1e-7)
    return ((scene.unsqueeze(2) * w.unsqueeze(1)).reshape(n, b * k).t() @ feat).view(b, k, feat.shape[1])


def class_prototypes_torch(feat, target, base):
    """(K, c): the mean feature of every class among the labels (divisor count + 1e-4), ``base`` for the others
    (get_adaptive_perspective :77-89, the ``unique`` loop as counts)."""
    k = base.shape[0]
    valid = (target >= 0) & (target < k)
    hot = F.one_hot(target.clamp(0, k - 1), k).to(feat.dtype) * valid.to(feat.dtype).unsqueeze(1)
    count = hot.sum(0)
    mean = (hot.t() @ feat) / (count.unsqueeze(1) + 1e-4)
    return torch.where((count > 0).unsqueeze(1), mean, base)


def cosine_logits_torch(x, proto, offset=None, scale=1.0, offset_host=None):
    """``scale * normalize(x) @ normalize(proto).T`` (get_pred); proto (K, c), or (B, K, c) with the scenes' ``offset``."""
    xh, ph = F.normalize(x, 2, 1), F.normalize(proto, 2, -1)
    if proto.dim() == 2:
        return xh @ ph.t() * scale
    if offset_host is not None:
        return torch.cat([xh[a:b] @ ph[s].t() for s, (a, b) in enumerate(_bounds(offset_host))], 0) * scale
    n, (b, k, c) = x.shape[0], proto.shape
    every = (xh @ ph.reshape(b * k, c).t()).view(n, b, k)
    sid = _scene_ids(offset, n)
    return every.gather(1, sid.view(n, 1, 1).expand(n, 1, k)).squeeze(1) * scale


def distill_loss_torch(pred, soft, target, smoothness=0.5, eps=0):
    """get_distill_loss (:151-198) without ``unique``, boolean indexing or host branches; the gradient reaches ``pred`` only."""
    n, k = soft.shape
    soft = soft.detach()
    valid = target != -1
    bad = valid & ((target < 0) | (target >= k))
    sm = F.softmax(soft, 1)
    hot = F.one_hot(torch.where(valid, target, torch.zeros_like(target)).clamp(0, k - 1), k).to(pred.dtype)
    label = smoothness * sm + (1 - smoothness) * hot
    if eps > 0:
        label = label * (1 - eps) + (1 - label) * eps / (k - 1)
    loss = (-1 * F.log_softmax(pred, 1) * label).sum(1)
    entropy = -1 * (sm * torch.log(sm + 1e-4)).sum(1) * valid.to(pred.dtype)
    cls = F.one_hot(target.clamp(0, k - 1), k).to(pred.dtype) * (valid & ~bad).to(pred.dtype).unsqueeze(1)
    count = cls.sum(0)
    num, den = cls.t() @ (loss * entropy), cls.t() @ entropy
    present = count > 0
    per = torch.where(present, num / (den + 1e-4), torch.zeros_like(num))
    np_ = present.sum().to(pred.dtype)
    out = torch.where(np_ > 0, per.sum() / (np_ + 1e-4), torch.zeros_like(np_))
    return torch.where(bad.any(), torch.full_like(out, float("nan")), out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Fused nodes (csrc/cac.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _be():
    from . import _native

    return _native.hip_backend()


def _fused(rows, k, *others):
    if FORCE_TORCH or not (rows.is_cuda and rows.dim() == 2 and rows.dtype == torch.float32 and rows.shape[0] > 0):
        return False
    if any(t is not None and (not t.is_cuda or (t.is_floating_point() and t.dtype != torch.float32)) for t in others):
        return False
    return _be().cac_supported(k, rows.shape[1])


class _SoftPrototypes(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, logits, offset, conf_thresh):
        proto, mass = _be().cac_soft_proto_forward(feat, logits, offset, conf_thresh)
        ctx.save_for_backward(feat, logits, offset, proto, mass)
        ctx.conf_thresh = conf_thresh
        return proto

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        feat, logits, offset, proto, mass = ctx.saved_tensors
        gfeat, glogits = _be().cac_soft_proto_backward(feat, logits, offset, ctx.conf_thresh, proto, mass, g.contiguous().float(),
                                                       ctx.needs_input_grad[1])
        return gfeat, glogits, None, None


class _ClassPrototypes(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, target, base):
        proto, count = _be().cac_label_proto_forward(feat, target, base)
        ctx.save_for_backward(target, count)
        return proto

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        target, count = ctx.saved_tensors
        g = g.contiguous().float()
        gbase = torch.where((count > 0).unsqueeze(1), torch.zeros_like(g), g) if ctx.needs_input_grad[2] else None   # ((K, c): tiny)
        return _be().cac_label_proto_backward(target, count, g), None, gbase


class _CosineLogits(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, proto, offset, scale):
        ctx.save_for_backward(x, proto, offset)
        ctx.scale = scale
        return _be().cac_cosine_forward(x, proto, offset, scale)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, proto, offset = ctx.saved_tensors
        gx, gproto = _be().cac_cosine_backward(x, proto, offset, ctx.scale, g.contiguous().float())
        return gx, gproto, None, None


class _DistillLoss(torch.autograd.Function):
    """The forward leaves the unscaled gradient and the class coefficients; the backward only reads them (retain_graph)."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, pred, soft, target, smoothness):
        loss, grad, acc = _be().cac_distill_forward(pred, soft, target, smoothness)
        ctx.save_for_backward(grad, target, acc)
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, gy):
        grad, target, acc = ctx.saved_tensors
        return _be().cac_distill_backward(grad, target, acc, gy.contiguous().float()), None, None, None


def _offset32(offset):
    return offset if offset.dtype == torch.int32 and offset.is_contiguous() else offset.int().contiguous()


def soft_prototypes(feat, logits, offset, conf_thresh=0.0, offset_host=None):
    """Per-scene soft prototypes (B, K, c); gradients into ``feat`` and ``logits``.  ``offset_host`` only serves the composition."""
    if _fused(feat, logits.shape[1], logits, offset) and logits.dim() == 2:
        return _SoftPrototypes.apply(feat.contiguous(), logits.contiguous(), _offset32(offset), float(conf_thresh))
    return soft_prototypes_torch(feat, logits, offset, conf_thresh, offset_host)


def class_prototypes(feat, target, base):
    """Label prototypes (K, c) over the whole batch; the gradient reaches ``feat`` (and ``base`` on the rows it supplies)."""
    if _fused(feat, base.shape[0], base, target) and target.dtype == torch.int64:
        return _ClassPrototypes.apply(feat.contiguous(), target.contiguous(), base.contiguous())
    return class_prototypes_torch(feat, target, base)


def cosine_logits(x, proto, offset=None, scale=1.0, offset_host=None):
    """``scale * cos(x_n, proto[k])``; proto (K, c), or per-scene (B, K, c) with ``offset``."""
    if _fused(x, proto.shape[-2], proto, offset) and proto.shape[-1] == x.shape[1]:
        return _CosineLogits.apply(x.contiguous(), proto.contiguous(), None if proto.dim() == 2 else _offset32(offset), float(scale))
    return cosine_logits_torch(x, proto, offset, scale, offset_host)


def distill_loss(pred, soft, target, smoothness=0.5, eps=0):
    """The distillation loss between the refined logits (``pred``, differentiated) and the label-side logits (``soft``, constant)."""
    if (eps == 0 and not FORCE_TORCH and pred.is_cuda and pred.dim() == 2 and pred.dtype == torch.float32 and soft.dtype == torch.float32
            and soft.shape == pred.shape and target.dtype == torch.int64 and 0 < pred.shape[1] <= 256 and pred.shape[0] > 0):
        return _DistillLoss.apply(pred.contiguous(), soft.detach().contiguous(), target.contiguous(), float(smoothness))
    return distill_loss_torch(pred, soft, target, smoothness, eps)


# ---------------------------------------------------------------------------------------------------------------------------------------
@MODELS.register_module("CAC-v1m1")
class CACSegmentor(nn.Module):
    """The reference's constructor, submodule names and ``state_dict`` keys; train -> {loss, seg_loss, pre_loss, pre_self_loss, kl_loss},
    eval with labels -> {loss (of the PRE-logits, as the reference), seg_logits (refined)}, test -> {seg_logits}."""

    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None, cos_temp=15, main_weight=1, pre_weight=1,
                 pre_self_weight=1, kl_weight=1, conf_thresh=0, detach_pre_logits=False):
        super().__init__()
        self.num_classes = num_classes
        self.cos_temp = cos_temp
        self.main_weight = main_weight
        self.pre_weight = pre_weight
        self.pre_self_weight = pre_self_weight
        self.kl_weight = kl_weight
        self.conf_thresh = conf_thresh
        self.detach_pre_logits = detach_pre_logits
        c = backbone_out_channels
        self.backbone = build_model(backbone)
        self.seg_head = _Linear(c, num_classes)
        self.proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.apd_proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.feat_proj_layer = nn.Sequential(_Linear(c, c, bias=False), nn.BatchNorm1d(c), nn.ReLU(inplace=True), _Linear(c, c))
        self.criteria = build_criteria(criteria)

    def _feat_proj(self, x):
        """feat_proj_layer on (rows, c): Linear -> BatchNorm1d -> ReLU -> Linear through the nodes PointTransformerV2's seg_head uses."""
        lin, bn, _, out = self.feat_proj_layer
        if dense.linbn_ok(lin, bn, x):
            return out(dense.linear_bn_act(lin, bn, x, True))
        return out(dense.bn_act(bn, lin(x), relu=True))

    def _scene_rows(self, data_dict, n):
        host = data_dict.get("offset_host")
        if host is None:
            host = data_dict["offset"].tolist()   # the ONE host read of the head (train mode without offset_host)
        bounds = _bounds(host)
        if bounds[-1][1] != n:
            raise ValueError(f"CAC-v1m1: offset ends at {bounds[-1][1]} for {n} rows")
        return bounds

    def refine(self, feat, seg_logits, data_dict):
        """post_refine_proto_batch (:97-149) * cos_temp."""
        offset, host = data_dict["offset"], data_dict.get("offset_host")
        weight = self.seg_head.weight
        pred = seg_logits.detach() if self.detach_pre_logits else seg_logits
        proto = soft_prototypes(feat, pred, offset, self.conf_thresh, host)
        proto = self.proj(torch.cat([proto, weight.unsqueeze(0).expand(proto.shape[0], -1, -1)], -1))
        if self.training:   # the BatchNorm sees one scene at a time, in order: batch statistics and one running update per scene
            bounds = self._scene_rows(data_dict, feat.shape[0])
            if any(b - a == 1 for a, b in bounds):
                raise ValueError("Expected more than 1 value per channel when training: CAC-v1m1 normalises every scene on its own, "
                                 "and this batch has a one-row scene")
            x = torch.cat([self._feat_proj(feat[a:b]) for a, b in bounds], 0)
        else:               # running statistics: row-wise, the whole batch at once
            x = self._feat_proj(feat)
        return cosine_logits(x, proto, offset, float(self.cos_temp), host)

    def adaptive_perspective(self, feat, target):
        """get_adaptive_perspective (:72-95) * cos_temp."""
        weight = self.seg_head.weight
        proto = class_prototypes(feat, target, weight.detach())
        proto = self.apd_proj(torch.cat([proto, weight], -1))
        return cosine_logits(self._feat_proj(feat), proto, None, float(self.cos_temp))

    @dense.fp32_path
    def forward(self, data_dict):
        feat = self.backbone(data_dict)
        seg_logits = self.seg_head(feat)
        refine_logits = self.refine(feat, seg_logits, data_dict)
        if self.training:
            target = data_dict["segment"]
            cac_pred = self.adaptive_perspective(feat, target)
            seg_loss = self.criteria(refine_logits, target) * self.main_weight
            pre_loss = self.criteria(cac_pred, target) * self.pre_weight
            pre_self_loss = self.criteria(seg_logits, target) * self.pre_self_weight
            kl_loss = distill_loss(refine_logits, cac_pred.detach(), target) * self.kl_weight
            loss = seg_loss + pre_loss + pre_self_loss + kl_loss
            return dict(loss=loss, seg_loss=seg_loss, pre_loss=pre_loss, pre_self_loss=pre_self_loss, kl_loss=kl_loss)
        if "segment" in data_dict.keys():
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]), seg_logits=refine_logits)
        return dict(seg_logits=refine_logits)

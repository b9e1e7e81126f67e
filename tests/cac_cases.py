"""Shared by tests/golden/make_golden_cac.py, test_cac_cpu.py and test_gpu_cac.py: the cases of tests/golden/ops_cac_ref.npz and
model_cac_ref.npz, their inputs (regenerated from seeds: the fixtures hold results only, with a checksum of the inputs), the four op
chains and the tolerance rule.

Op chains -- each is ONE method of the reference's ``CACSegmentor`` with its small MLPs stubbed out (``proj`` / ``apd_proj`` keep the
first c columns of their input, ``feat_proj_layer`` is the identity), so that a chain is exactly a composition of this package's ops:

    refine    post_refine_proto_batch(feat, logits, W, offset) = cosine_logits(feat, soft_prototypes(feat, logits, offset, thr), offset)
    adaptive  get_adaptive_perspective(feat, target, base, W)  = cosine_logits(feat, class_prototypes(feat, target, base))
    pred      get_pred(feat, base)                             = cosine_logits(feat, base)
    distill   get_distill_loss(logits, soft, target)           = distill_loss(logits, soft, target)

Each chain is differentiated with a fixed upstream gradient ``gout`` (the scalar sum(out * gout); distill: the loss itself) with respect
to every input that carries a gradient.

Tolerance (the rule of tests/criteria_cases.py; nothing measured goes into it).  For every case the same chain is evaluated in float64
(this package's composition: test_cac_cpu.py pins it to the reference's fp32 result by the same rule); the result under test may be off by
at most 2x the error of the reference's own fp32 result (``<case>_<chain>_<tensor>_e32`` in the fixture, against the reference's own
float64 run) and never has to be closer than FLOOR_ULP fp32 ulps of the largest magnitude of the tensor.  FLOOR_ULP counts the roundings
on the longest path to an element: softmax (exp, sum, quotient: 3), the normaliser quotient (1), the class sum's final rounding (1), the
two norms (sqrt + quotient each: 4), the dot product's final rounding (1), the scale (1), and for a gradient the same path walked back
once more: 11 forward, 22 for a gradient; one bound is used for both: 24.  A gradient of a cosine chain is a difference of terms of the
magnitude of the chain's output times the upstream gradient, and it can cancel analytically (a one-row scene: cos(F, proto) = 1 whatever
F is, its gradient is rounding noise in the reference as well): the floor of such a gradient is therefore taken relative to
max(|gradient|, |output|), never relative to a vanishing gradient alone.  The distillation loss's gradient keeps its own scale."""
import os

import numpy as np
import torch

ULP = 2.0 ** -23
FLOOR_ULP = 24
CHAINS = ("refine", "adaptive", "pred", "distill")
# name: (scene sizes, K, c, share of ignored rows (1.0: all), absent classes, threshold on, detach_pre_logits, seed, extras)
CASES = {
    "n1_k2_c32": ([1], 2, 32, 0.0, (), False, False, 501, ()),
    "n2_k13_c24_thr": ([2], 13, 24, 0.0, (), True, False, 502, ()),
    "n63_k20_c48_thr_detach": ([63], 20, 48, 0.1, (3, 7), True, True, 503, ()),
    "n257_k13_c24_zero_row": ([257], 13, 24, 0.1, (5,), False, False, 504, ("zero_row",)),
    "n257_k13_c48_thr": ([257], 13, 48, 0.0, (), True, False, 505, ()),
    "n33_k65_c96_thr": ([33], 65, 96, 0.1, (), True, False, 506, ()),
    "n33_k200_c48_thr": ([33], 200, 48, 0.1, (), True, False, 507, ()),
    "n63_k13_c24_all_ignored": ([63], 13, 24, 1.0, (), False, False, 508, ()),
    "scenes_k13_c24_thr": ([1500, 7, 700], 13, 24, 0.1, (11,), True, False, 509, ("quiet_scene",)),
    "scenes_k2_c32_detach": ([1500, 7, 700], 2, 32, 0.1, (), False, True, 510, ()),
    "scenes_k200_c48_thr_detach": ([24, 7, 16], 200, 48, 0.1, (), True, True, 511, ("quiet_scene",)),
}
KEEP_ROWS = 128   # results of more rows are stored every ceil(rows / KEEP_ROWS)-th row (the fixtures stay under 1 MB)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def thin(a):
    a = np.asarray(a)
    return a[::-(-a.shape[0] // KEEP_ROWS)] if a.ndim >= 2 and a.shape[0] > KEEP_ROWS else a


def inputs(name):
    """CPU fp32 inputs of a case: feat (N, c), logits (N, K), soft (N, K), gout (N, K), base (K, c), target (N), offset (B) int32,
    offset_host.  ``zero_row``: one all-zero feature row; ``quiet_scene``: the second scene's logits are nearly flat, so none of its rows
    passes a threshold."""
    sizes, k, c, ignored, absent, _, _, seed, extras = CASES[name]
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    feat = torch.randn(n, c, generator=g)
    logits = 2.0 * torch.randn(n, k, generator=g)
    soft = 2.0 * torch.randn(n, k, generator=g)
    gout = torch.randn(n, k, generator=g)
    base = torch.randn(k, c, generator=g)
    present = torch.tensor([j for j in range(k) if j not in absent])
    target = present[torch.randint(0, len(present), (n,), generator=g)]
    if ignored >= 1.0:
        target[:] = -1
    elif ignored > 0 and n > 2:
        target[torch.randperm(n, generator=g)[: max(1, int(round(ignored * n)))]] = -1
    ends = np.cumsum(sizes)
    if "zero_row" in extras:
        feat[n // 3] = 0.0
    if "quiet_scene" in extras:
        logits[ends[0]:ends[1]] *= 0.01
    return dict(feat=feat, logits=logits, soft=soft, gout=gout, base=base, target=target,
                offset=torch.tensor(ends, dtype=torch.int32), offset_host=[int(v) for v in ends])


def checksum(inp):
    return np.array([float(inp[k].double().sum()) for k in ("feat", "logits", "soft", "gout", "base", "target")])


def pick_threshold(maxima32, maxima64):
    """The rule of the fixtures: the threshold sits in the middle of the widest gap of the sorted row maxima between the 30th and the 70th
    percentile, and that half-gap is at least 100x the fp32-vs-float64 difference of the maxima -- so no row is near the kink."""
    m = np.sort(np.asarray(maxima64, dtype=np.float64))
    n = len(m)
    if n == 1:
        thr, half = 0.5 * m[0], 0.5 * m[0]
    else:
        lo, hi = (int(0.3 * (n - 1)), max(int(np.ceil(0.7 * (n - 1))), int(0.3 * (n - 1)) + 1)) if n > 2 else (0, 1)
        gaps = m[lo + 1:hi + 1] - m[lo:hi]
        i = int(np.argmax(gaps))
        thr, half = 0.5 * (m[lo + i] + m[lo + i + 1]), 0.5 * gaps[i]
    diff = float(np.abs(np.asarray(maxima32, dtype=np.float64) - np.asarray(maxima64, dtype=np.float64)).max())
    assert half >= 100.0 * diff and half > 0, (half, diff)
    return float(np.float32(thr))


def load(which="ops"):
    return np.load(os.path.join(GOLDEN, f"{which}_cac_ref.npz"))


def chain(name, which, ops, inp, thr, dtype=None, device=None):
    """Run one chain with the ops of ``ops`` (the package's fused entry points or its ``*_torch`` compositions as a namespace) -> dict
    of detached results: ``out`` and one gradient per differentiated input."""
    _, k, c, _, _, _, detach, _, _ = CASES[name]
    cast = lambda t: t.to(device=device or t.device, dtype=(dtype or t.dtype) if t.is_floating_point() else t.dtype)
    t = {key: (cast(v) if torch.is_tensor(v) else v) for key, v in inp.items()}
    leaf = lambda key: t[key].detach().clone().requires_grad_()
    if which == "refine":
        feat, logits = leaf("feat"), leaf("logits")
        pred = logits.detach() if detach else logits
        proto = ops.soft_prototypes(feat, pred, t["offset"], thr, t["offset_host"])
        out = ops.cosine_logits(feat, proto, t["offset"], 1.0, t["offset_host"])
        wrt = {"feat": feat} if detach else {"feat": feat, "logits": logits}
        extra = {"proto": proto.detach()}
    elif which == "adaptive":
        feat, base = leaf("feat"), leaf("base")
        out = ops.cosine_logits(feat, ops.class_prototypes(feat, t["target"], base))
        wrt, extra = {"feat": feat, "base": base}, {}
    elif which == "pred":
        feat, base = leaf("feat"), leaf("base")
        out = ops.cosine_logits(feat, base)
        wrt, extra = {"feat": feat, "base": base}, {}
    else:
        logits = leaf("logits")
        out = ops.distill_loss(logits, t["soft"], t["target"])
        wrt, extra = {"logits": logits}, {}
    res = dict(out=out.detach(), **extra)
    if out.requires_grad:
        (out if out.dim() == 0 else (out * t["gout"]).sum()).backward()
    for key, v in wrt.items():
        res["g_" + key] = v.grad.detach() if v.grad is not None else torch.zeros_like(v)
    return res


def torch_ops():
    import types

    from pointcloudpdf_amd import cac

    return types.SimpleNamespace(soft_prototypes=cac.soft_prototypes_torch, class_prototypes=cac.class_prototypes_torch,
                                 cosine_logits=cac.cosine_logits_torch, distill_loss=cac.distill_loss_torch)


def fused_ops():
    from pointcloudpdf_amd import cac

    return cac


def bound(ref_err, truth, out_scale=0.0):
    """``out_scale``: max |output| of a cosine chain when ``truth`` is one of its gradients (module docstring), else 0."""
    scale = max(float(np.abs(np.asarray(truth, dtype=np.float64)).max()) if np.size(truth) else 0.0, float(out_scale))
    return max(2.0 * float(ref_err), FLOOR_ULP * ULP * scale)


def check_chain(name, which, res, truth, golden, report=print):
    """Every tensor of a chain's result against the float64 ``truth`` by the rule of the module docstring -> the failing tensors."""
    fails = []
    out_scale = float(truth["out"].abs().max()) if which != "distill" and truth["out"].numel() else 0.0
    for key, t64 in truth.items():
        t = t64.double().cpu().numpy()
        e = err(res[key].double().cpu().numpy(), t)
        b = bound(golden[f"{name}_{which}_{key}_e32"], t, out_scale if key.startswith("g_") else 0.0)
        report(f"{name} {which} {key}: error {e:.3e} (reference {float(golden[f'{name}_{which}_{key}_e32']):.3e}, bound {b:.3e})")
        if not e <= b:
            fails.append((key, e, b))
    return fails


def err(value, truth):
    return float(np.abs(np.asarray(value, dtype=np.float64) - np.asarray(truth, dtype=np.float64)).max()) if np.size(truth) else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# Model fixture: CAC-v1m1 over PT-v2m2 (ptv2_cases.CFG with num_classes = 0), K = 13, c = 24
# ---------------------------------------------------------------------------------------------------------------------------------------
MODEL_K, MODEL_C = 13, 24
# The parameters' draw.  Chosen by make_golden_cac.py's assertions alone, from the reference's own runs: the first seed from 33 on for which
# no row's confidence is near the threshold in train mode and the reference's fp32 gradients are at rounding level (< 1e-5) of its float64
# run.  On 33 and 37 they are at 1e-4 .. 6e-4: a near-tie in PT-v2m2's grid max pooling sends a cell's gradient to another point in fp32
# than in float64, and every implementation's rounding flips its own cells; 34 has a row near the threshold.
MODEL_SEED = 35
CRITERIA = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
# case -> (train, with labels, recipe settings)
MODEL_CASES = {"train_recipe": (True, True, True), "train_default": (True, True, False), "eval": (False, True, True),
               "test": (False, False, True)}
LOSS_TERMS = ("loss", "seg_loss", "pre_loss", "pre_self_loss", "kl_loss")
MODEL_GRADS = ["seg_head.weight", "proj.0.weight", "apd_proj.2.weight", "feat_proj_layer.0.weight", "feat_proj_layer.1.weight",
               "backbone.patch_embed.proj.0.weight", "backbone.enc_stages.1.down.fc.weight", "backbone.dec_stages.0.up.proj_skip.0.weight"]


def model_kwargs(recipe, conf_thresh):
    """Constructor arguments besides the backbone: the recipe's (configs/scannet/semseg-cac-v1m1-2-ptv2-lovasz.py: detach_pre_logits=True
    and a confidence threshold) or the constructor defaults."""
    kw = dict(num_classes=MODEL_K, backbone_out_channels=MODEL_C, criteria=CRITERIA)
    if recipe:
        kw.update(cos_temp=15, main_weight=1, pre_weight=1, pre_self_weight=1, kl_weight=1, conf_thresh=conf_thresh, detach_pre_logits=True)
    return kw


def run_model(model, b, train, labels):
    """One forward (+ backward in train mode) -> the returned dict, detached, and the parameter gradients."""
    model.train(train)
    dtype = next(model.parameters()).dtype
    data = dict(coord=b["coord"].to(dtype) if dtype == torch.float64 else b["coord"], feat=b["feat"].to(dtype), offset=b["offset"])
    if "offset_host" in b:
        data["offset_host"] = b["offset_host"]
    if labels:
        data["segment"] = b["segment"]
    model.zero_grad(set_to_none=True)
    if train:
        out = model(data)
        out["loss"].backward()
        grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
    else:
        with torch.no_grad():
            out = model(data)
        grads = {}
    return {k: v.detach() for k, v in out.items()}, grads

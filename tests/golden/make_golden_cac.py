#!/usr/bin/env python3
"""Generate tests/golden/ops_cac_ref.npz and model_cac_ref.npz by running the REFERENCE's own ``CACSegmentor``.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_cac.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py over stub ``pointcept.models.builder`` (``MODELS``
    registers nothing, ``build_model`` returns the module it is given) and ``pointcept.models.losses`` (``build_criteria`` sums the
    reference's own ``CrossEntropyLoss`` (losses/misc.py) and ``LovaszLoss`` (losses/lovasz.py), loaded as in make_golden_criteria.py /
    make_golden_lovasz.py);
  * for the model fixture, the reference's own PT-v2m2 through the loader of make_golden_ptv2.py.
The build container has no GPU: ``Tensor.cuda`` is a no-op while the reference runs.

ops_cac_ref.npz -- the four op chains of tests/cac_cases.py (one reference method each, its small MLPs stubbed out), every case in fp32
and in float64.  Stored per case and chain: the reference's fp32 results (rows thinned, cac_cases.thin) and, per tensor, the error of
that fp32 result against the reference's own float64 run (on all rows); the inputs are regenerated from seeds (cac_cases.inputs; their checksum is
stored).  A thresholded case takes its ``conf_thresh`` from cac_cases.pick_threshold (asserted there: no row is near the kink).

model_cac_ref.npz -- ``CACSegmentor`` over PT-v2m2 (ptv2_cases.CFG, num_classes=0) on ptv2_cases.batch(): train with the recipe's
settings, train with the constructor defaults, eval with labels, test.  Stored: the state-dict and returned keys, the loss terms, the
thinned refined logits, float64 gradients of cac_cases.MODEL_GRADS with the reference's own fp32 error, and the ``feat_proj_layer.1``
buffers after one training forward.  The parameters' draw (cac_cases.MODEL_SEED) is one on which the
reference's own fp32 gradients are at rounding level of its float64 run (asserted: see make_model)."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import cac_cases as cc  # noqa: E402
import make_golden as mg  # noqa: E402  (where the reference tree lives)
import make_golden_criteria as mgc  # noqa: E402
import make_golden_lovasz as mgl  # noqa: E402

REF = mg.REF
KINK_FREE = 1e-5   # the reference's own fp32-vs-float64 gradient error above which a draw sits on a max-pooling near-tie (make_model)


class _NoCuda:
    """``Tensor.cuda`` is the identity inside the block."""

    def __enter__(self):
        self._cuda = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self._cuda
        return False


class _StableSort:
    """``torch.sort`` is stable inside the block: PT-v2m2 sorts cluster ids (v2m2:263) and the Lovasz loss its errors, both without a
    defined order among equal elements (make_golden_ptv2.py does the same for the backbone alone)."""

    def __enter__(self):
        self._sort = torch.sort

        def sort(x, *a, **k):
            for key, v in zip(("dim", "descending"), a):
                k.setdefault(key, v)
            k.setdefault("stable", True)
            return self._sort(x, **k)

        torch.sort = sort

    def __exit__(self, *exc):
        torch.sort = self._sort
        return False


def load_reference():
    misc = mgc.load_reference()
    lovasz = mgl.load_reference()
    kinds = {"CrossEntropyLoss": misc.CrossEntropyLoss, "LovaszLoss": lovasz.LovaszLoss}

    def build_criteria(cfg):
        with _NoCuda():
            mods = [kinds[dict(c)["type"]](**{k: v for k, v in dict(c).items() if k != "type"}) for c in (cfg or [])]

        def criteria(pred, target):
            if not mods:
                return pred
            if pred.dtype != torch.float64:
                return sum(m(pred, target) for m in mods)
            # the float64 run: the reference's _lovasz_grad calls ``.float()`` on its counts, which would mix dtypes in its dot product
            as_float = torch.Tensor.float
            torch.Tensor.float = lambda self, *a, **k: self.double()
            try:
                return sum(m(pred, target) for m in mods)
            finally:
                torch.Tensor.float = as_float

        return criteria

    class _Registry:
        @staticmethod
        def register_module(*a, **k):
            return lambda cls: cls

    for name in ("pointcept", "pointcept.models"):
        if name not in sys.modules:   # (make_golden.install_reference, when it ran first, left the packages it needs)
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
    builder = types.ModuleType("pointcept.models.builder")
    builder.MODELS, builder.build_model = _Registry(), (lambda module: module)
    losses = types.ModuleType("pointcept.models.losses")
    losses.build_criteria = build_criteria
    sys.modules["pointcept.models.builder"], sys.modules["pointcept.models.losses"] = builder, losses
    spec = importlib.util.spec_from_file_location(
        "ref_cac", os.path.join(REF, "pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_cac"] = mod
    spec.loader.exec_module(mod)
    return mod


class _FirstColumns(nn.Module):
    """Stand-in of ``proj`` / ``apd_proj`` in the op chains: cat[prototypes, W] -> the prototypes; remembers them."""

    def __init__(self, c):
        super().__init__()
        self.c, self.seen = c, []

    def forward(self, z):
        self.seen.append(z[:, :self.c].detach())
        return z[:, :self.c]


def reference_chains(ref, name, dtype, thr):
    """The four chains of a case through the reference's own methods -> {chain: {tensor: numpy}}."""
    sizes, k, c, _, _, _, detach, _, _ = cc.CASES[name]
    inp = cc.inputs(name)
    f = lambda key: inp[key].to(dtype).clone()
    head = ref.CACSegmentor(num_classes=k, backbone_out_channels=c, backbone=nn.Identity(), criteria=None, conf_thresh=thr,
                            detach_pre_logits=detach)
    head.proj, head.apd_proj, head.feat_proj_layer = _FirstColumns(c), _FirstColumns(c), nn.Identity()
    gout, target = f("gout"), inp["target"]
    out = {}
    with _NoCuda():
        feat, logits = f("feat").requires_grad_(), f("logits").requires_grad_()
        y = head.post_refine_proto_batch(feat=feat, pred=logits, proto=f("base"), offset=inp["offset"])
        (y * gout).sum().backward()
        out["refine"] = dict(out=y, proto=torch.stack(head.proj.seen), g_feat=feat.grad)
        if not detach:
            out["refine"]["g_logits"] = logits.grad
        feat, base = f("feat").requires_grad_(), f("base").requires_grad_()
        y = head.get_adaptive_perspective(feat=feat, target=target, new_proto=base, proto=f("base"))
        (y * gout).sum().backward()
        out["adaptive"] = dict(out=y, g_feat=feat.grad, g_base=base.grad if base.grad is not None else torch.zeros_like(base))
        feat, base = f("feat").requires_grad_(), f("base").requires_grad_()
        y = ref.CACSegmentor.get_pred(feat, base)
        (y * gout).sum().backward()
        out["pred"] = dict(out=y, g_feat=feat.grad, g_base=base.grad)
        logits = f("logits").requires_grad_()
        y = ref.CACSegmentor.get_distill_loss(pred=logits, soft=f("soft"), target=target)
        if y.requires_grad:
            y.backward()
        out["distill"] = dict(out=y, g_logits=logits.grad if logits.grad is not None else torch.zeros_like(logits))
    return {ch: {key: v.detach().numpy() for key, v in d.items()} for ch, d in out.items()}


def make_ops(ref):
    out = {"cases": np.array(list(cc.CASES))}
    for name, (sizes, k, c, _, _, thresholded, _, _, _) in cc.CASES.items():
        inp = cc.inputs(name)
        thr = 0.0
        if thresholded:
            maxima = [torch.softmax(inp["logits"].to(d), 1).max(1)[0].numpy() for d in (torch.float32, torch.float64)]
            thr = cc.pick_threshold(*maxima)
        r32, r64 = (reference_chains(ref, name, d, thr) for d in (torch.float32, torch.float64))
        out[f"{name}_thr"], out[f"{name}_checksum"] = np.float32(thr), cc.checksum(inp)
        for ch in cc.CHAINS:
            for key, v in r32[ch].items():
                out[f"{name}_{ch}_{key}"] = cc.thin(v)
                out[f"{name}_{ch}_{key}_e32"] = np.array(cc.err(v, r64[ch][key]))
            print(name, ch, {key: f"{float(out[f'{name}_{ch}_{key}_e32']):.2e}/{float(np.abs(r64[ch][key]).max()) if r64[ch][key].size else 0:.2e}"
                             for key in r32[ch]}, "thr", thr)
    path = os.path.join(HERE, "ops_cac_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


def make_model(ref, ptv2):
    import ptv2_cases as pc
    from pointcloudpdf_amd import synthetic

    b = pc.batch()

    def build(recipe, thr, dtype):
        backbone = ptv2.PointTransformerV2(unpool_backend="map", pe_multiplier=False, drop_path_rate=0.0, **dict(pc.CFG, num_classes=0))
        kw = cc.model_kwargs(recipe, thr)
        model = ref.CACSegmentor(backbone=backbone, **kw)
        synthetic.fill_parameters_deterministic(model, seed=cc.MODEL_SEED)
        return model.to(dtype)

    # the recipe's threshold, by the rule of the op fixture, from the pre-logits of the model itself (eval mode)
    maxima = []
    with _NoCuda(), _StableSort():
        for dtype in (torch.float32, torch.float64):
            model = build(True, 0.0, dtype).eval()
            with torch.no_grad():
                bb = dict(coord=b["coord"].to(dtype), feat=b["feat"].to(dtype), offset=b["offset"])
                maxima.append(torch.softmax(model.seg_head(model.backbone(bb)), 1).max(1)[0].numpy())
    try:
        thr = cc.pick_threshold(*maxima)
    except AssertionError as e:   # no gap wide enough at model level: the thresholded cases stay at op level
        print("model fixture: no admissible threshold", e, "-> conf_thresh = 0")
        thr = 0.0
    # (train mode moves the pre-logits through the batch statistics: the rule is checked again on the train-mode maxima below)
    out = {"conf_thresh": np.float32(thr)}
    for case, (train, labels, recipe) in cc.MODEL_CASES.items():
        res = {}
        for dtype in (torch.float32, torch.float64):
            with _NoCuda(), _StableSort():
                model = build(recipe, thr, dtype)
                seen = []
                hook = model.seg_head.register_forward_hook(lambda m, i, o: seen.append(torch.softmax(o.detach(), 1).max(1)[0].numpy()))
                res[dtype] = cc.run_model(model, b, train, labels) + (model, seen[0])
                hook.remove()
        (o32, g32, m32, mx32), (o64, g64, _, mx64) = res[torch.float32], res[torch.float64]
        if recipe and thr > 0:
            side = lambda m: np.asarray(m) >= thr
            margin = float(np.abs(np.asarray(mx64, dtype=np.float64) - thr).min())
            assert np.array_equal(side(mx32), side(mx64)) and margin >= 100.0 * float(np.abs(mx32.astype(np.float64) - mx64).max()), \
                (case, margin, "a row is near the threshold in this mode: pick conf_thresh = 0 for the model fixture")
        out[f"{case}_keys"] = np.array(sorted(o32.keys()))
        for key in o32:
            a, t = o32[key].numpy(), o64[key].numpy()
            out[f"{case}_{key}"] = cc.thin(a)
            out[f"{case}_{key}_e32"] = np.array(cc.err(a, t) / max(float(np.abs(t).max()), 1e-300))
            print(case, key, "fp32 vs fp64 (max-rel)", f"{float(out[f'{case}_{key}_e32']):.2e}")
        if train:
            for gname in cc.MODEL_GRADS:
                t64 = pc.part(g64[gname])
                scale = float(np.abs(g64[gname]).max())
                out[f"{case}_g64_{gname}"], out[f"{case}_scale_{gname}"] = t64, np.array(scale)
                out[f"{case}_e32_{gname}"] = np.array(np.abs(pc.part(g32[gname]).astype(np.float64) - t64).max() / scale)
                print(f"   {gname}: scale {scale:.3e} reference fp32 error {float(out[f'{case}_e32_{gname}']):.3e}")
                # Kink-free draw: PT-v2m2's grid MAX pooling routes a cell's gradient to its arg max, and a near-tie between two points
                # of a cell is resolved differently by any two roundings of the same network (fp32 against float64 here) -- a discrete
                # change of every gradient upstream of the pooling, 1e-4 of its scale per flipped cell, where rounding alone leaves
                # 1e-6.  A draw on which the reference's own fp32 run is at rounding level took the float64 run's branches everywhere;
                # only such a draw can be compared by "2 x the reference's own error" (cac_cases.MODEL_SEED is chosen by this assertion)
                assert float(out[f"{case}_e32_{gname}"]) < KINK_FREE, (case, gname, "pick another cac_cases.MODEL_SEED (--seed N to try one)")
            for bname, v in m32.feat_proj_layer[1].state_dict().items():
                out[f"{case}_buffer_{bname}"] = v.numpy()
        if case == "train_recipe":
            out["state_dict_keys"] = np.array(list(m32.state_dict().keys()))
    path = os.path.join(HERE, "model_cac_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if "--seed" in sys.argv:
        cc.MODEL_SEED = int(sys.argv[sys.argv.index("--seed") + 1])
    ptv2 = None
    if "--ops-only" not in sys.argv:   # (first: its loader installs the reference's own packages, the stubs below then replace two of them)
        import make_golden_ptv2

        ptv2 = make_golden_ptv2.load_reference()
    ref = load_reference()
    if "--model-only" not in sys.argv:
        make_ops(ref)
    if ptv2 is not None:
        make_model(ref, ptv2)

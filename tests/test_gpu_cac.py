"""GPU suite: the context-aware classifier head as HIP passes (csrc/cac.hip through pointcloudpdf_amd/cac.py) against the fixtures of the
reference's own ``CACSegmentor`` (tests/golden/ops_cac_ref.npz, model_cac_ref.npz) -- every op chain of tests/cac_cases.py forward and
backward by its tolerance rule, bit-reproducibility, the conventions for bad / ignored labels, capture into a hipGraph without memset
nodes, the model over PT-v2m2, scene independence and a short training run."""
import numpy as np
import pytest
import torch

import cac_cases as cc
import ptv2_cases as pc
from helpers import REL_TOL, max_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return cc.load("ops")


@pytest.fixture(scope="module")
def model_golden():
    return cc.load("model")


@pytest.fixture(scope="module")
def truths(golden):
    """The float64 evaluation of every chain on the device, computed once (test_cac_cpu.py pins it to the reference)."""
    out = {}
    for name in cc.CASES:
        inp, thr = cc.inputs(name), float(golden[f"{name}_thr"])
        for which in cc.CHAINS:
            out[name, which] = cc.chain(name, which, cc.torch_ops(), inp, thr, dtype=torch.float64, device=DEV)
    return out


def _cfg(recipe, thr):
    return dict(type="CAC-v1m1", backbone=dict(type="PT-v2m2", unpool_backend="map", pe_multiplier=False, drop_path_rate=0.0,
                                               **dict(pc.CFG, num_classes=0)), **cc.model_kwargs(recipe, thr))


def _build(recipe, thr):
    from pointcloudpdf_amd import cac, point_transformer_v2, synthetic  # noqa: F401  (register the classes)
    from pointcloudpdf_amd.registry import MODELS

    model = MODELS.build(_cfg(recipe, thr))
    synthetic.fill_parameters_deterministic(model, seed=cc.MODEL_SEED)
    return model.to(DEV)


def test_fused_class_and_node_types():
    from pointcloudpdf_amd import _native, cac

    be = _native.hip_backend()
    for k, c in [(20, 48), (13, 48), (13, 24), (200, 48), (2, 32)]:
        assert be.cac_supported(k, c)
    assert not be.cac_supported(65, 96)
    inp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cc.inputs("n63_k20_c48_thr_detach").items()}
    feat, logits = inp["feat"].requires_grad_(), inp["logits"].requires_grad_()
    proto = cac.soft_prototypes(feat, logits, inp["offset"], 0.4)
    assert type(proto.grad_fn).__name__ == "_SoftPrototypesBackward"
    assert type(cac.class_prototypes(feat, inp["target"], inp["base"]).grad_fn).__name__ == "_ClassPrototypesBackward"
    assert type(cac.cosine_logits(feat, proto, inp["offset"]).grad_fn).__name__ == "_CosineLogitsBackward"
    assert type(cac.distill_loss(logits, inp["soft"], inp["target"]).grad_fn).__name__ == "_DistillLossBackward"
    wide = torch.randn(8, 96, device=DEV, requires_grad=True)
    assert "CosineLogits" not in type(cac.cosine_logits(wide, torch.randn(65, 96, device=DEV)).grad_fn).__name__   # the composition


@pytest.mark.parametrize("which", cc.CHAINS)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_ops_match_the_reference(golden, truths, name, which):
    """Forward and every input gradient of every case (the fused kernels for the cases of the fused class, the composition on the
    device for (65, 96)) by the rule of cac_cases: at most 2x the reference's own fp32 error, floor in fp32 ulps."""
    inp, thr = cc.inputs(name), float(golden[f"{name}_thr"])
    ours = cc.chain(name, which, cc.fused_ops(), inp, thr, device=DEV)
    fails = cc.check_chain(name, which, ours, truths[name, which], golden)
    assert not fails, (name, which, fails)


@pytest.mark.parametrize("name", ["scenes_k13_c24_thr", "scenes_k200_c48_thr_detach", "n257_k13_c48_thr"])
def test_ops_are_bit_reproducible(golden, name):
    inp, thr = cc.inputs(name), float(golden[f"{name}_thr"])
    for which in cc.CHAINS:
        runs = [cc.chain(name, which, cc.fused_ops(), inp, thr, device=DEV) for _ in range(3)]
        for other in runs[1:]:
            for key, v in runs[0].items():
                assert torch.equal(v, other[key]), (name, which, key)


def test_label_conventions():
    from pointcloudpdf_amd import cac

    inp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cc.inputs("n257_k13_c24_zero_row").items()}
    pred, target = inp["logits"].clone().requires_grad_(), inp["target"]
    loss = cac.distill_loss(pred, inp["soft"], torch.full_like(target, -1))
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(pred.grad.abs().max()) == 0.0
    bad = target.clone()
    bad[5] = 13
    assert bool(torch.isnan(cac.distill_loss(pred, inp["soft"], bad)))
    proto = cac.class_prototypes(inp["feat"], target, inp["base"])
    assert torch.equal(proto[5], inp["base"][5]) and not torch.equal(proto[4], inp["base"][4])   # class 5 is absent from the labels
    assert torch.equal(cac.class_prototypes(inp["feat"], torch.full_like(target, -1), inp["base"]), inp["base"])


def _head(model, feat, target, data):
    """The head as ``CACSegmentor.forward`` chains it in train mode, without backbone and criteria."""
    from pointcloudpdf_amd import cac

    logits = model.seg_head(feat)
    refine = model.refine(feat, logits, data)
    pred = model.adaptive_perspective(feat, target)
    return refine, pred, cac.distill_loss(refine, pred.detach(), target)


def test_head_captures_without_memset_nodes(golden):
    """The head on static feature, label and offset tensors in one ``torch.cuda.graph``: three replays, other device work in between,
    equal the eager result bit for bit; the graph holds no memset node."""
    from pointcloudpdf_amd import engine

    name = "scenes_k13_c24_thr"
    inp = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in cc.inputs(name).items()}
    model = _build(True, float(golden[f"{name}_thr"])).train()
    data = dict(offset=inp["offset"], offset_host=inp["offset_host"])
    feat, target = inp["feat"], inp["target"]

    def run():
        model.zero_grad(set_to_none=True)
        x = feat.detach().clone().requires_grad_()
        refine, pred, kl = _head(model, x, target, data)
        (refine.square().mean() + pred.square().mean() + kl).backward()
        return [refine.detach(), pred.detach(), kl.detach(), x.grad, model.seg_head.weight.grad, model.proj[0].weight.grad]

    buffers = {k: v.clone() for k, v in model.feat_proj_layer[1].state_dict().items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # (eager on the capture's stream: the parameters' gradient nodes are bound to the stream of their first use)
        eager = [t.clone() for t in run()]
    s.synchronize()
    model.feat_proj_layer[1].load_state_dict(buffers)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=s):
        static = run()
    census = engine.graph_node_census(g.raw_cuda_graph())
    assert census["kernel"] > 20 and census["memset"] == 0, census
    for _ in range(3):
        model.feat_proj_layer[1].load_state_dict(buffers)
        for t in static:
            t.fill_(float("nan"))
        torch.randn(1 << 16, device=DEV).sum()   # (other device work between the replays)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, static):
            assert torch.equal(a, b)


@pytest.mark.parametrize("case", list(cc.MODEL_CASES))
def test_model_matches_the_reference_class(model_golden, case):
    """Logits and losses within REL_TOL, gradients by the rule of tests/ptv2_cases.py: max(2 x the reference's own fp32 error, REL_TOL).
    Measured on the MI355X (draw cac_cases.MODEL_SEED, chosen from the reference's own runs to be free of max-pooling near-ties): logits and
    loss terms 6e-08 .. 6e-07; the head's five tensors 4e-07 .. 4e-06 (reference 3e-07 .. 8e-07); the three backbone tensors 3.8e-05 ..
    8.9e-05 (reference 8e-07 .. 3e-06) -- inside REL_TOL, and unchanged when the head runs as its torch compositions."""
    g = model_golden
    train, labels, recipe = cc.MODEL_CASES[case]
    model = _build(recipe, float(g["conf_thresh"]))
    out, grads = cc.run_model(model, pc.batch(DEV), train, labels)
    assert sorted(out.keys()) == list(g[f"{case}_keys"])
    fails = []
    for key, v in out.items():
        e = max_rel(cc.thin(v.cpu().numpy()), g[f"{case}_{key}"])
        print(case, key, f"{e:.3e}")
        if not e <= REL_TOL:
            fails.append((key, e))
    if train:
        for name in cc.MODEL_GRADS:
            scale, ref_err = float(g[f"{case}_scale_{name}"]), float(g[f"{case}_e32_{name}"])
            e = float(np.abs(pc.part(grads[name]).astype(np.float64) - g[f"{case}_g64_{name}"]).max() / scale)
            print(f"  {name}: error {e:.3e} (reference {ref_err:.3e}, bound {max(2.0 * ref_err, REL_TOL):.3e})")
            if not e <= max(2.0 * ref_err, REL_TOL):
                fails.append((name, e, ref_err))
        state = model.feat_proj_layer[1].state_dict()
        assert int(state["num_batches_tracked"]) == len(pc.SIZES) + 1
        for bname in ("running_mean", "running_var"):
            assert max_rel(state[bname].cpu().numpy(), g[f"{case}_buffer_{bname}"]) <= REL_TOL, bname
    assert not fails, (case, fails)


def test_eval_forward_is_scene_independent(model_golden):
    from pointcloudpdf_amd import synthetic

    model = _build(True, float(model_golden["conf_thresh"])).eval()
    b = pc.batch(DEV)
    with torch.no_grad():
        both = model(dict(coord=b["coord"], feat=b["feat"], offset=b["offset"], offset_host=b["offset_host"]))["seg_logits"]
        start = 0
        for i, size in enumerate(pc.SIZES):
            one = synthetic.make_batch([size], first_scene_id=pc.FIRST_SCENE + i, grid_size=pc.GRID, device=DEV)
            assert torch.equal(one["coord"], b["coord"][start:start + size])
            alone = model(dict(coord=one["coord"], feat=one["feat"], offset=one["offset"], offset_host=one["offset_host"]))["seg_logits"]
            e = max_rel(alone.cpu().numpy(), both[start:start + size].cpu().numpy())
            print("scene", i, "alone vs in the batch:", f"{e:.3e}", "bit-identical" if torch.equal(alone, both[start:start + size]) else "")
            assert e <= REL_TOL
            start += size


def test_training_runs_and_is_bit_reproducible(model_golden):
    from pointcloudpdf_amd import engine, optim, synthetic

    b = pc.batch(DEV)

    def three_steps():
        step = engine.build_seg_step(dict(model=_cfg(True, float(model_golden["conf_thresh"]))))
        synthetic.fill_parameters_deterministic(step.model, seed=cc.MODEL_SEED)
        step.to(DEV).train()
        train = engine.TrainStep(step, optim.FusedAdamW(step.parameters(), lr=1e-3, weight_decay=0.02), graph=False)
        outs = [train(b) for _ in range(3)]
        return [torch.stack([o[k].detach() for k in cc.LOSS_TERMS]) for o in outs]

    first, second = three_steps(), three_steps()
    for a, c in zip(first, second):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, c), (a, c)
    assert not torch.equal(first[0], first[2])

"""CPU suite: the context-aware classifier (CAC-v1m1) -- the torch compositions of pointcloudpdf_amd/cac.py and ``CACSegmentor`` on the CPU
oracle against the fixtures produced by the reference's OWN class (tests/golden/ops_cac_ref.npz, model_cac_ref.npz, written by
tests/golden/make_golden_cac.py), and the ``semseg`` step builder."""
import numpy as np
import pytest
import torch

import cac_cases as cc
import ptv2_cases as pc
from helpers import REL_TOL, max_rel


@pytest.fixture(scope="module")
def golden():
    return cc.load("ops")


@pytest.fixture(scope="module")
def model_golden():
    return cc.load("model")


def _model_cfg(recipe, thr):
    kw = cc.model_kwargs(recipe, thr)
    return dict(type="CAC-v1m1", backbone=dict(type="PT-v2m2", unpool_backend="map", pe_multiplier=False, drop_path_rate=0.0,
                                               **dict(pc.CFG, num_classes=0)), **kw)


def _build(recipe, thr, dtype=torch.float32):
    from pointcloudpdf_amd import cac, point_transformer_v2, synthetic  # noqa: F401  (register the classes)
    from pointcloudpdf_amd.registry import MODELS

    model = MODELS.build(_model_cfg(recipe, thr))
    synthetic.fill_parameters_deterministic(model, seed=cc.MODEL_SEED)
    return model.to(dtype)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_inputs_are_the_fixture_inputs(golden, name):
    assert np.array_equal(cc.checksum(cc.inputs(name)), golden[f"{name}_checksum"])


@pytest.mark.parametrize("which", cc.CHAINS)
@pytest.mark.parametrize("name", list(cc.CASES))
def test_compositions_match_the_reference_methods(golden, name, which):
    """The fp32 composition by the rule of cac_cases, and the float64 composition -- the truth of the GPU tests -- pinned to the
    reference's fp32 result the same way (the reference's own error against ITS float64 run is the bound's first term)."""
    inp, thr = cc.inputs(name), float(golden[f"{name}_thr"])
    truth = cc.chain(name, which, cc.torch_ops(), inp, thr, dtype=torch.float64)
    ours = cc.chain(name, which, cc.torch_ops(), inp, thr)
    assert set(truth) == {k[len(name) + len(which) + 2:] for k in golden.files if k.startswith(f"{name}_{which}_") and not k.endswith("_e32")}
    assert not cc.check_chain(name, which, ours, truth, golden)
    thinned = {k: torch.from_numpy(cc.thin(v.cpu().numpy())) for k, v in truth.items()}
    stored = {k: torch.from_numpy(np.asarray(golden[f"{name}_{which}_{k}"])) for k in truth}
    assert not cc.check_chain(name, which, stored, thinned, golden)


def test_compositions_without_host_offsets_agree(golden):
    """The scene sums as one-hot products (no ``offset_host``) against the sliced form."""
    from pointcloudpdf_amd import cac

    name = "scenes_k13_c24_thr"
    inp, thr = cc.inputs(name), float(golden[f"{name}_thr"])
    a = cac.soft_prototypes_torch(inp["feat"], inp["logits"], inp["offset"], thr, inp["offset_host"])
    b = cac.soft_prototypes_torch(inp["feat"], inp["logits"], inp["offset"], thr)
    assert max_rel(b.numpy(), a.numpy()) < 1e-5
    ya = cac.cosine_logits_torch(inp["feat"], a, inp["offset"], 15.0, inp["offset_host"])
    yb = cac.cosine_logits_torch(inp["feat"], a, inp["offset"], 15.0)
    assert max_rel(yb.numpy(), ya.numpy()) < 1e-5


def test_distill_loss_conventions():
    from pointcloudpdf_amd import cac

    g = torch.Generator().manual_seed(3)
    pred, soft = torch.randn(9, 5, generator=g, requires_grad=True), torch.randn(9, 5, generator=g)
    target = torch.tensor([0, 1, 1, -1, 4, 4, 4, -1, 0])
    loss = cac.distill_loss(pred, soft, torch.full_like(target, -1))
    loss.backward()
    assert float(loss) == 0.0 and float(pred.grad.abs().max()) == 0.0
    bad = target.clone()
    bad[2] = 7
    assert torch.isnan(cac.distill_loss(pred, soft, bad))
    assert float(cac.distill_loss(pred, soft, target, eps=0.1)) != float(cac.distill_loss(pred, soft, target))
    base = torch.randn(5, 6, generator=g)
    proto = cac.class_prototypes(torch.randn(9, 6, generator=g), target, base)
    assert torch.equal(proto[[2, 3]], base[[2, 3]]) and not torch.equal(proto[0], base[0])


def test_state_dict_keys_are_the_reference_keys(model_golden):
    assert list(_build(True, 0.1).state_dict().keys()) == list(model_golden["state_dict_keys"])


@pytest.mark.parametrize("case", list(cc.MODEL_CASES))
def test_model_matches_the_reference_class(use_oracle, model_golden, case):
    g = model_golden
    train, labels, recipe = cc.MODEL_CASES[case]
    model = _build(recipe, float(g["conf_thresh"]))
    out, grads = cc.run_model(model, pc.batch(), train, labels)
    assert sorted(out.keys()) == list(g[f"{case}_keys"])
    for key, v in out.items():
        e = max_rel(cc.thin(v.numpy()), g[f"{case}_{key}"])
        print(case, key, f"{e:.3e}")
        assert e <= REL_TOL, (case, key, e)
    if train:
        for name in cc.MODEL_GRADS:
            scale, ref_err = float(g[f"{case}_scale_{name}"]), float(g[f"{case}_e32_{name}"])
            e = float(np.abs(pc.part(grads[name]).astype(np.float64) - g[f"{case}_g64_{name}"]).max() / scale)
            print(f"  {name}: error {e:.3e} (reference {ref_err:.3e})")
            assert e <= max(2.0 * ref_err, REL_TOL), (case, name, e, ref_err)
        # B + 1 BatchNorm updates, scenes in order, then the batch
        state = model.feat_proj_layer[1].state_dict()
        assert int(state["num_batches_tracked"]) == int(g[f"{case}_buffer_num_batches_tracked"]) == len(pc.SIZES) + 1
        for bname in ("running_mean", "running_var"):
            assert max_rel(state[bname].numpy(), g[f"{case}_buffer_{bname}"]) <= REL_TOL, bname


def test_one_row_scene_raises_in_train_mode(use_oracle):
    model = _build(True, 0.0).train()
    feat = torch.randn(5, cc.MODEL_C)
    data = dict(offset=torch.tensor([4, 5], dtype=torch.int32), offset_host=[4, 5])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model.refine(feat, model.seg_head(feat), data)
    model.eval()
    assert model.refine(feat, model.seg_head(feat), data).shape == (5, cc.MODEL_K)


def test_seg_step_builder(use_oracle, model_golden):
    from pointcloudpdf_amd import engine, optim

    b = pc.batch()
    step = engine.build_seg_step(dict(model=_model_cfg(True, float(model_golden["conf_thresh"]))))
    assert type(step.model).__name__ == "CACSegmentor"
    out = step.train()(b)
    assert sorted(out) == sorted(cc.LOSS_TERMS) and out["loss"].requires_grad and not out["kl_loss"].requires_grad
    assert sorted(step.eval()(b)) == ["loss", "seg_logits"]
    opt = optim.build_optimizer(dict(type="AdamW", lr=0.001, weight_decay=0.02), step)
    assert sum(len(gr["params"]) for gr in opt.param_groups) == len(list(step.parameters()))
    plain = engine.build_seg_step(dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PT-v2m2", **pc.CFG),
                                                  criteria=cc.CRITERIA)))
    out = plain.train()(b)
    assert list(out) == ["loss"] and out["loss"].requires_grad
    with pytest.raises(KeyError):
        engine.build_seg_step(dict(recognizer=dict(type="MaxProbability")))


def test_open_seg_step_refuses_cac(model_golden):
    from pointcloudpdf_amd import engine

    cfg = dict(model=_model_cfg(True, 0.1), recognizer=dict(type="MaxProbability", method="msp"))
    with pytest.raises(NotImplementedError, match="CAC-v1m1"):
        engine.build_open_seg_step(cfg)


def test_cac_entries_validate_before_any_launch():
    import ctypes

    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    lib.pdf_cac_workspace_floats.restype = ctypes.c_long
    lib.pdf_cac_workspace_floats.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    for k, c in [(20, 48), (13, 48), (13, 24), (200, 48), (2, 32)]:
        assert lib.pdf_cac_supported(k, c) == 1, (k, c)
    for k, c in [(65, 96), (13, 22), (300, 48), (0, 48)]:
        assert lib.pdf_cac_supported(k, c) == 0, (k, c)
    assert lib.pdf_cac_workspace_floats(2207, 13, 24, 3) == 2 * 3 * 13 * 28 and lib.pdf_cac_workspace_floats(10, 65, 96, 1) == 0
    L, I, P, F = ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)
    f = lib.pdf_cac_soft_proto_forward
    f.restype, f.argtypes = I, [L, I, I, I, P, P, P, F, P, P, P, P]
    assert f(10, 65, 96, 1, p, p, p, 0.0, p, p, p, None) == -1 and f(0, 13, 24, 1, p, p, p, 0.0, p, p, p, None) == -1
    assert f(10, 13, 24, 1, p, None, p, 0.0, p, p, p, None) == -1
    d = lib.pdf_cac_distill_forward
    d.restype, d.argtypes = I, [L, I, P, P, P, F, P, P, P, P, P]
    assert d(10, 300, p, p, p, 0.5, p, p, p, p, None) == -1 and d(10, 13, p, p, None, 0.5, p, p, p, p, None) == -1

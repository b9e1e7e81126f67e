"""CPU suite of the sparse convolutions and SpUNet-v1m1: the composition path's tables against a brute force, the three operators and
their gradients against the dense float64 oracle (tests/spunet_cases.py), the model against the fixture of the reference's own class
(tests/golden/make_golden_spunet.py) and the three recipes' steps."""
import os

import numpy as np
import pytest
import torch

import spunet_cases as sc
from pointcloudpdf_amd import sparse_conv as spconv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_spunet_ref.npz")
SETS = sc.site_sets()


@pytest.mark.parametrize("name", list(SETS))
def test_tables_equal_the_brute_force(name):
    indices, shape = SETS[name]
    geo = spconv.SpGeometry.build(indices, 2, [(3, 5), (3,)], shape)
    for ks in (3, 5):
        assert torch.equal(geo.subm(0, ks), sc.subm_table_brute(indices, ks)), f"{name}: k = {ks}"
    parent, code, coarse, children = sc.down_brute(indices, shape)
    st = geo.steps[0]
    assert torch.equal(st.parent, parent) and torch.equal(st.code, code) and torch.equal(st.children, children)
    assert torch.equal(geo.levels[1]["indices"], coarse)                      # ascending (batch, d0, d1, d2)
    assert torch.equal(geo.subm(1, 3), sc.subm_table_brute(coarse, 3))
    assert geo.has_duplicates == (name == "dups")


@pytest.mark.parametrize("name", [n for n in SETS if n != "dups"])
def test_mirror_identity(name):
    """nbr[i, k] = j  <=>  nbr[j, K - 1 - k] = i (what the HIP input gradient relies on); it holds wherever no site is duplicated."""
    indices, _ = SETS[name]
    for ks in (3, 5):
        tbl = sc.subm_table_brute(indices, ks).long()
        K = ks ** 3
        i, k = torch.nonzero(tbl >= 0, as_tuple=True)
        assert torch.equal(tbl[tbl[i, k], K - 1 - k], i)


def test_bad_coordinates_raise():
    for bad in ([[0, -1, 0, 0]], [[0, 0, 1 << 16, 0]], [[1 << 15, 0, 0, 0]]):
        with pytest.raises(RuntimeError):
            spconv.SpGeometry.build(torch.tensor([[0, 1, 1, 1]] + bad, dtype=torch.int32), 1, [(3,)])


def _run(kind, indices, shape, case, dtype):
    geo = spconv.SpGeometry.build(indices, 2, [(), ()], shape)
    x, w = case["x"].to(dtype).requires_grad_(), case["w"].to(dtype).requires_grad_()
    b = None if case["b"] is None else case["b"].to(dtype).requires_grad_()
    fn = dict(subm=spconv.subm_conv, down=spconv.down_conv, inverse=spconv.inverse_conv)[kind]
    out = fn(x, w, b, geo, 0)
    grads = torch.autograd.grad(out, [x, w] + ([b] if b is not None else []), case["g"].to(dtype))
    return out, grads


@pytest.mark.parametrize("kind", ["subm", "down", "inverse"])
@pytest.mark.parametrize("name", ["one", "n65", "dense500", "twin", "origin", "dups", "odd_trunc"])
def test_operators_match_the_dense_oracle(kind, name):
    indices, shape = SETS[name]
    for cin, cout, ks in [(32, 32, 3), (6, 32, 5), (24, 40, 3)]:
        if kind != "subm" and ks == 5:
            continue
        case = sc.oracle(kind, indices, shape, cin, cout, ks, seed=11)
        out, grads = _run(kind, indices, shape, case, torch.float64)   # float64: the definitions agree to rounding of float64
        for got, want in [(out, case["out"]), (grads[0], case["gx"]), (grads[1], case["gw"]), (grads[2], case["gb"])]:
            assert got.shape == want.shape and float((got.detach() - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        out, grads = _run(kind, indices, shape, case, torch.float32)   # fp32 composition inside the a-priori bound
        tag = f"{kind}/{name}/{cin}->{cout}"
        sc.check(tag + " out", out, case["out"], case["tol_out"])
        sc.check(tag + " gx", grads[0], case["gx"], case["tol_gx"])
        sc.check(tag + " gw", grads[1], case["gw"], case["tol_gw"])
        sc.check(tag + " gb", grads[2], case["gb"], case["tol_gb"])


def test_inverse_needs_its_key():
    indices, _ = SETS["n65"]
    x = spconv.SparseConvTensor(torch.zeros(65, 32), indices)
    with pytest.raises(KeyError):
        spconv.SparseInverseConv3d(32, 32, 2, indice_key="nope")(x)
    down = spconv.SparseConv3d(32, 64, 2, stride=2, bias=False, indice_key="a")
    up = spconv.SparseInverseConv3d(64, 32, 2, bias=False, indice_key="a")
    assert down.weight.shape == (64, 2, 2, 2, 32) and up.weight.shape == (32, 2, 2, 2, 64)
    y = up(down(x))
    assert y.features.shape == (65, 32) and torch.equal(y.indices, indices) and y.level == 0


def test_entries_validate_before_any_launch():
    """The supported-shape probe and the argument checks of the new entries need no GPU."""
    import ctypes

    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    assert [lib.pdf_spconv_supported(*a) for a in [(3, 32, 32), (3, 384, 256), (3, 256, 384), (2, 96, 96), (5, 6, 32), (5, 9, 32),
                                                    (3, 24, 40), (3, 416, 32), (5, 32, 32), (7, 6, 32)]] == [1, 1, 1, 1, 2, 2, 0, 0, 0, 0]
    L, I, P = ctypes.c_long, ctypes.c_int, ctypes.c_void_p
    lib.pdf_spconv_gather.argtypes = [L, L, L, I, I, I, P, P, I, P, P, P, L, L, L, P, P, P]
    lib.pdf_spconv_wgrad.argtypes = [L, L, I, I, I, P, P, P, I, P, P, P]
    lib.pdf_spconv_sort_sites.argtypes = [L, P, P, P, P, P, P]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)
    assert lib.pdf_spconv_gather(0, 0, 4, 32, 32, 27, p, p, 0, None, None, p, 1, 32, 864, None, p, None) == 0      # no rows: nothing to do
    assert lib.pdf_spconv_gather(4, 4, 4, 32, 32, 27, None, p, 0, None, None, p, 1, 32, 864, None, p, None) == -1
    assert lib.pdf_spconv_gather(4, 4, 4, 32, 32, 28, p, p, 0, None, None, p, 1, 32, 896, None, p, None) == -1     # K > 27
    assert lib.pdf_spconv_gather(4, 4, 4, 24, 40, 27, p, p, 0, None, None, p, 1, 24, 648, None, p, None) == -3     # outside the class
    assert lib.pdf_spconv_wgrad(4, 4, 27, 32, 40, p, p, p, 0, p, p, None) == -3
    assert lib.pdf_spconv_wgrad(4, 4, 27, 32, 32, p, p, None, 0, p, p, None) == -1
    assert lib.pdf_spconv_sort_sites(0, p, p, p, p, p, None) == -1


# ---------------------------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def build_model(dtype=torch.float32):
    from pointcloudpdf_amd import sparse_unet  # noqa: F401
    from pointcloudpdf_amd.registry import MODELS

    return MODELS.build(dict(type="SpUNet-v1m1", **sc.MODEL_KW)).to(dtype)


def test_registry_and_state_dict_keys(golden):
    model = build_model()
    sd = model.state_dict()
    keys = [str(k) for k in golden["keys"]]
    assert list(sd.keys()) == keys
    assert [list(sd[k].shape) for k in keys] == [[int(v) for v in s if v >= 0] for s in golden["shapes"]]
    for k in ("conv_input.0.weight", "down.0.0.weight", "enc.0.block0.conv1.weight", "up.0.0.weight", "dec.3.block0.proj.0.weight",
              "final.weight"):
        assert k in sd


def load_inputs(golden, device="cpu", dtype=torch.float32):
    return dict(grid_coord=torch.from_numpy(golden["grid_coord"]).to(device), feat=torch.from_numpy(golden["feat"]).to(device, dtype),
                offset=torch.from_numpy(golden["offset"]).to(device), segment=torch.from_numpy(golden["segment"]).to(device))


def model_against_fixture(golden, device, dtype=torch.float32):
    """Logits (train and eval), CE loss, named gradients and BatchNorm buffers against the fixture's float64 values: 1e-4 of the tensor's
    largest magnitude (the project's parity bar); prints every measured figure beside the reference run's own fp32 error."""
    model = build_model(dtype).to(device)
    sc.named_weights(model, int(golden["seed"]))
    data = load_inputs(golden, device, dtype)
    rows = torch.from_numpy(golden["rows"]).to(device)
    worst = {}

    def rel(name, got, want, ref_err, scale=None):
        want = torch.from_numpy(np.asarray(want)).double()
        err = float((got.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()) if scale is None else float(scale), 1e-30)
        worst[name] = err
        print(f"{name}: {err:.3e} of the largest magnitude (the reference's own fp32 run: {float(ref_err):.3e})")
        return err

    model.train()
    logits = model(dict(data))
    loss = torch.nn.functional.cross_entropy(logits, data["segment"], ignore_index=-1)
    names = [str(k) for k in golden["grad_names"]]
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [params[k] for k in names])
    rel("train logits", logits[rows], golden["train_logits"], golden["err_train_logits"])
    rel("loss", loss.reshape(1), golden["loss"].reshape(1), golden["err_loss"])
    for i, (k, g) in enumerate(zip(names, grads)):
        rel("grad " + k, g.reshape(-1)[::int(golden[f"grad_stride_{i}"])], golden[f"grad_{i}"], golden["err_grads"][i], golden[f"grad_max_{i}"])
    sd = model.state_dict()
    for i, k in enumerate(str(v) for v in golden["buffer_names"]):
        rel("buffer " + k, sd[k].reshape(-1), golden[f"buffer_{i}"].reshape(-1), 0.0)
    model2 = build_model(dtype).to(device)
    sc.named_weights(model2, int(golden["seed"]))
    model2.eval()
    with torch.no_grad():
        rel("eval logits", model2(dict(data))[rows], golden["eval_logits"], golden["err_eval_logits"])
    bad = {k: v for k, v in worst.items() if not v <= 1e-4}
    assert not bad, f"outside 1e-4 of the largest magnitude: {bad}"
    return worst


def test_model_matches_the_fixture_on_cpu(golden):
    model_against_fixture(golden, "cpu")


RECIPES = {
    "semseg-spunet-v1m1-0-base": dict(type="DefaultSegmentor", backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=13,
                                      channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(1,) * 8),
                                      criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]),
    "semseg-cac-v1m1-0-spunet-base": dict(type="CAC-v1m1", num_classes=13, backbone_out_channels=96,
                                          backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0,
                                                        channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(1,) * 8),
                                          criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)],
                                          cos_temp=15, main_weight=1, pre_weight=1, pre_self_weight=1, kl_weight=1, conf_thresh=0,
                                          detach_pre_logits=False),
    "semseg-cac-v1m1-1-spunet-lovasz": dict(type="CAC-v1m1", num_classes=13, backbone_out_channels=96,
                                            backbone=dict(type="SpUNet-v1m1", in_channels=6, num_classes=0,
                                                          channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(1,) * 8),
                                            criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                                                      dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)],
                                            cos_temp=15, main_weight=1, pre_weight=1, pre_self_weight=1, kl_weight=1, conf_thresh=0,
                                            detach_pre_logits=False),
}


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_recipes_build_and_step_on_cpu(recipe, golden):
    """The `model` sections of the three reference recipes (ScanNet's 20 classes and layers cut down to the fixture's 13 and (1,) * 8)."""
    from pointcloudpdf_amd import engine

    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=RECIPES[recipe]))
    step.train()
    out = step(load_inputs(golden))
    assert torch.isfinite(out["loss"]) and out["loss"].requires_grad
    out["loss"].backward()
    got = [p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in step.parameters() if p.requires_grad]
    assert all(got)

"""GPU suite of the sparse convolutions (csrc/sparse_conv.hip) and SpUNet-v1m1: geometry kernels against the brute force, every pass at
every width against the dense float64 oracle inside the a-priori fp32 bound (tests/spunet_cases.py), bit-reproducibility, the model
against the fixture of the reference's own class, and the CAC-over-SpUNet step."""
import functools

import numpy as np
import pytest
import torch

import spunet_cases as sc
import test_spunet_cpu as cpu
from pointcloudpdf_amd import sparse_conv as spconv

pytestmark = pytest.mark.gpu
SETS = sc.site_sets()
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return np.load(cpu.GOLDEN, allow_pickle=False)


def forbid_compositions(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a torch composition ran where the HIP node must")

    monkeypatch.setattr(spconv, "table_conv_torch", boom)
    monkeypatch.setattr(spconv, "code_conv_torch", boom)


@pytest.mark.parametrize("name", list(SETS))
def test_geometry_kernels_equal_the_brute_force(name):
    indices, shape = SETS[name]
    geo = spconv.SpGeometry.build(indices.to(DEV), 2, [(3, 5), (3,)], shape)
    assert geo.hip
    for ks in (3, 5):
        assert torch.equal(geo.subm(0, ks).cpu(), sc.subm_table_brute(indices, ks)), f"{name}: k = {ks}"
    parent, code, coarse, children = sc.down_brute(indices, shape)
    st = geo.steps[0]
    assert torch.equal(st.parent.cpu(), parent) and torch.equal(st.children.cpu(), children)
    assert torch.equal(st.code.cpu()[parent >= 0], code[parent >= 0])
    assert torch.equal(geo.levels[1]["indices"].cpu(), coarse)                # ascending (batch, d0, d1, d2)
    assert torch.equal(geo.subm(1, 3).cpu(), sc.subm_table_brute(coarse, 3))
    assert geo.has_duplicates == (name == "dups")
    # the code buckets: every row with a parent exactly once, in a tile of its own code
    perm, tile_code, rows = st.bucket
    perm, tile_code = perm.cpu()[:rows], tile_code.cpu()[: rows // 128]
    listed = perm[perm >= 0]
    assert torch.equal(torch.sort(listed).values, torch.nonzero(parent >= 0).squeeze(1).int())
    assert torch.equal(code[listed.long()], tile_code.repeat_interleave(128)[perm >= 0])
    assert bool((perm[rows:] < 0).all()) if perm.numel() > rows else True


def test_bad_coordinates_raise_on_the_device():
    for bad in ([[0, -1, 0, 0]], [[0, 0, 1 << 16, 0]], [[1 << 15, 0, 0, 0]]):
        with pytest.raises(RuntimeError):
            spconv.SpGeometry.build(torch.tensor([[0, 1, 1, 1]] + bad, dtype=torch.int32, device=DEV), 2, [(3,), (3,)])


@functools.lru_cache(maxsize=None)
def _oracle(kind, name, cin, cout, ks):
    indices, shape = SETS[name]
    return sc.oracle(kind, indices, shape, cin, cout, ks, seed=23)


def _run(kind, geo, case):
    x, w = case["x"].float().to(DEV).requires_grad_(), case["w"].float().to(DEV).requires_grad_()
    b = case["b"].float().to(DEV).requires_grad_()
    fn = dict(subm=spconv.subm_conv, down=spconv.down_conv, inverse=spconv.inverse_conv)[kind]
    out = fn(x, w, b, geo, 0)
    return out, torch.autograd.grad(out, [x, w, b], case["g"].float().to(DEV))


# (the stem's widths exist as a SubM layer only)
PASSES = [(w, kind, name) for w in sc.WIDTHS for kind in ("subm", "down", "inverse") if kind == "subm" or w[2] == 3 for name in ("n65", "dense500")]


@pytest.mark.parametrize("width,kind,name", PASSES, ids=[f"{w[0]}to{w[1]}k{w[2]}-{k}-{n}" for w, k, n in PASSES])
def test_every_pass_at_every_width(width, kind, name, monkeypatch):
    cin, cout, ks = width
    case = _oracle(kind, name, cin, cout, ks)
    indices, shape = SETS[name]
    geo = spconv.SpGeometry.build(indices.to(DEV), 2, [(ks,), ()], shape)
    if width == sc.UNSUPPORTED:
        assert spconv._be().spconv_supported(ks, cin, cout) == 0    # ... and must take the composition
        monkeypatch.setattr(spconv._SubMFn, "apply", None)
        monkeypatch.setattr(spconv._DownFn, "apply", None)
        monkeypatch.setattr(spconv._InverseFn, "apply", None)
    else:
        forbid_compositions(monkeypatch)
    out, grads = _run(kind, geo, case)
    tag = f"{kind}/{name}/{cin}->{cout}"
    sc.check(tag + " out", out, case["out"], case["tol_out"])
    sc.check(tag + " gx", grads[0], case["gx"], case["tol_gx"])
    sc.check(tag + " gw", grads[1], case["gw"], case["tol_gw"])
    sc.check(tag + " gb", grads[2], case["gb"], case["tol_gb"])
    if kind == "subm" and ks == 3:   # for the record: fp32 dense conv3d on the CPU against the same truth
        dense32 = sc.subm_dense(case["x"].float(), case["w"].float(), case["b"].float(), indices)
        print(f"{tag}: fp32 dense conv3d on the CPU is {float((dense32.double() - case['out']).abs().max()):.3e} off")


@pytest.mark.parametrize("name", ["one", "n63", "n64", "n257", "twin", "origin", "dups", "odd_trunc"])
def test_passes_on_the_edge_site_sets(name, monkeypatch):
    """Tile edges, one site, two scenes with equal coordinates, coordinate 0, duplicated sites (composition by rule), truncation."""
    indices, shape = SETS[name]
    geo = spconv.SpGeometry.build(indices.to(DEV), 2, [(3,), ()], shape)
    if name != "dups":
        forbid_compositions(monkeypatch)
    for kind in ("subm", "down", "inverse"):
        case = _oracle(kind, name, 64, 32, 3)
        out, grads = _run(kind, geo, case)
        tag = f"{kind}/{name}"
        sc.check(tag + " out", out, case["out"], case["tol_out"])
        sc.check(tag + " gx", grads[0], case["gx"], case["tol_gx"])
        sc.check(tag + " gw", grads[1], case["gw"], case["tol_gw"])
        sc.check(tag + " gb", grads[2], case["gb"], case["tol_gb"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------------------------
def _model(golden):
    model = cpu.build_model().to(DEV)
    sc.named_weights(model, int(golden["seed"]))
    return model


def _loss_and_grads(model, data):
    logits = model(dict(data))
    loss = torch.nn.functional.cross_entropy(logits, data["segment"], ignore_index=-1)
    return [logits.detach(), loss.detach()] + [g for g in torch.autograd.grad(loss, list(model.parameters()))]


def test_model_runs_the_hip_nodes(golden, monkeypatch):
    forbid_compositions(monkeypatch)
    monkeypatch.setattr(spconv._Linear1, "__call__", None)      # (the k = 1 layers go through dense.linear's own products)
    model = _model(golden).train()
    _loss_and_grads(model, cpu.load_inputs(golden, DEV))


def test_model_matches_the_fixture(golden):
    cpu.model_against_fixture(golden, DEV)


def test_geometry_handed_in_is_bit_identical_and_runs_repeat(golden):
    data = cpu.load_inputs(golden, DEV)
    model = _model(golden).train()
    runs = [_loss_and_grads(model, data) for _ in range(3)]           # three evaluations: loss and all gradients bit-identical
    with_geo = dict(data, spunet_geometry=model.make_geometry(data["grid_coord"], data["offset"]))
    runs.append(_loss_and_grads(model, with_geo))
    runs.append(_loss_and_grads(model, with_geo))                      # the same object again
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_batched_scenes_equal_the_scenes_alone(golden):
    data = cpu.load_inputs(golden, DEV)
    model = _model(golden).eval()
    with torch.no_grad():
        both = model(dict(data))
        ends = [int(v) for v in golden["offset"]]
        for a, b in zip([0] + ends[:-1], ends):
            one = dict(grid_coord=data["grid_coord"][a:b], feat=data["feat"][a:b], offset=torch.tensor([b - a], dtype=torch.int32, device=DEV))
            assert torch.equal(model(one), both[a:b])


def test_cac_over_spunet_step_lowers_its_loss(golden):
    from pointcloudpdf_amd import engine

    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=cpu.RECIPES["semseg-cac-v1m1-1-spunet-lovasz"])).to(DEV)
    step.train()
    opt = engine.FusedSGD(step.parameters(), lr=0.05, momentum=0.9, weight_decay=0.0001)
    train = engine.TrainStep(step, opt, graph=False)
    data = cpu.load_inputs(golden, DEV)
    losses = [float(train(data)["loss"]) for _ in range(6)]
    print("losses:", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]

"""GPU suite of MSC-v1m1: the two nodes of csrc/scene_contrast.hip against their float64 compositions under the a-priori rule of
msc_cases.py (nothing measured goes into a bound), their bit-reproducibility, the memory of the InfoNCE node at the recipe's shape, the
model against the fixture of the reference's own class with the recorded draws, and one training step of the recipe."""
import numpy as np
import pytest
import torch

import msc_cases as mc
import test_msc_cpu as cpu
from pointcloudpdf_amd import _native, engine, losses, masked_scene_contrast as msc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# row tile = column tile = 128; a split of the columns holds one tile up to 23 tiles (P <= 2944) and two from 24 tiles on (12 splits at
# 24 tiles, 13 at 25): 127 / 128 / 129 around the tile, 2943 / 2944 / 2945 around the change of the split, 3071 / 3072 / 3073 around the
# end of the last two-tile split
NCE_SHAPES = [(1, 32), (2, 32), (33, 32), (64, 96), (65, 96), (257, 96), (700, 96), (130, 256), (127, 32), (128, 32), (129, 32), (3000, 32),
              (2943, 32), (2944, 32), (2945, 32), (3071, 32), (3072, 32), (3073, 32)]
TEMPERATURES = (0.25, 0.4, 1.0)


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN, allow_pickle=False)


def run_nce(f1, f2, match, t):
    f1, f2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    loss, pos, neg = losses.matched_info_nce(f1, f2, match, t)
    g1, g2 = torch.autograd.grad(loss, [f1, f2])
    return dict(loss=loss.detach(), pos_sim=pos, neg_sim=neg, g1=g1, g2=g2)


@pytest.mark.parametrize("case", range(len(NCE_SHAPES)))
def test_info_nce_node_matches_the_float64_composition(case):
    P, C = NCE_SHAPES[case]
    assert _native.hip_backend().msc_nce_supported(C)
    f1, f2, match = mc.nce_case(P, C, P + 7, P + 3, seed=case, device=DEV)
    for t in TEMPERATURES:
        got = run_nce(f1, f2, match, t)
        assert got["loss"].dtype == torch.float32 and got["loss"].dim() == 0 and not got["pos_sim"].requires_grad
        truth, S = mc.nce_truth(f1, f2, match, t)
        ratio = mc.nce_worst_ratio(got, truth, S, P, C)
        print(f"P={P} C={C} t={t}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0
        # rows no pair points at are written as zeros by the pass itself
        unmatched = torch.ones(f1.shape[0], dtype=torch.bool, device=DEV)
        unmatched[match[:, 0]] = False
        assert unmatched.any() and not got["g1"][unmatched].any()


def test_info_nce_index_outside_its_view_acts_as_a_zero_row():
    """include/pdfops.h: a pair whose index lies outside its view reads nothing -- the result is that of a zero feature row in its place
    (bit for bit), and the rows of the view receive no gradient from it."""
    f1, f2, match = mc.nce_case(130, 32, 137, 133, seed=9, device=DEV)
    bad = match.clone()
    bad[5, 1] = f2.shape[0]                       # one past the last row of view 2
    bad[7, 0] = -1
    got = run_nce(f1, f2, bad, 0.4)
    pad1, pad2 = torch.cat([f1, torch.zeros_like(f1[:1])]), torch.cat([f2, torch.zeros_like(f2[:1])])
    inside = bad.clone()
    inside[5, 1], inside[7, 0] = f2.shape[0], f1.shape[0]      # the zero rows appended to the views
    want = run_nce(pad1, pad2, inside, 0.4)
    assert all(torch.equal(got[k], want[k]) for k in ("loss", "pos_sim", "neg_sim"))
    assert torch.equal(got["g1"], want["g1"][:-1]) and torch.equal(got["g2"], want["g2"][:-1]) and torch.isfinite(got["g1"]).all()


def test_info_nce_other_shapes_take_the_composition():
    f1, f2, match = mc.nce_case(65, 40, 70, 70, seed=3, device=DEV)
    assert not _native.hip_backend().msc_nce_supported(40)
    for a, b in ((f1, f2), (f1[:, :32].double().contiguous(), f2[:, :32].double().contiguous())):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        got = losses.matched_info_nce(a, b, match, 0.4)
        a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        want = losses.matched_info_nce_reference(a2, b2, match, 0.4)
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and got[0].dtype == a.dtype
        got[0].backward()
        want[0].backward()
        assert torch.equal(a.grad, a2.grad) and torch.equal(b.grad, b2.grad)


def test_info_nce_node_is_bit_reproducible():
    f1, f2, match = mc.nce_case(700, 96, 707, 703, seed=21, device=DEV)
    assert int(torch.bincount(match[:, 1]).max()) >= 3          # a view-2 row matched three times
    runs = [run_nce(f1, f2, match, 0.4) for _ in range(2)]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    assert torch.isfinite(runs[0]["g1"]).all() and torch.isfinite(runs[0]["g2"]).all() and float(runs[0]["g2"].abs().max()) > 0


def test_info_nce_memory_at_the_recipe_shape():
    P, C, t = 8192, 96, 0.4
    f1, f2, match = mc.nce_case(P, C, 9000, 9000, seed=5, device=DEV)
    run_nce(f1[:200].contiguous(), f2[:200].contiguous(), match[:64] % 200, t)      # (library loaded, kernels resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = run_nce(f1, f2, match, t)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print(f"peak memory over forward + backward at P = {P}, C = {C}: {delta / 2 ** 20:.1f} MiB (one similarity matrix: {P * P * 4 / 2 ** 20:.0f} MiB)")
    assert delta < P * P * 4
    with torch.no_grad():       # the float64 composition of the loss alone
        a, b = f1[match[:, 0]].double(), f2[match[:, 1]].double()
        a, b = a / (a.norm(dim=1, keepdim=True) + 1e-7), b / (b.norm(dim=1, keepdim=True) + 1e-7)
        sim = a @ b.t()
        lse, diag = torch.logsumexp(sim / t, dim=1), torch.diagonal(sim)
        truth, S = float((lse - diag / t).mean()), float((lse.abs() + diag.abs() / t).mean())
    e = abs(float(got["loss"]) - truth)
    print(f"loss error {e:.3e}, bound {mc.gamma(2 * P + 8 * C + 64) * S:.3e}")
    assert e <= mc.gamma(2 * P + 8 * C + 64) * S
    assert torch.isfinite(got["g1"]).all() and torch.isfinite(got["g2"]).all()


# ---- reconstruction heads ---------------------------------------------------------------------------------------------------------------
def recon_case(kind, n, C, variant, seed):
    rng = np.random.default_rng(seed)
    n1, n2 = n, n + (3 if n > 1 else 0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)
    f1, f2, w, b, t1, t2 = f(n1, C), f(n2, C), f(3, C) * 0.3, f(3) * 0.2, f(n1, 3), f(n2, 3)
    m1 = torch.from_numpy(rng.random(n1) < 0.4).to(DEV)
    m2 = torch.from_numpy(rng.random(n2) < 0.4).to(DEV)
    m1[0] = True      # (n = 1: the one row is masked)
    if variant == "view2_empty":
        m2[:] = False
    elif variant == "both_empty":
        m1[:] = False
        m2[:] = False
    elif variant == "zero_prediction":      # a masked row whose prediction is exactly zero: zero features under a zero bias
        b = torch.zeros_like(b)
        f1[0] = 0
    return kind, f1, f2, m1, m2, w, b, t1, t2


def run_recon(kind, f1, f2, m1, m2, w, b, t1, t2):
    f1, f2, w, b = (x.clone().requires_grad_(True) for x in (f1, f2, w, b))
    loss = msc.masked_reconstruction(kind, f1, f2, m1, m2, w, b, t1, t2)
    if bool(torch.isnan(loss)):
        return dict(loss=loss.detach())
    g1, g2, gw, gb = torch.autograd.grad(loss, [f1, f2, w, b])
    return dict(loss=loss.detach(), gf=torch.cat([g1, g2]), gw=gw, gb=gb)


@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_reconstruction_node_matches_the_float64_composition(n, C):
    assert _native.hip_backend().msc_recon_supported(C)
    for kind in ("color", "normal"):
        for variant in ("plain", "view2_empty") + (("zero_prediction",) if kind == "normal" else ()):
            args = recon_case(kind, n, C, variant, seed=n + C)
            got, again = run_recon(*args), run_recon(*args)
            assert all(torch.equal(got[k], again[k]) for k in got)          # two runs are bit-identical
            truth, S = mc.recon_truth(*args)
            ratio = mc.recon_worst_ratio(got, truth, S, C)
            print(f"{kind} n={n} C={C} {variant}: {truth['count']} masked rows, worst error / bound = {ratio:.3f}")
            assert ratio <= 1.0
            unmasked = ~torch.cat([args[3], args[4]])
            assert not got["gf"][unmasked].any()
            if variant == "zero_prediction":
                assert torch.isfinite(got["gf"]).all() and float(got["gf"][0].abs().max()) > 1e6      # t / 1e-10 through the weights: no NaN
        args = recon_case(kind, n, C, "both_empty", seed=n)
        assert bool(torch.isnan(run_recon(*args)["loss"]))                   # 0 / 0, as upstream


def test_reconstruction_other_shapes_take_the_composition():
    args = recon_case("color", 65, 40, "plain", seed=2)
    assert not _native.hip_backend().msc_recon_supported(40)
    got = msc.masked_reconstruction(*args)
    assert torch.equal(got, msc.masked_reconstruction_composition(*args))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["a", "b"])
def test_model_on_the_fixture_with_the_recorded_draws(golden, run):
    model, _ = cpu.build_model(golden, run, DEV)
    data = mc.inputs_of(golden, DEV)
    results = []
    for ahead in (False, True):
        draws = msc.RecordedDraws(mc.draws_of(golden, run))
        results.append(cpu.run_model(golden, run, model, data, draws=draws, geometry_ahead=ahead))
    out, grads, seen = results[0]
    assert out["loss"].is_cuda and seen["match"].is_cuda
    worst = cpu.check_run(golden, run, out, grads, seen)      # masks and pairs exact, terms and gradients within the fixture's bound
    print(f"run {run}: worst error / bound = {worst:.3f}")
    # make_geometry ahead of the forward: bit-identical to the inline one
    assert all(torch.equal(out[k], results[1][0][k]) for k in out) and all(torch.equal(grads[k], results[1][1][k]) for k in grads)


def test_recipe_trains_one_step():
    """One TrainStep(graph=False) step of build_seg_step over a narrow SpUNet-v1m1 on about 3,000 voxels per view."""
    rng = np.random.default_rng(31)
    views = {1: [], 2: []}
    for _ in range(2):
        cells = rng.permutation(24 ** 3)[:3600]
        grid = np.stack([cells // 576, (cells // 24) % 24, cells % 24], 1)
        for v in (1, 2):
            views[v].append(grid[np.sort(rng.permutation(3600)[:1500 + 20 * v])])
    data = {}
    for v in (1, 2):
        grid = torch.from_numpy(np.concatenate(views[v]).astype(np.int32)).to(DEV)
        origin = grid.float() * 0.02
        a = 0.3 * v
        rot = torch.tensor([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=torch.float32, device=DEV)
        color = torch.sin(origin * 9 + v)
        data.update({f"view{v}_origin_coord": origin, f"view{v}_coord": origin @ rot.t(), f"view{v}_grid_coord": grid, f"view{v}_color": color,
                     f"view{v}_feat": torch.cat([color, torch.cos(origin * 5)], dim=1),
                     f"view{v}_offset": torch.tensor(np.cumsum([x.shape[0] for x in views[v]]), dtype=torch.int32, device=DEV)})
    torch.manual_seed(0)
    step = engine.build_seg_step(dict(model=cpu.RECIPE)).to(DEV)
    step.train()
    opt = engine.build_optimizer(dict(type="SGD", lr=0.01, momentum=0.9), step, None)
    train = engine.TrainStep(step, opt, graph=False)
    out = train(data)
    assert set(out) == {"loss", "nce_loss", "pos_sim", "neg_sim", "color_loss"} and bool(torch.isfinite(out["loss"]))
    m = step.model
    for name, p in (("mask_token", m.mask_token), ("color_head.weight", m.color_head.weight), ("stem", m.backbone.conv_input[0].weight)):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name

"""GPU suite of the incremental stage: the fused distillation loss (csrc/incr_distill.hip) against a float64 composition, the learner
against the reference's classes (tests/golden/model_incr_ref.npz), and engine.IncrSegStep captured, replayed and trained."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
from test_incremental_cpu import CASES, GRADS, run_learner

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _reference64(pred, teacher, lab, tp, tt):
    """Loss and d loss / d pred in float64 (pointpdf_incr_v1m1_base.py:69-86 restated)."""
    p64, t64 = pred.double().cpu(), teacher.double().cpu()
    n, cs = p64.shape
    t = torch.zeros(n, cs, dtype=torch.float64)
    t[:, :t64.shape[1]] = torch.softmax(t64 / tt, 1)
    lab = lab.cpu()
    valid = lab != -1
    t[valid] = torch.nn.functional.one_hot(lab[valid], cs).double()
    logp = torch.log_softmax(p64 / tp, 1)
    loss = float((torch.xlogy(t, t) - t * logp).sum() / n)
    grad = (torch.softmax(p64 / tp, 1) * t.sum(1, keepdim=True) - t) / (tp * n)
    return loss, grad


def _labels(n, cs, mode, g):
    lab = torch.full((n,), -1, dtype=torch.long)
    if mode == "some":
        lab[torch.rand(n, generator=g) < 0.3] = 0
        lab = torch.where(lab == 0, torch.randint(0, cs, (n,), generator=g), lab)
    elif mode == "all":
        lab = torch.randint(0, cs, (n,), generator=g)
    return lab.to(DEV)


def _fused(pred, teacher, lab, tp, tt):
    from pointcloudpdf_amd import incremental

    p = pred.clone().requires_grad_(True)
    loss = incremental.IncrDistillKlLoss(tp, tt)(p, teacher, lab)
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4097, 200000])
@pytest.mark.parametrize("cs,ct", [(15, 13), (2, 1), (20, 20), (64, 60)])
def test_fused_kl_matches_float64(n, cs, ct):
    g = torch.Generator().manual_seed(n * 131 + cs)
    pred = (3 * torch.randn(n, cs, generator=g)).to(DEV)
    teacher = (3 * torch.randn(n, ct, generator=g)).to(DEV)
    for tp, tt in [(1.0, 1.0), (2.0, 0.5)]:
        for mode in ("none", "some", "all"):
            lab = _labels(n, cs, mode, g)
            loss, grad = _fused(pred, teacher, lab, tp, tt)
            want, gwant = _reference64(pred, teacher, lab, tp, tt)
            assert abs(float(loss) - want) <= 2e-5 * abs(want) + 1e-6, (n, cs, ct, tp, tt, mode, float(loss), want)
            r = helpers.max_rel(grad.cpu().numpy(), gwant.numpy())
            assert r <= 2e-5, (n, cs, ct, tp, tt, mode, r)


def test_fused_kl_runs_on_the_kernel_and_guards_its_inputs():
    from pointcloudpdf_amd import _native, incremental

    pred = torch.randn(300, 15, device=DEV, requires_grad=True)
    teacher = torch.randn(300, 13, device=DEV)
    lab = torch.full((300,), -1, dtype=torch.long, device=DEV)
    loss = incremental.IncrDistillKlLoss()(pred, teacher, lab)
    assert "FusedIncrKl" in type(loss.grad_fn.next_functions[0][0]).__name__   # (loss * loss_weight over the kernel's node)
    # a label that is neither -1 nor a class id: NaN loss, no host sync needed to see it
    bad = lab.clone()
    bad[17] = 15
    assert torch.isnan(incremental.IncrDistillKlLoss()(pred, teacher, bad)).item()
    bad[17] = -3
    assert torch.isnan(incremental.IncrDistillKlLoss()(pred, teacher, bad)).item()
    lib = _native.hip_backend().lib
    ws = torch.empty(int(lib.pdf_incr_kl_workspace_floats()), device=DEV)
    grad = torch.empty_like(pred)
    s = ctypes.c_void_p(_native.raw_stream())
    args = (pred.data_ptr(), teacher.data_ptr(), lab.data_ptr(), -1, 1.0, 1.0, grad.data_ptr(), ws.data_ptr(), ws.data_ptr() + 8, s)
    assert lib.pdf_incr_kl_forward(0, 15, 13, *args) == -1          # n < 1
    assert lib.pdf_incr_kl_forward(300, 12, 13, *args) == -1        # Ct > Cs
    assert lib.pdf_incr_kl_forward(300, 65, 13, *args) == -3        # Cs > 64
    assert lib.pdf_incr_kl_forward(300, 15, 13, *args) == 0


def test_fused_kl_is_bit_reproducible_and_differentiable_twice():
    from pointcloudpdf_amd import incremental

    g = torch.Generator().manual_seed(5)
    pred = torch.randn(200000, 15, generator=g).to(DEV)
    teacher = torch.randn(200000, 13, generator=g).to(DEV)
    lab = _labels(200000, 15, "some", g)
    runs = [_fused(pred, teacher, lab, 1.0, 1.0) for _ in range(3)]
    for loss, grad in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(grad, runs[0][1])
    p = pred.clone().requires_grad_(True)
    loss = incremental.IncrDistillKlLoss(loss_weight=2.0)(p, teacher, lab)
    (g1,) = torch.autograd.grad(loss, p, retain_graph=True)
    loss.backward()
    assert torch.equal(g1, p.grad)
    assert torch.equal(g1, 2.0 * runs[0][1])


@pytest.mark.parametrize("case", list(CASES))
def test_learner_matches_reference_class_on_gpu(golden_dir, case):
    golden = np.load(os.path.join(golden_dir, "model_incr_ref.npz"))
    torch.backends.cuda.matmul.allow_tf32 = False
    out, student, teacher, learner = run_learner(case, golden, device="cuda")
    assert sorted(out.keys()) == list(golden[f"{case}_keys"])
    helpers.assert_close(out["loss"], golden[f"{case}_loss"], helpers.REL_TOL, f"{case} loss")
    if "seg_logits" in out:
        helpers.assert_close(helpers.thin(out["seg_logits"].detach().cpu().numpy()), golden[f"{case}_seg_logits"], helpers.REL_TOL, "seg_logits")
    if CASES[case][0]:
        helpers.assert_close(helpers.thin(student.cpu().numpy()), golden[f"{case}_student_logits"], helpers.REL_TOL, "student logits")
        helpers.assert_close(helpers.thin(teacher.cpu().numpy()), golden[f"{case}_teacher_logits"], helpers.REL_TOL, "teacher logits")
        named = dict(learner.incr_backbone.named_parameters())
        for k in GRADS:
            g = named[k].grad.detach().cpu().numpy()
            g = g[:helpers.GRAD_ROWS] if g.ndim >= 2 else g
            tol = helpers.GRAD_TOL if helpers.well_conditioned(k) else helpers.LOOSE_GRAD_TOL
            helpers.assert_close(g, golden[f"{case}_grad_{k}"], tol, f"{case} grad {k}")
        assert all(p.grad is None for p in learner.teacher_model.parameters())


def _incr_batch(sizes, first_scene_id):
    from pointcloudpdf_amd import data_path, synthetic

    b = synthetic.make_batch(sizes, first_scene_id=first_scene_id, device=DEV, unknown=())
    _, b["segment_incr"] = data_path.remap_label(b["segment"], {5: 13, 9: 14})
    return b


def _step(backbone="PointTransformer-Seg38"):
    from pointcloudpdf_amd import engine, synthetic

    step = engine.IncrSegStep(backbone=backbone)
    synthetic.fill_parameters_deterministic(step.teacher, seed=1)
    synthetic.fill_parameters_deterministic(step.student, seed=2)
    return step.to(DEV).train()


def test_step_modes_and_parameters():
    step = _step()
    assert step.training and step.learner.training and step.student.training and not step.teacher.training
    assert all(not p.requires_grad for p in step.teacher.parameters())
    trainable = {id(p) for p in step.parameters() if p.requires_grad}
    assert trainable == {id(p) for p in step.student.parameters()}
    assert step.student.cls[3].weight.shape[0] == 15 and step.teacher.backbone.cls[3].weight.shape[0] == 13


def test_captured_incr_step_replays_the_eager_step():
    """engine.IncrSegStep captured once (``batch_keys``: segment_incr at a fixed address) and replayed on other batches of the same sizes:
    loss and every student gradient equal the eager step; several FusedSGD steps leave the teacher's parameters and BatchNorm buffers
    untouched; the graph holds no memset node."""
    from pointcloudpdf_amd import engine
    from pointcloudpdf_amd.geometry import GeometryPrefetcher

    sizes = [6000, 5000]
    step = _step()
    batches = [_incr_batch(sizes, 40 + 10 * i) for i in range(3)]
    teacher0 = {k: v.detach().clone() for k, v in step.teacher.state_dict().items()}
    cap = engine.CapturedStep(step, batches[0], debug_graph=True)
    assert cap.keys == step.batch_keys
    assert cap.node_census()["memset"] == 0, cap.node_census()
    pf = GeometryPrefetcher(depth=2)
    tickets = pf.submit_group(batches)
    params = [p for p in step.parameters() if p.requires_grad]
    opt = engine.FusedSGD(step.student.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    for b, t in zip(batches, tickets):
        geom = pf.get(t)
        state = {n: v.detach().clone() for n, v in step.named_buffers()}
        out = cap(b, geom)
        got = dict(loss=out["loss"].detach().clone(), grads=[p.grad.detach().clone() for p in params])
        assert torch.equal(cap.static["segment_incr"], b["segment_incr"])
        with torch.no_grad():
            for n, v in step.named_buffers():
                v.copy_(state[n])
        for p in params:
            p.grad = None
        ref = step(dict(coord=b["coord"], feat=b["feat"], offset=b["offset"], offset_host=b["offset_host"], segment_incr=b["segment_incr"],
                        pdf_geometry=geom))
        ref["loss"].backward()
        assert abs(float(got["loss"]) - float(ref["loss"])) <= 2e-6 * abs(float(ref["loss"])), (float(got["loss"]), float(ref["loss"]))
        gscale = max(float(p.grad.abs().max()) for p in params)
        for p, g in zip(params, got["grads"]):
            assert float((p.grad - g).abs().max()) <= 2e-3 * float(p.grad.abs().max()) + 1e-4 * gscale
        for p, g in zip(params, got["grads"]):
            p.grad = g
        opt.step()
    torch.cuda.synchronize()
    for k, v in step.teacher.state_dict().items():
        assert torch.equal(v, teacher0[k]), f"teacher tensor {k} changed"


def test_one_geometry_prepass_serves_both_networks():
    """kNN / FPS launches of one eager step without a prefetched geometry: exactly those of the student's forward alone."""
    from pointcloudpdf_amd import _native

    step = _step()
    b = _incr_batch([6000, 5000], 70)
    be = _native.hip_backend()
    counts = {"knn_query": 0, "farthest_point_sampling": 0}
    originals = {}
    for name in counts:
        orig = getattr(be, name)
        originals[name] = (name in be.__dict__, orig)

        def wrapped(*a, _orig=orig, _n=name, **k):
            counts[_n] += 1
            return _orig(*a, **k)

        setattr(be, name, wrapped)
    try:
        d = dict(coord=b["coord"], feat=b["feat"], offset=b["offset"], offset_host=b["offset_host"], segment_incr=b["segment_incr"])
        step(dict(d))["loss"].backward()
        full = dict(counts)
        for k in counts:
            counts[k] = 0
        step.student(dict(d))
        alone = dict(counts)
    finally:
        for name, (own, orig) in originals.items():
            if own:
                setattr(be, name, orig)
            else:
                delattr(be, name)
    assert full == alone and alone["farthest_point_sampling"] > 0 and alone["knn_query"] > 0, (full, alone)


@pytest.mark.parametrize("amp", [False, True])
def test_train_loop_decreases_the_loss(amp):
    from pointcloudpdf_amd import engine

    step = _step()
    b = _incr_batch([6000, 5000], 80)
    opt = engine.FusedSGD(step.student.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    scaler = engine.DeviceGradScaler(DEV) if amp else None
    train = engine.TrainStep(step, opt, exchange=engine.FlatGradAllReduce(step), scaler=scaler, autocast=torch.float16 if amp else None)
    losses = []
    for _ in range(20):
        losses.append(float(train(dict(b))["loss"]))
    assert train.capture_error is None and train.captured is not None
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-3:]) < 0.95 * np.mean(losses[:3]), losses


def test_full_size_captured_incr_step_is_finite():
    from pointcloudpdf_amd import engine

    step = _step("PointTransformer-Seg50")
    b = _incr_batch([100000, 100000], 11)
    cap = engine.CapturedStep(step, b)
    from pointcloudpdf_amd.geometry import Geometry

    out = cap(b, Geometry(b["coord"], b["offset"], b["offset_host"]).precompute())
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item()
    assert all(torch.isfinite(p.grad).all().item() for p in step.student.parameters())

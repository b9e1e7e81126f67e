"""GPU suite of FusedAdamW / FusedAdam (csrc/optim.hip: k_adam_tick + k_adam) against torch.optim.AdamW / Adam.

The bound, everywhere: for every tensor, and for the parameter, exp_avg and exp_avg_sq alike, our largest deviation from a float64 run
of torch's single-tensor optimizer is at most max(2 x the deviation of torch's own float32 run from that float64 run,
2 * 2^-23 * max|x|).  The factor 2 allows for fused multiply-adds on the device; it is not a measurement.  Every test prints the
measured ratio ours / torch-fp32 before it asserts (run with -s); DESIGN.md section 8h records it."""
import copy
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
CFG4 = dict(type="OneCycleLR", max_lr=0.005, pct_start=0.05, anneal_strategy="cos", div_factor=10.0, final_div_factor=1000.0)


def _check(label, ours, ref64, ref32, worst):
    """ours / ref32: float32 tensors, ref64: the float64 run.  Records ours / torch-fp32 in ``worst`` and returns the failure, if any."""
    ref64 = ref64.detach().cpu().double()
    mine = float((ours.detach().cpu().double() - ref64).abs().max())
    theirs = float((ref32.detach().cpu().double() - ref64).abs().max())
    bound = max(2.0 * theirs, 2.0 * ULP * float(ref64.abs().max()))
    worst.append((mine / theirs if theirs > 0 else (0.0 if mine == 0 else float("inf")), label, mine, theirs, bound))
    return None if mine <= bound else (label, mine, theirs, bound)


def _check_state(tag, ours_opt, pa, o64, p64, o32, p32, worst):
    bad = []
    for k, (x, y64, y32) in enumerate(zip(pa, p64, p32)):
        bad.append(_check(f"{tag} p[{k}]", x, y64, y32, worst))
        if y64 in o64.state and "exp_avg" in o64.state[y64]:
            for key in ("exp_avg", "exp_avg_sq"):
                bad.append(_check(f"{tag} {key}[{k}]", ours_opt.state[x][key], o64.state[y64][key], o32.state[y32][key], worst))
            steps = (float(ours_opt.state[x]["step"]), float(o64.state[y64]["step"]), float(o32.state[y32]["step"]))
            assert steps[0] == steps[1] == steps[2], (tag, k, steps)
        else:   # never had a gradient: torch holds no state; ours holds zeros and step 0
            assert float(ours_opt.state[x]["step"]) == 0.0 and not ours_opt.state[x]["exp_avg"].any()
    return [b for b in bad if b is not None]


def _report(name, worst):
    top = max(worst)
    print(f"\n[{name}] ours / torch-fp32 deviation from the fp64 run: max ratio {top[0]:.3f} at {top[1]} (ours {top[2]:.3e}, torch fp32 {top[3]:.3e}, "
          f"bound {top[4]:.3e}); {len(worst)} comparisons, median ratio {float(np.median([w[0] for w in worst if np.isfinite(w[0])])):.3f}")


def _inputs(seed):
    """The shapes of test_fused_sgd_matches_torch_sgd (odd lengths, several chunks, a 4-byte-aligned view) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(3,), (13, 32), (70001,), (4096,), (512, 513), (9, 3, 3)]
    base = [torch.randn(s, generator=g) for s in shapes]
    flat = torch.randn(1001, generator=g)
    return g, base, flat


def _trajectory(name, ours_cls, torch_cls, groups, hyper, iters=40, sched=CFG4, table_cache=True):
    """``groups``: list of (indices, overrides).  Runs ours on the GPU and torch's single-tensor optimizer on the CPU in fp64 and fp32 from
    the same inputs, OneCycleLR with config 4's arguments stepped every iteration."""
    from pointcloudpdf_amd import optim

    g, base, flat = _inputs(3)
    pa = [torch.nn.Parameter(b.clone().cuda()) for b in base] + [torch.nn.Parameter(flat.clone().cuda()[1:])]   # (4-byte aligned only)
    assert pa[-1].data_ptr() % 16 == 4
    p32 = [torch.nn.Parameter(b.clone()) for b in base] + [torch.nn.Parameter(flat.clone()[1:])]
    p64 = [torch.nn.Parameter(b.double()) for b in base] + [torch.nn.Parameter(flat.double()[1:])]

    def grouped(ps):
        return [dict(params=[ps[i] for i in idx], **over) for idx, over in groups]

    oa = ours_cls(grouped(pa), **hyper)
    oa._table_cache_on = table_cache     # (off: the ring of full-size tables, of which a group fills only its own rows)
    o32 = torch_cls(grouped(p32), foreach=False, **hyper)
    o64 = torch_cls(grouped(p64), foreach=False, **hyper)
    max_lr = [over.get("lr", hyper["lr"]) for _, over in groups]
    scheds = [optim.build_scheduler(dict(sched, max_lr=max_lr), o, iters) for o in (oa, o32, o64)]
    scales = [1.0, 0.1, 0.01, 0.3, 0.03, 1.0, 0.5]    # gradient scales 1e-2 .. 1
    worst, bad = [], []
    for it in range(iters):
        for o in (oa, o32, o64):
            o.zero_grad(set_to_none=True)
        for k in range(len(pa)):
            if k == 1 and it in (1, 3):
                continue   # no gradient this iteration: skipped, and its step count falls behind, in all three
            gr = torch.randn(p32[k].shape, generator=g) * scales[k]
            if k == 3:
                gr[::5] = 0.0      # exact zeros in the gradient
                if it < 2:
                    gr[7::5] = 0.0
            pa[k].grad, p32[k].grad, p64[k].grad = gr.cuda(), gr.clone(), gr.double()
        assert oa.param_groups[0]["betas"] == o32.param_groups[0]["betas"] and oa.param_groups[0]["lr"] == o32.param_groups[0]["lr"]
        for o in (oa, o32, o64):
            o.step()
        for s in scheds:
            s.step()
        if it in (0, 1, 4, iters - 1):
            torch.cuda.synchronize()
            bad += _check_state(f"it{it}", oa, pa, o64, p64, o32, p32, worst)
    _report(name, worst)
    assert not bad, bad
    assert float(oa.state[pa[1]]["step"]) == iters - 2 and float(oa.state[pa[0]]["step"]) == iters
    return oa, pa


def test_fused_adamw_follows_torch_adamw_under_one_cycle():
    """Test 1 of the issue: 40 iterations, OneCycleLR of config 4 (lr AND beta1 move every iteration), one group."""
    from pointcloudpdf_amd import engine

    oa, pa = _trajectory("adamw", engine.FusedAdamW, torch.optim.AdamW, [(list(range(7)), {})], dict(lr=0.005, weight_decay=0.02))
    assert oa.param_groups[0]["betas"][0] != 0.9     # (the cycle moved beta1, and the kernel was handed the moved value)


def test_fused_adam_l2_form_follows_torch_adam():
    from pointcloudpdf_amd import engine

    _trajectory("adam-l2", engine.FusedAdam, torch.optim.Adam, [(list(range(7)), {})], dict(lr=0.005, weight_decay=0.02))


def test_two_parameter_groups_follow_their_own_hyper_parameters():
    from pointcloudpdf_amd import engine

    groups = [([0, 2, 4, 6], {}), ([1, 3, 5], dict(lr=0.0005, weight_decay=0.2))]
    oa, pa = _trajectory("two groups", engine.FusedAdamW, torch.optim.AdamW, groups, dict(lr=0.005, weight_decay=0.02), table_cache=False)
    assert oa.param_groups[0]["weight_decay"] == 0.02 and oa.param_groups[1]["weight_decay"] == 0.2
    assert oa.param_groups[1]["lr"] == pytest.approx(oa.param_groups[0]["lr"] / 10.0, rel=1e-9)


def _model(dev, seed=5):
    from pointcloudpdf_amd import engine, synthetic

    step = engine.OpenSegStep("PointTransformer-Seg26").to(dev)
    synthetic.fill_parameters_deterministic(step, seed=seed)
    step.train()
    return step


def _small_batch(dev):
    from pointcloudpdf_amd import synthetic
    from pointcloudpdf_amd.geometry import Geometry

    batch = synthetic.make_batch([3000, 2400], first_scene_id=60, device=dev)
    geom = Geometry(batch["coord"], batch["offset"], batch["offset_host"]).precompute()
    return dict(batch, pdf_geometry=geom)


def test_real_gradients_through_train_step():
    """Ten iterations of OpenSegStep(Seg26) + recognizer through engine.TrainStep with FusedAdamW; the gradients of every iteration are
    handed to shadow torch.optim.AdamW runs (fp32 and fp64, single-tensor, CPU) on cloned parameters: the optimizer alone is compared,
    on BatchNorm and bias tensors and whatever all-zero gradients the model produces."""
    from pointcloudpdf_amd import engine

    dev = torch.device("cuda", 0)
    step, batch = _model(dev), _small_batch(dev)
    params = [p for p in step.parameters() if p.requires_grad]
    hyper = dict(lr=0.005, weight_decay=0.02)
    opt = engine.FusedAdamW(params, **hyper)
    p32 = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    p64 = [torch.nn.Parameter(p.detach().cpu().double()) for p in params]
    o32, o64 = torch.optim.AdamW(p32, foreach=False, **hyper), torch.optim.AdamW(p64, foreach=False, **hyper)
    scheds = [engine.build_scheduler(CFG4, o, 10) for o in (opt, o32, o64)]
    train = engine.TrainStep(step, opt, graph=False)
    losses, zero_grads = [], 0
    for it in range(10):
        losses.append(float(train(batch)["loss"].detach()))       # forward, backward, FusedAdamW.step(); the gradients stay on the parameters
        for p, y32, y64 in zip(params, p32, p64):
            y32.grad = None if p.grad is None else p.grad.detach().cpu().clone()
            y64.grad = None if p.grad is None else p.grad.detach().cpu().double()
            zero_grads += int(p.grad is not None and not bool(p.grad.any()))
        o32.step(); o64.step()
        for s in scheds:
            s.step()
    engine.release_autograd_state(step)
    assert all(np.isfinite(losses)), losses
    worst = []
    bad = _check_state("step10", opt, params, o64, p64, o32, p32, worst)
    _report(f"real gradients, {len(params)} tensors, {zero_grads} all-zero gradients", worst)
    assert not bad, bad[:10]
    assert any(p.dim() == 1 for p in params)       # (BatchNorm weights / biases are among them)


def test_graph_replay_equals_the_eager_run():
    """TrainStep(graph=True): forward + backward replayed, FusedAdamW + OneCycleLR outside the graph -> the eager losses and parameters, bit for bit."""
    from pointcloudpdf_amd import engine

    dev = torch.device("cuda", 0)
    batch = _small_batch(dev)

    def run(graph):
        step = _model(dev)
        opt = engine.FusedAdamW([p for p in step.parameters() if p.requires_grad], lr=0.005, weight_decay=0.02)
        sched = engine.build_scheduler(CFG4, opt, 10)
        train = engine.TrainStep(step, opt, graph=graph)
        losses = []
        for _ in range(10):
            losses.append(train(batch)["loss"].detach().clone())     # (a replayed step hands back the graph's own output tensor)
            sched.step()
        torch.cuda.synchronize()
        assert graph == (train.captured is not None), train.capture_error
        out = [float(v) for v in losses], [p.detach().clone() for p in step.parameters()], [float(opt.state[p]["step"]) for p in opt.params]
        engine.release_autograd_state(step)
        return out

    (le, pe, se), (lg, pg, sg) = run(False), run(True)
    assert le == lg, (le, lg)
    assert all(torch.equal(a, b) for a, b in zip(pe, pg))
    assert se == sg and max(se) == 10.0


def _guarded(fn):
    """Run ``fn`` with torch's sync debug mode on; -> the warnings about the host waiting for the device."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]


def test_device_grad_scaler_drives_fused_adamw():
    """DeviceGradScaler + FusedAdamW against torch.amp.GradScaler + torch.optim.AdamW (fp32 and fp64 parameters) on the same scaled
    gradients.  An iteration with an inf / a nan leaves p, exp_avg, exp_avg_sq and EVERY step count bit-identical and halves the scale; the
    clean iteration after a skipped first one is step 1 (its bias correction included); nothing between the backward and update() makes
    the host wait for the device."""
    from pointcloudpdf_amd import engine

    g = torch.Generator(device="cuda").manual_seed(11)
    shapes = [(7,), (33, 64), (70001,), (4096,)]
    pa = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g)) for s in shapes]
    p32 = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    p64 = [torch.nn.Parameter(p.detach().double()) for p in pa]
    hyper = dict(lr=0.005, weight_decay=0.02)
    oa = engine.FusedAdamW(pa, **hyper)
    o32, o64 = torch.optim.AdamW(p32, foreach=False, **hyper), torch.optim.AdamW(p64, foreach=False, **hyper)
    sa = engine.DeviceGradScaler("cuda", init_scale=1024.0, growth_interval=2)
    s32, s64 = (torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2) for _ in range(2))
    for s in (s32, s64):
        s.scale(torch.zeros(1, device="cuda"))   # (torch creates its scale tensor lazily, in scale())
    plan = ["inf", "ok", "ok", "nan", "ok", "ok", "ok"]
    assert _guarded(lambda: float(sa.scale_tensor)), "the guard itself: a host read of a device scalar must be reported"
    worst, bad, done = [], [], 0
    for it, kind in enumerate(plan):
        before = [[t.clone() for t in (p.detach(), oa.state[p]["exp_avg"], oa.state[p]["exp_avg_sq"], oa.state[p]["step"])] for p in pa]
        scale = s32.get_scale()
        assert sa.get_scale() == scale == s64.get_scale(), (it, sa.get_scale(), scale)
        for x, y32, y64 in zip(pa, p32, p64):
            gr = torch.randn(x.shape, device="cuda", generator=g)
            x.grad, y32.grad, y64.grad = (gr * scale).clone(), (gr * scale).clone(), (gr * scale).double()   # what scale(loss).backward() leaves
        if kind != "ok":
            for ps in (pa, p32, p64):
                ps[2].grad[12345] = float("inf") if kind == "inf" else float("nan")
        reads = _guarded(lambda: (sa.step(oa), sa.update()))
        assert not reads, reads
        s32.step(o32); s32.update()
        s64.step(o64); s64.update()
        torch.cuda.synchronize()
        if kind != "ok":
            for p, (p0, m0, v0, n0) in zip(pa, before):
                st = oa.state[p]
                assert torch.equal(p.detach(), p0) and torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0), (it, kind)
                assert torch.equal(st["step"], n0) and float(n0) == done, (it, kind, float(st["step"]), done)
            assert sa.get_scale() == scale * 0.5
        else:
            done += 1
            assert all(float(oa.state[p]["step"]) == done for p in pa), (it, [float(oa.state[p]["step"]) for p in pa], done)
            bad += _check_state(f"it{it}", oa, pa, o64, p64, o32, p32, worst)
    _report("amp", worst)
    assert not bad, bad
    assert sa.get_scale() == s32.get_scale() and done == 5


def test_moved_parameters_and_a_cpu_torch_checkpoint():
    """Pointers are read at every step: after ``p.data = p.data.clone()`` the new storage is updated and the step counts go on; after
    ``load_state_dict`` of a checkpoint trained by torch.optim.AdamW on the CPU (its ``step`` tensors stay on the CPU) the next step
    moves the state to the device and continues the counts."""
    from pointcloudpdf_amd import engine

    g, base, flat = _inputs(9)
    hyper = dict(lr=0.005, weight_decay=0.02)
    pc = [torch.nn.Parameter(b.clone()) for b in base]
    oc = torch.optim.AdamW(pc, foreach=False, **hyper)
    grads = [[torch.randn(b.shape, generator=g) * 0.1 for b in base] for _ in range(5)]
    for it in range(3):
        for p, gr in zip(pc, grads[it]):
            p.grad = gr.clone()
        oc.step()
    pa = [torch.nn.Parameter(p.detach().clone().cuda()) for p in pc]
    oa = engine.FusedAdamW(pa, lr=1.0, betas=(0.5, 0.5), weight_decay=0.0)
    oa.load_state_dict(copy.deepcopy(oc.state_dict()))
    assert oa.param_groups[0]["lr"] == 0.005 and oa.param_groups[0]["betas"] == (0.9, 0.999)
    assert not oa.state[pa[0]]["step"].is_cuda                      # torch's policy for that key: left where the checkpoint had it
    for it in (3, 4):
        for x, y, gr in zip(pa, pc, grads[it]):
            x.grad, y.grad = gr.cuda(), gr.clone()
        if it == 4:                                                 # moved parameters (model.to(), load_state_dict(assign=True))
            old = pa[2].data
            with torch.no_grad():
                pa[2].data = pa[2].data.clone()
            kept = old.clone()
        oa.step(); oc.step()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(pa, pc)):
            st = oa.state[x]
            assert st["step"].is_cuda and st["exp_avg"].is_cuda and float(st["step"]) == it + 1 == float(oc.state[y]["step"])
            for ours, theirs in ((x.detach(), y.detach()), (st["exp_avg"], oc.state[y]["exp_avg"]), (st["exp_avg_sq"], oc.state[y]["exp_avg_sq"])):
                err = float((ours.cpu() - theirs).abs().max())
                assert err <= 4 * ULP * max(float(theirs.abs().max()), 1e-30), (it, k, err)
    assert torch.equal(old, kept) and not torch.equal(pa[2].detach(), kept)     # the old storage was left alone, the new one updated

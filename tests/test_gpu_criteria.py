"""GPU suite: the passes of csrc/criteria.hip -- the full cross-entropy, focal, dice and binary focal losses -- through the modules, the
C ABI and a captured step.  Tolerance rule: criteria_cases.py (error against the float64 evaluation at most 2x the error of the
reference's own fp32 result -- the fixture, or the fp32 torch composition on the device for the shapes the fixture cannot hold)."""
import ctypes

import numpy as np
import pytest
import torch

import criteria_cases as cc

pytestmark = pytest.mark.gpu

IGNORE = -1
CASES = cc.case_ids()
REDUCE = {"none": 0, "mean": 1, "sum": 2}

# Shapes the fixture cannot hold.  name: (kind, N, C, seed, constructor arguments).  257: one row past a workgroup; 300,001 x 3: beyond the
# block cap (1024 workgroups of 256 rows), so the grid-stride loop and its last partial trip run; 64 / 65: both sides of the lane-per-row
# boundary; 5000 x 65: beyond the block cap of the wave-per-row kernels (1024 workgroups of 4 rows); 200 classes.
RAMP = "ramp"
SHAPES = {
    "ce_n257_c13": ("ce", 257, 13, 501, dict(weight=RAMP, label_smoothing=0.1)),
    "ce_n300001_c3": ("ce", 300001, 3, 502, dict(weight=RAMP, label_smoothing=0.1)),
    "ce_n300001_c3_none": ("ce", 300001, 3, 503, dict(weight=RAMP, reduction="none")),
    "ce_n257_c64": ("ce", 257, 64, 504, dict(weight=RAMP)),
    "ce_n257_c65": ("ce", 257, 65, 505, dict(weight=RAMP, label_smoothing=0.1)),
    "ce_n5000_c65_plain": ("ce", 5000, 65, 506, dict()),
    "ce_n1000_c200_sum": ("ce", 1000, 200, 507, dict(label_smoothing=0.2, reduction="sum")),
    "focal_n257_c13": ("focal", 257, 13, 511, dict(alpha=RAMP)),
    "focal_n300001_c3": ("focal", 300001, 3, 512, dict()),
    "focal_n257_c64": ("focal", 257, 64, 513, dict(gamma=1.5)),
    "focal_n257_c65_sum": ("focal", 257, 65, 514, dict(alpha=RAMP, reduction="sum")),
    "focal_n1000_c200": ("focal", 1000, 200, 515, dict(gamma=3.0, alpha=0.25)),
    "dice_n257_c13": ("dice", 257, 13, 521, dict()),
    "dice_n300001_c3": ("dice", 300001, 3, 522, dict()),
    "dice_n257_c64": ("dice", 257, 64, 523, dict(smooth=0.5, exponent=3)),
    "dice_n257_c65": ("dice", 257, 65, 524, dict(ignore_index=7)),
    "dice_n5000_c65": ("dice", 5000, 65, 525, dict()),
    "dice_n1000_c200": ("dice", 1000, 200, 526, dict(smooth=0.5, exponent=1.5)),
    "dice_n300_c300": ("dice", 300, 300, 527, dict()),   # (two column chunks of the class sums)
    "bfocal_n257": ("bfocal", 257, 1, 531, dict()),
    "bfocal_n300001_soft": ("bfocal", 300001, 1, 532, dict(gamma=1.5, alpha=0.25)),
    "bfocal_n300001_prob_elementwise": ("bfocal", 300001, 1, 533, dict(logits=False, reduce=False)),
}


def make_shape(name):
    kind, n, c, seed, kw = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    kw = {k: ([round(0.2 + 0.7 * (j + 0.5) / c, 4) for j in range(c)] if isinstance(v, str) and v == RAMP else v) for k, v in kw.items()}
    if kind == "bfocal":
        x = 2.0 * torch.randn(n, generator=g)
        if not kw.get("logits", True):
            x = torch.sigmoid(x)
        t = torch.rand(n, generator=g) if "soft" in name else torch.randint(0, 2, (n,), generator=g).float()
        return kind, kw, x, t
    x = 2.0 * torch.randn(n, c, generator=g)
    t = torch.randint(0, c, (n,), generator=g)
    t[torch.randperm(n, generator=g)[: max(1, n // 10)]] = kw.get("ignore_index", IGNORE)
    return kind, kw, x, t


@pytest.fixture(scope="module")
def golden(golden_dir):
    return cc.load(golden_dir)


@pytest.fixture(scope="module")
def backend():
    from pointcloudpdf_amd import _native

    return _native.hip_backend()


def check(name, kind, kw, x, t, ref_loss, ref_grad):
    """The module on the device against the float64 evaluation on the device; the yardstick is the given reference result."""
    module = cc.build(kind, kw)   # (imports the package before the first device call)
    dx, dt = x.cuda(), t.cuda()
    loss64, grad64 = cc.truth(kind, kw, dx, dt)
    loss, grad = cc.loss_and_grad(module, dx, dt)
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and loss.shape == loss64.shape and grad.shape == grad64.shape
    e, e_ref = cc.err(loss, loss64), cc.err(ref_loss, loss64)
    g, g_ref = cc.err(grad, grad64), cc.err(ref_grad, grad64)
    print(f"{name}: loss error {e:.3e} (reference {e_ref:.3e}, bound {cc.bound(e_ref, loss64):.3e}), gradient error {g:.3e} "
          f"(reference {g_ref:.3e}, bound {cc.bound(g_ref, grad64):.3e})")
    assert e <= cc.bound(e_ref, loss64), (e, e_ref)
    assert g <= cc.bound(g_ref, grad64), (g, g_ref)


@pytest.mark.parametrize("kind,name", CASES, ids=[n for _, n in CASES])
def test_fixture_case_on_the_device(golden, kind, name):
    x, t, kw, ref_loss, ref_grad = cc.case(golden, name)
    check(name, kind, kw, x, t, ref_loss, ref_grad)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_beyond_the_fixture(name):
    import pointcloudpdf_amd  # noqa: F401  (before the first device call)

    kind, kw, x, t = make_shape(name)
    ref_loss, ref_grad = cc.loss_and_grad(lambda a, b: cc.composition(kind, kw, a, b), x.cuda(), t.cuda())   # fp32 composition, device
    check(name, kind, kw, x, t, ref_loss.cpu(), ref_grad.cpu())


# ---- the raw C ABI ---------------------------------------------------------------------------------------------------------------------
def _stream():
    from pointcloudpdf_amd import _native

    return ctypes.c_void_p(_native.raw_stream())


def _acc(lib, c, dev):
    lib.pdf_criteria_workspace_floats.restype = ctypes.c_long
    return torch.empty(int(lib.pdf_criteria_workspace_floats(c)), dtype=torch.float32, device=dev)


def abi_ce(lib, x, t, w, eps, reduction, ignore=IGNORE, gy=None):
    n, c = x.shape
    grad, acc = torch.empty_like(x), _acc(lib, c, x.device)
    loss = torch.empty(n if reduction == "none" else 1, device=x.device)
    assert lib.pdf_ce_ex_forward(n, c, x.data_ptr(), t.data_ptr(), None if w is None else w.data_ptr(), eps, REDUCE[reduction], ignore,
                                 grad.data_ptr(), acc.data_ptr(), loss.data_ptr(), _stream()) == 0
    gy = torch.ones_like(loss) if gy is None else gy
    out = torch.empty_like(x)
    assert lib.pdf_ce_ex_backward(n, c, grad.data_ptr(), acc.data_ptr(), gy.data_ptr(), REDUCE[reduction], out.data_ptr(), _stream()) == 0
    return loss, out, grad


def abi_focal(lib, x, t, alpha_vec, alpha, gamma, reduction, ignore=IGNORE):
    n, c = x.shape
    grad, acc, loss, out = torch.empty_like(x), _acc(lib, c, x.device), torch.empty(1, device=x.device), torch.empty_like(x)
    assert lib.pdf_focal_forward(n, c, x.data_ptr(), t.data_ptr(), None if alpha_vec is None else alpha_vec.data_ptr(), alpha, gamma,
                                 REDUCE[reduction], ignore, grad.data_ptr(), acc.data_ptr(), loss.data_ptr(), _stream()) == 0
    gy = torch.ones(1, device=x.device)
    assert lib.pdf_focal_backward(n, c, grad.data_ptr(), acc.data_ptr(), gy.data_ptr(), out.data_ptr(), _stream()) == 0
    return loss, out, grad


def abi_dice(lib, x, t, smooth, exponent, ignore=IGNORE):
    n, c = x.shape
    prob, acc, loss, out = torch.empty_like(x), _acc(lib, c, x.device), torch.empty(1, device=x.device), torch.empty_like(x)
    assert lib.pdf_dice_forward(n, c, x.data_ptr(), t.data_ptr(), smooth, exponent, ignore, prob.data_ptr(), acc.data_ptr(), loss.data_ptr(),
                                _stream()) == 0
    gy = torch.ones(1, device=x.device)
    assert lib.pdf_dice_backward(n, c, prob.data_ptr(), t.data_ptr(), ignore, exponent, acc.data_ptr(), gy.data_ptr(), out.data_ptr(),
                                 _stream()) == 0
    return loss, out, prob


def abi_bfocal(lib, x, t, alpha, gamma, logits, reduce):
    n = x.shape[0]
    grad, acc, out = torch.empty_like(x), _acc(lib, 1, x.device), torch.empty_like(x)
    loss = torch.empty(1 if reduce else n, device=x.device)
    assert lib.pdf_bfocal_forward(n, x.data_ptr(), t.data_ptr(), alpha, gamma, int(logits), int(reduce), grad.data_ptr(), acc.data_ptr(),
                                  loss.data_ptr(), _stream()) == 0
    gy = torch.ones_like(loss)
    assert lib.pdf_bfocal_backward(n, grad.data_ptr(), acc.data_ptr(), gy.data_ptr(), int(reduce), out.data_ptr(), _stream()) == 0
    return loss, out, grad


def ten(module, x, t):
    """Ten evaluations of module(x, t) + backward with other device work in between -> the first result, all bit-identical."""
    other = torch.randn(1 << 18, device="cuda")
    got = []
    for i in range(10):
        loss, grad = cc.loss_and_grad(module, x, t)
        got.append((loss.clone(), grad.clone()))
        if i % 2:
            other = torch.sort(other * 1.0001)[0] + other.flip(0).cumsum(0)[-1] * 0
    torch.cuda.synchronize()
    assert all(torch.equal(a[0], got[0][0]) and torch.equal(a[1], got[0][1]) for a in got[1:])
    return got[0]


def test_modules_equal_the_abi_and_ten_evaluations_are_bit_identical(backend):
    from pointcloudpdf_amd import losses, segmentor

    lib = backend.lib
    _, kw, x, t = make_shape("ce_n300001_c3")
    x, t = x.cuda(), t.cuda()
    w = torch.tensor(kw["weight"], device="cuda")
    loss, grad = ten(segmentor.CrossEntropyLoss(weight=kw["weight"], label_smoothing=0.1, loss_weight=0.5), x, t)
    raw = abi_ce(lib, x, t, w, 0.1, "mean")
    assert float(loss) == 0.5 * float(raw[0]) and torch.equal(grad, raw[1] * 0.5)
    _, kw, x65, t65 = make_shape("ce_n257_c65")
    loss, grad = ten(segmentor.CrossEntropyLoss(weight=kw["weight"], reduction="none"), x65.cuda(), t65.cuda())
    raw = abi_ce(lib, x65.cuda(), t65.cuda(), torch.tensor(kw["weight"], device="cuda"), 0.0, "none")
    assert torch.equal(loss, raw[0]) and torch.equal(grad, raw[1])
    loss, grad = ten(losses.FocalLoss(gamma=1.5, alpha=0.25, loss_weight=0.5), x, t)
    raw = abi_focal(lib, x, t, None, 0.25, 1.5, "mean")
    assert float(loss) == 0.5 * float(raw[0]) and torch.equal(grad, raw[1] * 0.5)
    loss, grad = ten(losses.DiceLoss(smooth=0.5, exponent=3, loss_weight=0.5), x, t)
    raw = abi_dice(lib, x, t, 0.5, 3.0)
    assert float(loss) == 0.5 * float(raw[0]) and torch.equal(grad, raw[1] * 0.5)
    _, _, xb, tb = make_shape("bfocal_n300001_soft")
    loss, grad = ten(losses.BinaryFocalLoss(gamma=1.5, alpha=0.25, loss_weight=0.5), xb.cuda(), tb.cuda())
    raw = abi_bfocal(lib, xb.cuda(), tb.cuda(), 0.25, 1.5, True, True)
    assert float(loss) == 0.5 * float(raw[0]) and torch.equal(grad, raw[1] * 0.5)
    # under autocast the nodes keep fp32 tensors
    with torch.autocast("cuda", dtype=torch.bfloat16):
        xa = x.clone().requires_grad_()
        out = losses.FocalLoss(gamma=1.5, alpha=0.25, loss_weight=0.5)(xa, t)
    assert out.dtype == torch.float32 and float(out) == 0.5 * float(abi_focal(lib, x, t, None, 0.25, 1.5, "mean")[0])


def test_bad_labels_and_refused_arguments(backend):
    from pointcloudpdf_amd import losses, segmentor

    lib = backend.lib
    _, kw, x, t = make_shape("ce_n257_c13")
    x, t = x.cuda(), t.cuda()
    for bad in (13, -7):
        tb = t.clone()
        tb[200] = bad
        assert torch.isnan(segmentor.CrossEntropyLoss(weight=kw["weight"])(x, tb)).item()
        rows = segmentor.CrossEntropyLoss(weight=kw["weight"], reduction="none")(x, tb)
        assert torch.isnan(rows[200]).item() and int(torch.isnan(rows).sum()) == 1
        assert torch.isnan(losses.FocalLoss()(x, tb)).item()
        clamped = t.clone()
        clamped[200] = 12 if bad > 0 else 0
        assert torch.equal(losses.DiceLoss()(x, tb), losses.DiceLoss()(x, clamped))
    # every row ignored: focal and dice give 0 with a zero gradient, the mean cross-entropy NaN (torch's rule)
    none = torch.full_like(t, IGNORE)
    for crit in (losses.FocalLoss(), losses.FocalLoss(reduction="sum"), losses.DiceLoss()):
        loss, grad = cc.loss_and_grad(crit, x, none)
        assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0
    assert torch.isnan(segmentor.CrossEntropyLoss(label_smoothing=0.1)(x, none)).item()
    # null or mis-sized arguments are refused before a launch
    p, q = x.data_ptr(), t.data_ptr()
    assert lib.pdf_criteria_workspace_floats(0) == 0
    assert lib.pdf_ce_ex_forward(0, 13, p, q, None, 0.0, 1, IGNORE, p, p, p, None) == -1
    assert lib.pdf_ce_ex_forward(4, 0, p, q, None, 0.0, 1, IGNORE, p, p, p, None) == -1
    assert lib.pdf_ce_ex_forward(4, 13, p, None, None, 0.0, 1, IGNORE, p, p, p, None) == -1
    assert lib.pdf_ce_ex_forward(4, 13, p, q, None, 1.5, 1, IGNORE, p, p, p, None) == -1
    assert lib.pdf_ce_ex_forward(4, 13, p, q, None, 0.0, 3, IGNORE, p, p, p, None) == -1
    assert lib.pdf_ce_ex_backward(4, 13, p, p, None, 1, p, None) == -1
    assert lib.pdf_focal_forward(4, 13, p, q, None, 0.5, 2.0, 0, IGNORE, p, p, p, None) == -1     # no elementwise focal loss
    assert lib.pdf_focal_forward(4, 13, None, q, None, 0.5, 2.0, 1, IGNORE, p, p, p, None) == -1
    assert lib.pdf_focal_backward(-1, 13, p, p, p, p, None) == -1
    assert lib.pdf_dice_forward(4, 13, p, q, 1.0, 0.0, IGNORE, p, p, p, None) == -1               # exponent must be positive
    assert lib.pdf_dice_forward(4, 13, p, q, 1.0, 2.0, IGNORE, None, p, p, None) == -1
    assert lib.pdf_dice_backward(4, 13, p, q, IGNORE, 2.0, None, p, p, None) == -1
    assert lib.pdf_bfocal_forward(0, p, p, 0.5, 2.0, 1, 1, p, p, p, None) == -1
    assert lib.pdf_bfocal_backward(4, p, p, None, 1, p, None) == -1
    with pytest.raises(ValueError):
        backend.ce_ex_forward(x, t, torch.ones(12, device="cuda"), 0.0, "mean", IGNORE)
    with pytest.raises(TypeError):
        backend.focal_forward(x.double(), t, 0.5, 2.0, "mean", IGNORE)
    with pytest.raises(ValueError):
        backend.dice_forward(x, t[:-1], 1.0, 2.0, IGNORE)
    with pytest.raises(ValueError):
        losses.FocalLoss(alpha=[0.5, 0.5])(x, t)


def test_double_backward_leaves_the_saved_buffers_untouched():
    from pointcloudpdf_amd import losses, segmentor

    _, kw, x, t = make_shape("ce_n257_c65")
    dt, w = t.cuda(), torch.tensor(kw["weight"], device="cuda")
    _, _, xb, tb = make_shape("bfocal_n257")
    nodes = [(x, lambda a: segmentor._FusedCEEx.apply(a, dt, w, 0.1, "mean", IGNORE)),
             (x, lambda a: segmentor._FusedCEEx.apply(a, dt, w, 0.0, "none", IGNORE).sum()),
             (x, lambda a: losses._FusedFocal.apply(a, dt, 0.5, 2.0, "mean", IGNORE)),
             (x, lambda a: losses._FusedDice.apply(a, dt, 1.0, 2.0, IGNORE)),
             (xb, lambda a: losses._FusedBinaryFocal.apply(a, tb.cuda(), 0.5, 2.0, True, True))]
    for inp, node in nodes:
        dx = inp.cuda().requires_grad_()
        out = node(dx)
        fn = out.grad_fn if type(out.grad_fn).__name__.startswith("_Fused") else out.grad_fn.next_functions[0][0]
        assert type(fn).__name__.startswith("_Fused")
        buffers = fn.saved_tensors                      # (the tensors themselves: still there after the graph is freed)
        saved = [s.clone() for s in buffers]
        (out * 3.0).backward(retain_graph=True)
        first = dx.grad.clone()
        dx.grad = None
        (out * 3.0).backward()
        assert torch.equal(dx.grad, first) and float(first.abs().max()) > 0
        # (bit patterns: the workspace's unused slots are never written and may hold anything, NaN patterns included)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(saved, buffers) if a.is_floating_point())


def test_plain_cross_entropy_still_runs_the_original_pass(backend, monkeypatch):
    """No weight, no smoothing, mean, C <= 64: ``pdf_ce_forward`` as before, bit-equal to the raw call of that entry."""
    from pointcloudpdf_amd import segmentor

    lib = backend.lib
    g = torch.Generator().manual_seed(77)
    x, t = (2.0 * torch.randn(1000, 13, generator=g)).cuda(), torch.randint(-1, 13, (1000,), generator=g).cuda()
    calls = {"plain": 0, "ex": 0}
    plain, ex = lib.pdf_ce_forward, backend._fn["ce_ex_forward"]
    assert backend._fn["ce_forward"] is plain   # (the launch path's table holds the library's own function objects)
    monkeypatch.setitem(backend._fn, "ce_forward", lambda *a: (calls.__setitem__("plain", calls["plain"] + 1), plain(*a))[1])
    monkeypatch.setitem(backend._fn, "ce_ex_forward", lambda *a: (calls.__setitem__("ex", calls["ex"] + 1), ex(*a))[1])
    loss, grad = cc.loss_and_grad(segmentor.CrossEntropyLoss(), x, t)
    assert calls == {"plain": 1, "ex": 0}
    dl, acc, out = torch.empty_like(x), torch.empty(int(lib.pdf_ce_workspace_floats()), device="cuda"), torch.empty(1, device="cuda")
    assert plain(1000, 13, x.data_ptr(), t.data_ptr(), IGNORE, dl.data_ptr(), acc.data_ptr(), out.data_ptr(), _stream()) == 0
    gy, raw = torch.ones(1, device="cuda"), torch.empty_like(x)
    assert lib.pdf_ce_backward(1000, 13, dl.data_ptr(), acc.data_ptr(), gy.data_ptr(), raw.data_ptr(), _stream()) == 0
    assert torch.equal(loss.reshape(1), out) and torch.equal(grad, raw)
    segmentor.CrossEntropyLoss(label_smoothing=0.1)(x, t)
    segmentor.CrossEntropyLoss()(torch.randn(8, 65, device="cuda"), t[:8])
    assert calls == {"plain": 1, "ex": 2}


def test_class_vectors_are_uploaded_eagerly_and_never_inside_a_capture(monkeypatch):
    from pointcloudpdf_amd import losses, segmentor

    _, kw, x, t = make_shape("ce_n257_c13")
    x, t = x.cuda(), t.cuda()
    for crit in (segmentor.CrossEntropyLoss(weight=kw["weight"]), losses.FocalLoss(alpha=kw["weight"])):
        assert crit.state_dict() == {}
        with monkeypatch.context() as m:   # (no capture is begun: the refusal comes before any device work)
            m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(RuntimeError, match="eager forward"):
                crit(x, t)
        eager = crit(x, t)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            captured = crit(x, t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def test_captured_step_with_the_new_criteria_is_one_graph_without_memset_nodes():
    """Weighted, smoothed CE + Focal + Dice in the model's and the recognizer's criteria: the step captures as ONE graph that holds no
    memset node; five replays equal five eager steps bit for bit; replays queued back to back equal synchronised ones."""
    from pointcloudpdf_amd import engine, synthetic
    from pointcloudpdf_amd.geometry import Geometry

    def crit(c):
        return [dict(type="CrossEntropyLoss", weight=[0.5 + k / c for k in range(c)], label_smoothing=0.1, loss_weight=1.0, ignore_index=-1),
                dict(type="FocalLoss", gamma=2.0, alpha=0.5, loss_weight=1.0, ignore_index=-1),
                dict(type="DiceLoss", smooth=1, exponent=2, loss_weight=1.0, ignore_index=-1)]

    dev = torch.device("cuda", 0)
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg50", in_channels=6, num_classes=13), criteria=crit(13)),
               recognizer=dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=crit(14), loss_weight=0.1,
                               step_loss_weight=False, num_classes=13, start_epoch=0, kp_ball_radius=0.1, kp_max_neighbor=64,
                               adaptive_radius=False, condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100,
                               slide_window=True))
    step = engine.build_open_seg_step(cfg).to(dev)
    synthetic.fill_parameters_deterministic(step, seed=3)
    step.train()
    batch = synthetic.make_batch([2500, 2100], first_scene_id=70, device=dev)
    geom = Geometry(batch["coord"], batch["offset"], batch["offset_host"]).precompute(**step.prepass_plan)
    state = {k: v.detach().clone() for k, v in step.state_dict().items()}
    params = [p for p in step.parameters() if p.requires_grad]

    def five(run, sync=True):
        step.load_state_dict(state)
        torch.cuda.manual_seed(7)       # the pseudo-label pass draws its seeds from the device generator
        res = []
        for _ in range(5):
            for p in params:
                p.grad = None
            out = run()
            if sync:
                torch.cuda.synchronize()
            res.append((out["loss"].detach().clone(), out["recognizer_loss"].detach().clone(), [p.grad.detach().clone() for p in params]))
        torch.cuda.synchronize()
        return res

    def eager_step():
        out = step(dict(batch, pdf_geometry=geom))
        out["loss"].backward()
        return out

    eager = five(eager_step)
    engine.release_autograd_state(step)
    cap = engine.CapturedStep(step, batch, geom=geom, debug_graph=True)
    assert cap.graph is not None and cap.graph2 is None and cap.segments is None
    census = cap.node_census()
    assert census["kernel"] > 300 and census["memset"] == 0, census
    replayed = five(lambda: cap(batch, geom))
    queued = five(lambda: cap(batch, geom), sync=False)
    assert float(eager[0][1]) > 0 and np.isfinite(float(eager[0][0]))
    for i, (a, b, q) in enumerate(zip(eager, replayed, queued)):
        for other, what in ((b, "replay"), (q, "back-to-back replay")):
            assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]), (what, i, float(a[0]), float(other[0]))
            bad = [j for j, (x, y) in enumerate(zip(a[2], other[2])) if not torch.equal(x, y)]
            assert not bad, (what, i, len(bad))
    engine.release_autograd_state(step)

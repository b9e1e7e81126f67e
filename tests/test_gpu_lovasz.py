"""GPU suite: the Lovasz-softmax pass of csrc/lovasz.hip, through the C ABI and through autograd.

Three comparisons, each with the bound its own error budget allows:
  * ``prob`` against torch.softmax on the device: 1e-6 absolute;
  * the sort / Jaccard / softmax-backward stages against ``losses.lovasz_softmax_reference(probas=prob, dtype=float64)`` evaluated on the
    CPU from the KERNEL's probabilities: the errors |fg - p| are exact IEEE operations on identical fp32 inputs, so both sides sort alike
    and break ties by row; only fp32 rounding of the final products remains -> 1e-5 of the largest magnitude at every shape;
  * end to end against the fp64 restatement from the logits: the loss (continuous under order swaps) within 1e-4 relative at every
    shape; the gradient within 1e-4 of its largest magnitude on the cases with N <= 300 whose errors are well separated (``GAP_ULP``: a
    swap of two near-equal errors moves an element by up to 1/G of the largest gradient, which is legitimate).
The restatement itself is pinned to the reference by tests/test_lovasz_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IGNORE = -1
TILE = 2048          # csrc/tile_sort.h: keys per sort tile
STAGE_TOL = 1e-5     # of the largest magnitude
E2E_TOL = 1e-4
GAP_ULP = 16

# name: (N, C, seed, options).  N: 1, 2, around the wave (63 / 64 / 65), 257, around a sort tile (2047 / 2048 / 2049), exactly two tiles,
# two tiles + 3, 20,000.
# options: absent = classes without a row, ignored = share of ignored rows, seen = class_seen, single = (class, row) with ONE
# foreground row, only = every row has this class
CASES = {
    "n1_c2": (1, 2, 31, {}),
    "n2_c2": (2, 2, 32, {}),
    "n63_c13": (63, 13, 133, {}),
    "n64_c14": (64, 14, 34, {"single": (3, 17)}),
    "n65_c20": (65, 20, 35, {"absent": (0, 19)}),
    "n257_c13_absent": (257, 13, 37, {"absent": (5, 9), "ignored": 0.1}),
    "n257_c64": (257, 64, 37, {}),
    "n300_c14_only": (300, 14, 1138, {"only": 6}),
    "n2047_c13": (TILE - 1, 13, 45, {}),
    "n2048_c13": (TILE, 13, 46, {}),
    "n2049_c13_ignored": (TILE + 1, 13, 39, {"ignored": 0.1}),
    "n4096_c3_ignored": (2 * TILE, 3, 47, {"ignored": 0.1}),
    "n4099_c14_seen": (2 * TILE + 3, 14, 40, {"seen": (0, 2, 3, 7, 13), "ignored": 0.1}),
    "n4099_c64": (2 * TILE + 3, 64, 41, {"absent": (11,)}),
    "n20000_c20": (20000, 20, 42, {"ignored": 0.1, "absent": (17,), "single": (4, 12345)}),
    "n20000_c2": (20000, 2, 43, {}),
    "n300_c13_all_ignored": (300, 13, 44, {"ignored": 1.0}),
}
# every case with N <= 300 but the all-ignored one (its gradient is zero: nothing to scale by); n257_c64 is the one on the 64-column
# instantiations of the row kernels
E2E_GRAD_CASES = ["n1_c2", "n2_c2", "n63_c13", "n64_c14", "n65_c20", "n257_c13_absent", "n257_c64", "n300_c14_only"]


def make_case(name):
    n, c, seed, opt = CASES[name]
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(n, c, generator=g)
    single = opt.get("single")
    absent = set(opt.get("absent", ())) | ({single[0]} if single else set())
    present = torch.tensor([k for k in range(c) if k not in absent])
    labels = present[torch.randint(0, len(present), (n,), generator=g)]
    if "only" in opt:
        labels[:] = opt["only"]
    share = opt.get("ignored", 0.0)
    if share > 0:
        labels[torch.randperm(n, generator=g)[: max(1, int(round(share * n)))]] = IGNORE
    if single:
        labels[single[1]] = single[0]
    return logits, labels, (list(opt["seen"]) if "seen" in opt else None)


def run_abi(logits, labels, seen=None, ignore=IGNORE):
    """One call of pdf_lovasz_forward on the current stream -> prob, dlogits, [loss, classes] (device tensors)."""
    from pointcloudpdf_amd import _native

    lib = _native.hip_backend().lib
    n, c = logits.shape
    prob, dlogits = torch.empty_like(logits), torch.empty_like(logits)
    out = torch.empty(2, device=logits.device)
    ws = torch.empty(int(lib.pdf_lovasz_workspace_bytes(n, c)), dtype=torch.uint8, device=logits.device)
    mask = None
    if seen is not None:
        mask = torch.zeros(c, dtype=torch.uint8)
        mask[seen] = 1
        mask = mask.to(logits.device)
    rc = lib.pdf_lovasz_forward(n, c, logits.data_ptr(), labels.data_ptr(), ignore, mask.data_ptr() if mask is not None else None,
                                prob.data_ptr(), dlogits.data_ptr(), out.data_ptr(), ws.data_ptr(), ctypes.c_void_p(_native.raw_stream()))
    assert rc == 0, rc
    return prob, dlogits, out


def softmax_backward64(p, g):
    return p * (g - (g * p).sum(1, keepdim=True))


@pytest.fixture(scope="module")
def results():
    """Every case once: inputs, the kernel's outputs (copied to the host) and the two fp64 references.  Shared, read-only."""
    from pointcloudpdf_amd import losses

    res = {}
    for name in CASES:
        logits, labels, seen = make_case(name)
        dl, dy = logits.cuda(), labels.cuda()
        prob, dlogits, out = run_abi(dl, dy, seen)
        soft = torch.softmax(dl, 1)
        torch.cuda.synchronize()
        prob, dlogits, out, soft = prob.cpu(), dlogits.cpu(), out.cpu(), soft.cpu()
        # (a) from the kernel's own probabilities
        p32 = prob.clone().requires_grad_()
        stage_loss = losses.lovasz_softmax_reference(None, labels, IGNORE, seen, probas=p32, dtype=torch.float64)
        stage_loss.backward()
        stage_grad = softmax_backward64(prob.double(), p32.grad.double())
        # (b) from the logits, all in fp64
        x64 = logits.double().requires_grad_()
        e2e_loss = losses.lovasz_softmax_reference(x64, labels, IGNORE, seen)
        e2e_loss.backward()
        res[name] = dict(logits=logits, labels=labels, seen=seen, prob=prob, dlogits=dlogits, out=out, soft=soft,
                         stage_loss=float(stage_loss.detach()), stage_grad=stage_grad, e2e_loss=float(e2e_loss.detach()), e2e_grad=x64.grad)
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_probabilities_equal_torch_softmax(results, name):
    r = results[name]
    err = float((r["prob"] - r["soft"]).abs().max())
    print(name, "prob abs err", err)
    assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("name", list(CASES))
def test_sort_and_jaccard_stage_from_the_kernels_probabilities(results, name):
    r = results[name]
    labels, c = r["labels"], r["logits"].shape[1]
    kept = labels[labels != IGNORE]
    classes = [k for k in kept.unique().tolist() if r["seen"] is None or k in r["seen"]]
    assert float(r["out"][1]) == len(classes), (name, float(r["out"][1]), classes)
    scale = float(r["stage_grad"].abs().max())
    if not classes:                                              # every row ignored: exactly zero
        assert float(r["out"][0]) == 0.0 and not r["dlogits"].any()
        return
    e_loss = abs(float(r["out"][0]) - r["stage_loss"]) / abs(r["stage_loss"])
    e_grad = float((r["dlogits"].double() - r["stage_grad"]).abs().max()) / scale
    print(name, "stage loss err", e_loss, "grad err", e_grad, "classes", len(classes), "of", c)
    assert e_loss <= STAGE_TOL and e_grad <= STAGE_TOL, (name, e_loss, e_grad)
    assert not r["dlogits"][labels == IGNORE].any()              # ignored rows: exactly zero


@pytest.mark.parametrize("name", list(CASES))
def test_loss_end_to_end_from_the_logits(results, name):
    r = results[name]
    if r["e2e_loss"] == 0.0:
        assert float(r["out"][0]) == 0.0
        return
    err = abs(float(r["out"][0]) - r["e2e_loss"]) / abs(r["e2e_loss"])
    print(name, "e2e loss err", err)
    assert err <= E2E_TOL, (name, err)


def ulp32(x):
    x = x.float()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def assert_errors_are_separated(logits, labels):
    """The condition under which the order -- and so the gradient -- of the fp64 restatement is the kernel's: inside every class
    consecutive sorted errors differ by more than GAP_ULP ulp (fp32) -- of the error, and on a foreground row also of the probability
    1 - e it is formed from, whose own rounding is what moves it."""
    p = torch.softmax(logits.double(), 1)[labels != IGNORE]
    lab = labels[labels != IGNORE]
    for k in lab.unique().tolist():
        fg = lab == k
        e, order = torch.sort((fg.double() - p[:, k]).abs(), descending=True, stable=True)
        if e.numel() < 2:
            continue
        unit = torch.where(fg[order], torch.maximum(ulp32(e), ulp32(1.0 - e)), ulp32(e))
        gap = e[:-1] - e[1:]
        assert bool((gap > GAP_ULP * torch.maximum(unit[:-1], unit[1:])).all()), (k, float((gap / torch.maximum(unit[:-1], unit[1:])).min()))


@pytest.mark.parametrize("name", E2E_GRAD_CASES)
def test_gradient_end_to_end_on_well_separated_cases(results, name):
    r = results[name]
    assert r["logits"].shape[0] <= 300
    assert_errors_are_separated(r["logits"], r["labels"])
    err = float((r["dlogits"].double() - r["e2e_grad"]).abs().max()) / float(r["e2e_grad"].abs().max())
    print(name, "e2e grad err", err)
    assert err <= E2E_TOL, (name, err)


def test_ties_and_saturation_follow_the_stable_order():
    """Blocks of identical rows (equal errors in every class: the order inside a block is the rows' own) and logits of +-120 (p is
    exactly 0 or 1: e == 0 on the rows that are right, where |.| has gradient 0; e == 1 on the rows that are wrong)."""
    from pointcloudpdf_amd import losses

    g = torch.Generator().manual_seed(50)
    n, c = 2 * TILE + 77, 13
    base = 2.0 * torch.randn(97, c, generator=g)
    logits = base[torch.arange(n) % 97].clone()                 # every row ~43 times, 97 rows apart: ties across waves and tiles
    labels = torch.randint(0, c, (97,), generator=g)[torch.arange(n) % 97].clone()
    labels[torch.randperm(n, generator=g)[:400]] = IGNORE
    sat = torch.randperm(n, generator=g)[:600]
    hot = torch.randint(0, c, (600,), generator=g)
    logits[sat] = -120.0
    logits[sat, hot] = 120.0
    wrong = sat[:200]
    labels[wrong] = (hot[:200] + 1) % c                           # saturated on another class: e == 1 twice per row
    labels[sat[200:]] = hot[200:]                                 # saturated and right: e == 0 in every class
    prob, dlogits, out = run_abi(logits.cuda(), labels.cuda())
    torch.cuda.synchronize()
    prob, dlogits, out = prob.cpu(), dlogits.cpu(), out.cpu()
    assert set(prob[sat].unique().tolist()) == {0.0, 1.0}
    p32 = prob.clone().requires_grad_()
    want = losses.lovasz_softmax_reference(None, labels, IGNORE, probas=p32, dtype=torch.float64, stable=True)
    want.backward()
    dprob = p32.grad.double()
    ref = softmax_backward64(prob.double(), dprob)
    e_loss = abs(float(out[0]) - float(want.detach())) / float(want.detach())
    e_grad = float((dlogits.double() - ref).abs().max()) / float(ref.abs().max())
    print("ties: loss err", e_loss, "grad err", e_grad)
    assert e_loss <= STAGE_TOL and e_grad <= STAGE_TOL, (e_loss, e_grad)
    # e == 0: the gradient is exactly zero (rows that are saturated and right have e == 0 in every class)
    right = sat[200:]
    right = right[labels[right] != IGNORE]
    assert len(right) > 300 and not dlogits[right].any() and not dprob[right].any()


def test_bad_label_poisons_the_loss_and_bad_arguments_are_refused():
    from pointcloudpdf_amd import _native

    lib = _native.hip_backend().lib
    logits, labels, _ = make_case("n257_c13_absent")
    labels = labels.clone()
    labels[200] = 13
    _, _, out = run_abi(logits.cuda(), labels.cuda())
    assert torch.isnan(out[0]).item()
    labels[200] = -7
    _, _, out = run_abi(logits.cuda(), labels.cuda())
    assert torch.isnan(out[0]).item()
    x = torch.zeros(4, 65, device="cuda")
    assert lib.pdf_lovasz_workspace_bytes(4, 65) == 0 and lib.pdf_lovasz_workspace_bytes(0, 13) == 0
    args = (x.data_ptr(), x.data_ptr(), IGNORE, None, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None)
    assert lib.pdf_lovasz_forward(4, 65, *args) == -3          # C > 64
    assert lib.pdf_lovasz_forward(0, 13, *args) == -1          # n < 1
    assert lib.pdf_lovasz_forward(4, 13, x.data_ptr(), None, IGNORE, None, x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None) == -1


def test_module_equals_the_abi_and_ten_evaluations_are_bit_identical(results):
    from pointcloudpdf_amd import losses

    name = "n4099_c14_seen"
    r = results[name]
    loss = losses.LovaszLoss(mode="multiclass", class_seen=r["seen"], ignore_index=IGNORE, loss_weight=0.5)
    dl, dy = r["logits"].cuda(), r["labels"].cuda()
    other = torch.randn(1 << 18, device="cuda")
    got = []
    for i in range(10):
        x = dl.clone().requires_grad_()
        out = loss(x, dy)
        out.backward()
        got.append((out.detach().clone(), x.grad.clone()))
        if i % 2:                                               # other device work on the stream in between
            other = torch.sort(other * 1.0001)[0] + other.flip(0).cumsum(0)[-1] * 0
    torch.cuda.synchronize()
    assert all(torch.equal(a[0], got[0][0]) and torch.equal(a[1], got[0][1]) for a in got[1:])
    assert float(got[0][0]) == 0.5 * float(r["out"][0])
    assert torch.equal(got[0][1].cpu(), r["dlogits"] * 0.5)
    # under autocast the node keeps fp32 tensors
    with torch.autocast("cuda", dtype=torch.bfloat16):
        x = dl.clone().requires_grad_()
        out = loss(x, dy)
    out.backward()
    assert out.dtype == torch.float32 and torch.equal(out.detach(), got[0][0]) and torch.equal(x.grad, got[0][1])


def test_class_mask_is_uploaded_eagerly_and_never_inside_a_capture(results, monkeypatch):
    """``class_seen`` reaches the kernel as a byte mask uploaded on first use: a first use while the stream captures is refused (a
    host-to-device copy must not be recorded), after one eager forward the cached mask serves captures."""
    from pointcloudpdf_amd import losses

    r = results["n4099_c14_seen"]
    dl, dy = r["logits"].cuda(), r["labels"].cuda()
    loss = losses.LovaszLoss(mode="multiclass", class_seen=r["seen"], ignore_index=IGNORE)
    with monkeypatch.context() as m:   # (no capture is begun: the refusal comes before any device work)
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="eager forward"):
            loss(dl, dy)
    eager = loss(dl, dy)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = loss(dl, dy)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager) and float(eager) == float(r["out"][0])


def test_double_backward_leaves_the_saved_buffer_untouched(results):
    from pointcloudpdf_amd import losses

    r = results["n2049_c13_ignored"]
    x = r["logits"].cuda().requires_grad_()
    out = losses.LovaszLoss(mode="multiclass", ignore_index=IGNORE)(x, r["labels"].cuda()) * 3.0
    out.backward(retain_graph=True)
    first = x.grad.clone()
    x.grad = None
    out.backward()
    assert torch.equal(x.grad, first) and torch.equal(first.cpu(), r["dlogits"] * 3.0)


def test_captured_step_with_both_criteria_is_one_graph_without_memset_nodes():
    """CE + Lovasz in the model's and the recognizer's criteria (the reference's recipes): the step captures as ONE graph that holds no
    memset node; five replays equal five eager steps bit for bit; replays queued back to back equal synchronised ones."""
    from pointcloudpdf_amd import engine, synthetic
    from pointcloudpdf_amd.geometry import Geometry

    dev = torch.device("cuda", 0)
    crit = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
            dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg50", in_channels=6, num_classes=13), criteria=crit),
               recognizer=dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=crit, loss_weight=0.1,
                               step_loss_weight=False, num_classes=13, start_epoch=0, kp_ball_radius=0.1, kp_max_neighbor=64,
                               adaptive_radius=False, condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100,
                               slide_window=True))
    step = engine.build_open_seg_step(cfg).to(dev)
    synthetic.fill_parameters_deterministic(step, seed=3)
    step.train()
    assert step.recognizer.pseudo_mask_fn.capturable
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

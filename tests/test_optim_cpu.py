"""CPU suite of pointcloudpdf_amd/optim.py: FusedAdamW's checkpoint layout against torch.optim.AdamW, the parameter groups and the
schedulers the builders make from the reference's config dicts, the refused options, and the argument validation of the new C entries
(no launch, no GPU).  The arithmetic of the kernel is a GPU test (tests/test_gpu_optim.py)."""
import copy
import ctypes
import math
import types

import pytest
import torch


class _Lib:
    def pdf_sgd_chunk(self):
        return 4096


def _stub():
    return types.SimpleNamespace(lib=_Lib())


def test_fused_adamw_state_dict_round_trip():
    """FusedAdamW's checkpoint in torch.optim.AdamW and back: same param-group keys, same state keys; the torch optimizer loaded from our
    checkpoint takes the step AdamW's formulas give from our moments and step counts."""
    from pointcloudpdf_amd import engine, optim

    assert engine.FusedAdamW is optim.FusedAdamW and engine.FusedAdam is optim.FusedAdam
    g = torch.Generator().manual_seed(0)
    shapes = [(5,), (3, 4), (17,)]
    pa = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    lr, b1, b2, eps, wd = 0.005, 0.9, 0.99, 1e-8, 0.02
    fused = optim.FusedAdamW(pa, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, backend=_stub())
    ref = torch.optim.AdamW(pb, lr=1.0, betas=(0.5, 0.5), weight_decay=0.5)
    assert set(fused.param_groups[0]) == set(ref.param_groups[0])
    for k, p in enumerate(pa):
        st = fused.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].dtype == torch.float32 and st["step"].dim() == 0
        st["step"].fill_(3 + k)
        st["exp_avg"].copy_(torch.randn(p.shape, generator=g))
        st["exp_avg_sq"].copy_(torch.rand(p.shape, generator=g))
    ref.load_state_dict(copy.deepcopy(fused.state_dict()))
    grp = ref.param_groups[0]
    assert grp["lr"] == lr and grp["betas"] == (b1, b2) and grp["eps"] == eps and grp["weight_decay"] == wd
    assert not grp["amsgrad"] and not grp["maximize"] and grp.get("decoupled_weight_decay", True)
    grads = [torch.randn(p.shape, generator=g) for p in pb]
    for p, gr in zip(pb, grads):
        p.grad = gr.clone()
    ref.step()
    for k, (x, y, gr) in enumerate(zip(pa, pb, grads)):
        st, step = fused.state[x], 4 + k
        m = st["exp_avg"].double() * b1 + (1 - b1) * gr.double()
        v = st["exp_avg_sq"].double() * b2 + (1 - b2) * gr.double() ** 2
        want = x.detach().double() * (1 - lr * wd) - lr / (1 - b1 ** step) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
        assert torch.allclose(y.detach().double(), want, rtol=1e-6, atol=1e-7)
        assert float(ref.state[y]["step"]) == step
    # and back: torch.optim.AdamW's checkpoint in FusedAdamW
    fused2 = optim.FusedAdamW([torch.nn.Parameter(p.detach().clone()) for p in pb], lr=9.0, betas=(0.1, 0.2), weight_decay=0.0, backend=_stub())
    fused2.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert fused2.param_groups[0]["lr"] == lr and fused2.param_groups[0]["betas"] == (b1, b2) and fused2.param_groups[0]["weight_decay"] == wd
    assert set(fused2.param_groups[0]) == set(ref.param_groups[0])
    for q, y in zip(fused2.param_groups[0]["params"], pb):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(fused2.state[q][key], ref.state[y][key])
        assert float(fused2.state[q]["step"]) == float(ref.state[y]["step"])
    # the table of a step: state is normalised to {float32, the parameter's device, 0-dim step} and laid out as the kernel's 64-byte record
    q0 = fused2.param_groups[0]["params"][0]
    fused2.state[q0]["step"] = torch.tensor(7, dtype=torch.int64)
    fused2.state[q0]["exp_avg"] = fused2.state[q0]["exp_avg"].double()
    ps = fused2.param_groups[0]["params"]
    rows = torch.zeros((len(ps), fused2.COLS), dtype=torch.int64).numpy()
    fused2._state_columns(rows, ps)
    st = fused2.state[q0]
    assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 7.0 and st["exp_avg"].dtype == torch.float32
    assert fused2.COLS == 8 and rows[0, 2] == st["exp_avg"].data_ptr() and rows[0, 3] == st["exp_avg_sq"].data_ptr() and rows[0, 4] == st["step"].data_ptr()
    # FusedAdam: torch.optim.Adam's keys, the L2 form
    adam = optim.FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, weight_decay=0.1, backend=_stub())
    tadam = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, weight_decay=0.1)
    assert set(adam.param_groups[0]) == set(tadam.param_groups[0]) and not adam.param_groups[0]["decoupled_weight_decay"]


def test_fused_sgd_rides_on_the_shared_base():
    from pointcloudpdf_amd import engine, optim

    assert issubclass(engine.FusedSGD, optim.FusedOptimizer) and issubclass(optim.FusedAdamW, optim.FusedOptimizer)
    sgd = engine.FusedSGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, backend=_stub())
    adam = optim.FusedAdamW([torch.nn.Parameter(torch.zeros(3))], backend=_stub())
    assert sgd.COLS == 4 and sgd.UNSCALE == "pdf_grad_unscale" and adam.UNSCALE == "pdf_adam_grad_unscale"
    assert all(t.shape == (1, 4) for t in sgd._tabs) and all(t.shape == (1, 8) for t in adam._tabs)
    with pytest.raises(TypeError, match="DeviceGradScaler drives"):
        engine.DeviceGradScaler("cpu").unscale_(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))]))


def _first_match(named, keywords):
    out = [[] for _ in range(len(keywords) + 1)]
    for n, p in named:
        for i, kw in enumerate(keywords):
            if kw in n:
                out[i + 1].append(n)
                break
        else:
            out[0].append(n)
    return out


def test_build_optimizer_groups_follow_the_first_matching_keyword():
    """configs/s3dis/openseg-st-v1m1-0-origin-*.py: AdamW lr 0.006 with param_dicts = [dict(keyword="blocks", lr=0.0006)]."""
    from pointcloudpdf_amd import engine, optim

    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008)
    frozen = [n for n, _ in step.named_parameters()][3::11]
    for n, p in step.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    opt = optim.build_optimizer(dict(type="AdamW", lr=0.006, weight_decay=0.05), step, param_dicts=[dict(keyword="blocks", lr=0.0006)])
    assert type(opt) is optim.FusedAdamW and len(opt.param_groups) == 2
    names = {id(p): n for n, p in step.named_parameters()}
    got = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    want = _first_match([(n, p) for n, p in step.named_parameters() if p.requires_grad], ["blocks"])
    assert got == want and want[0] and want[1]
    flat = [n for g in got for n in g]
    assert len(flat) == len(set(flat)) and not set(flat) & set(frozen)
    assert set(flat) | set(frozen) == {n for n, _ in step.named_parameters()}
    assert [g["lr"] for g in opt.param_groups] == [0.006, 0.0006]
    assert all(g["weight_decay"] == 0.05 and g["betas"] == (0.9, 0.999) for g in opt.param_groups)
    # several entries: the first keyword that matches wins; momentum / weight_decay of an entry are the group's own
    net = torch.nn.Sequential()
    net.add_module("blocks", torch.nn.Linear(2, 2))
    net.add_module("head", torch.nn.Linear(2, 2))
    net.add_module("blocks_head", torch.nn.Linear(2, 2))
    opt = optim.build_optimizer(dict(type="SGD", lr=0.5, momentum=0.9, weight_decay=1e-4), net,
                                param_dicts=[dict(keyword="head", lr=0.1, momentum=0.8), dict(keyword="blocks", weight_decay=0.0)])
    assert type(opt) is engine.FusedSGD
    names = {id(p): n for n, p in net.named_parameters()}
    got = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert got == _first_match(list(net.named_parameters()), ["head", "blocks"]) == [[], ["head.weight", "head.bias", "blocks_head.weight", "blocks_head.bias"],
                                                                                      ["blocks.weight", "blocks.bias"]]
    assert [(g["lr"], g["momentum"], g["weight_decay"]) for g in opt.param_groups] == [(0.5, 0.9, 1e-4), (0.1, 0.8, 1e-4), (0.5, 0.9, 0.0)]
    # no param_dicts: one group of the trainable parameters; the names the reference registers
    net.head.bias.requires_grad_(False)
    opt = optim.build_optimizer(dict(type="Adam", lr=1e-3), net)
    assert type(opt) is optim.FusedAdam and len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 5
    assert all(p is not net.head.bias for p in opt.param_groups[0]["params"])
    with pytest.raises(KeyError, match="Lion"):
        optim.build_optimizer(dict(type="Lion", lr=1e-3), net)


def _lrs(sched, opt, steps, key="lr"):
    out = []
    for _ in range(steps):
        out.append([g[key] for g in opt.param_groups])
        opt.step()
        sched.step()
    return out


def _plain(lr=0.5):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=lr, momentum=0.9)


def test_build_scheduler_matches_torch_and_the_reference_formulas():
    from pointcloudpdf_amd import optim

    T = 200
    L = torch.optim.lr_scheduler
    # the three that are torch's own classes
    a, b = _plain(), _plain()
    assert _lrs(optim.build_scheduler(dict(type="MultiStepLR", milestones=[0.6, 0.8], gamma=0.1), a, T), a, T) == \
        _lrs(L.MultiStepLR(b, milestones=[0.6 * T, 0.8 * T], gamma=0.1), b, T)
    a, b = _plain(), _plain()
    assert _lrs(optim.build_scheduler(dict(type="CosineAnnealingLR", eta_min=1e-5), a, T), a, T) == _lrs(L.CosineAnnealingLR(b, T_max=T, eta_min=1e-5), b, T)
    a, b = _plain(), _plain()
    assert _lrs(optim.build_scheduler(dict(type="CosineAnnealingLR"), a, T), a, T) == _lrs(L.CosineAnnealingLR(b, T_max=T, eta_min=0), b, T)
    # OneCycleLR on a fused AdamW with two groups (config 5's max_lr list): lr AND betas[0] move
    cfg4 = dict(type="OneCycleLR", max_lr=[0.005, 0.0005], pct_start=0.05, anneal_strategy="cos", div_factor=10.0, final_div_factor=1000.0)
    pa = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
    pb = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
    a = optim.FusedAdamW([dict(params=pa[:1]), dict(params=pa[1:], lr=0.0005)], lr=0.005, weight_decay=0.02, backend=types.SimpleNamespace(lib=_Lib()))
    b = torch.optim.AdamW([dict(params=pb[:1]), dict(params=pb[1:], lr=0.0005)], lr=0.005, weight_decay=0.02)
    sa = optim.build_scheduler(cfg4, a, T)
    sb = L.OneCycleLR(b, max_lr=[0.005, 0.0005], total_steps=T, pct_start=0.05, anneal_strategy="cos", div_factor=10.0, final_div_factor=1000.0)
    seq_a, seq_b = [], []
    for _ in range(T):
        seq_a.append([(g["lr"], g["betas"]) for g in a.param_groups])
        seq_b.append([(g["lr"], g["betas"]) for g in b.param_groups])
        a.step(); b.step()        # (no gradients: nothing to launch)
        sa.step(); sb.step()
    assert seq_a == seq_b
    assert min(x[0][1][0] for x in seq_a) == 0.85 and max(x[0][1][0] for x in seq_a) == 0.95 and seq_a[0][0][0] == pytest.approx(0.005 / 10.0, rel=1e-12)
    # the reference's defaults where the config leaves them out: pct_start 0.3, div 25, final_div 1e4, momentum 0.85 .. 0.95
    a, b = _plain(), _plain()
    assert _lrs(optim.build_scheduler(dict(type="OneCycleLR", max_lr=0.5), a, T), a, T) == \
        _lrs(L.OneCycleLR(b, max_lr=0.5, total_steps=T, pct_start=0.3, div_factor=25.0, final_div_factor=1e4, base_momentum=0.85, max_momentum=0.95), b, T)
    # the three LambdaLR forms: the closed formulas of pointcept/utils/scheduler.py
    base = 0.5

    def warm(s, milestones=(0.6, 0.8), gamma=0.1, rate=0.05, scale=1e-6):
        factor = 1.0
        for m in milestones:
            if s < m * T:
                break
            factor *= gamma
        w = 1 - (1 - s / rate / T) * (1 - scale) if s <= rate * T else 1.0
        return base * w * factor

    closed = {
        "MultiStepWithWarmupLR": (dict(milestones=[0.6, 0.8]), warm),
        "PolyLR": (dict(), lambda s: base * (1 - s / (T + 1)) ** 0.9),
        "ExpLR": (dict(), lambda s: base * 0.9 ** (s / T)),
    }
    for kind, (kw, formula) in closed.items():
        a = _plain(base)
        got = [x[0] for x in _lrs(optim.build_scheduler(dict(type=kind, **kw), a, T), a, T)]
        want = [formula(s) for s in range(T)]
        assert got == pytest.approx(want, rel=1e-12, abs=0), kind
    a = _plain(base)
    got = [x[0] for x in _lrs(optim.build_scheduler(dict(type="PolyLR", power=2.0), a, T), a, T)]
    assert got == pytest.approx([base * (1 - s / (T + 1)) ** 2.0 for s in range(T)], rel=1e-12)
    assert sorted(optim.SCHEDULERS) == ["CosineAnnealingLR", "ExpLR", "MultiStepLR", "MultiStepWithWarmupLR", "OneCycleLR", "PolyLR"]
    with pytest.raises(KeyError, match="StepLR"):
        optim.build_scheduler(dict(type="StepLR"), _plain(), T)


def test_unsupported_options_are_refused_not_ignored():
    from pointcloudpdf_amd import optim

    def make(**kw):
        p = torch.nn.Parameter(torch.zeros(4))
        p.grad = torch.zeros(4)
        return optim.FusedAdamW([p], lr=1e-3, backend=_stub(), **kw)

    for option in ("amsgrad", "maximize", "differentiable"):
        with pytest.raises(RuntimeError, match=option):
            make(**{option: True}).step()
        opt = make()
        opt.param_groups[0][option] = True      # (a loaded checkpoint can carry it)
        with pytest.raises(RuntimeError, match=option):
            opt.step()
    with pytest.raises(ValueError, match="beta parameter at index 0"):
        make(betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="beta parameter at index 1"):
        make(betas=(0.9, -0.1))
    with pytest.raises(ValueError, match="epsilon"):
        make(eps=-1e-8)
    with pytest.raises(ValueError, match="learning rate"):
        optim.FusedAdam([torch.nn.Parameter(torch.zeros(4))], lr=-1.0, backend=_stub())
    with pytest.raises(ValueError, match="weight_decay"):
        make(weight_decay=-0.1)
    with pytest.raises(TypeError, match="nonsense"):
        make(nonsense=1)


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import build

    return ctypes.CDLL(build.build_library())


def test_adam_entries_validate_arguments_without_a_gpu(lib):
    """pdf_adam_step / pdf_adam_grad_unscale: PDF_ERR_BAD_ARG before any launch, PDF_OK for an empty chunk list."""
    I, D, P = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    f = lib.pdf_adam_step
    f.restype = I
    f.argtypes = [I, I, P, P, D, D, D, D, D, I, P, P]
    buf = (ctypes.c_long * 64)()
    ptr = ctypes.cast(buf, P)
    good = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)

    def call(nchunks=1, ntensors=1, tab=ptr, chunks=ptr, decoupled=1, **kw):
        h = dict(good, **kw)
        return f(nchunks, ntensors, tab, chunks, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], decoupled, None, None)

    assert call(nchunks=0) == 0 and call(nchunks=0, ntensors=0, tab=None, chunks=None) == 0
    assert call(tab=None) == -1 and call(chunks=None) == -1 and call(nchunks=-1) == -1 and call(ntensors=0) == -1 and call(ntensors=-2) == -1
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=float("nan")), dict(eps=-1e-8), dict(lr=-1e-3),
                dict(lr=float("nan")), dict(wd=-0.1)):
        assert call(**bad) == -1, bad
        assert call(nchunks=0, **bad) == -1, bad      # (hyper-parameters are checked whether or not there is work)
    u = lib.pdf_adam_grad_unscale
    u.restype = I
    u.argtypes = [I, P, P, P, P, P]
    assert u(0, None, None, None, None, None) == 0
    assert u(1, None, ptr, ptr, ptr, None) == -1 and u(1, ptr, None, ptr, ptr, None) == -1 and u(1, ptr, ptr, None, ptr, None) == -1
    assert u(1, ptr, ptr, ptr, None, None) == -1 and u(-1, ptr, ptr, ptr, ptr, None) == -1
    from pointcloudpdf_amd import _native

    be = _native.HipBackend(lib)   # (binds every prototype, the new ones included; no GPU call)
    assert be.lib.pdf_adam_step.argtypes[4] is ctypes.c_double and _native.ABI_VERSION >= 7

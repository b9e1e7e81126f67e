"""GPU suite: the independent launches paired inside a Bottleneck's backward and a TransitionDown's forward.

  - csrc/rowlin.hip: pdf_rowlin_wgrad_group_dgrad -- the five grouped weight gradients and the input gradient gx (+)= dy W in ONE launch
    (rl2::k_wg_fwd) -- against pdf_rowlin_forward followed by pdf_rowlin_wgrad_group;
  - csrc/block.hip: pdf_bottleneck_backward, which issues that pair, with PDFOPS_PAIR unset and PDFOPS_PAIR=0 in one process;
  - csrc/transition_down.hip: pdf_td_forward, whose two Gram products share a launch (rl2::k_wg2_roww) and a slab reduction, likewise.

Every problem of a paired launch runs the body of its single launch over the grid of its single launch, so the bar is equality of bits
(torch.equal), not a tolerance.  The entry reports whether the product went out in the gradients' launch; every case states which it
expects, so a dispatch that always fell back would fail."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
NG = 5

# (c, n, mma_input, paired): VW = 2 with tail rows | VW = 4, slab product | group form, 12 tail rows | widest | past the group form's
# 16,384 rows: the product takes the slab form k_fwd<128, 4>, for which no pair is built -- a fallback | reduced-precision operands: fallback
CASES = [(32, 530, 0, 1), (64, 1000, 0, 1), (128, 780, 0, 1), (512, 300, 0, 1), (128, 17000, 0, 0), (128, 780, 1, 0)]


def _ptrs(tensors):
    return (P * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


@pytest.mark.parametrize("c,n,mma,want", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [1, 0])
def test_grouped_weight_gradients_with_the_input_gradient(c, n, mma, want, accumulate, monkeypatch):
    from pointcloudpdf_amd import _native

    lib = _native.hip_backend().lib
    gen = torch.Generator(device="cuda").manual_seed(c + n)
    st = torch.cuda.current_stream().cuda_stream
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    g = [rnd(n, c) for _ in range(NG)]
    x = [rnd(n, c) for _ in range(NG)]
    # the Bottleneck's prologues: four folded BatchNorm + ReLU, one identity
    scale = [rnd(c) for _ in range(NG - 1)] + [None]
    shift = [rnd(c) for _ in range(NG - 1)] + [None]
    relu = (ctypes.c_int * NG)(1, 1, 1, 1, 0)
    dy, w, gx0 = g[4], rnd(c, c), rnd(n, c)
    nws = int(lib.pdf_rowlin_wgrad_ws_floats(n, c, c, NG))

    def run(paired_entry):
        dw = [torch.full((c, c), float("nan"), device="cuda") for _ in range(NG)]
        db = [None] + [torch.full((c,), float("nan"), device="cuda") for _ in range(3)] + [None]
        ws = torch.full((nws,), float("nan"), device="cuda")
        gx = gx0.clone()
        took = ctypes.c_int(-1)
        tabs = (_ptrs(g), _ptrs(x), _ptrs(scale), _ptrs(shift), relu, _ptrs(dw), _ptrs(db))
        if paired_entry:
            assert lib.pdf_rowlin_wgrad_group_dgrad(n, c, c, NG, tabs[0], c, tabs[1], c, *tabs[2:], P(ws.data_ptr()), P(dy.data_ptr()),
                                                    P(w.data_ptr()), P(gx.data_ptr()), accumulate, ctypes.byref(took), mma, P(st)) == 0
        else:
            assert lib.pdf_rowlin_forward(n, c, c, P(dy.data_ptr()), c, P(w.data_ptr()), 1, None, None, None, 0, P(gx.data_ptr()), c, accumulate,
                                          None, mma, P(st)) == 0
            assert lib.pdf_rowlin_wgrad_group(n, c, c, NG, tabs[0], c, tabs[1], c, *tabs[2:], P(ws.data_ptr()), mma, P(st)) == 0
        torch.cuda.synchronize()
        return [gx] + dw + [b for b in db if b is not None], took.value

    ref, _ = run(False)
    new, took = run(True)
    assert took == want
    monkeypatch.setenv("PDFOPS_PAIR", "0")
    off, took_off = run(True)
    assert took_off == 0
    for got in (new, off):
        for a, b in zip(got, ref):
            assert torch.isfinite(b).all() and torch.equal(a, b), (a - b).abs().max().item()


# (cin, n): vector widths 2 + 2 | 4 + 2 with tail rows | 4 + 2, several row splits
@pytest.mark.parametrize("cin,n", [(32, 300), (64, 530), (256, 97), (128, 5000)])
def test_row_weighted_gram_pair_reports_one_launch(cin, n, monkeypatch):
    """The two Gram products of pdf_td_forward through pdf_rowlin_wgrad2_roww against two pdf_rowlin_wgrad_roww calls (one workspace, as
    the forward issued them before): the same bits, ONE product launch unless PDFOPS_PAIR=0 or the operands are reduced-precision."""
    from pointcloudpdf_amd import _native

    lib = _native.hip_backend().lib
    gen = torch.Generator(device="cuda").manual_seed(cin + n)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(n, cin, device="cuda", generator=gen)
    z = torch.randn(n, 32, device="cuda", generator=gen)
    z[:, 3] = torch.randint(0, 9, (n,), device="cuda", generator=gen).float()   # the row weight: a count
    ws_n = [int(lib.pdf_rowlin_wgrad_ws_floats(n, cin, o, 1)) for o in (cin, 32)]
    assert int(lib.pdf_td_fwd_scratch_floats(n, cin)) == sum(ws_n)
    roww = P(z.data_ptr() + 12)
    new = lambda: (torch.full((cin, cin), float("nan"), device="cuda"), torch.full((32, cin), float("nan"), device="cuda"),
                   torch.full((sum(ws_n) + 64,), float("nan"), device="cuda"))
    gxx0, gz0, ws0 = new()
    assert lib.pdf_rowlin_wgrad_roww(n, cin, cin, P(x.data_ptr()), cin, P(x.data_ptr()), cin, P(gxx0.data_ptr()), roww, 32, P(ws0.data_ptr()), 0, P(st)) == 0
    assert lib.pdf_rowlin_wgrad_roww(n, cin, 32, P(z.data_ptr()), 32, P(x.data_ptr()), cin, P(gz0.data_ptr()), None, 0, P(ws0.data_ptr()), 0, P(st)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gxx0).all() and torch.isfinite(gz0).all()

    def pair(mma):
        gxx, gz, ws = new()
        took = ctypes.c_int(-1)
        tab = (P * 10)(x.data_ptr(), x.data_ptr(), gxx.data_ptr(), None, ws.data_ptr(),
                       z.data_ptr(), x.data_ptr(), gz.data_ptr(), None, ws.data_ptr() + 4 * ws_n[0])
        assert lib.pdf_rowlin_wgrad2_roww(n, cin, cin, n, cin, 32, tab, roww, 32, ctypes.byref(took), mma, P(st)) == 0
        torch.cuda.synchronize()
        assert torch.isnan(ws[sum(ws_n):]).all()   # nothing past the queried scratch
        return gxx, gz, took.value

    gxx, gz, took = pair(0)
    assert took == 1 and torch.equal(gxx, gxx0) and torch.equal(gz, gz0)
    assert pair(1)[2] == 0
    monkeypatch.setenv("PDFOPS_PAIR", "0")
    gxx, gz, took = pair(0)
    assert took == 0 and torch.equal(gxx, gxx0) and torch.equal(gz, gz0)


def _cloud(sizes, gen):
    pts = [torch.rand(s, 3, device="cuda", generator=gen) + 10.0 * i for i, s in enumerate(sizes)]
    return torch.cat(pts).contiguous(), torch.tensor(sizes, device="cuda").cumsum(0).int()


def _collect(mod, y, grads):
    out = {"y": y.detach()}
    out.update({"gin_%d" % i: g for i, g in enumerate(grads)})
    out.update({"g_" + n: p.grad for n, p in mod.named_parameters() if p.grad is not None})
    out.update({"b_" + n: b.detach().clone() for n, b in mod.named_buffers()})
    return out


def _same(a, b, min_grads):
    assert set(a) == set(b) and len([k for k in a if k.startswith("g_")]) >= min_grads
    for k in b:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max().item())
    assert all(a[k].abs().sum().item() > 0 for k in a if k.startswith("gin_"))


@pytest.mark.parametrize("sizes,nsample,c", [((150, 150), 16, 64), ((150, 150), 8, 32), ((97,), 16, 128), ((60,), 16, 512)])
@pytest.mark.parametrize("moments", [True, False])
def test_bottleneck_with_and_without_pairing(sizes, nsample, c, moments, monkeypatch):
    """Forward + backward of a Bottleneck: output, input gradient, every parameter gradient (S3 / S4 included) and every buffer."""
    from pointcloudpdf_amd import _native, synthetic
    from pointcloudpdf_amd.geometry import Geometry
    from pointcloudpdf_amd.point_transformer import Bottleneck

    be = _native.hip_backend()
    gen = torch.Generator(device="cuda").manual_seed(nsample + c)
    coord, offset = _cloud(sizes, gen)
    geom = Geometry(coord, offset)
    idx, _ = geom.knn(nsample, 0, 0)
    geom.rel_moments(nsample, 0)
    n = coord.shape[0]
    base = Bottleneck(c, c, 8, nsample).cuda()
    synthetic.fill_parameters_deterministic(base, seed=9)
    base.train()
    x0 = torch.randn(n, c, device="cuda", generator=gen)
    gout = torch.randn(n, c, device="cuda", generator=gen)
    monkeypatch.setattr(be, "use_moments", moments)
    res = []
    for pair in (None, "0"):
        if pair is not None:
            monkeypatch.setenv("PDFOPS_PAIR", pair)
        mod = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        y = mod([geom.coord(0), x, geom.offset(0)])[1]
        y.backward(gout)
        res.append(_collect(mod, y, [x.grad]))
    _same(res[0], res[1], 14)
    for name in ("linear_p.0.weight", "linear_p.0.bias", "linear_p.1.weight", "linear_p.1.bias", "linear_p.3.weight"):   # S4 | S3
        assert res[0]["g_transformer." + name].abs().sum().item() > 0, name


@pytest.mark.parametrize("sizes,cin,cout", [((150, 150), 32, 64), ((97,), 256, 512)])
def test_transition_down_with_and_without_pairing(sizes, cin, cout, monkeypatch):
    """Forward + backward of a TransitionDown (stride 4, nsample 16): output, running statistics and all gradients."""
    from pointcloudpdf_amd import dense, synthetic
    from pointcloudpdf_amd.geometry import Geometry
    from pointcloudpdf_amd.point_transformer import TransitionDown

    gen = torch.Generator(device="cuda").manual_seed(cin + cout)
    coord, offset = _cloud(sizes, gen)
    geom = Geometry(coord, offset)
    base = TransitionDown(cin, cout, 4, 16).cuda()
    synthetic.fill_parameters_deterministic(base, seed=11)
    base.train()
    x0 = torch.randn(coord.shape[0], cin, device="cuda", generator=gen)
    assert TransitionDown.fused and dense.transition_down_ok(base, x0)
    res = []
    gout = None
    for pair in (None, "0"):
        if pair is not None:
            monkeypatch.setenv("PDFOPS_PAIR", pair)
        mod = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        y = mod([geom.coord(0), x, geom.offset(0)])[1]
        if gout is None:
            gout = torch.randn(y.shape, device="cuda", generator=gen)
        y.backward(gout)
        res.append(_collect(mod, y, [x.grad]))
    _same(res[0], res[1], 3)
    assert any(k.startswith("b_") and "running" in k for k in res[0])

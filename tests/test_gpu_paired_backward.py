"""GPU suite: the nodes whose independent launches are paired (csrc/block.hip: pdf_transition_up_backward; csrc/fused_layer.hip: the
layer backward's two inverse-table gathers, alone and inside pdf_bottleneck_backward) with PDFOPS_PAIR unset and PDFOPS_PAIR=0 in one
process.  A paired launch runs every problem's body over the grid of its single launch, so the bar is equality of bits (torch.equal) on
every output, gradient and buffer."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("fine,coarse,k2,o", [((37, 37), (9, 9), 64, 32), ((301, 301), (77, 77), 128, 64), ((301, 301), (77, 77), 256, 128),
                                              ((301, 301), (77, 77), 512, 256), ((37, 37), (9, 9), 512, 512)])
def test_transition_up_node_with_and_without_pairing(fine, coarse, k2, o, monkeypatch):
    from pointcloudpdf_amd import dense, synthetic
    from pointcloudpdf_amd.point_transformer import TransitionUp

    gen = torch.Generator(device="cuda").manual_seed(k2 + o)
    p1, o1 = _cloud(fine, gen)
    p2, o2 = _cloud(coarse, gen)
    x1_0 = torch.randn(p1.shape[0], o, device="cuda", generator=gen)
    x2_0 = torch.randn(p2.shape[0], k2, device="cuda", generator=gen)
    gout = torch.randn(p1.shape[0], o, device="cuda", generator=gen)
    base = TransitionUp(k2, o).cuda()
    synthetic.fill_parameters_deterministic(base, seed=7)
    base.train()
    assert dense.TUFUSED
    res = []
    for pair in (None, "0"):
        if pair is not None:
            monkeypatch.setenv("PDFOPS_PAIR", pair)
        mod = copy.deepcopy(base)
        x1, x2 = x1_0.clone().requires_grad_(True), x2_0.clone().requires_grad_(True)
        y = mod([p1, x1, o1], [p2, x2, o2])
        y.backward(gout)
        res.append(_collect(mod, y, [x1.grad, x2.grad]))
    _same(res[0], res[1], 8)


# (scene sizes, nsample, c, kNN moments given): the slab B3 with the closed-form block | the level-1 forms | a wide block | the open form
@pytest.mark.parametrize("sizes,nsample,c,moments", [((150, 150), 16, 64, True), ((150, 150), 8, 32, True), ((97,), 16, 128, True),
                                                     ((150, 150), 16, 64, False)])
@pytest.mark.parametrize("whole_block", [True, False])
def test_layer_backward_with_and_without_pairing(sizes, nsample, c, moments, whole_block, monkeypatch):
    """The Bottleneck (pdf_bottleneck_backward) and the attention layer alone (pdf_pt_layer_backward): every gradient, S3 / S4 included."""
    from pointcloudpdf_amd import _native, synthetic
    from pointcloudpdf_amd.geometry import Geometry
    from pointcloudpdf_amd.point_transformer import Bottleneck, PointTransformerLayer

    be = _native.hip_backend()
    gen = torch.Generator(device="cuda").manual_seed(nsample + c)
    coord, offset = _cloud(sizes, gen)
    geom = Geometry(coord, offset)
    idx, _ = geom.knn(nsample, 0, 0)
    geom.rel_moments(nsample, 0)
    assert _native.moments_of(idx) is not None
    n = coord.shape[0]
    base = (Bottleneck(c, c, 8, nsample) if whole_block else PointTransformerLayer(c, c, 8, nsample)).cuda()
    synthetic.fill_parameters_deterministic(base, seed=9)
    base.train()
    x0 = torch.randn(n, c, device="cuda", generator=gen)
    gout = torch.randn(n, c, device="cuda", generator=gen)
    res = []
    monkeypatch.setattr(be, "use_moments", moments)
    for pair in (None, "0"):
        if pair is not None:
            monkeypatch.setenv("PDFOPS_PAIR", pair)
        mod = copy.deepcopy(base)
        x = x0.clone().requires_grad_(True)
        y = mod([geom.coord(0), x, geom.offset(0)])
        y = y[1] if whole_block else y
        y.backward(gout)
        res.append(_collect(mod, y, [x.grad]))
    _same(res[0], res[1], 14)
    for name in ("linear_p.0.weight", "linear_p.0.bias", "linear_p.1.weight", "linear_p.1.bias", "linear_p.3.weight"):   # S4 | S3
        key = "g_" + ("transformer." if whole_block else "") + name
        assert res[0][key].abs().sum().item() > 0, key

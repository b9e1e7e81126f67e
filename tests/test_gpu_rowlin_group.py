"""GPU suite: the group form of the streaming Linear kernels (csrc/rowlin2_impl.h: k_fwd_group) against the slab form (k_fwd).

Every case runs the same call twice through the wrappers of _native.py, with PDFOPS_RL_FORM=slab and PDFOPS_RL_FORM=group (read at every
launch), and requires identical bits on every output and on the used partial rows: the group form multiplies the same operands in the same
order per output element and reduces the statistics in the same order, so nothing may differ.  The case with 780 rows of every variant is
also held to the float64 product with the bounds of test_gpu_pointwise.py::test_rowlin_forward_dgrad_wgrad (max_rel 2e-6 on outputs, 1e-4
on column sums, 1e-5 on column sums of squares; the two BatchNorm-backward sums of the dgrad variant are signed sums like the column sum
and take its 1e-4).

Rows: one partial tile (1), an exact tile (16), one row more (17), one row short of / past a row block of 64 (63, 65), several row blocks
(257) and the level-5 size (780), where the capped grid of the launches without statistics gives a wave two tiles."""
import contextlib
import os

import pytest
import torch

from helpers import max_rel

pytestmark = pytest.mark.gpu

ROWS = [1, 16, 17, 63, 65, 257, 780]
WIDTHS = [128, 256, 512]


@contextlib.contextmanager
def _form(name):
    prev = os.environ.get("PDFOPS_RL_FORM")
    os.environ["PDFOPS_RL_FORM"] = name
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop("PDFOPS_RL_FORM", None)
        else:
            os.environ["PDFOPS_RL_FORM"] = prev


def _both(fn):
    """fn() -> list of tensors, run under either form; asserts identical bits and returns the group form's tensors."""
    with _form("slab"):
        a = fn()
    with _form("group"):
        b = fn()
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for i, (s, g) in enumerate(zip(a, b)):
        assert s.shape == g.shape and torch.equal(s, g), f"output {i}: {(s != g).sum().item()} of {s.numel()} elements differ"
    return b


def _with_partial(y, partial):
    rows = partial._pdf_rows
    return [y, partial[: rows * 2 * y.shape[1]].clone(), torch.tensor([rows])]


def _be():
    from pointcloudpdf_amd import _native

    return _native.hip_backend()


def _gen(*seed):
    return torch.Generator(device="cuda").manual_seed(sum(seed))


def _coef(k, g):
    sc = torch.rand(k, device="cuda", generator=g) + 0.5
    sh = torch.randn(k, device="cuda", generator=g) * 0.3
    return torch.cat([sc, sh, torch.zeros(2 * k, device="cuda")]), sc, sh


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_qkv_product(n, k):
    be, g = _be(), _gen(n, k, 1)
    x = torch.randn(n, k, device="cuda", generator=g)
    ws = [torch.randn(k, k, device="cuda", generator=g) / k ** 0.5 for _ in range(3)]
    bs = [torch.randn(k, device="cuda", generator=g) for _ in range(3)]
    coef, sc, sh = _coef(k, g)
    for pre in (False, True):
        ys = _both(lambda: be.rowlin_multi([x], ws, bs, coef=coef if pre else None, relu=pre, nout=3))
        if n == 780:
            fx = torch.relu(x * sc + sh) if pre else x
            for y, w, b in zip(ys, ws, bs):
                assert max_rel(y.cpu().numpy(), (fx.double() @ w.double().t() + b.double()).cpu().numpy()) < 2e-6


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_qkv_product_reduced_precision(n, k, mode):
    from pointcloudpdf_amd import _native

    be, g = _be(), _gen(n, k, 2)
    x = torch.randn(n, k, device="cuda", generator=g)
    ws = [torch.randn(k, k, device="cuda", generator=g) / k ** 0.5 for _ in range(3)]
    bs = [torch.randn(k, device="cuda", generator=g) for _ in range(3)]
    coef, _, _ = _coef(k, g)
    with _native.mma_input(mode):
        for pre in (False, True):
            _both(lambda: be.rowlin_multi([x], ws, bs, coef=coef if pre else None, relu=pre, nout=3))


@pytest.mark.parametrize("k", [128, 256])   # (three inputs at 512 are three accumulating launches of the single-input kernel)
@pytest.mark.parametrize("n", ROWS)
def test_three_input_dgrad_with_batchnorm_sums(n, k):
    be, g = _be(), _gen(n, k, 3)
    z = torch.randn(n, k, device="cuda", generator=g) * 1.7 + 0.4
    gamma = torch.rand(k, device="cuda", generator=g) + 0.5
    gamma[::5] *= -1.0
    beta = torch.randn(k, device="cuda", generator=g) * 0.3
    ws = [torch.randn(k, k, device="cuda", generator=g) / k ** 0.5 for _ in range(3)]
    gs = [torch.randn(n, k, device="cuda", generator=g) for _ in range(3)]
    mean = z.double().mean(0)
    rstd = (z.double().var(0, unbiased=False) + 1e-5).rsqrt()
    scale = gamma.double() * rstd
    coef = torch.cat([scale.float(), (beta.double() - mean * scale).float(), mean.float(), rstd.float()])

    def run(train, relu):
        out = be.rowlin_dgrad_bn_backward(gs, ws, z, coef, training=train, relu=relu)
        assert out is not None
        return [t.clone() for t in out]

    for relu in (True, False):
        _both(lambda: run(True, relu))
    if n == 780:   # eval mode without the ReLU: d z = (sum_i G_i W_i) * scale, d beta = sum_n g, d gamma = sum_n g xhat -- no kinks, plain products
        dz, dgamma, dbeta = _both(lambda: run(False, False))
        c = coef.double()
        gd = sum(gi.double() @ w.double() for gi, w in zip(gs, ws))
        assert max_rel(dz.cpu().numpy(), (gd * c[:k]).cpu().numpy()) < 2e-6
        assert max_rel(dbeta.cpu().numpy(), gd.sum(0).cpu().numpy()) < 1e-4
        assert max_rel(dgamma.cpu().numpy(), (gd * (z.double() - c[2 * k:3 * k]) * c[3 * k:]).sum(0).cpu().numpy()) < 1e-4


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_single_output_with_statistics(n, k):
    be, g = _be(), _gen(n, k, 4)
    x = torch.randn(n, k, device="cuda", generator=g)
    w = torch.randn(k, k, device="cuda", generator=g) / k ** 0.5
    b = torch.randn(k, device="cuda", generator=g)
    coef, sc, sh = _coef(k, g)
    for pre in (False, True):
        y, part, rows = _both(lambda: _with_partial(*be.rowlin(x, w, b, coef=coef if pre else None, relu=True, stats=True)))
        if n == 780:
            ref = (torch.relu(x * sc + sh) if pre else x).double() @ w.double().t() + b.double()
            ps = part.view(int(rows), 2 * k).double().sum(0)
            assert max_rel(y.cpu().numpy(), ref.cpu().numpy()) < 2e-6
            assert max_rel(ps[:k].cpu().numpy(), ref.sum(0).cpu().numpy()) < 1e-4
            assert max_rel(ps[k:].cpu().numpy(), (ref * ref).sum(0).cpu().numpy()) < 1e-5


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_accumulate_and_strided_input(n, k):
    be, g = _be(), _gen(n, k, 5)
    go = torch.randn(n, k, device="cuda", generator=g)
    w = torch.randn(k, k, device="cuda", generator=g) / k ** 0.5
    b = torch.randn(k, device="cuda", generator=g)
    y0 = torch.randn(n, k, device="cuda", generator=g)
    big = torch.randn(n, k + 8, device="cuda", generator=g)   # a view with row stride > K
    (acc,) = _both(lambda: [be.rowlin(go, w, transpose_w=True, out=y0.clone(), accumulate=True)[0]])
    (ys,) = _both(lambda: [be.rowlin(big[:, :k], w, b)[0]])
    if n == 780:
        assert max_rel(acc.cpu().numpy(), (y0.double() + go.double() @ w.double()).cpu().numpy()) < 2e-6
        assert max_rel(ys.cpu().numpy(), (big[:, :k].double() @ w.double().t() + b.double()).cpu().numpy()) < 2e-6


def test_wide_input_keeps_its_path():
    """k = 1024 (780 x 1024 x 512): two 512-wide column windows in one launch of the slab form, whatever the switch says."""
    be, g = _be(), _gen(780, 1024, 6)
    x = torch.randn(780, 1024, device="cuda", generator=g)
    w = torch.randn(512, 1024, device="cuda", generator=g) / 32.0
    b = torch.randn(512, device="cuda", generator=g)
    with _form("auto"):
        (ya,) = [be.rowlin(x, w, b)[0]]
    (y,) = _both(lambda: [be.rowlin(x, w, b)[0]])
    assert torch.equal(y, ya)
    assert max_rel(y.cpu().numpy(), (x.double() @ w.double().t() + b.double()).cpu().numpy()) < 2e-6


def test_uncovered_shape_runs_unchanged():
    """o = 48 at K = 64 is outside the group form: PDFOPS_RL_FORM=group leaves the launch as it was."""
    be, g = _be(), _gen(1000, 64, 48)
    x = torch.randn(1000, 64, device="cuda", generator=g)
    w = torch.randn(48, 64, device="cuda", generator=g) / 8.0
    b = torch.randn(48, device="cuda", generator=g)
    y, part, rows = _both(lambda: _with_partial(*be.rowlin(x, w, b, relu=True, stats=True)))
    ref = x.double() @ w.double().t() + b.double()
    assert max_rel(y.cpu().numpy(), ref.cpu().numpy()) < 2e-6
    assert max_rel(part.view(int(rows), 96).double().sum(0)[:48].cpu().numpy(), ref.sum(0).cpu().numpy()) < 1e-4

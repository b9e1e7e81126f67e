"""GPU suite: the product kernels of a TransitionUp join as two-problem launches (csrc/rowlin2_impl.h: k_fwd_stats2 / k_fwd2 / k_fwd_group2 /
k_wg2 behind pdf_rowlin_forward_stats2 / pdf_rowlin_dgrad2 / pdf_rowlin_wgrad2) against two single launches.  Every problem of a paired launch runs the body of its
single launch over the grid of its single launch, so the bar is equality of bits (torch.equal), not a tolerance.  The entries report
whether the two products went out as one launch; every case states which it expects, so a dispatch that always fell back would fail."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p

# (k1, k2) of the model's joins; o = k1
WIDTHS = [(32, 64), (64, 128), (128, 256), (256, 512), (512, 512)]
# rows of the two problems: no multiple of 16 or 64, problem 1 below one 256-row weight-gradient split | below one row tile
SIZES = [(333, 85), (17, 5)]
# (k1, k2, n1, n2, PDFOPS_RL_FORM or None)
CASES = [(k1, k2, n1, n2, None) for k1, k2 in WIDTHS for n1, n2 in SIZES]
CASES += [(128, 256, 16400, 4100, None)]                       # problem 0 in the slab form, problem 1 in the group form
CASES += [(256, 512, 333, 85, "slab"), (256, 512, 333, 85, "group")]
CASES += [(k1, k2, 16400, 85, None) for k1, k2 in WIDTHS]      # the two weight-gradient row splits differ


def _table(tensors):
    return (P * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _lib():
    from pointcloudpdf_amd import _native

    return _native.hip_backend().lib


def _ids(case):
    return "k%dx%d_n%dx%d_%s" % case


def _group_form(k, n, form):
    """the form launch_fwd gives a one-input product with reduction width k over n rows (csrc/rowlin2_impl.h: group_form_wanted)"""
    return k >= 128 and (form == "group" or (form is None and n <= 16384))


def _forward_pairs(case):
    """paired forward kernels exist for the model's joins in the forms its row counts give: slab below K = 128, group from there on"""
    k1, k2, n1, n2, form = case
    return _group_form(k1, n1, form) == (k1 >= 128) and _group_form(k2, n2, form) == (k2 >= 128)


def _input_gradient_pairs(case):
    """both problems reduce over o = k1: one kernel when they take the same form, the slab form only at o = 32 / 64"""
    k1, k2, n1, n2, form = case
    return _group_form(k1, n1, form) == _group_form(k1, n2, form) == (k1 >= 128)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] != 16400 or c[3] != 85], ids=_ids)
@pytest.mark.parametrize("bias", [True, False])
def test_forward_pair(case, bias, monkeypatch):
    """pdf_rowlin_forward_stats2 against two pdf_rowlin_forward calls with statistics: outputs and partial rows (PDFOPS_PAIR=0 too)."""
    k1, k2, n1, n2, form = case
    o = k1
    lib = _lib()
    if form:
        monkeypatch.setenv("PDFOPS_RL_FORM", form)
    gen = torch.Generator(device="cuda").manual_seed(20 + k1 + n1)
    st = torch.cuda.current_stream().cuda_stream
    prob = [dict(n=n, k=k, x=torch.randn(n, k, device="cuda", generator=gen), w=torch.randn(o, k, device="cuda", generator=gen),
                 b=torch.randn(o, device="cuda", generator=gen) if bias else None) for n, k in ((n1, k1), (n2, k2))]
    new = lambda q: (torch.zeros(q["n"], o, device="cuda"), torch.zeros(int(lib.pdf_rowlin_partial_floats(q["n"], o)), device="cuda"))
    res = {}
    for pair in ("single", "1", "0"):
        out, tab = [], []
        for q in prob:
            y, part = new(q)
            out.append((y, part, int(lib.pdf_rowlin_partial_rows(q["n"], q["k"], o))))
            tab += [q["x"], q["w"], q["b"], y, part]
            if pair == "single":
                assert lib.pdf_rowlin_forward(q["n"], q["k"], o, q["x"].data_ptr(), q["k"], q["w"].data_ptr(), 0, None if q["b"] is None else q["b"].data_ptr(),
                                              None, None, 0, y.data_ptr(), o, 0, part.data_ptr(), 0, P(st)) == 0
        if pair != "single":
            monkeypatch.setenv("PDFOPS_PAIR", pair)
            took = ctypes.c_int(-1)
            assert lib.pdf_rowlin_forward_stats2(n1, k1, n2, k2, o, _table(tab), ctypes.byref(took), 0, P(st)) == 0
            assert took.value == int(pair == "1" and _forward_pairs(case))
        res[pair] = out
    torch.cuda.synchronize()
    for pair in ("1", "0"):
        for s, t in zip(res["single"], res[pair]):
            assert s[0].abs().sum().item() > 0 and torch.equal(s[0], t[0])
            rows = s[2] * 2 * o
            assert s[1][:rows].abs().sum().item() > 0 and torch.equal(s[1], t[1])
            assert s[1][rows:].abs().sum().item() == 0      # nothing past the problem's own rows


def test_forward_pair_outside_the_paired_widths():
    """(k1, k2) that no paired kernel covers come back through two single launches: the same outputs and rows."""
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(24)
    st = torch.cuda.current_stream().cuda_stream
    for o, k1, k2 in [(32, 64, 32), (64, 128, 128), (48, 32, 64), (32, 48, 64)]:
        n1, n2 = 333, 85
        prob = [dict(n=n, k=k, x=torch.randn(n, k, device="cuda", generator=gen), w=torch.randn(o, k, device="cuda", generator=gen))
                for n, k in ((n1, k1), (n2, k2))]
        new = lambda q: (torch.zeros(q["n"], o, device="cuda"), torch.zeros(int(lib.pdf_rowlin_partial_floats(q["n"], o)), device="cuda"))
        single, paired, tab = [], [], []
        for q in prob:
            y, part = new(q)
            assert lib.pdf_rowlin_forward(q["n"], q["k"], o, q["x"].data_ptr(), q["k"], q["w"].data_ptr(), 0, None, None, None, 0, y.data_ptr(), o, 0,
                                          part.data_ptr(), 0, P(st)) == 0
            single.append((y, part))
        for q in prob:
            y, part = new(q)
            paired.append((y, part))
            tab += [q["x"], q["w"], None, y, part]
        took = ctypes.c_int(-1)
        assert lib.pdf_rowlin_forward_stats2(n1, k1, n2, k2, o, _table(tab), ctypes.byref(took), 0, P(st)) == 0 and took.value == 0
        torch.cuda.synchronize()
        for s, t in zip(single, paired):
            assert s[0].abs().sum().item() > 0 and torch.equal(s[0], t[0]) and torch.equal(s[1], t[1]), (o, k1, k2)


@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("pair", ["1", "0"])
def test_input_gradient_pair(case, pair, monkeypatch):
    """pdf_rowlin_dgrad2 against two pdf_rowlin_forward calls with transpose_w = 1 (PDFOPS_PAIR=0: the entry's own two launches)."""
    k1, k2, n1, n2, form = case
    o = k1
    lib = _lib()
    if form:
        monkeypatch.setenv("PDFOPS_RL_FORM", form)
    gen = torch.Generator(device="cuda").manual_seed(21 + k1 + n1)
    st = torch.cuda.current_stream().cuda_stream
    prob = [dict(n=n, k=k, g=torch.randn(n, o, device="cuda", generator=gen), w=torch.randn(o, k, device="cuda", generator=gen))
            for n, k in ((n1, k1), (n2, k2))]
    single, tab, paired = [], [], []
    for q in prob:
        gx = torch.zeros(q["n"], q["k"], device="cuda")
        assert lib.pdf_rowlin_forward(q["n"], o, q["k"], q["g"].data_ptr(), o, q["w"].data_ptr(), 1, None, None, None, 0, gx.data_ptr(), q["k"], 0, None,
                                      0, P(st)) == 0
        single.append(gx)
    for q in prob:
        gx = torch.zeros(q["n"], q["k"], device="cuda")
        paired.append(gx)
        tab += [q["g"], q["w"], gx]
    monkeypatch.setenv("PDFOPS_PAIR", pair)
    took = ctypes.c_int(-1)
    assert lib.pdf_rowlin_dgrad2(n1, k1, n2, k2, o, _table(tab), ctypes.byref(took), 0, P(st)) == 0
    assert took.value == int(pair == "1" and _input_gradient_pairs(case))
    torch.cuda.synchronize()
    for s, t in zip(single, paired):
        assert s.abs().sum().item() > 0 and torch.equal(s, t)


@pytest.mark.parametrize("case", [c for c in CASES if c[4] is None], ids=_ids)   # (the weight-gradient kernel has one form)
@pytest.mark.parametrize("bias", [True, False])
def test_weight_gradient_pair(case, bias, monkeypatch):
    """pdf_rowlin_wgrad2 (ONE product launch, ONE slab reduction) against two pdf_rowlin_wgrad calls: dW and db."""
    k1, k2, n1, n2, _ = case
    o = k1
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(22 + k1 + n1)
    st = torch.cuda.current_stream().cuda_stream
    prob = [dict(n=n, k=k, g=torch.randn(n, o, device="cuda", generator=gen), x=torch.randn(n, k, device="cuda", generator=gen))
            for n, k in ((n1, k1), (n2, k2))]
    new = lambda q: (torch.zeros(o, q["k"], device="cuda"), torch.zeros(o, device="cuda"),
                     torch.zeros(max(int(lib.pdf_rowlin_wgrad_ws_floats(q["n"], q["k"], o, 1)), 1), device="cuda"))
    res = {}
    for pair in ("single", "1", "0"):
        out, tab = [], []
        for q in prob:
            dw, db, ws = new(q)
            out.append((dw, db))
            tab += [q["g"], q["x"], dw, db if bias else None, ws]
            if pair == "single":
                assert lib.pdf_rowlin_wgrad(q["n"], q["k"], o, q["g"].data_ptr(), o, q["x"].data_ptr(), q["k"], None, None, 0, dw.data_ptr(),
                                            db.data_ptr() if bias else None, ws.data_ptr(), 0, P(st)) == 0
        if pair != "single":
            monkeypatch.setenv("PDFOPS_PAIR", pair)
            took = ctypes.c_int(-1)
            assert lib.pdf_rowlin_wgrad2_paired(n1, k1, o, n2, k2, o, _table(tab), ctypes.byref(took), 0, P(st)) == 0
            assert took.value == int(pair == "1")   # (k1, k2 and o = k1 take one vector width in every case)
        res[pair] = out
    torch.cuda.synchronize()
    for pair in ("1", "0"):
        for s, t in zip(res["single"], res[pair]):
            assert s[0].abs().sum().item() > 0 and torch.equal(s[0], t[0]) and torch.equal(s[1], t[1])
            assert (s[1].abs().sum().item() > 0) == bias


def test_unpaired_combinations_fall_back_to_the_same_bits():
    """Widths that no paired kernel covers -- a reduction width outside the streaming kernels, output widths on different slab widths,
    a null input gradient -- come back through two single launches."""
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(23)
    st = torch.cuda.current_stream().cuda_stream
    for o, k1, k2, skip in [(48, 32, 64, None), (32, 96, 64, None), (64, 64, 16, None), (64, 64, 128, 0), (64, 64, 128, 1)]:
        n1, n2 = 333, 85
        prob = [dict(n=n, k=k, g=torch.randn(n, o, device="cuda", generator=gen), w=torch.randn(o, k, device="cuda", generator=gen))
                for n, k in ((n1, k1), (n2, k2))]
        single, tab, paired = [], [], []
        for i, q in enumerate(prob):
            gx = torch.zeros(q["n"], q["k"], device="cuda")
            if i != skip:
                assert lib.pdf_rowlin_forward(q["n"], o, q["k"], q["g"].data_ptr(), o, q["w"].data_ptr(), 1, None, None, None, 0, gx.data_ptr(), q["k"], 0,
                                              None, 0, P(st)) == 0
            single.append(gx)
        for i, q in enumerate(prob):
            gx = torch.zeros(q["n"], q["k"], device="cuda")
            paired.append(gx)
            tab += [q["g"], q["w"], None if i == skip else gx]
        took = ctypes.c_int(-1)
        assert lib.pdf_rowlin_dgrad2(n1, k1, n2, k2, o, _table(tab), ctypes.byref(took), 0, P(st)) == 0 and took.value == 0
        torch.cuda.synchronize()
        for i, (s, t) in enumerate(zip(single, paired)):
            assert (s.abs().sum().item() > 0) == (i != skip) and torch.equal(s, t), (o, k1, k2, skip)


@pytest.mark.parametrize("mma", [1, 2])
def test_reduced_precision_products_take_two_launches(mma):
    """The paired kernels are built for fp32 operands: with mma_input 1 / 2 the three entries issue the single launches of that mode."""
    lib = _lib()
    gen = torch.Generator(device="cuda").manual_seed(25 + mma)
    st = torch.cuda.current_stream().cuda_stream
    o, n, k = 64, (333, 85), (64, 128)
    x = [torch.randn(n[i], k[i], device="cuda", generator=gen) for i in range(2)]
    g = [torch.randn(n[i], o, device="cuda", generator=gen) for i in range(2)]
    w = [torch.randn(o, k[i], device="cuda", generator=gen) for i in range(2)]
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    part = lambda i: z(int(lib.pdf_rowlin_partial_floats(n[i], o)))
    ws = lambda i: z(max(int(lib.pdf_rowlin_wgrad_ws_floats(n[i], k[i], o, 1)), 1))
    one, two = [], []
    for i in range(2):
        y, pr, gx, dw, db = z(n[i], o), part(i), z(n[i], k[i]), z(o, k[i]), z(o)
        assert lib.pdf_rowlin_forward(n[i], k[i], o, x[i].data_ptr(), k[i], w[i].data_ptr(), 0, None, None, None, 0, y.data_ptr(), o, 0, pr.data_ptr(), mma, P(st)) == 0
        assert lib.pdf_rowlin_forward(n[i], o, k[i], g[i].data_ptr(), o, w[i].data_ptr(), 1, None, None, None, 0, gx.data_ptr(), k[i], 0, None, mma, P(st)) == 0
        assert lib.pdf_rowlin_wgrad(n[i], k[i], o, g[i].data_ptr(), o, x[i].data_ptr(), k[i], None, None, 0, dw.data_ptr(), db.data_ptr(), ws(i).data_ptr(), mma, P(st)) == 0
        one.append((y, pr, gx, dw, db))
        two.append((z(n[i], o), part(i), z(n[i], k[i]), z(o, k[i]), z(o)))
    keep = [ws(0), ws(1)]
    took = ctypes.c_int(-1)
    assert lib.pdf_rowlin_forward_stats2(n[0], k[0], n[1], k[1], o, _table([t for i in range(2) for t in (x[i], w[i], None, two[i][0], two[i][1])]),
                                         ctypes.byref(took), mma, P(st)) == 0 and took.value == 0
    assert lib.pdf_rowlin_dgrad2(n[0], k[0], n[1], k[1], o, _table([t for i in range(2) for t in (g[i], w[i], two[i][2])]), ctypes.byref(took), mma, P(st)) == 0
    assert took.value == 0
    assert lib.pdf_rowlin_wgrad2_paired(n[0], k[0], o, n[1], k[1], o, _table([t for i in range(2) for t in (g[i], x[i], two[i][3], two[i][4], keep[i])]),
                                        ctypes.byref(took), mma, P(st)) == 0 and took.value == 0
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        for u, v in zip(a, b):
            assert u.abs().sum().item() > 0 and torch.equal(u, v)

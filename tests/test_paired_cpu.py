"""CPU suite: the paired product entries (ABI 20) validate their arguments before anything is launched, and their rows are in the binding's
table.  The library loads without a GPU; a launch there would come back as a positive HIP error code, never as PDF_ERR_BAD_ARG."""
import ctypes

import pytest

BAD, UNSUPPORTED = -1, -3
L, I, P = ctypes.c_long, ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    sig = {"pdf_rowlin_forward_stats2": [L, I, L, I, I, P, P, I, P], "pdf_rowlin_dgrad2": [L, I, L, I, I, P, P, I, P],
           "pdf_rowlin_wgrad2_paired": [L, I, I, L, I, I, P, P, I, P]}
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I, argtypes
    return lib


@pytest.fixture(scope="module")
def buf():
    return (ctypes.c_float * 4096)()   # (only its address is used)


def table(buf, count, null=()):
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return (P * count)(*[None if i in null else base + 64 * i for i in range(count)])


def test_abi_rows():
    from pointcloudpdf_amd import _abi, _native

    assert _native.ABI_VERSION >= 20
    assert _abi.ENTRIES["pdf_rowlin_forward_stats2"] == ("s", "liliippip")
    assert _abi.ENTRIES["pdf_rowlin_dgrad2"] == ("s", "liliippip")
    assert _abi.ENTRIES["pdf_rowlin_wgrad2_paired"] == ("s", "liiliippip")


@pytest.mark.parametrize("pair", [None, "0"])
def test_forward_pair_validates_before_any_launch(lib, buf, pair, monkeypatch):
    if pair is not None:
        monkeypatch.setenv("PDFOPS_PAIR", pair)
    fw = lambda n0, k0, n1, k1, o, t, mma=0: lib.pdf_rowlin_forward_stats2(n0, k0, n1, k1, o, t, None, mma, None)
    t10 = table(buf, 10)
    assert fw(100, 32, 50, 64, 32, None) == BAD
    assert fw(0, 32, 50, 64, 32, t10) == BAD and fw(100, 32, -3, 64, 32, t10) == BAD
    assert fw(100, 0, 50, 64, 32, t10) == BAD and fw(100, 32, 50, 64, 0, t10) == BAD
    assert fw(100, 32, 50, 64, 32, t10, mma=3) == BAD
    for i in (0, 1, 3, 4, 5, 6, 8, 9):
        assert fw(100, 32, 50, 64, 32, table(buf, 10, null=(i,))) == BAD, i   # (2, 7: the biases are optional)
    off = table(buf, 10)
    off[5] = off[5] + 4                                          # x of problem 1 not 16-byte aligned: no statistics layout for it
    assert fw(100, 32, 50, 64, 32, off) == BAD


@pytest.mark.parametrize("pair", [None, "0"])
def test_input_gradient_pair_validates_before_any_launch(lib, buf, pair, monkeypatch):
    if pair is not None:
        monkeypatch.setenv("PDFOPS_PAIR", pair)
    dg = lambda n0, k0, n1, k1, o, t, mma=0: lib.pdf_rowlin_dgrad2(n0, k0, n1, k1, o, t, None, mma, None)
    t6 = table(buf, 6)
    assert dg(100, 32, 50, 64, 32, None) == BAD
    assert dg(0, 32, 50, 64, 32, t6) == BAD and dg(100, 32, -3, 64, 32, t6) == BAD
    assert dg(100, 0, 50, 64, 32, t6) == BAD and dg(100, 32, 50, 64, 0, t6) == BAD
    assert dg(100, 32, 50, 64, 32, t6, mma=3) == BAD and dg(100, 32, 50, 64, 32, t6, mma=-1) == BAD
    for i in (0, 1, 3, 4):
        assert dg(100, 32, 50, 64, 32, table(buf, 6, null=(i,))) == BAD, i   # (2, 5: a null input gradient is not computed)


@pytest.mark.parametrize("pair", [None, "0"])
def test_weight_gradient_pair_validates_before_any_launch(lib, buf, pair, monkeypatch):
    if pair is not None:
        monkeypatch.setenv("PDFOPS_PAIR", pair)
    wg = lambda n0, k0, o0, n1, k1, o1, t, mma=0: lib.pdf_rowlin_wgrad2_paired(n0, k0, o0, n1, k1, o1, t, None, mma, None)
    t10 = table(buf, 10)
    assert wg(100, 32, 32, 50, 64, 32, None) == BAD and wg(100, 32, 32, 0, 64, 32, t10) == BAD and wg(100, 32, 32, 50, 64, 32, t10, mma=5) == BAD
    for i in (0, 1, 2, 4, 5, 6, 7, 9):
        assert wg(100, 32, 32, 50, 64, 32, table(buf, 10, null=(i,))) == BAD, i
    assert wg(100, 48, 32, 50, 64, 32, t10) == UNSUPPORTED and wg(100, 32, 32, 50, 64, 48, t10) == UNSUPPORTED
    off = table(buf, 10)
    off[5] = off[5] + 4                                          # g of problem 1 not 16-byte aligned
    assert wg(100, 32, 32, 50, 64, 32, off) == UNSUPPORTED

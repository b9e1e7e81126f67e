"""CPU suite: the TransitionUp entries and the two-problem entries (ABI 19) validate their arguments before anything is launched.  The
library loads without a GPU; a launch there would come back as a positive HIP error code, never as PDF_ERR_BAD_ARG / PDF_ERR_UNSUPPORTED."""
import ctypes

import pytest

BAD, UNSUPPORTED = -1, -3
L, I, F, P = ctypes.c_long, ctypes.c_int, ctypes.c_float, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    sig = {
        "pdf_transition_up_supported": [I, I, I],
        "pdf_transition_up_forward": [L, I, L, I, I, P, I, F, F, I, P],
        "pdf_transition_up_backward": [L, I, L, I, I, P, I, I, P],
        "pdf_bn_coef_from_partial2": [I, L, I, I, L, I, P, F, F, P],
        "pdf_bn_act_backward2": [L, I, L, I, P, I, P],
        "pdf_rowlin_wgrad2": [L, I, I, L, I, I, P, I, P],
    }
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I, argtypes
    return lib


@pytest.fixture(scope="module")
def buf():
    return (ctypes.c_float * 4096)()   # (64-byte aligned by the allocator's page-sized block; only its address is used)


def table(buf, count, null=()):
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return (P * count)(*[None if i in null else base + 64 * i for i in range(count)])


def test_support_rule(lib):
    for k1, k2, o, want in [(32, 64, 32, 1), (512, 512, 512, 1), (256, 512, 256, 1), (64, 128, 64, 1), (48, 64, 32, 0), (32, 1024, 32, 0),
                            (32, 64, 48, 0), (32, 64, 16, 0), (32, 64, 2048, 0), (32, 64, 96, 0)]:
        assert lib.pdf_transition_up_supported(k1, k2, o) == want, (k1, k2, o)


def test_forward_validates_before_any_launch(lib, buf):
    fwd = lambda n1, k1, n2, k2, o, t, training=1, mma=0: lib.pdf_transition_up_forward(n1, k1, n2, k2, o, t, training, 1e-5, 0.1, mma, None)
    full = table(buf, 24)
    assert fwd(100, 32, 30, 64, 32, None) == BAD
    assert fwd(0, 32, 30, 64, 32, full) == BAD and fwd(100, 32, 0, 64, 32, full) == BAD and fwd(-5, 32, 30, 64, 32, full) == BAD
    assert fwd(100, 32, 30, 64, 32, full, mma=3) == BAD
    for i in range(24):
        if i in (2, 9, 16):
            continue                                             # (the two biases and the visiting order are optional)
        assert fwd(100, 32, 30, 64, 32, table(buf, 24, null=(i,))) == BAD, i
    assert fwd(100, 48, 30, 64, 32, full) == UNSUPPORTED        # k1 outside the streaming kernels
    assert fwd(100, 32, 30, 1024, 32, full) == UNSUPPORTED      # k2
    assert fwd(100, 32, 30, 64, 48, full) == UNSUPPORTED        # o % 32
    assert fwd(100, 32, 30, 64, 96, full) == UNSUPPORTED        # o no divisor of 1024 (pdf_bn_supported)
    assert fwd(100, 32, 30, 64, 32, full, training=0) == UNSUPPORTED
    off = table(buf, 24)
    off[17] = off[17] + 4                                        # z1 not 16-byte aligned
    assert fwd(100, 32, 30, 64, 32, off) == UNSUPPORTED
    assert fwd(1 << 31, 32, 30, 64, 32, full) == UNSUPPORTED     # n1 * (o / 4) past the gather kernels' 32-bit element count


def test_backward_validates_before_any_launch(lib, buf):
    bwd = lambda n1, k1, n2, k2, o, t, mma=0: lib.pdf_transition_up_backward(n1, k1, n2, k2, o, t, 0, mma, None)
    full = table(buf, 24)
    assert bwd(100, 32, 30, 64, 32, None) == BAD
    assert bwd(0, 32, 30, 64, 32, full) == BAD and bwd(100, 32, -1, 64, 32, full) == BAD
    assert bwd(100, 32, 30, 64, 32, full, mma=-1) == BAD
    for i in range(24):
        if i in (12, 13, 14):
            continue                                             # (source order and the two input gradients are optional)
        assert bwd(100, 32, 30, 64, 32, table(buf, 24, null=(i,))) == BAD, i
    assert bwd(100, 32, 30, 96, 32, full) == UNSUPPORTED
    assert bwd(100, 32, 30, 64, 16, full) == UNSUPPORTED
    off = table(buf, 24)
    off[15] = off[15] + 8                                        # gradient block 1: its [d beta | d gamma] slot is read 16 bytes at a time
    assert bwd(100, 32, 30, 64, 32, off) == UNSUPPORTED


def test_two_problem_entries_validate_before_any_launch(lib, buf):
    t12, t10 = table(buf, 12), table(buf, 10)
    fin = lambda r0, n0, c0, r1, n1, c1, t: lib.pdf_bn_coef_from_partial2(r0, n0, c0, r1, n1, c1, t, 1e-5, 0.1, None)
    assert fin(4, 100, 32, 4, 50, 64, None) == BAD
    assert fin(0, 100, 32, 4, 50, 64, t12) == BAD and fin(4, 100, 32, 4, 0, 64, t12) == BAD
    assert fin(4, 100, 32, 4, 50, 64, table(buf, 12, null=(0,))) == BAD
    assert fin(4, 100, 32, 4, 50, 64, table(buf, 12, null=(11,))) == BAD
    assert fin(4, 100, 32, 4, 50, 64, table(buf, 12, null=(3,))) == BAD          # running mean without running variance
    assert fin(4, 100, 32, 4, 50, 96, t12) == UNSUPPORTED
    bwd = lambda n0, c0, n1, c1, t: lib.pdf_bn_act_backward2(n0, c0, n1, c1, t, 1, None)
    assert bwd(100, 32, 50, 64, None) == BAD and bwd(0, 32, 50, 64, t12) == BAD
    for i in range(12):
        assert bwd(100, 32, 50, 64, table(buf, 12, null=(i,))) == BAD, i
    assert bwd(100, 30, 50, 64, t12) == UNSUPPORTED
    wg = lambda n0, k0, o0, n1, k1, o1, t, mma=0: lib.pdf_rowlin_wgrad2(n0, k0, o0, n1, k1, o1, t, mma, None)
    assert wg(100, 32, 32, 50, 64, 64, None) == BAD and wg(100, 32, 32, 0, 64, 64, t10) == BAD and wg(100, 32, 32, 50, 64, 64, t10, mma=5) == BAD
    for i in (0, 1, 2, 4, 5, 6, 7, 9):
        assert wg(100, 32, 32, 50, 64, 64, table(buf, 10, null=(i,))) == BAD, i   # (3, 8: the bias gradients are optional)
    assert wg(100, 48, 32, 50, 64, 64, t10) == UNSUPPORTED and wg(100, 32, 32, 50, 64, 48, t10) == UNSUPPORTED

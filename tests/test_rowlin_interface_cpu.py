"""CPU suite: the dense Linear entries (csrc/rowlin.hip over csrc/rowlin2.h) keep the workspace and statistics sizes they hand out --
dense.py packs these into shared scratch buffers, so a changed size moves every address behind it -- and refuse malformed calls with the
same status, before anything is launched.  The expected values are literals recorded from the library of the commit BEFORE the host
code moved onto described problems (one plan for size and launch); they never come from the code under test.  The library loads without
a GPU; no call here is valid enough to launch (a launch would come back as a positive HIP error code)."""
import ctypes

import pytest

BAD, UNSUPPORTED = -1, -3
L, I, P = ctypes.c_long, ctypes.c_int, ctypes.c_void_p
NS = (1, 63, 64, 65, 255, 256, 257, 780, 3124, 12496, 49984, 200000)
KO = ((32, 32), (32, 48), (32, 64), (64, 16), (64, 64), (128, 128), (256, 512), (512, 512), (3, 32), (6, 13), (33, 65), (48, 48), (1024, 512))
# (k, o, ng) -> pdf_rowlin_wgrad_ws_floats(n, k, o, ng) over NS
WS_FLOATS = {
    (32, 32, 1): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (32, 32, 3): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (32, 32, 5): (5280, 5280, 5280, 5280, 5280, 5280, 10560, 21120, 68640, 258720, 827904, 3303168),
    (32, 48, 1): (8448, 8448, 8448, 8448, 8448, 8448, 16896, 33792, 109824, 413952, 1655808, 6606336),
    (32, 48, 3): (8448, 8448, 8448, 8448, 8448, 8448, 16896, 33792, 109824, 413952, 1655808, 6606336),
    (32, 48, 5): (8448, 8448, 8448, 8448, 8448, 8448, 16896, 33792, 109824, 413952, 1655808, 6606336),
    (32, 64, 1): (8448, 8448, 8448, 8448, 8448, 8448, 16896, 33792, 109824, 413952, 1655808, 6606336),
    (32, 64, 3): (8448, 8448, 8448, 8448, 8448, 8448, 16896, 33792, 109824, 413952, 1655808, 6606336),
    (32, 64, 5): (10560, 10560, 10560, 10560, 10560, 10560, 21120, 42240, 137280, 517440, 1655808, 6606336),
    (64, 16, 1): (8320, 8320, 8320, 8320, 8320, 8320, 16640, 33280, 108160, 407680, 1630720, 6506240),
    (64, 16, 3): (8320, 8320, 8320, 8320, 8320, 8320, 16640, 33280, 108160, 407680, 1630720, 6506240),
    (64, 16, 5): (8320, 8320, 8320, 8320, 8320, 8320, 16640, 33280, 108160, 407680, 1630720, 6506240),
    (64, 64, 1): (16640, 16640, 16640, 16640, 16640, 16640, 33280, 66560, 216320, 815360, 3261440, 8003840),
    (64, 64, 3): (16640, 16640, 16640, 16640, 16640, 16640, 33280, 66560, 216320, 815360, 3261440, 8003840),
    (64, 64, 5): (20800, 20800, 20800, 20800, 20800, 20800, 41600, 83200, 270400, 1019200, 3261440, 8003840),
    (128, 128, 1): (66048, 66048, 66048, 66048, 66048, 66048, 132096, 264192, 858624, 3236352, 7991808, 8454144),
    (128, 128, 3): (66048, 66048, 66048, 66048, 66048, 66048, 132096, 264192, 858624, 3236352, 7991808, 8454144),
    (128, 128, 5): (82560, 82560, 82560, 82560, 82560, 82560, 165120, 330240, 1073280, 3236352, 7991808, 8454144),
    (256, 512, 1): (526336, 526336, 526336, 526336, 526336, 526336, 1052672, 2105344, 6842368, 8421376, 8421376, 8421376),
    (256, 512, 3): (526336, 526336, 526336, 526336, 526336, 526336, 1052672, 2105344, 6842368, 8421376, 8421376, 8421376),
    (256, 512, 5): (657920, 657920, 657920, 657920, 657920, 657920, 1315840, 2631680, 6842368, 8421376, 8421376, 8421376),
    (512, 512, 1): (1050624, 1050624, 1050624, 1050624, 1050624, 1050624, 2101248, 4202496, 8404992, 8404992, 8404992, 8404992),
    (512, 512, 3): (1050624, 1050624, 1050624, 1050624, 1050624, 1050624, 2101248, 4202496, 8404992, 8404992, 8404992, 8404992),
    (512, 512, 5): (1313280, 1313280, 1313280, 1313280, 1313280, 1313280, 2626560, 4202496, 8404992, 8404992, 8404992, 8404992),
    (3, 32, 1): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (3, 32, 3): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (3, 32, 5): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (6, 13, 1): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (6, 13, 3): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (6, 13, 5): (4224, 4224, 4224, 4224, 4224, 4224, 8448, 16896, 54912, 206976, 827904, 3303168),
    (33, 65, 1): (24960, 24960, 24960, 24960, 24960, 24960, 49920, 99840, 324480, 1223040, 4892160, 8211840),
    (33, 65, 3): (24960, 24960, 24960, 24960, 24960, 24960, 49920, 99840, 324480, 1223040, 4892160, 8211840),
    (33, 65, 5): (24960, 24960, 24960, 24960, 24960, 24960, 49920, 99840, 324480, 1223040, 4892160, 8211840),
    (48, 48, 1): (16640, 16640, 16640, 16640, 16640, 16640, 33280, 66560, 216320, 815360, 3261440, 8003840),
    (48, 48, 3): (16640, 16640, 16640, 16640, 16640, 16640, 33280, 66560, 216320, 815360, 3261440, 8003840),
    (48, 48, 5): (16640, 16640, 16640, 16640, 16640, 16640, 33280, 66560, 216320, 815360, 3261440, 8003840),
    (1024, 512, 1): (2099200, 2099200, 2099200, 2099200, 2099200, 2099200, 4198400, 8396800, 8396800, 8396800, 8396800, 8396800),
    (1024, 512, 3): (2099200, 2099200, 2099200, 2099200, 2099200, 2099200, 4198400, 8396800, 8396800, 8396800, 8396800, 8396800),
    (1024, 512, 5): (2099200, 2099200, 2099200, 2099200, 2099200, 2099200, 4198400, 8396800, 8396800, 8396800, 8396800, 8396800),
}
# (k, o) -> pdf_rowlin_partial_rows(n, k, o) over NS
PARTIAL_ROWS = {
    (32, 32): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (32, 48): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (32, 64): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (64, 16): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (64, 64): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (128, 128): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (256, 512): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (512, 512): (1, 1, 1, 2, 4, 4, 5, 13, 49, 196, 781, 1024),
    (3, 32): (1, 1, 1, 1, 2, 2, 3, 7, 25, 98, 391, 1563),
    (6, 13): (1, 1, 1, 1, 2, 2, 3, 7, 25, 98, 391, 1563),
    (33, 65): (1, 1, 1, 1, 2, 2, 3, 7, 25, 98, 391, 1563),
    (48, 48): (1, 1, 1, 1, 2, 2, 3, 7, 25, 98, 391, 1563),
    (1024, 512): (1, 1, 1, 1, 2, 2, 3, 7, 25, 98, 391, 1563),
}
# o -> pdf_rowlin_partial_floats(n, o) over NS
PARTIAL_FLOATS = {
    13: (4126, 4126, 4126, 4152, 4204, 4204, 4230, 4438, 5374, 9196, 24406, 44738),
    16: (4132, 4132, 4132, 4164, 4228, 4228, 4260, 4516, 5668, 10372, 29092, 54116),
    32: (4164, 4164, 4164, 4228, 4356, 4356, 4420, 4932, 7236, 16644, 54084, 104132),
    48: (4196, 4196, 4196, 4292, 4484, 4484, 4580, 5348, 8804, 22916, 79076, 154148),
    64: (4228, 4228, 4228, 4356, 4612, 4612, 4740, 5764, 10372, 29188, 104068, 204164),
    65: (4230, 4230, 4230, 4360, 4620, 4620, 4750, 5790, 10470, 29580, 105630, 207290),
    128: (4356, 4356, 4356, 4612, 5124, 5124, 5380, 7428, 16644, 54276, 204036, 404228),
    512: (5124, 5124, 5124, 6148, 8196, 8196, 9220, 17412, 54276, 204804, 803844, 1604612),
}


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    sig = {"pdf_rowlin_wgrad_ws_floats": (L, [L, I, I, I]), "pdf_rowlin_partial_rows": (I, [L, I, I]), "pdf_rowlin_partial_floats": (L, [L, I]),
           "pdf_rowlin_forward": (I, [L, I, I, P, L, P, I, P, P, P, I, P, L, I, P, I, P]),
           "pdf_rowlin_multi": (I, [L, I, I, I, I, P, L, P, I, P, P, P, I, P, L, I, I, P]),
           "pdf_rowlin_wgrad_group": (I, [L, I, I, I, P, L, P, L, P, P, P, P, P, P, I, P]),
           "pdf_rowlin_dgrad_bstats": (I, [L, I, I, I, P, L, P, P, L, P, L, P, I, P, P, I, P]),
           "pdf_rowlin_forward_roww": (I, [L, I, I, P, L, P, I, P, L, I, P, L, I, P]),
           "pdf_rowlin_wgrad_roww": (I, [L, I, I, P, L, P, L, P, P, L, P, I, P])}
    for name, (restype, argtypes) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


@pytest.fixture(scope="module")
def buf():
    return (ctypes.c_float * 4096)()   # (only its address is used)


def ptr(buf, i):
    base = ctypes.addressof(buf)
    return base + (-base) % 16 + 64 * i


def table(buf, count, null=()):
    return (P * count)(*[None if i in null else ptr(buf, 8 + i) for i in range(count)])


def test_the_case_table_is_the_one_asked_for():
    assert set(WS_FLOATS) == {(k, o, ng) for k, o in KO for ng in (1, 3, 5)} and set(PARTIAL_ROWS) == set(KO)
    assert set(PARTIAL_FLOATS) == {o for _, o in KO}
    assert all(len(v) == len(NS) for t in (WS_FLOATS, PARTIAL_ROWS, PARTIAL_FLOATS) for v in t.values())


@pytest.mark.parametrize("k,o", KO)
def test_sizes_are_those_of_the_commit_before(lib, k, o):
    for ng in (1, 3, 5):
        assert tuple(lib.pdf_rowlin_wgrad_ws_floats(n, k, o, ng) for n in NS) == WS_FLOATS[k, o, ng], ng
    assert tuple(lib.pdf_rowlin_partial_rows(n, k, o) for n in NS) == PARTIAL_ROWS[k, o]
    assert tuple(lib.pdf_rowlin_partial_floats(n, o) for n in NS) == PARTIAL_FLOATS[o]


def test_forward_refuses_before_any_launch(lib, buf):
    x, w, y = ptr(buf, 0), ptr(buf, 1), ptr(buf, 2)
    fw = lambda n, ldx, mma: lib.pdf_rowlin_forward(n, 32, 32, x, ldx, w, 0, None, None, None, 0, y, 32, 0, None, mma, None)
    assert fw(0, 32, 0) == BAD
    assert fw(100, 31, 0) == BAD
    assert fw(100, 32, 3) == BAD and fw(100, 32, -1) == BAD


def test_multi_refuses_before_any_launch(lib, buf):
    t = table(buf, 4)
    mu = lambda nin, nout: lib.pdf_rowlin_multi(100, 32, 32, nin, nout, t, 32, t, 0, None, None, None, 0, t, 32, 0, 0, None)
    assert mu(4, 1) == BAD
    assert mu(2, 2) == BAD


def test_weight_gradient_group_refuses_before_any_launch(lib, buf):
    t6, none6, relu, ws = table(buf, 6), (P * 6)(), (I * 6)(), ptr(buf, 3)
    wg = lambda k, ng, scale, shift: lib.pdf_rowlin_wgrad_group(100, k, 32, ng, t6, 32, t6, k, scale, shift, relu, t6, None, ws, 0, None)
    assert wg(32, 6, none6, none6) == BAD
    assert wg(32, 2, None, none6) == BAD
    assert wg(32, 2, t6, none6) == BAD                          # scale[i] without shift[i]
    assert wg(48, 2, none6, none6) == UNSUPPORTED


def test_shapes_outside_the_streaming_kernels_are_unsupported(lib, buf):
    t3, a, b, c, d = table(buf, 3), ptr(buf, 0), ptr(buf, 1), ptr(buf, 2), ptr(buf, 3)
    rows = I(0)
    assert lib.pdf_rowlin_dgrad_bstats(100, 48, 32, 1, t3, 48, t3, a, 32, b, 32, c, 1, d, ctypes.addressof(rows), 0, None) == UNSUPPORTED
    assert lib.pdf_rowlin_forward_roww(100, 32, 24, a, 32, b, 0, c, 24, 0, d, 1, 0, None) == UNSUPPORTED
    assert lib.pdf_rowlin_wgrad_roww(100, 32, 24, a, 24, b, 32, c, d, 1, ptr(buf, 4), 0, None) == UNSUPPORTED

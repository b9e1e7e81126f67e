"""CPU suite: the size query and the ABI behind the launches paired in a Bottleneck's backward and a TransitionDown's forward."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pointcloudpdf_amd import _abi, build

    lib = ctypes.CDLL(build.build_library())
    _abi.bind(lib)
    return lib


# (rows, cin) of the model's four TransitionDown nodes at 2 x 100k points, and two small ones
@pytest.mark.parametrize("n,cin", [(200000, 32), (50000, 64), (12500, 128), (3124, 256), (300, 32), (97, 256)])
def test_td_forward_scratch_holds_both_workspaces(lib, n, cin):
    """The two Gram products of pdf_td_forward run in one launch: each needs its own slabs."""
    a, b = lib.pdf_rowlin_wgrad_ws_floats(n, cin, cin, 1), lib.pdf_rowlin_wgrad_ws_floats(n, cin, 32, 1)
    assert a > 0 and b > 0
    assert lib.pdf_td_fwd_scratch_floats(n, cin) == a + b


def test_abi_22_in_header_library_and_binding(lib):
    from pointcloudpdf_amd import _abi, _native

    header = open(os.path.join(ROOT, "include", "pdfops.h")).read()
    assert int(re.search(r"#define\s+PDF_ABI_VERSION\s+(\d+)", header).group(1)) == 22
    assert lib.pdf_abi_version() == 22 and _native.ABI_VERSION == 22
    assert _abi.ENTRIES["pdf_rowlin_wgrad_group_dgrad"] == ("s", "liiiplplpppppppppipip")
    assert _abi.ENTRIES["pdf_rowlin_wgrad2_roww"] == ("s", "liiliipplpip")


def test_paired_entry_validates_before_launching(lib):
    """Null tables and a bad product-input mode are refused without a device."""
    f = lib.pdf_rowlin_wgrad_group_dgrad
    took = ctypes.c_int(7)
    assert f(64, 32, 32, 5, None, 32, None, 32, None, None, None, None, None, None, None, None, None, 0, ctypes.byref(took), 0, None) == -1
    assert took.value == 0
    assert f(64, 32, 32, 5, None, 32, None, 32, None, None, None, None, None, None, None, None, None, 0, None, 3, None) == -1

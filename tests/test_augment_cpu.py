"""CPU suite: host side of the device augmentation (pointcloudpdf_amd/augment.py) -- list parsing, scene-key draws, the Philox
convention the kernel follows, and GridSample's dispatch of float64 coordinates to pdf_grid_hash_f64."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = (1 << 64) - 1


def _philox(ctr, key):
    """Philox4x64-10 as csrc/augment.hip computes it (Python integers)."""
    c, k0, k1 = list(ctr), key & M64, key >> 64
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B97F4A7C15) & M64, (k1 + 0xBB67AE8584CAA73B) & M64
        p0, p1 = 0xD2E7470EE14C6C93 * c[0], 0xCA5A826395121157 * c[2]
        c = [(p1 >> 64) ^ c[1] ^ k0, p1 & M64, (p0 >> 64) ^ c[3] ^ k1, p0 & M64]
    return c


def test_philox_convention_matches_numpy():
    """numpy.random.Philox(counter=c, key=k).random_raw(4) is the block of counter c + 1."""
    for key in (0, 5, (1 << 64) + 7):
        for c in (0, 17, M64):
            want = [int(v) for v in np.random.Philox(counter=c, key=key).random_raw(4)]
            assert _philox([(c + 1) & M64, (c + 1) >> 64, 0, 0], key) == want


def test_compose_builds_every_pdf_list():
    from pointcloudpdf_amd import augment

    with open(os.path.join(GOLDEN, "pdf_train_transforms.json")) as f:
        lists = json.load(f)
    assert len(lists) == 5
    for name, cfgs in lists.items():
        pipe = augment.Compose(cfgs)
        assert [type(t).__name__ for t in pipe.transforms] == [c["type"] for c in cfgs], name


def test_unknown_type_is_refused_by_name():
    from pointcloudpdf_amd import augment

    with pytest.raises(KeyError, match="RandomShift"):
        augment.Compose([dict(type="RandomScale"), dict(type="RandomShift", shift=[0.2, 0.2, 0.2])])


def test_scene_key_draws_are_deterministic_and_differ_across_keys():
    from pointcloudpdf_amd import augment

    a = [augment.SceneDraws(7).rand() for _ in range(2)]
    d1, d2, d3 = augment.SceneDraws(7), augment.SceneDraws(7), augment.SceneDraws(8)
    s1 = [d1.random(), d1.rand(), d1.uniform(0.9, 1.1)]
    s2 = [d2.random(), d2.rand(), d2.uniform(0.9, 1.1)]
    s3 = [d3.random(), d3.rand(), d3.uniform(0.9, 1.1)]
    assert s1 == s2 and s1 != s3 and a[0] == a[1]
    assert 0.9 <= s1[2] < 1.1


def test_recorded_draws_are_checked_in_order():
    from pointcloudpdf_amd import augment

    r = augment.RecordedDraws([("random", np.array(0.25)), ("uniform", np.array([1.05]))])
    assert r.random() == 0.25
    with pytest.raises(RuntimeError, match="uniform"):
        r.rand()


class _Spy:
    def __init__(self):
        self.calls = []

    def grid_hash(self, coord, offset, gs, min_grid, f32):
        self.calls.append(("grid_hash", coord.dtype))
        return self._out(coord)

    def grid_hash_f64(self, coord, offset, gs, min_grid):
        self.calls.append(("grid_hash_f64", coord.dtype))
        return self._out(coord)

    @staticmethod
    def _out(coord):
        g = torch.floor(coord.double() / 0.5).long()
        g -= g.min(0)[0]
        return g, g[:, 0] * 1000003 + g[:, 1] * 1009 + g[:, 2]


def test_grid_sample_dispatches_on_coordinate_dtype():
    from pointcloudpdf_amd import _native, voxelize

    spy = _Spy()
    prev = _native._set_backend_for_testing(spy)
    try:
        c = torch.rand(50, 3, dtype=torch.float64)
        off = torch.tensor([20, 50], dtype=torch.int32)
        voxelize.grid_sample(c, off, 0.5)
        voxelize.grid_sample(c.float(), off, 0.5)
        with pytest.raises(ValueError):
            voxelize.grid_sample(c, off, 0.5, float32_division=True)
    finally:
        _native._set_backend_for_testing(prev)
    assert spy.calls == [("grid_hash_f64", torch.float64), ("grid_hash", torch.float32)]


def test_augment_entries_validate_before_any_launch():
    import ctypes

    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    lib.pdf_aug_points.restype = I
    lib.pdf_aug_points.argtypes = [I, L, P, I, P, P, P, P, P, P, P]
    lib.pdf_aug_bounds.argtypes = [I, P, P, P, P, P, P]
    lib.pdf_philox4x64.argtypes = [L, L, L, L, P, P]
    lib.pdf_grid_hash_f64.argtypes = [L, I, P, P, ctypes.c_double, ctypes.c_double, ctypes.c_double, P, P, P, P]
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, P)
    assert lib.pdf_aug_points(0, 10, p, 1, p, None, None, p, None, None, None) == -1      # no scene
    assert lib.pdf_aug_points(1, 10, None, 1, p, None, None, p, None, None, None) == -1   # no offsets
    assert lib.pdf_aug_points(1, 0, p, 1, p, None, None, p, None, None, None) == 0        # no points
    assert lib.pdf_aug_bounds(1, p, None, None, p, p, None) == -1
    assert lib.pdf_philox4x64(-1, 0, 0, 0, p, None) == -1
    assert lib.pdf_grid_hash_f64(10, 1, p, p, 0.0, 1.0, 1.0, p, p, p, None) == -1          # grid size 0
    assert lib.pdf_aug_bounds_workspace_doubles(2) == 2 * 64 * 12

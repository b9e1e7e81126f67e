"""CPU suite: the adaptive search radius of the PDF pseudo-label pass (the reference's adaptive_radius=True, pointpdf_v1m1_base.py:137-149)
on the oracle path, and the recognizer that builds its own pass from a reference config section.  No golden fixture for the adaptive
branch (see adaptive_cases.py): equality against a brute-force restatement."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_cases  # noqa: E402

# configs/scannet/openseg-pt-v1-0-pointpdf-v1m1-base.py:40-58 (the arguments upstream's class takes)
SCANNET_RECOGNIZER = dict(
    type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"),
    criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)], loss_weight=0.04, step_loss_weight=False, num_classes=20,
    start_epoch=61, kp_ball_radius=0.02 * 5, kp_max_neighbor=64, condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15,
    num_seed=100, slide_window=True, adaptive_radius=False)


@pytest.fixture(scope="module")
def scenes():
    return adaptive_cases.five_scenes()


def test_adaptive_radii_is_the_reference_expression(scenes):
    from pointcloudpdf_amd import pseudo_label as pl

    coord, offset, shortest = scenes
    radii = pl.adaptive_radii(coord, offset)
    assert radii.dtype == torch.float32 and radii.shape == (5,)
    s = 0
    for i, e in enumerate(offset.tolist()):
        c = coord[s:e]
        ext = (c.max(0)[0] - c.min(0)[0] + 1e-6) / 16
        assert radii[i] == ext.min()
        if shortest[i] is not None:
            assert int(ext.argmin()) == shortest[i]
        s = e
    assert radii[2] == (torch.tensor(2.0) + 1e-6) / 16 and abs(float(radii[2]) - 0.125) < 1e-7 and radii[3] == torch.tensor(1e-6) / 16 and radii[4] == torch.tensor(1e-6) / 16


def test_flat_scene_holds_pairs_beyond_its_natural_cell_but_within_the_accepted_distance(scenes):
    """Scene (e) is what shows a grid whose cells follow the radius alone: its radius is 6e-8, the cell its extents and point count ask for
    (the setup kernel's cbrt(volume / n), at least longest / 1000) is below a millimetre, and `d2 <= 1e-5` accepts pairs up to 3.16 mm apart."""
    coord, offset, _ = scenes
    ends = offset.tolist()
    c = coord[ends[3]:ends[4]]
    ext = (c.max(0)[0] - c.min(0)[0]).clamp(min=1e-6)
    cell = max(float((ext.prod() / c.shape[0]) ** (1.0 / 3.0)), float(ext.max()) / 1000.0)
    d2 = ((c[:, None] - c[None]) ** 2).sum(-1)
    pairs = (d2 <= 1e-5) & ~torch.eye(c.shape[0], dtype=torch.bool)
    beyond = pairs & (d2 > (2 * cell) ** 2)          # farther apart than two cells: outside the 27 cells of such a grid for certain
    assert cell < 1e-3 and int(pairs.sum()) // 2 >= 8 and int(beyond.sum()) // 2 >= 5, (cell, int(pairs.sum()), int(beyond.sum()))


@pytest.mark.parametrize("k", [64, 8])
def test_adaptive_radius_neighbors_equal_brute_force(use_oracle, scenes, k):
    from pointcloudpdf_amd import pseudo_label as pl

    coord, offset, _ = scenes
    want = adaptive_cases.brute_force(coord, offset, pl.adaptive_radii(coord, offset), k)
    got = pl.radius_neighbors(coord, offset, "adaptive", k)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    raw = pl.radius_neighbors(coord, offset, "adaptive", k, raw=True)
    assert raw.dtype == torch.int32 and torch.equal(raw.long(), want)
    # the table is not the fixed-radius one, every point whose row is not full finds itself, the cluster fills its rows, the degenerate scenes hold only themselves
    assert not torch.equal(got, pl.radius_neighbors(coord, offset, 0.1, k))
    own = torch.arange(coord.shape[0])
    assert ((got == own[:, None]).sum(1) == 1)[(got < 0).any(1)].all()
    ends = offset.tolist()
    assert (got[ends[1]:ends[1] + 600] >= 0).all()
    assert torch.equal(got[ends[2]:ends[3]], torch.tensor([[ends[2]] + [-1] * (k - 1)]))
    assert int((got[ends[3]:] >= 0).sum()) >= 300 + 16          # the flat scene: itself + the pairs within 3.16 mm
    empty = torch.tensor([ends[0], ends[0], ends[1]], dtype=torch.int32)          # a scene without points: extent 0
    assert pl.adaptive_radii(coord[:ends[1]], empty)[1] == torch.tensor(1e-6) / 16
    assert torch.equal(pl.radius_neighbors(coord[:ends[1]], empty, "adaptive", k), got[:ends[1]])
    with pytest.raises(ValueError):
        pl.radius_neighbors(coord, offset, "adaptiv", k)


def test_recognizer_builds_its_pass_from_the_config_section():
    from pointcloudpdf_amd import recognizer  # noqa: F401  (registers the classes)
    from pointcloudpdf_amd.registry import RECOGNIZER

    rec = RECOGNIZER.build(SCANNET_RECOGNIZER)
    assert rec.pseudo_mask_fn is not None and rec.pseudo_mask_fn.prepass_plan == {"radius": (0.1, 64)}
    assert rec.pseudo_mask_fn.capturable and rec.pseudo_mask_fn.accepts_geometry and rec.pseudo_mask_fn.accepts_offset_host
    rec = RECOGNIZER.build(dict(SCANNET_RECOGNIZER, adaptive_radius=True))
    assert rec.pseudo_mask_fn.prepass_plan == {"radius": ("adaptive", 64)}

    def mine(coord, seg_logits, offset):
        return torch.zeros(coord.shape[0], dtype=torch.bool)

    rec = RECOGNIZER.build(dict(SCANNET_RECOGNIZER, adaptive_radius=True, pseudo_mask_fn=mine))
    assert rec.pseudo_mask_fn is mine
    bare = {k: v for k, v in SCANNET_RECOGNIZER.items() if k not in ("kp_ball_radius", "kp_max_neighbor")}
    rec = RECOGNIZER.build(bare)
    assert rec.pseudo_mask_fn is None
    with pytest.raises(NotImplementedError):
        rec.get_pseudo_mask(torch.zeros(4, 3), torch.zeros(4, 20), torch.tensor([4], dtype=torch.int32))


def test_config_built_pass_runs_the_section_s_settings(use_oracle, monkeypatch):
    """The pass the recognizer builds hands the section's arguments to ``get_pseudo_mask`` (adaptive radius included)."""
    from pointcloudpdf_amd import pseudo_label as pl, recognizer  # noqa: F401
    from pointcloudpdf_amd.registry import RECOGNIZER

    seen = {}

    def spy(coord, seg_logits, offset, **kw):
        seen.update(kw)
        return torch.zeros(coord.shape[0], dtype=torch.bool)

    monkeypatch.setattr(pl, "get_pseudo_mask", spy)
    rec = RECOGNIZER.build(dict(SCANNET_RECOGNIZER, adaptive_radius=True, beta=2, num_seed=50))
    rec.get_pseudo_mask(torch.zeros(4, 3), torch.zeros(4, 20), torch.tensor([4], dtype=torch.int32))
    assert seen["radius"] == "adaptive" and seen["max_neighbor"] == 64 and seen["neighbors"] is None
    assert {k: seen[k] for k in ("condition_from", "beta", "seed_from", "seed_range", "num_seed", "slide_window")} == dict(
        condition_from="msp", beta=2, seed_from="ml", seed_range=0.15, num_seed=50, slide_window=True)


def test_adaptive_entry_validates_before_any_launch():
    """pdf_radius_neighbors_self_adaptive: null pointers, more than 64 scenes, a divisor <= 0, a negative pad, a bad nsample and a short
    workspace are argument errors before anything is launched (no GPU needed); no points: nothing to do."""
    import ctypes

    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    I, F, P, L = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_long
    f = lib.pdf_radius_neighbors_self_adaptive
    f.restype, f.argtypes = I, [I, I, F, F, P, P, I, P, P, P, P, L, P]
    lib.pdf_knn_workspace_bytes.restype, lib.pdf_knn_workspace_bytes.argtypes = L, [I, I, I]
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)
    need = lib.pdf_knn_workspace_bytes(2, 10, 0)
    BAD, NSAMPLE = -1, -2
    assert f(0, 8, 16.0, 1e-6, p, p, 2, p, p, p, p, need, None) == 0
    assert f(-1, 8, 16.0, 1e-6, p, p, 2, p, p, p, p, need, None) == BAD
    assert f(10, 8, 16.0, 1e-6, None, p, 2, p, p, p, p, need, None) == BAD
    assert f(10, 8, 16.0, 1e-6, p, p, 2, p, p, None, p, need, None) == BAD          # no radii
    assert f(10, 8, 16.0, 1e-6, p, p, 65, p, p, p, p, need, None) == BAD
    assert f(10, 8, 16.0, 1e-6, p, p, 0, p, p, p, p, need, None) == BAD
    assert f(10, 8, 0.0, 1e-6, p, p, 2, p, p, p, p, need, None) == BAD
    assert f(10, 8, float("nan"), 1e-6, p, p, 2, p, p, p, p, need, None) == BAD
    assert f(10, 8, 16.0, -1.0, p, p, 2, p, p, p, p, need, None) == BAD
    assert f(10, 0, 16.0, 1e-6, p, p, 2, p, p, p, p, need, None) == NSAMPLE
    assert f(10, 1025, 16.0, 1e-6, p, p, 2, p, p, p, p, need, None) == NSAMPLE
    assert f(10, 8, 16.0, 1e-6, p, p, 2, p, p, p, None, need, None) == BAD          # no workspace
    assert f(10, 8, 16.0, 1e-6, p, p, 2, p, p, p, p, need - 1, None) == BAD         # short workspace

"""GPU suite: the per-scene adaptive search radius of the PDF pseudo-label pass on the device (pdf_radius_neighbors_self_adaptive), through the
pre-pass, the captured training step and a recognizer built from a reference config section.  Every comparison is equality.  No golden
fixture for the adaptive branch (see adaptive_cases.py): the radii are pinned against ``pseudo_label.adaptive_radii`` (the reference's
expression), the table against the fixed-radius entry called scene by scene with that radius."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_cases  # noqa: E402

pytestmark = pytest.mark.gpu

CE = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]
PASS = dict(condition_from="msp", beta=1.5, seed_from="ml", seed_range=0.15, num_seed=100, slide_window=True)
# configs/scannet/openseg-pt-v1-0-pointpdf-v1m1-base.py:40-58
SCANNET_RECOGNIZER = dict(type="PointPdf-v1m1", recognizer=dict(type="PointTransformer-Recognizer"), criteria=CE, loss_weight=0.04,
                          step_loss_weight=False, num_classes=20, start_epoch=61, kp_ball_radius=0.02 * 5, kp_max_neighbor=64,
                          adaptive_radius=False, **PASS)


@pytest.fixture(scope="module")
def scenes():
    coord, offset, _ = adaptive_cases.five_scenes()
    from pointcloudpdf_amd import pseudo_label as pl

    return coord.cuda(), offset.cuda(), offset.tolist(), pl.adaptive_radii(coord, offset)


@pytest.mark.parametrize("nsample", [64, 8])
def test_table_and_radii_are_exact_on_the_five_scene_batch(scenes, nsample):
    from pointcloudpdf_amd import _native, pseudo_label as pl

    hip = _native.hip_backend()
    coord, offset, ends, want_radii = scenes
    idx, dist2, radii = hip.radius_neighbors_self_adaptive(nsample, coord, offset)
    assert idx.dtype == torch.int32 and idx.shape == dist2.shape == (coord.shape[0], nsample)
    assert torch.equal(radii.cpu(), want_radii) and torch.equal(pl.adaptive_radii(coord, offset), radii)
    s = 0
    for e, r in zip(ends, want_radii.tolist()):
        i1, d1 = hip.radius_neighbors_self(nsample, float(r), coord[s:e].contiguous(), torch.tensor([e - s], dtype=torch.int32, device="cuda"))
        assert torch.equal(idx[s:e], torch.where(i1 >= 0, i1 + s, i1)), (s, e)
        assert torch.equal(dist2[s:e], d1), (s, e)
        s = e
    # ... and the contract itself, restated without any grid (the fixed entry above walks the same cells as the adaptive one)
    want = adaptive_cases.brute_force(coord.cpu(), offset.cpu(), want_radii, nsample)
    assert torch.equal(idx.cpu().long(), want)
    flat = idx[ends[3]:ends[4]]
    assert int((flat >= 0).sum()) >= 300 + 16                    # scene (e): pairs within 3.16 mm, several grid cells of 0.67 mm apart
    # the cluster of scene (c) overflows the kernel's candidate list (its rows are the scene's first points), the degenerate scenes find themselves
    c0 = ends[1]
    first = torch.arange(c0, c0 + nsample, dtype=torch.int32, device="cuda")
    assert torch.equal(idx[c0 + 700], first) and torch.equal(idx[c0 + 5], first)
    assert idx[ends[2]].tolist() == [ends[2]] + [-1] * (nsample - 1) and float(dist2[ends[2], 0]) == 0.0
    assert torch.equal(pl.radius_neighbors(coord, offset, "adaptive", nsample, raw=True), idx)
    assert torch.equal(pl.radius_neighbors(coord, offset, "adaptive", nsample), idx.long())


def test_more_than_64_scenes_fall_back_to_one_query_per_scene(monkeypatch):
    """65 small scenes (one of them without points): the grid workspace holds 64, so the backend queries scene by scene with the radii read
    on the host -- same radii, same table as the brute force -- and refuses to do that while the stream is capturing."""
    from pointcloudpdf_amd import _native, pseudo_label as pl

    hip = _native.hip_backend()
    g = torch.Generator().manual_seed(9)
    sizes = [40 + (i * 7) % 23 for i in range(65)]
    sizes[17] = 0
    coord = torch.cat([torch.rand(n, 3, generator=g) * torch.tensor([1.0 + 0.1 * (i % 5), 0.8, 0.5 + 0.05 * (i % 3)]) for i, n in enumerate(sizes)])
    offset = torch.tensor(np.cumsum(sizes), dtype=torch.int32)
    want_radii = pl.adaptive_radii(coord, offset)
    assert want_radii[17] == torch.tensor(1e-6) / 16
    idx, dist2, radii = hip.radius_neighbors_self_adaptive(16, coord.cuda(), offset.cuda())
    assert torch.equal(radii.cpu(), want_radii) and idx.shape == dist2.shape == (sum(sizes), 16)
    assert torch.equal(idx.cpu().long(), adaptive_cases.brute_force(coord, offset, want_radii, 16))
    # the first 64 scenes alone go through the one-call entry: the same rows
    n64 = int(offset[63])
    i64, d64, r64 = hip.radius_neighbors_self_adaptive(16, coord[:n64].cuda(), offset[:64].cuda())
    assert torch.equal(i64, idx[:n64]) and torch.equal(d64, dist2[:n64]) and torch.equal(r64, radii[:64])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)   # (no capture is begun: the refusal comes before any device work)
    with pytest.raises(_native.PdfOpsError, match="capture"):
        hip.radius_neighbors_self_adaptive(16, coord.cuda(), offset.cuda())


def test_prepass_hands_out_the_adaptive_table(monkeypatch):
    from pointcloudpdf_amd import engine, pseudo_label as pl, synthetic
    from pointcloudpdf_amd.geometry import Geometry

    fn = pl.make_pseudo_mask_fn(radius="adaptive", max_neighbor=64, **PASS)
    plan = fn.prepass_plan
    assert plan == {"radius": ("adaptive", 64)} and fn.capturable
    # two batches whose scenes have different extents (rooms of 9,000 / 7,000 points; a larger room and a small crop)
    batches = [synthetic.make_batch(sz, first_scene_id=40 + 3 * i, kind="scannet", device="cuda") for i, sz in enumerate([[9000, 7000], [12000, 3000]])]
    inline = [pl.radius_neighbors(b["coord"], b["offset"], "adaptive", 64, raw=True) for b in batches]
    radii = torch.cat([pl.adaptive_radii(b["coord"], b["offset"]) for b in batches]).tolist()
    assert len(set(radii)) == 4
    for b, want in zip(batches, inline):
        g = Geometry(b["coord"], b["offset"], b["offset_host"]).precompute(**plan)
        got = g.radius_cached("adaptive", 64)
        assert got is not None and got.dtype == torch.int32 and torch.equal(got, want)
        assert g.radius_cached(0.1, 64) is None and g.radius("adaptive", 64) is got
    grouped = list(engine.GroupedGeometryLoader(iter(batches), group=2, **plan))
    torch.cuda.synchronize()
    assert len(grouped) == 2
    for b, want in zip(grouped, inline):
        assert torch.equal(b["pdf_geometry"].radius_cached("adaptive", 64), want)
    # the pass reads the pre-pass's table and runs no query of its own
    calls = []
    real = pl.radius_neighbors
    monkeypatch.setattr(pl, "radius_neighbors", lambda *a, **k: calls.append(a[2]) or real(*a, **k))
    gen = torch.Generator(device="cuda").manual_seed(2)
    for b in grouped:
        logits = 0.4 * torch.randn(b["coord"].shape[0], 20, device="cuda", generator=gen)
        torch.cuda.manual_seed(11)
        want = fn(b["coord"], logits, b["offset"], offset_host=b["offset_host"])
        assert calls == ["adaptive"]
        torch.cuda.manual_seed(11)
        got = fn(b["coord"], logits, b["offset"], offset_host=b["offset_host"], geometry=b["pdf_geometry"])
        assert calls == ["adaptive"] and torch.equal(got, want)
        calls.clear()


def test_captured_step_with_the_adaptive_pass_is_one_graph():
    from pointcloudpdf_amd import engine, pseudo_label as pl, synthetic
    from pointcloudpdf_amd.geometry import Geometry

    dev = torch.device("cuda", 0)
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=dict(type="PointTransformer-Seg26", in_channels=9, num_classes=20), criteria=CE),
               recognizer=dict(SCANNET_RECOGNIZER, start_epoch=0, adaptive_radius=True))
    step = engine.build_open_seg_step(cfg).to(dev)
    synthetic.fill_parameters_deterministic(step, seed=3)
    step.train()
    assert step.prepass_plan == {"radius": ("adaptive", 64)} and step.recognizer.pseudo_mask_fn.capturable
    batch = synthetic.make_batch([2048, 1600], first_scene_id=20, kind="scannet", device=dev, unknown=(4, 7, 14, 16))
    geom = Geometry(batch["coord"], batch["offset"], batch["offset_host"]).precompute()   # (no radius table: the pass queries inside the step)
    state = {k: v.detach().clone() for k, v in step.state_dict().items()}
    params = [p for p in step.parameters() if p.requires_grad]

    def three(run):
        step.load_state_dict(state)
        torch.cuda.manual_seed(7)       # the pass draws its seeds from the device generator
        res = []
        for _ in range(3):
            for p in params:
                p.grad = None
            out = run()
            torch.cuda.synchronize()
            res.append((out["loss"].detach().clone(), out["recognizer_loss"].detach().clone(), out["score"].detach().clone(),
                        [p.grad.detach().clone() for p in params]))
        return res

    def eager_step():
        out = step(dict(batch, pdf_geometry=geom))
        out["loss"].backward()
        return out

    eager = three(eager_step)
    logits = step.hooks["backbone"]["forward_output"].detach().clone()
    engine.release_autograd_state(step)
    cap = engine.CapturedStep(step, batch, geom=geom)
    assert cap.graph is not None and cap.graph2 is None and cap.segments is None     # ONE graph: the radii never came to the host
    replayed = three(lambda: cap(batch, geom))
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (i, float(a[0]), float(b[0]))
        assert float(a[1]) > 0
        bad = [j for j, (x, y) in enumerate(zip(a[3], b[3])) if not torch.equal(x, y)]
        assert not bad, (i, len(bad))
    # the option is honoured: not the mask of the fixed radius
    fixed = pl.make_pseudo_mask_fn(radius=0.1, max_neighbor=64, **PASS)
    torch.cuda.manual_seed(5)
    m_adaptive = step.recognizer.get_pseudo_mask(batch["coord"], logits, batch["offset"], batch["offset_host"])
    torch.cuda.manual_seed(5)
    m_fixed = fixed(batch["coord"], logits, batch["offset"], offset_host=batch["offset_host"])
    assert m_adaptive.shape == m_fixed.shape and not torch.equal(m_adaptive, m_fixed)
    engine.release_autograd_state(step)


def test_config_built_recognizer_trains_past_start_epoch():
    from pointcloudpdf_amd import engine, pseudo_label as pl, synthetic
    from pointcloudpdf_amd.registry import RECOGNIZER

    step = engine.OpenSegStep(in_channels=9, num_classes=20, loss_weight=0.04)
    rec = RECOGNIZER.build(dict(SCANNET_RECOGNIZER, start_epoch=0))            # no function passed: the section's own pass
    assert rec.pseudo_mask_fn is not None and rec.pseudo_mask_fn is not engine.default_pseudo_mask
    rec.model_hooks = step.hooks
    rec.set_epoch(0)
    rec.trigger_operation()
    step.recognizer = rec
    step = step.cuda()
    synthetic.fill_parameters_deterministic(step, seed=4)
    step.train()
    batch = synthetic.make_batch([6000, 5000], first_scene_id=60, kind="scannet", device="cuda", unknown=(4, 7, 14, 16))
    np.random.seed(0)
    out = step(batch)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]).item() and float(out["recognizer_loss"]) > 0
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in step.parameters())
    logits = step.hooks["backbone"]["forward_output"].detach().clone()
    hand = pl.make_pseudo_mask_fn(radius=0.02 * 5, max_neighbor=64, **PASS)
    torch.cuda.manual_seed(9)
    got = rec.get_pseudo_mask(batch["coord"], logits, batch["offset"], batch["offset_host"])
    torch.cuda.manual_seed(9)
    want = hand(batch["coord"], logits, batch["offset"], offset_host=batch["offset_host"])
    assert torch.equal(got, want) and 0 < int(want.sum()) < want.numel()
    engine.release_autograd_state(step)

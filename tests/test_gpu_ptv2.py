"""GPU suite: PointTransformer-V2 (PT-v2m2) -- csrc/grid_pool.hip and csrc/gva.hip against the torch compositions of
pointcloudpdf_amd/point_transformer_v2.py on the same device tensors, and the model against the fixture of the reference's own class
(tests/golden/model_ptv2_ref.npz).

Tolerances (nothing measured goes into them).  Grid pooling: exact.  The GVA nodes: the error against the composition evaluated in float64
is at most 2x the float32 composition's own error against it, and never has to be closer than 4 fp32 ulps of the result's largest
magnitude (criteria_cases.bound: the rule of test_gpu_criteria.py).  Model: logits / loss within helpers.REL_TOL, gradients by the rule
of tests/ptv2_cases.py."""
import os

import numpy as np
import pytest
import torch

import criteria_cases as cc
import helpers
import ptv2_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ptv2():
    from pointcloudpdf_amd import point_transformer_v2

    return point_transformer_v2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "model_ptv2_ref.npz"))


@pytest.fixture(scope="module")
def batch():
    return pc.batch("cuda")


# ---- grid pooling ---------------------------------------------------------------------------------------------------------------------
def _pool_case(name):
    g = torch.Generator().manual_seed(31)
    if name == "one_point":
        return torch.tensor([[0.3, 1.7, 0.2]]), [1], 0.1
    if name == "single_cell":
        return 5.0 + 0.09 * torch.rand(300, 3, generator=g), [300], 0.1
    if name == "three_uneven":   # 2,049 and 4,097: one past the sort's 2,048-key tile, one past two tiles
        sizes = [7, 2049, 4097]
        return torch.rand(sum(sizes), 3, generator=g) * torch.tensor([6.0, 4.0, 2.5]), sizes, 0.25
    if name == "borders":        # coordinates snapped to multiples of the cell size: points on cell borders
        sizes = [900, 1300]
        return torch.randint(0, 40, (sum(sizes), 3), generator=g).float() * 0.1, sizes, 0.1
    if name == "huge_grid":      # 100 m at a 0.01 m cell: 10^12 cells, more than 2^32
        sizes = [1500, 1500]
        xyz = torch.rand(sum(sizes), 3, generator=g) * 100.0
        xyz[::3] = xyz[1::3][: xyz[::3].shape[0]] + 0.001 * torch.rand(xyz[::3].shape, generator=g)   # (some shared cells)
        return xyz, sizes, 0.01
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_point", "single_cell", "three_uneven", "borders", "huge_grid"])
def test_grid_pooling_equals_the_composition(ptv2, name):
    xyz, sizes, cell = _pool_case(name)
    xyz = xyz.cuda().contiguous()
    offset = torch.tensor(sizes).cumsum(0).int().cuda()
    ref = ptv2.grid_partition_torch(xyz, offset, cell)
    got = ptv2.grid_partition(xyz, offset, cell)
    assert got.m == ref.m and got.cluster.dtype == torch.int64
    if name == "huge_grid":
        batch_ids = ptv2.offset2batch(offset, xyz.shape[0])
        keys = ptv2.voxel_keys(xyz - ptv2.scene_bounds(xyz, offset)[0][batch_ids], batch_ids, cell)
        assert int(keys.max()) > 2 ** 32
    if name == "single_cell":
        assert got.m == 1
    for field in ("cluster", "idx_ptr", "sorted", "offset"):
        assert torch.equal(getattr(got, field).long(), getattr(ref, field).long()), field
    assert torch.equal(got.counts.long(), ref.counts.long())
    assert torch.equal(got.coord, ref.coord), "pooled coordinates are bit-exact"
    g = torch.Generator().manual_seed(32)
    for c in (7, 48, 96):
        feat = torch.randn(xyz.shape[0], c, generator=g).relu_().cuda().requires_grad_(True)   # (after a ReLU: ties at zero)
        out, arg = ptv2._SegMax.apply(feat, got.cluster, got.idx_ptr, got.sorted)
        assert torch.equal(arg.long(), ptv2.segment_argmax_torch(feat, ref.idx_ptr, ref.sorted)), c
        out_ref = ptv2.segment_max_torch(feat, ref.idx_ptr, ref.sorted)
        assert torch.equal(out, out_ref), c
        w = torch.randn(got.m, c, generator=g).cuda()
        assert torch.equal(torch.autograd.grad((out * w).sum(), feat)[0], torch.autograd.grad((out_ref * w).sum(), feat)[0]), c
        coarse = torch.randn(got.m, c, generator=g).cuda().requires_grad_(True)
        up, up_ref = ptv2.map_unpool(coarse, got), ptv2.map_unpool_torch(coarse, ref)
        assert up.grad_fn.name().startswith("_MapUnpoolBackward") and torch.equal(up, up_ref), c
        wf = torch.randn(xyz.shape[0], c, generator=g).cuda()
        assert torch.equal(torch.autograd.grad((up * wf).sum(), coarse)[0], torch.autograd.grad((up_ref * wf).sum(), coarse)[0]), c


# ---- grouped vector attention ---------------------------------------------------------------------------------------------------------
SHAPES = [(48, 6, 8), (48, 6, 16), (96, 12, 16), (384, 48, 16), (512, 64, 16), (24, 3, 5), (32, 8, 16), (20, 2, 3)]
FUSED = {shape: shape[0] // shape[1] == 8 for shape in SHAPES}   # (32, 8, 16) and (20, 2, 3) lie outside the fused attend class


def _table(n, s, g):
    """A 5-point scene (rows padded with -1 past its five neighbours) next to a full scene."""
    small = min(5, n)
    idx = torch.full((n, s), -1, dtype=torch.int32)
    for i in range(small):
        row = torch.randperm(small, generator=g)[:s]
        idx[i, : row.shape[0]] = row.int()
    if n > small:
        idx[small:] = torch.randint(small, n, (n - small, s), generator=g, dtype=torch.int32)
    return idx


def _errors(got, ref32, ref64):
    return cc.err(got, ref64), cc.bound(cc.err(ref32, ref64), ref64)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"c{c}_g{g}_s{s}" for c, g, s in SHAPES])
def test_gva_nodes_against_the_float64_composition(ptv2, shape, n):
    c, groups, s = shape
    g = torch.Generator().manual_seed(1000 * c + 10 * s + n)
    idx = _table(n, s, g).cuda()
    mk = lambda *sh: torch.randn(*sh, generator=g).cuda()
    q, k, v, logits, pem, peb = mk(n, c), mk(n, c), mk(n, c), 2.0 * mk(n, s, groups), 1.0 + 0.5 * mk(n, s, c), mk(n, s, c)
    w_rel, w_out = mk(n, s, c), mk(n, c)
    for use_pem, use_peb in ((False, False), (True, False), (False, True), (True, True)):
        def evaluate(rel_fn, att_fn, dtype):
            ins = [t.to(dtype).requires_grad_(True) for t in (q, k, v, logits)]
            pm = pem.to(dtype).requires_grad_(True) if use_pem else None
            pb = peb.to(dtype).requires_grad_(True) if use_peb else None
            rel = rel_fn(ins[0], ins[1], idx, pm, pb)
            out = att_fn(ins[3], ins[2], pb, idx)
            wanted = ins + [t for t in (pm, pb) if t is not None]
            grads = torch.autograd.grad((rel * w_rel.to(dtype)).sum() + (out * w_out.to(dtype)).sum(), wanted)
            return [rel.detach(), out.detach()] + list(grads)

        names = ["rel", "out", "g_query", "g_key", "g_value", "g_logits"] + (["g_pem"] if use_pem else []) + (["g_peb"] if use_peb else [])
        ref64 = evaluate(ptv2.gva_relation_torch, ptv2.gva_attend_torch, torch.float64)
        ref32 = evaluate(ptv2.gva_relation_torch, ptv2.gva_attend_torch, torch.float32)
        got = evaluate(ptv2.gva_relation, ptv2.gva_attend, torch.float32)
        again = evaluate(ptv2.gva_relation, ptv2.gva_attend, torch.float32)
        probe = ptv2.gva_attend(logits.requires_grad_(True), v, peb if use_peb else None, idx)
        assert probe.grad_fn.name().startswith("_GvaAttendBackward") == FUSED[shape], "which path the attend node took"
        probe = ptv2.gva_relation(q.requires_grad_(True), k, idx, pem if use_pem else None, peb if use_peb else None)
        assert probe.grad_fn.name().startswith("_GvaRelationBackward"), "the relation node takes every shape"
        for name, a, b, r32, r64 in zip(names, got, again, ref32, ref64):
            assert torch.equal(a, b), f"{name}: two runs differ"
            e, bound = _errors(a, r32, r64)
            print(f"{shape} n={n} pem={use_pem} peb={use_peb} {name}: error {e:.3e} (composition {cc.err(r32, r64):.3e}, bound {bound:.3e})")
            assert e <= bound, (name, use_pem, use_peb, e, bound)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_model_matches_the_reference_class(ptv2, golden, batch, case):
    """Tables and pooled coordinates bit-exact, logits / loss within REL_TOL, gradients by the rule of ptv2_cases.  Measured on MI355X
    over the eight cases: logits 3.8e-7 ... 1.9e-6 and loss 0 (both against the reference's fp32 run), every stored gradient <= 2.0e-6 of its
    float64 run (the reference's own fp32 run: up to 1.9e-3 on four patch_embed tensors of the two cases without pe_multiplier); the
    test prints every figure."""
    torch.manual_seed(0)
    model = pc.build(ptv2.PointTransformerV2, case).cuda()
    geom = model.make_geometry(batch["coord"], batch["offset"], batch["offset_host"])
    out = pc.run(model, batch, pc.CASES[case][2], geometry=geom)
    pc.check_geometry(geom, golden)
    pc.check_case(case, out, golden, model, ptv2.PointBatchNorm, helpers.REL_TOL)


@pytest.mark.parametrize("backend", ["map", "interp"])
def test_geometry_handed_in_or_computed_inline_is_bit_identical(ptv2, batch, backend):
    model = pc.build(ptv2.PointTransformerV2, f"{backend}_pem_train").cuda()
    a = pc.run(model, batch, True)
    geom = model.make_geometry(batch["coord"], batch["offset"], batch["offset_host"])
    b = pc.run(model, batch, True, geometry=geom)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])
    for k, g in a["grads"].items():
        assert g is None or np.array_equal(g, b["grads"][k]), k


def test_three_evaluations_are_bit_identical(ptv2, batch):
    model = pc.build(ptv2.PointTransformerV2, "interp_pem_train").cuda()
    runs = [pc.run(model, batch, True) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r["loss"], runs[0]["loss"]) and torch.equal(r["logits"], runs[0]["logits"])
        for k, g in runs[0]["grads"].items():
            assert g is None or np.array_equal(g, r["grads"][k]), k


def test_model_runs_the_hip_nodes(ptv2, batch, monkeypatch):
    """No quiet fall-back: with every composition made to raise, forward + backward of the fixture model still run, and every HIP entry
    of the two kernel families is called."""
    from pointcloudpdf_amd import _native

    def refuse(name):
        def fn(*a, **k):
            raise AssertionError(f"{name}: the torch composition ran on device tensors")
        return fn

    for name in ("gva_relation_torch", "gva_attend_torch", "grid_partition_torch", "segment_mean_torch", "segment_max_torch", "map_unpool_torch"):
        monkeypatch.setattr(ptv2, name, refuse(name))
    be, calls = _native.hip_backend(), {}
    entries = ("grid_pool_partition", "grid_pool_mean", "grid_pool_max", "grid_pool_max_backward", "grid_unpool_forward", "grid_unpool_backward",
               "gva_relation_forward", "gva_relation_backward", "gva_attend_forward", "gva_attend_backward")
    for name in entries:
        def counted(*a, _fn=getattr(be, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(be, name, counted)
    model = pc.build(ptv2.PointTransformerV2, "map_pem_train").cuda()
    out = pc.run(model, batch, True)
    assert torch.isfinite(out["loss"])
    blocks = 1 + sum(pc.CFG["enc_depths"]) + sum(pc.CFG["dec_depths"])
    assert calls["grid_pool_partition"] == calls["grid_pool_mean"] == calls["grid_pool_max"] == calls["grid_pool_max_backward"] == 2
    assert calls["grid_unpool_forward"] == calls["grid_unpool_backward"] == 2
    for name in entries[6:]:
        assert calls[name] == blocks, (name, calls)


def test_batched_scenes_equal_the_scenes_alone(ptv2):
    """The partition starts at every scene's own minimum and only the key strides use the batch-wide maximum: in eval mode a batch is
    independent forwards."""
    from pointcloudpdf_amd import synthetic

    sizes = [1100, 700, 900]
    b = synthetic.make_batch(sizes, first_scene_id=40, grid_size=0.3, device="cuda")
    model = pc.build(ptv2.PointTransformerV2, "map_pem_eval").cuda()
    with torch.no_grad():
        whole = model.make_geometry(b["coord"], b["offset"], b["offset_host"])
        logits = model(dict(coord=b["coord"], feat=b["feat"], offset=b["offset"], ptv2_geometry=whole))
        ends = [0] + b["offset_host"]
        for s in range(3):
            a, z = ends[s], ends[s + 1]
            one = dict(coord=b["coord"][a:z].contiguous(), feat=b["feat"][a:z].contiguous(), offset=torch.tensor([z - a], dtype=torch.int32, device="cuda"))
            geom = model.make_geometry(one["coord"], one["offset"])
            alone = model(dict(one, ptv2_geometry=geom))
            helpers.assert_close(logits[a:z], alone, helpers.REL_TOL, f"scene {s} logits")
            lo, hi = a, z
            for i, part in enumerate(geom.stages):
                wp = whole.stages[i]
                c0 = int(wp.offset[s - 1]) if s else 0
                assert torch.equal(wp.cluster[lo:hi] - c0, part.cluster), (s, i)
                assert torch.equal(wp.sorted[lo:hi] - lo, part.sorted) and torch.equal(wp.coord[c0:int(wp.offset[s])], part.coord), (s, i)
                lo, hi = c0, int(wp.offset[s])
            lo, hi = a, z
            for level in range(3):
                for k in pc.LEVEL_NEIGHBOURS[level]:
                    t = whole.knn(level, k)[lo:hi]
                    assert torch.equal(torch.where(t >= 0, t - lo, t), geom.knn(level, k)), (s, level, k)
                if level < 2:
                    lo, hi = (int(whole.stages[level].offset[s - 1]) if s else 0), int(whole.stages[level].offset[s])


def _step_cfg(num_classes=13):
    bb = dict(type="PT-v2m2", unpool_backend="map", **dict(pc.CFG, num_classes=num_classes))
    criteria = [dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    return dict(model=dict(type="DefaultSegmentor", backbone=bb, criteria=criteria), recognizer=dict(type="MaxProbability", method="msp"),
                optimizer=dict(type="AdamW", lr=0.002, weight_decay=0.02))


def test_built_step_trains(ptv2, batch):
    from pointcloudpdf_amd import engine, optim, synthetic

    cfg = _step_cfg()
    step = engine.build_open_seg_step(cfg)
    synthetic.fill_parameters_deterministic(step, seed=5)
    step = step.cuda().train()
    opt = optim.build_optimizer(cfg["optimizer"], step)
    assert isinstance(opt, optim.FusedAdamW) and isinstance(step.model.backbone, ptv2.PointTransformerV2)
    data = dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"], segment=batch["segment"])
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss = step(data)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_openseg_tester_end_to_end(ptv2, golden_dir, monkeypatch):
    from pointcloudpdf_amd import engine, synthetic, testing
    from test_gpu_tester import make_cfg
    from test_tester_cpu import CASES, K, case_scene

    ref = np.load(os.path.join(golden_dir, "tester_ref.npz"))
    step = engine.build_open_seg_step(_step_cfg(K))
    synthetic.fill_parameters_deterministic(step, seed=6)
    step = step.cuda()
    scene = case_scene(ref, CASES["f32_center"])
    from pointcloudpdf_amd import geometry

    def no_prepass(*a, **k):
        raise AssertionError("the PT-v1 geometry pre-pass ran for a backbone that builds its own geometry")

    monkeypatch.setattr(geometry.Geometry, "__init__", no_prepass)
    tester = testing.OpenSegTester(step, make_cfg(2))
    st = tester.scene_tester
    assert st.own_geometry and st.st_backbone is None
    seen, forward = [], st.forward_fn

    def watched(b):
        seen.append(sorted(k for k in b if k.endswith("_geometry")))
        return forward(b)

    st.forward_fn = watched
    res = tester.test([scene])
    assert seen and all(keys == [] for keys in seen) and st._loader is None   # the batches reach the forward as they are
    assert 0 <= res["mIoU"] <= 1 and 0 <= res["auroc"] <= 1 and res["scenes"]["golden"]["aupr"] is not None

"""CPU suite: PointTransformer-V2 (PT-v2m2) -- the torch compositions of pointcloudpdf_amd/point_transformer_v2.py on the CPU oracle
against the fixture produced by the reference's OWN class (tests/golden/model_ptv2_ref.npz, tests/golden/make_golden_ptv2.py)."""
import os

import numpy as np
import pytest
import torch

import helpers
import ptv2_cases as pc

CPU_TOL = 1e-6   # logits and loss of the composition against the reference's fp32 run


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "model_ptv2_ref.npz"))


@pytest.fixture(scope="module")
def batch():
    return pc.batch()


def _ptv2():
    from pointcloudpdf_amd import point_transformer_v2

    return point_transformer_v2


@pytest.mark.parametrize("pem", [False, True])
def test_state_dict_keys_are_the_reference_keys(golden, pem):
    m = pc.build(_ptv2().PointTransformerV2, "map_pem_train" if pem else "map_nopem_train")
    assert list(m.state_dict().keys()) == list(golden["state_dict_keys_" + ("pem" if pem else "nopem")])
    for k in ["patch_embed.proj.0.weight", "enc_stages.0.down.fc.weight", "enc_stages.1.blocks.blocks.1.attn.linear_q.0.weight",
              "enc_stages.0.blocks.blocks.0.attn.weight_encoding.1.norm.running_var", "enc_stages.0.blocks.blocks.0.attn.weight_encoding.3.bias",
              "dec_stages.1.up.proj.0.bias", "seg_head.1.norm.weight", "seg_head.3.weight"]:
        assert k in m.state_dict(), k
    ident = _ptv2().PointTransformerV2(in_channels=6, num_classes=0, **{k: v for k, v in pc.CFG.items() if k not in ("in_channels", "num_classes")})
    assert isinstance(ident.seg_head, torch.nn.Identity)


def test_geometry_is_bit_exact(use_oracle, golden, batch):
    m = pc.build(_ptv2().PointTransformerV2, "interp_nopem_eval")
    geom = m.make_geometry(batch["coord"], batch["offset"], batch["offset_host"])
    pc.check_geometry(geom, golden)
    assert geom.stages[0].cluster.dtype == torch.int64 and len(geom.coords) == 3
    # a decoder stage shares the table of the encoder level it runs on when the neighbour counts are equal
    assert geom.knn(1, 16) is geom.knn(1, 16) and set(geom._knn) == {(0, 8), (0, 16), (1, 16), (2, 16)} and set(geom._interp) == {0, 1}


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_model_matches_the_reference_class(use_oracle, golden, batch, case):
    ptv2 = _ptv2()
    torch.manual_seed(0)
    model = pc.build(ptv2.PointTransformerV2, case)
    geom = model.make_geometry(batch["coord"], batch["offset"], batch["offset_host"])
    out = pc.run(model, batch, pc.CASES[case][2], geometry=geom)
    pc.check_geometry(geom, golden)
    pc.check_case(case, out, golden, model, ptv2.PointBatchNorm, CPU_TOL)


def test_geometry_handed_in_changes_nothing(use_oracle, batch):
    ptv2 = _ptv2()
    model = pc.build(ptv2.PointTransformerV2, "interp_pem_train")
    a = pc.run(model, batch, True)
    b = pc.run(model, batch, True, geometry=model.make_geometry(batch["coord"], batch["offset"]))
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"])


def test_checkpointing_gives_the_same_results(use_oracle, batch):
    ptv2 = _ptv2()
    plain = pc.run(pc.build(ptv2.PointTransformerV2, "map_pem_train"), batch, True)
    ckpt = pc.run(pc.build(ptv2.PointTransformerV2, "map_pem_train", enable_checkpoint=True), batch, True)
    assert torch.equal(plain["logits"], ckpt["logits"]) and torch.equal(plain["loss"], ckpt["loss"])
    top = max(float(np.abs(g).max()) for g in plain["grads"].values() if g is not None)
    for k, g in plain["grads"].items():
        if g is not None and np.abs(g).max() > 1e-6 * top:   # (analytically zero gradients are rounding noise in either run)
            # same arithmetic, but the oracle's threaded scatter-adds arrive in another order when the forward is recomputed
            assert np.abs(g - ckpt["grads"][k]).max() <= helpers.REL_TOL * np.abs(g).max(), k


def test_attention_dropout_takes_the_composed_path(use_oracle, batch):
    ptv2 = _ptv2()
    model = pc.build(ptv2.PointTransformerV2, "map_nopem_train", attn_drop_rate=0.5)
    torch.manual_seed(3)
    a = pc.run(model, batch, True)["logits"]
    model.eval()
    b = pc.run(model, batch, False)["logits"]
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)


# ---- the compositions against plain torch autograd in float64, tiny shapes ----------------------------------------------------------
def _tiny_table(n, s, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, s), generator=g, dtype=torch.int32)
    idx[0, s // 2:] = -1
    return idx


@pytest.mark.parametrize("pem,peb", [(False, False), (True, False), (False, True), (True, True)])
def test_gva_compositions_against_naive_float64(pem, peb):
    ptv2 = _ptv2()
    n, s, c, groups = 7, 5, 6, 3
    g = torch.Generator().manual_seed(5)
    idx = _tiny_table(n, s, 1)
    mk = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64, requires_grad=True)
    q, k, v, logits = mk(n, c), mk(n, c), mk(n, c), mk(n, s, groups)
    pm, pb = (mk(n, s, c) if pem else None), (mk(n, s, c) if peb else None)

    def naive(q, k, v, logits, pm, pb):
        rel = torch.zeros(n, s, c, dtype=torch.float64)
        out = torch.zeros(n, c, dtype=torch.float64)
        rows, orow = [], []
        for i in range(n):
            p = torch.softmax(logits[i], 0)
            acc = torch.zeros(c, dtype=torch.float64)
            for j in range(s):
                t = int(idx[i, j])
                r = (k[t] if t >= 0 else torch.zeros(c, dtype=torch.float64)) - q[i]
                r = r * pm[i, j] if pm is not None else r
                r = r + pb[i, j] if pb is not None else r
                rows.append(r)
                if t >= 0:
                    x = v[t] + (pb[i, j] if pb is not None else 0.0)
                    acc = acc + p[j].repeat_interleave(c // groups) * x
            orow.append(acc)
        return torch.stack(rows).view(n, s, c), torch.stack(orow)

    ins = [t for t in (q, k, v, logits, pm, pb) if t is not None]
    rel = ptv2.gva_relation_torch(q, k, idx, pm, pb)
    out = ptv2.gva_attend_torch(logits, v, pb, idx)
    rel_n, out_n = naive(q, k, v, logits, pm, pb)
    assert torch.allclose(rel, rel_n, rtol=1e-12, atol=1e-12) and torch.allclose(out, out_n, rtol=1e-12, atol=1e-12)
    wr, wo = torch.randn(n, s, c, generator=g, dtype=torch.float64), torch.randn(n, c, generator=g, dtype=torch.float64)
    ga = torch.autograd.grad((rel * wr).sum() + (out * wo).sum(), ins, allow_unused=True)
    gb = torch.autograd.grad((rel_n * wr).sum() + (out_n * wo).sum(), ins, allow_unused=True)
    for a, b in zip(ga, gb):
        assert (a is None) == (b is None) and (a is None or torch.allclose(a, b, rtol=1e-10, atol=1e-12))
    # the public nodes take the compositions for host tensors
    assert torch.equal(ptv2.gva_relation(q, k, idx, pm, pb), rel) and torch.equal(ptv2.gva_attend(logits, v, pb, idx), out)


def test_pooling_compositions_against_naive_float64():
    ptv2 = _ptv2()
    g = torch.Generator().manual_seed(9)
    coord = torch.rand(40, 3, generator=g, dtype=torch.float64) * torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64)
    coord[25:] += 5.0
    offset = torch.tensor([25, 40], dtype=torch.int32)
    part = ptv2.grid_partition(coord, offset, 0.4)
    batch = (torch.arange(40) >= 25).long()
    start = torch.stack([coord[:25].min(0).values, coord[25:].min(0).values])
    cell = torch.floor((coord - start[batch]) / 0.4).long()
    key = [(int(b), int(z), int(y), int(x)) for b, (x, y, z) in zip(batch, cell)]
    distinct = sorted(set(key))
    want = torch.tensor([distinct.index(k) for k in key])
    assert torch.equal(part.cluster, want) and part.m == len(distinct)
    assert torch.equal(part.sorted.long(), torch.sort(want, stable=True)[1]) and torch.equal(part.idx_ptr.long()[1:], torch.cumsum(torch.bincount(want), 0))
    assert part.offset.tolist() == [int(want[:25].max()) + 1, part.m]
    feat = torch.randn(40, 4, generator=g, dtype=torch.float64)
    feat[3] = feat[7]   # a tie where both rows share a cluster or not: the first row in point order wins
    feat.requires_grad_(True)
    up = torch.randn(part.m, 4, generator=g, dtype=torch.float64, requires_grad=True)
    pooled, mean = ptv2.segment_max(feat, part), part.coord
    arg = ptv2.segment_argmax_torch(feat, part.idx_ptr, part.sorted)
    for j in range(part.m):
        rows = torch.nonzero(want == j).flatten()
        assert torch.allclose(mean[j], coord[rows].mean(0), rtol=1e-13, atol=1e-13)
        assert torch.equal(pooled[j], feat[rows].max(0).values)
        for ch in range(4):
            assert int(arg[j, ch]) == int(rows[torch.nonzero(feat[rows, ch] == pooled[j, ch]).flatten()[0]])
    w = torch.randn(part.m, 4, generator=g, dtype=torch.float64)
    (gf,) = torch.autograd.grad((pooled * w).sum(), feat)
    expect = torch.zeros_like(gf).scatter_(0, arg, w)
    assert torch.equal(gf, expect)
    fine = ptv2.map_unpool(up, part)
    assert torch.equal(fine, up[part.cluster])
    wf = torch.randn(40, 4, generator=g, dtype=torch.float64)
    (gu,) = torch.autograd.grad((fine * wf).sum(), up)
    assert torch.allclose(gu, torch.zeros_like(gu).index_add_(0, part.cluster, wf), rtol=1e-13, atol=1e-13)
    assert torch.autograd.gradcheck(lambda x: ptv2.map_unpool(x, part), (up,))
    # an explicit start takes the composition and shifts the grid
    moved = ptv2.grid_partition(coord, offset, 0.4, start=start - 0.1)
    assert moved.m >= 1 and moved.cluster.shape == part.cluster.shape


# ---- registries and builders -----------------------------------------------------------------------------------------------------------
def test_builders_take_the_model_from_config_dicts(use_oracle, batch, caplog):
    from pointcloudpdf_amd import engine, recognizer
    from pointcloudpdf_amd.registry import MODELS

    ptv2 = _ptv2()
    assert "PT-v2m2" in MODELS
    bb = dict(type="PT-v2m2", unpool_backend="map", **pc.CFG)
    assert isinstance(MODELS.build(bb), ptv2.PointTransformerV2)
    cfg = dict(model=dict(type="DefaultSegmentor", backbone=bb, criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]),
               recognizer=dict(type="MaxProbability", method="msp"))
    step = engine.build_open_seg_step(cfg)
    assert isinstance(step.model.backbone, ptv2.PointTransformerV2) and isinstance(step.recognizer, recognizer.MaxProbability)
    # no hook section: of the PT-v1 default hooks only the backbone's own output exists on this model; the others are dropped and logged
    assert {k: sorted(v) for k, v in step.hooks.hooks.items()} == {"backbone": ["forward_output"]}
    assert "hook dropped" in caplog.text and "backbone.enc1" in caplog.text
    step.train()
    out = step(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"], segment=batch["segment"]))
    assert torch.isfinite(out["loss"]) and out["score"].shape == (batch["coord"].shape[0],)


def test_new_entries_validate_before_any_launch():
    """pdf_grid_pool_* / pdf_gva_*: null pointers, bad sizes and shapes outside the fused attend class are refused without a device."""
    import ctypes

    from pointcloudpdf_amd import build

    lib = ctypes.CDLL(build.build_library())
    L, I, P, F = ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    lib.pdf_grid_pool_workspace_bytes.restype, lib.pdf_grid_pool_workspace_bytes.argtypes = L, [L]
    lib.pdf_grid_pool_partition.argtypes = [L, P, P, I, P, P, F, P, P, P, P, P, P]
    lib.pdf_gva_attend_forward.argtypes = [L, L, I, I, I, P, P, P, P, P, P, P]
    lib.pdf_gva_relation_forward.argtypes = [L, L, I, I, P, P, P, P, P, P, P]
    buf = (ctypes.c_longlong * 4096)()
    p = ctypes.cast(buf, P)
    p = P((p.value + 255) // 256 * 256)
    assert lib.pdf_grid_pool_workspace_bytes(0) == 0 and lib.pdf_grid_pool_workspace_bytes(1000) > 1000 * 8
    assert lib.pdf_grid_pool_partition(0, p, p, 1, p, p, 0.1, p, p, p, p, p, None) == -1          # no points
    assert lib.pdf_grid_pool_partition(10, p, p, 1, p, p, 0.0, p, p, p, p, p, None) == -1         # cell size 0
    assert lib.pdf_grid_pool_partition(10, p, None, 1, p, p, 0.1, p, p, p, p, p, None) == -1      # no scene ends
    assert lib.pdf_gva_supported(48, 6, 16) == 1 and lib.pdf_gva_supported(512, 64, 64) == 1
    assert lib.pdf_gva_supported(32, 8, 16) == 0 and lib.pdf_gva_supported(20, 2, 3) == 0 and lib.pdf_gva_supported(48, 6, 65) == 0
    assert lib.pdf_gva_attend_forward(4, 4, 3, 20, 2, p, p, None, p, p, p, None) == -3             # outside the fused class
    assert lib.pdf_gva_attend_forward(4, 4, 16, 48, 6, None, p, None, p, p, p, None) == -1
    assert lib.pdf_gva_relation_forward(4, 4, 0, 48, p, p, p, None, None, p, None) == -1           # s < 1
    assert lib.pdf_gva_relation_forward(0, 4, 16, 48, p, p, p, None, None, p, None) == 0           # no rows: nothing to do

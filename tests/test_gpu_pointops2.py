"""GPU suite for SURVEY 8 row f-1: the HIP window-attention kernels (csrc/window_attention.hip) through the C ABI against the
oracle on identical seeded CSR graphs, and against the fixtures made by the reference's own autograd wrappers."""
import os

import numpy as np
import pytest
import torch

from helpers import assert_close
from test_pointops2_cpu import WINDOW_CASES, DenseEdgeList, chain, window_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p2():
    from pointcloudpdf_amd import _native
    from pointcloudpdf_amd.pointops2 import pointops

    assert torch.cuda.is_available()
    _native.hip_backend()   # raises if libpdfops.so is missing: no fallback
    return pointops


@pytest.mark.parametrize("tag", sorted(WINDOW_CASES))
def test_reference_wrapper_fixtures_on_gpu(p2, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "ops_pointops2_ref.npz"))
    res = chain(p2, window_graph(*WINDOW_CASES[tag]), dev="cuda")
    for key, val in res.items():
        assert_close(val, g[f"{tag}_{key}"], 2e-5, f"{tag} {key}")   # dot products: FMA contraction + atomic order


@pytest.mark.parametrize("cfg", [(21, 3000, 6, 16, 48, 300), (22, 800, 12, 16, 20, 60), (23, 500, 1, 8, 5, 30), (24, 64, 3, 20, 7, 1000),
                                 (25, 700, 3, 16, 10, 50), (26, 900, 2, 16, 60, 80), (27, 400, 2, 32, 30, 70), (28, 300, 2, 16, 70, 40)])
def test_hip_vs_oracle_bigger_graphs(p2, oracle_backend, cfg):
    """Edge lists longer than one workgroup pass (n_max 300 / 1000), 12 heads, a head size that is not a multiple of 4,
    empty queries.  The backward each case reaches: d = 16 with L = 10 / 20 / 48 / 60 (cases 21, 22, 25, 26) the atomic-free
    kernels of csrc/window_attention_bwd.hip; L = 70, d = 32 and d = 8 (cases 28, 27, 23) the LDS-atomic `_h` kernels; d = 20
    (case 24, no power of two) the generic kernels.  Oracle side = the same wrappers with the CPU backend injected."""
    from pointcloudpdf_amd import _native

    G = window_graph(*cfg)
    hip = chain(p2, G, dev="cuda")
    prev = _native._set_backend_for_testing(oracle_backend)
    try:
        ora = chain(p2, G, dev="cpu")
    finally:
        _native._set_backend_for_testing(prev)
    for key in hip:
        assert_close(hip[key], ora[key], 5e-5, f"{cfg} {key}")


@pytest.mark.parametrize("cfg", [(31, 5000, 3, 16, 64, 90), (32, 1200, 24, 16, 64, 85), (33, 700, 2, 16, 33, 120), (34, 900, 6, 16, 1, 40),
                                 (35, 2600, 12, 16, 64, 70)])
def test_atomic_free_backward_is_bit_reproducible_and_matches_the_atomic_kernels(p2, cfg):
    """csrc/window_attention_bwd.hip (round 5): grad_k / grad_v / the three table gradients as segmented sums over the edge list grouped
    by key / by query instead of fp32 atomics.  Two evaluations are BIT-identical (fixed summation order), and every gradient equals an
    independent implementation to rounding: with `wa_atomic_free = False` the same calls take the LDS-atomic `_h` kernels of
    csrc/window_attention.hip (k_dot3_bwd_h, k_step2rv_bwd_h) and k_step1_bwd.  3 / 6 / 12 / 24 heads (groups of three heads per
    workgroup), 2 heads (single-head groups), one-row tables, queries without edges, keys nobody attends to; n_max above 48 gives a quad
    of owners more than one 192-entry window (the in-place window loads of wb::k_table)."""
    from pointcloudpdf_amd import _native

    be = _native.hip_backend()
    assert be.wa_atomic_free
    G = window_graph(*cfg)
    a, b = chain(p2, G, dev="cuda"), chain(p2, G, dev="cuda")
    for key in a:
        assert torch.equal(a[key], b[key]), f"{cfg} {key}: two evaluations differ"
    be.wa_atomic_free = False
    try:
        c = chain(p2, G, dev="cuda")
    finally:
        be.wa_atomic_free = True
    for key in a:
        assert_close(a[key], c[key], 2e-5, f"{cfg} {key}")


@pytest.mark.parametrize("cfg", [(41, 4000, 3, 16, 64, 80), (42, 900, 24, 16, 48, 60), (43, 600, 2, 16, 20, 50)])
def test_fused_window_logits_equals_the_two_reference_ops(p2, cfg):
    """pointops.window_logits (one pass over the key rows) = attention_step1_v2 + dot_prod_with_idx_v3, values and all four gradients."""
    G = window_graph(*cfg)
    T = lambda t: t.cuda()
    off, i1, rel = T(G["offsets"]), T(G["index1"]), T(G["rel_idx"])
    go = torch.randn(G["m"], cfg[2], generator=torch.Generator().manual_seed(5)).cuda()
    res = []
    for fused in (True, False):
        q, k, tq, tk = (T(G[n]).clone().requires_grad_(True) for n in ("q", "k", "tq", "tk"))
        if fused:
            out = p2.window_logits(q, k, i1, off, G["n_max"], tq, tk, rel)
            assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("WindowLogits")
        else:
            out = p2.attention_step1_v2(q, k, i1, off, G["n_max"]) + p2.dot_prod_with_idx_v3(q, off, G["n_max"], k, i1, tq, tk, rel)
        out.backward(go)
        res.append(dict(out=out.detach().cpu(), gq=q.grad.cpu(), gk=k.grad.cpu(), gtq=tq.grad.cpu(), gtk=tk.grad.cpu()))
    for key in res[0]:
        assert_close(res[0][key], res[1][key], 2e-5, f"{cfg} {key}")


@pytest.mark.parametrize("cfg", [(51, 3000, 3, 16, 64, 80), (52, 700, 12, 16, 40, 60), (53, 500, 2, 16, 16, 50)])
def test_window_attention_core_equals_the_composed_reference_ops(p2, cfg):
    """pointops.window_attention_core on the (N, 3 C) rows of the qkv Linear (slices, query scale on the kernels, one gradient buffer)
    against the composition WindowAttention.forward spells out: permute copy, scale, step1 + dot_prod, segment softmax, step2."""
    seed, n, h, d, L, _ = cfg
    G = window_graph(*cfg)
    T = lambda t: t.cuda()
    off, i1, rel = T(G["offsets"]), T(G["index1"]), T(G["rel_idx"])
    qkv0 = torch.cat([G["q"].reshape(n, -1), G["k"].reshape(n, -1), G["v"].reshape(n, -1)], 1)
    go = torch.randn(n, h * d, generator=torch.Generator().manual_seed(7)).cuda()
    scale = d ** -0.5
    res = []
    for fused in (True, False):
        qkv = T(qkv0).clone().requires_grad_(True)
        tq, tk, tv = (T(G[nm]).clone().requires_grad_(True) for nm in ("tq", "tk", "tv"))
        if fused:
            out = p2.window_attention_core(qkv, i1, off, G["n_max"], tq, tk, tv, rel, scale)
            assert type(out.grad_fn).__name__.startswith("WindowAttentionCore")
        else:
            q, k, v = (t.contiguous() for t in qkv.reshape(n, 3, h, d).unbind(1))
            logits = p2.attention_step1_v2(q * scale, k, i1, off, G["n_max"]) + p2.dot_prod_with_idx_v3(q * scale, off, G["n_max"], k, i1, tq, tk, rel)
            out = p2.attention_step2_with_rel_pos_value_v2(p2.segment_softmax(logits, off), v, off, G["n_max"], i1, tv, rel).reshape(n, h * d)
        out.backward(go)
        res.append(dict(out=out.detach().cpu(), gqkv=qkv.grad.cpu(), gtq=tq.grad.cpu(), gtk=tk.grad.cpu(), gtv=tv.grad.cpu()))
    for key in res[0]:
        assert_close(res[0][key], res[1][key], 2e-5, f"{cfg} {key}")


@pytest.mark.parametrize("n,c", [(1, 48), (37, 48), (100000, 48), (40002, 96), (10002, 192), (2502, 384), (777, 32), (513, 512), (64, 20)])
def test_layernorm_kernel_matches_torch(n, c):
    """dense.LayerNorm (csrc/layernorm.hip) against torch.nn.LayerNorm: output, input gradient, d gamma, d beta; two evaluations of the
    backward are bit-identical."""
    from pointcloudpdf_amd import dense

    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=g) * 2.0 + 0.5).cuda()
    go = torch.randn(n, c, generator=g).cuda()
    ref, mine = torch.nn.LayerNorm(c).cuda(), dense.LayerNorm(c).cuda()
    with torch.no_grad():
        for m in (ref, mine):
            m.weight.copy_(torch.linspace(0.5, 1.5, c))
            m.bias.copy_(torch.linspace(-0.2, 0.3, c))
    outs = []
    for m in (ref, mine, mine):
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.backward(go)
        outs.append((y.detach().cpu(), xi.grad.cpu(), m.weight.grad.cpu().clone(), m.bias.grad.cpu().clone()))
    assert type(y.grad_fn).__name__.startswith("_LayerNormFn") or "View" in type(y.grad_fn).__name__
    for a, b, name in zip(outs[0], outs[1], ("y", "gx", "dgamma", "dbeta")):
        assert_close(b, a, 2e-5, f"layernorm {n}x{c} {name}")
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[2]))


def test_reference_test_script_shape_properties(p2):
    """The reference's own test scripts use N = 35000, M = 800000, C = 96, h = 6 (libs/pointops2/functions/
    test_attention_op_step1_v2.py:13-18): v2 / v3 against the dense edge-list formulas at that size."""
    g = torch.Generator().manual_seed(1)
    n, h, d, L, m = 35000, 6, 16, 48, 800000
    index0, _ = torch.sort(torch.randint(0, n, (m,), generator=g))
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), index0.bincount(minlength=n).cumsum(0)]).int()
    G = dict(offsets=offsets, index1=torch.randint(0, n, (m,), generator=g).int(), rel_idx=torch.randint(0, L, (m, 3), generator=g).int(),
             q=torch.rand(n, h, d, generator=g), k=torch.rand(n, h, d, generator=g), v=torch.rand(n, h, d, generator=g),
             tq=torch.rand(L, h, d, 3, generator=g), tk=torch.rand(L, h, d, 3, generator=g), tv=torch.rand(L, h, d, 3, generator=g),
             n_max=int((offsets[1:] - offsets[:-1]).max()), m=m)
    ours, dense = chain(p2, G, dev="cuda"), chain(DenseEdgeList, G, dev="cuda")
    for key in ours:
        assert_close(ours[key], dense[key], 1e-4, key)


def test_segmented_backward_matches_the_oracle_at_the_reference_test_shape(p2, oracle_backend):
    """csrc/window_attention_bwd.hip (segmented sums by query and by key, no atomics) against the oracle's restatement of the reference
    kernels at the size the reference's own test scripts use -- N = 35000, M = 800000, C = 96, h = 6 (libs/pointops2/functions/
    test_attention_op_step1_v2.py:13-18): outputs and all six input / table gradients; rounds 1-5 compared them on graphs of <= 5k nodes."""
    from pointcloudpdf_amd import _native

    g = torch.Generator().manual_seed(2)
    n, h, d, L, m = 35000, 6, 16, 48, 800000
    index0, _ = torch.sort(torch.randint(0, n, (m,), generator=g))
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), index0.bincount(minlength=n).cumsum(0)]).int()
    G = dict(offsets=offsets, index1=torch.randint(0, n, (m,), generator=g).int(), rel_idx=torch.randint(0, L, (m, 3), generator=g).int(),
             q=torch.randn(n, h, d, generator=g), k=torch.randn(n, h, d, generator=g), v=torch.randn(n, h, d, generator=g),
             tq=torch.randn(L, h, d, 3, generator=g) * 0.5, tk=torch.randn(L, h, d, 3, generator=g) * 0.5, tv=torch.randn(L, h, d, 3, generator=g) * 0.5,
             n_max=int((offsets[1:] - offsets[:-1]).max()), m=m)
    hip = chain(p2, G, dev="cuda")
    oracle_backend.set_num_threads(min(os.cpu_count() or 1, 32))
    prev = _native._set_backend_for_testing(oracle_backend)
    try:
        ora = chain(p2, G, dev="cpu")
    finally:
        _native._set_backend_for_testing(prev)
    assert set(hip) == set(ora) and len(hip) >= 7
    for key in hip:
        # table gradients sum ~50,000 edge terms per row (800,000 x 3 / 48): fp32 summation order; rows / outputs a few dozen
        assert_close(hip[key], ora[key], 2e-4 if key.startswith("gt") or "table" in key else 5e-5, key)


def test_empty_and_bad_arguments(p2):
    dev = "cuda"
    q = torch.randn(5, 2, 16, device=dev)
    off = torch.zeros(6, dtype=torch.int32, device=dev)
    e = torch.zeros(0, dtype=torch.int32, device=dev)
    assert p2.attention_step1_v2(q, q, e, off, 0).shape == (0, 2)
    with pytest.raises(ValueError):
        p2.attention_step1_v2(q, q, e, off[:-1].contiguous(), 0)


def test_v1_edge_list_forms_on_gpu(p2):
    from test_pointops2_cpu import DenseEdgeListV1, edge_list_case, run_edge_list_ops

    G = edge_list_case(seed=6, n=4000, h=6, d=16, L=48, m=90000)
    ours, dense = run_edge_list_ops(p2, G, dev="cuda"), run_edge_list_ops(DenseEdgeListV1, G, dev="cuda")
    for key in ours:
        assert_close(ours[key], dense[key], 1e-4, key)


def test_window_attention_module_on_gpu(p2):
    """The reference's WindowAttention block (stage-1 shape of the S3DIS config: dim 48, 3 heads, window 0.4 m ... scaled down) on the HIP
    kernels against the dense restatement with shared parameters: output, input gradient and all seven parameter gradients."""
    from test_pointops2_cpu import DenseWindowAttention, run_window_attention, window_attention_case

    mod, args = window_attention_case(dev="cuda", seed=4, n=6000, dim=96, heads=6, max_deg=60)
    ours, dense = run_window_attention(mod, DenseWindowAttention(mod), args)
    for key in ours:
        assert_close(ours[key], dense[key], 2e-4, key)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_stratified_model_matches_reference_classes_on_gpu(golden_dir, mode):
    """BASELINE config 5's model: ST-v1m1 + ST-v1m1-Recognizer on the HIP path (window attention, FPS / kNN / grouping / interpolation,
    radius neighbours) against the fixture produced by the reference's own classes (tests/golden/model_stratified.npz)."""
    import os
    import numpy as np
    import helpers

    g = np.load(os.path.join(golden_dir, "model_stratified.npz"))
    torch.backends.cuda.matmul.allow_tf32 = False
    out = helpers.run_stratified_case(mode, device="cuda")
    helpers.check_stratified_case(mode, out, g)


def test_stratified_training_step_through_the_engine():
    """OpenSegStep("ST-v1m1"): DefaultSegmentor + PointPdf-v1m1 over the ST hooks, one fwd + bwd at 2 x 20k points."""
    from pointcloudpdf_amd import engine, synthetic

    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).cuda()
    step.train()
    batch = synthetic.make_batch([20000, 18000], first_scene_id=60, device="cuda")
    out = step(batch)
    out["loss"].backward()
    assert torch.isfinite(out["loss"]).item() and out["score"].shape == (38000,)
    missing = [n for n, p in step.named_parameters() if p.grad is None]
    assert not missing, missing[:5]
    assert all(torch.isfinite(p.grad).all() for p in step.parameters())


def test_stratified_step_is_bit_reproducible():
    """OpenSegStep("ST-v1m1") three times on one batch with the same seeds (DropPath draws): loss, scores and every parameter gradient
    BIT-identical -- the window-attention backward sums grad_k / grad_v / the relative-position tables in a fixed order
    (csrc/window_attention_bwd.hip) and the norms' parameter gradients likewise (csrc/layernorm.hip).  The reference is not reproducible
    here (atomicAdd scatters, relative_pos_encoding_cuda_kernel_v2.cu:287-340)."""
    from pointcloudpdf_amd import engine, synthetic

    dev = torch.device("cuda", 0)
    batch = synthetic.make_batch([9000, 8000], first_scene_id=90, device=dev)
    runs = []
    for _ in range(3):
        torch.manual_seed(17)
        step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).to(dev)
        synthetic.fill_parameters_deterministic(step, seed=3)
        step.train()
        torch.manual_seed(23)
        out = step(dict(batch))
        out["loss"].backward()
        torch.cuda.synchronize()
        cur = {"loss": out["loss"].detach().clone(), "score": out["score"].detach().clone()}
        cur.update({n: p.grad.detach().clone() for n, p in step.named_parameters() if p.grad is not None})
        runs.append(cur)
    for other in runs[1:]:
        assert set(other) == set(runs[0])
        bad = [k for k in runs[0] if not torch.equal(runs[0][k], other[k])]
        assert not bad, f"{len(bad)} of {len(runs[0])} tensors differ between two evaluations, e.g. {bad[:8]}"


def test_stratified_prefetched_geometry_is_the_inline_geometry():
    """StratifiedPrefetcher (worker thread + side stream, one batch ahead) hands the forward the same FPS subsets and window edge
    tables it would compute itself: the tables are bit-identical to the inline ones, loss and scores of a training step agree to the
    run-to-run noise of the forward (the fused cross-entropy adds its per-block partial sums with float atomics)."""
    from pointcloudpdf_amd import engine, stratified, synthetic

    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).cuda()
    synthetic.fill_parameters_deterministic(step, seed=3)
    step.train()
    batches = [synthetic.make_batch([20000, 18000], first_scene_id=60 + 10 * i, device="cuda") for i in range(2)]
    bb = step.model.backbone
    pf = stratified.StratifiedPrefetcher(bb)
    tickets = [pf.submit(b) for b in batches]          # both queued before anything is consumed
    for b, t in zip(batches, tickets):
        with torch.random.fork_rng(devices=["cuda"]):
            torch.manual_seed(5)
            ref = step(dict(b))
        geom = pf.get(t)
        inline = bb.make_geometry(b["coord"], b["offset"]).precompute(bb.layers_by_level())
        assert set(geom.samples) == set(inline.samples) and set(geom.windows) == set(inline.windows) == {0, 1, 2, 3}
        for k in inline.samples:
            assert torch.equal(geom.samples[k][0], inline.samples[k][0]) and torch.equal(geom.samples[k][1], inline.samples[k][1]), k
        for lv in inline.windows:
            for parity, tab in inline.windows[lv].items():
                for x, y in zip(tab, geom.windows[lv][parity]):
                    assert torch.equal(x, y) if torch.is_tensor(x) else x == y, (lv, parity)
        assert set(geom.neighbors) == set(inline.neighbors) and ("ball",) in geom.neighbors
        with torch.random.fork_rng(devices=["cuda"]):
            torch.manual_seed(5)
            out = step(dict(b, st_geometry=geom))
        assert abs(float(ref["loss"]) - float(out["loss"])) <= 1e-5 * abs(float(ref["loss"]))
        assert (ref["score"] - out["score"]).abs().max() <= 1e-4 * ref["score"].abs().max()
    pf.close()


def test_stratified_geometry_shares_one_fps_run_per_level():
    """StratifiedGeometry takes a level's window-key subset (n // 8 + 1 per scene) and its TransitionDown sample (n / 4 + 1) from ONE
    farthest-point run -- the shorter one is the per-scene prefix of the longer (sampling_cuda_kernel.cu:42-127: the sample count only bounds
    the loop).  Every subset must be bit-identical to its own separate call, as the module forwards issue them."""
    from pointcloudpdf_amd import engine, stratified, synthetic
    from pointcloudpdf_amd.pointops2 import pointops

    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).cuda()
    bb = step.model.backbone
    for sizes in ([20000, 18000], [4097], [1500, 33000, 700]):
        b = synthetic.make_batch(sizes, first_scene_id=71, device="cuda")
        g = bb.make_geometry(b["coord"], b["offset"]).precompute()
        xyz, off = g.coord, g.offset
        for level in range(4):
            k_idx, k_off = g.samples[("keys", level)]
            want_off = stratified._strided_offsets(off, lambda n: n // 8 + 1)
            assert torch.equal(k_off, want_off)
            assert torch.equal(k_idx, pointops.furthestsampling(xyz, off, want_off)), ("keys", level, sizes)
            if level < 3:
                d_idx, d_off = g.samples[("down", level)]
                want_off = stratified._strided_offsets(off, lambda n: int(n * 0.25) + 1)
                assert torch.equal(d_off, want_off)
                assert torch.equal(d_idx, pointops.furthestsampling(xyz, off, want_off)), ("down", level, sizes)
                xyz, off = xyz[d_idx.long(), :].contiguous(), d_off


@pytest.mark.parametrize("n,m,cin,cout", [(5000, 34, 6, 48), (3001, 34, 12, 12), (700, 20, 3, 16), (257, 7, 16, 32)])
def test_kpconv_fused_matches_the_composed_form(n, m, cin, cout, monkeypatch):
    """KPConvLayer on the device: the influence-weighted gather (csrc/kpconv.hip) + one product with the (K * C_in, C_out) weight against
    the composed torch form (the (N, M, K) influence tensor and a batched product; stratified.KPConvLayer.forward) on the same neighbour
    table with missing neighbours (-1): output, feature gradient (float atomics: 1e-5), weight gradient."""
    from pointcloudpdf_amd import stratified

    g = torch.Generator(device="cuda").manual_seed(n + m + cin)
    pts = torch.rand(n, 3, device="cuda", generator=g)
    nb = torch.randint(0, n, (n, m), device="cuda", generator=g)
    nb[torch.rand(n, m, device="cuda", generator=g) < 0.2] = -1
    x0 = torch.randn(n, cin, device="cuda", generator=g)
    go = torch.randn(n, cout, device="cuda", generator=g)
    layer = stratified.KPConvLayer(cin, cout, point_influence=0.08).cuda()
    res = []
    for fused in (True, False):
        monkeypatch.setattr(stratified.KPConvLayer, "FUSED", fused)
        x = x0.clone().requires_grad_(True)
        layer.weight.grad = None
        y = layer(pts, pts, nb, x)
        y.backward(go)
        res.append((y.detach(), x.grad.clone(), layer.weight.grad.clone()))
    (ya, gxa, gwa), (yb, gxb, gwb) = res
    assert float(yb.abs().max()) > 0
    assert_close(ya, yb, 2e-5, "kpconv out")
    assert_close(gxa, gxb, 2e-5, "kpconv grad x")
    assert_close(gwa, gwb, 2e-5, "kpconv grad weight")


def test_stratified_group_prepass_is_the_per_batch_prepass():
    """StratifiedGeometry.precompute_group: the farthest-point chain of three batches as ONE launch sequence per level, sliced and rebased
    per batch, equals every batch's own precompute -- subsets, their scene ends and every window table bit-identical."""
    from pointcloudpdf_amd import engine, stratified, synthetic

    step = engine.OpenSegStep(backbone="ST-v1m1", loss_weight=0.008).cuda()
    bb = step.model.backbone
    batches = [synthetic.make_batch(sz, first_scene_id=80 + 7 * i, device="cuda") for i, sz in enumerate([[9000, 7000], [12000], [3000, 4100, 2500]])]
    geoms = [bb.make_geometry(b["coord"], b["offset"], b["offset_host"]) for b in batches]
    stratified.StratifiedGeometry.precompute_group(geoms, bb.layers_by_level())
    pf = stratified.StratifiedPrefetcher(bb)
    tickets = pf.submit_group(batches)
    for b, g, t in zip(batches, geoms, tickets):
        alone = bb.make_geometry(b["coord"], b["offset"], b["offset_host"]).precompute(bb.layers_by_level())
        threaded = pf.get(t)
        torch.cuda.synchronize()
        for got in (g, threaded):
            assert set(got.samples) == set(alone.samples) and set(got.windows) == set(alone.windows) == {0, 1, 2, 3}
            for k in alone.samples:
                assert torch.equal(got.samples[k][0], alone.samples[k][0]) and torch.equal(got.samples[k][1], alone.samples[k][1]), k
            for lv in alone.windows:
                for parity, tab in alone.windows[lv].items():
                    for x, y in zip(tab, got.windows[lv][parity]):
                        assert torch.equal(x, y) if torch.is_tensor(x) else x == y, (lv, parity)
            assert set(got.neighbors) == set(alone.neighbors) == {("ball",)} | {(kind, l) for kind in ("td", "up") for l in range(3)}
            for k, v in alone.neighbors.items():
                for x, y in zip(v if isinstance(v, tuple) else (v,), got.neighbors[k] if isinstance(v, tuple) else (got.neighbors[k],)):
                    assert torch.equal(x, y), k
    pf.close()


@pytest.mark.parametrize("case", ["two-scenes", "one-window", "own-window", "no-keys", "s3dis-20k"])
@pytest.mark.parametrize("parity", [0, 1])
def test_window_edge_builder_equals_the_reference_construction(oracle_backend, case, parity):
    """csrc/window_edges.hip (rows per query from two point-sized sorts) against oracle/window_tables.py (the reference's pair expansion +
    stable sort by query + quantised offsets, stratified_transformer_v1m1_origin.py:45-127, 282-292, 507): index_0 / index_1 / offsets /
    longest row / rel_idx bit-identical -- two scenes, every point in one window, every point alone in its window, an empty key subset,
    and an S3DIS-shaped scene at the model's first-level window size."""
    from pointcloudpdf_amd import _native, stratified, synthetic

    g = torch.Generator().manual_seed(5)
    ws, quant = 0.3, 0.02
    if case == "s3dis-20k":
        b = synthetic.make_batch([12000, 8000], first_scene_id=900, device="cpu")
        xyz, n = b["coord"].float(), 20000
        batch = (torch.arange(n) >= 12000).long()
        ws, quant = 0.16, 0.01
    else:
        n = 700
        xyz = torch.rand(n, 3, generator=g) * torch.tensor([1.5, 1.2, 0.4])
        batch = (torch.arange(n) >= 400).long() if case == "two-scenes" else torch.zeros(n, dtype=torch.long)
        if case == "one-window":
            xyz = xyz * 0.1
        if case == "own-window":
            n = 64
            xyz = (torch.stack(torch.meshgrid(torch.arange(4.), torch.arange(4.), torch.arange(4.), indexing="ij"), -1).reshape(-1, 3) + 0.5) * 1.0
            batch = torch.zeros(n, dtype=torch.long)
    ds = torch.zeros(0, dtype=torch.int32) if case == "no-keys" else torch.randperm(n, generator=g)[: n // 6 + 1].int()
    wsz = torch.tensor([ws] * 3)
    qgl = int((2 * ws + 1e-4) // quant)
    kf, kc, wk = stratified.window_keys(xyz, batch, wsz, xyz.min(0).values, parity)
    want = oracle_backend.window_edges(xyz, kf, kc, wk, ds, 2 * ws, quant, 2 * qgl - 1)
    be = _native.hip_backend()
    got = be.window_edges(xyz.cuda(), kf.cuda(), kc.cuda(), wk.cuda(), ds.cuda(), 2 * ws, quant, 2 * qgl - 1)
    names = ["index_0", "index_1", "offsets", "n_max", "rel_idx", "flag"]
    for name, a, b in zip(names, got, want):
        if torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a.cpu(), b), (case, parity, name)
        else:
            assert a == b, (case, parity, name, a, b)
    assert int(got[5]) == 0 and got[0].shape[0] > 0


@pytest.mark.parametrize("case", ["unit-box", "negative-coordinates", "on-the-cell-faces", "three-scenes", "s3dis-2x40k"])
@pytest.mark.parametrize("parity", [0, 1])
def test_window_key_kernel_equals_the_torch_composition(case, parity):
    """csrc/window_edges.hip we::k_keys against stratified.window_keys (torch_geometric's voxel_grid restated with torch ops,
    stratified_transformer_v1m1_origin.py:468-499, 91-94) evaluated on the CPU and on the device: fine key, coarse key and packed fine cell
    bit-identical -- random clouds, negative coordinates, points exactly on cell faces (where floorf(a / b) and torch's floor division
    part), three scenes, and two S3DIS-shaped scenes at the model's four window sizes."""
    from pointcloudpdf_amd import _native, stratified, synthetic

    g = torch.Generator().manual_seed(11 + parity)
    sizes, windows = [700], [0.3]
    if case == "s3dis-2x40k":
        b = synthetic.make_batch([40000, 37000], first_scene_id=910, device="cpu")
        xyz, sizes, windows = b["coord"].float(), [40000, 37000], [0.16, 0.32, 0.64, 1.28]
    else:
        if case == "three-scenes":
            sizes = [300, 1, 420]
        n = sum(sizes)
        xyz = torch.rand(n, 3, generator=g) * torch.tensor([1.5, 1.2, 0.4])
        if case == "negative-coordinates":
            xyz = xyz * 7.0 - torch.tensor([5.0, 3.3, 1.9])
        if case == "on-the-cell-faces":   # multiples of the window size (and of half of it), from an origin that is itself a multiple
            xyz = torch.randint(0, 12, (n, 3), generator=g).float() * 0.15 + torch.tensor([0.3, -0.6, 0.0])
            windows = [0.3, 0.15, 0.1]
    ends = torch.tensor(sizes).cumsum(0).int()
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    be = _native.hip_backend()
    lo, hi = xyz.min(0).values, xyz.max(0).values
    for ws in windows:
        wsz = torch.tensor([ws] * 3)
        want = stratified.window_keys(xyz, batch, wsz, lo, parity)
        on_dev = stratified.window_keys(xyz.cuda(), batch.cuda(), wsz.cuda(), lo.cuda(), parity)
        got = be.window_keys(xyz.cuda(), ends.cuda(), lo.cuda(), hi.cuda(), ws, parity)
        for name, a, b, c in zip(("kf", "kc", "wk"), got, want, on_dev):
            assert a.dtype == torch.int64 and torch.equal(a.cpu(), b), (case, parity, ws, name, int((a.cpu() != b).sum()))
            assert torch.equal(a, c), (case, parity, ws, name, "device composition")


@pytest.mark.parametrize("h", [1, 3, 6, 12, 24])
def test_segment_softmax_rows_through_lds_and_through_global_memory(p2, h):
    """pdf_segment_softmax_forward / _backward (scatter_softmax over the CSR rows, stratified_transformer_v1m1_origin.py:322-324): ragged
    rows -- empty ones, rows of one entry, window-sized rows (a wave's rows fit its LDS slice: staged path) and rows of thousands of
    entries (they do not: global-memory path) in one call -- against the dense formula in float64; forward rows sum to one."""
    g = torch.Generator().manual_seed(40 + h)
    lens = torch.cat([torch.randint(20, 60, (300,), generator=g), torch.tensor([0, 1, 0, 2, 5000, 1, 3000, 0]),
                      torch.randint(1, 90, (200,), generator=g), torch.tensor([900, 0, 0])])
    off = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)]).int()
    m = int(off[-1])
    x = (3.0 * torch.randn(m, h, generator=g)).cuda().requires_grad_(True)
    gy = torch.randn(m, h, generator=g).cuda()
    y = p2.segment_softmax(x, off.cuda())
    y.backward(gy)
    xr = x.detach().double().cpu().requires_grad_(True)
    rows = [xr[a:b].softmax(0) for a, b in zip(off[:-1].tolist(), off[1:].tolist()) if b > a]
    yr = torch.cat(rows)
    yr.backward(gy.double().cpu())
    assert (y.detach().cpu().double() - yr.detach()).abs().max() < 5e-6   # (__expf)
    assert (x.grad.cpu().double() - xr.grad).abs().max() < 2e-5 * gy.abs().max()
    sums = torch.zeros(lens.shape[0], h, dtype=torch.float64).index_add_(0, torch.repeat_interleave(torch.arange(lens.shape[0]), lens), y.detach().cpu().double())
    assert ((sums - 1.0).abs()[lens > 0] < 1e-5).all()


def test_segment_rows_in_any_owner_order_are_the_same_rows(p2):
    """pdf_wa_segment_rows_ordered: the visiting order of the owners (the queries window by window: what the edge builder leaves on a
    table's CSR offsets) changes which workgroup forms a row, not the row -- bit-identical outputs for the query-side pass with rows +
    table, and for the key-side pass over the transposed list; the window edge builder's order is a permutation sorted by window key."""
    from pointcloudpdf_amd import _native, stratified, synthetic

    be = _native.hip_backend()
    b = synthetic.make_batch([9000, 7000], first_scene_id=77, device="cuda")
    xyz, off = b["coord"], b["offset"]
    lo, hi = xyz.min(0).values, xyz.max(0).values
    kf, kc, wk = be.window_keys(xyz, off, lo, hi, 0.16, 0)
    ds = torch.arange(0, xyz.shape[0], 8, device="cuda", dtype=torch.int32)
    i0, i1, offsets, n_max, rel, flag = be.window_edges(xyz, kf, kc, wk, ds, 0.32, 0.01, 63)
    order = _native.window_order_of(offsets)
    n, m, h, d, L = xyz.shape[0], i1.shape[0], 3, 16, 64
    assert order is not None and order.dtype == torch.int32 and torch.equal(order.long().sort().values, torch.arange(n, device="cuda"))
    assert bool((kf[order.long()][1:] >= kf[order.long()][:-1]).all())
    g = torch.Generator(device="cuda").manual_seed(9)
    w = torch.rand(m, h, device="cuda", generator=g)
    X = torch.randn(n, h * d, device="cuda", generator=g)
    T = torch.randn(L, h, d, 3, device="cuda", generator=g)
    outs = []
    for o in (None, order, torch.randperm(n, device="cuda", generator=g).int()):
        out = torch.empty(n, h * d, device="cuda")
        be._wa_rows(n, h, d, L, offsets, None, i1, rel, w, X, T, out, order=o)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and float(outs[0].abs().max()) > 0
    key_off, key_edge, key_q, key_rel = _native.window_csc(i1, offsets, rel, n_keys=n)
    wk_ = be._wa_permute(w, key_edge)
    a, c = torch.empty(n, h * d, device="cuda"), torch.empty(n, h * d, device="cuda")
    be._wa_rows(n, h, d, 0, key_off, None, key_q, None, wk_, X, None, a)
    be._wa_rows(n, h, d, 0, key_off, None, key_q, None, wk_, X, None, c, order=order)
    assert torch.equal(a, c)
    # the key side's own order (window_csc): a permutation, longest rows first -- and the same rows again
    korder = _native.window_key_order(i1)
    klen = (key_off[1:] - key_off[:-1])[korder.long()]
    assert korder.dtype == torch.int32 and torch.equal(korder.long().sort().values, torch.arange(n, device="cuda")) and bool((klen[1:] <= klen[:-1]).all())
    be._wa_rows(n, h, d, 0, key_off, None, key_q, None, wk_, X, None, c, order=korder)
    assert torch.equal(a, c)

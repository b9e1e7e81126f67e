#!/usr/bin/env python3
"""Generate tests/golden/model_ptv2_ref.npz by running the REFERENCE's own ``PointTransformerV2`` (PT-v2m2).

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_ptv2.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
  * pointcept/models/point_transformer_v2/point_transformer_v2m2_base.py -- every class of the model;
  * libs/pointops/functions/*.py over the oracle-backed ``pointops._C`` stub of make_golden.py (kNN; grouping / interpolation are the
    reference's python formulations).
Third-party modules this image lacks are stand-ins (parity unpinned): ``torch_geometric.nn.pool.voxel_grid`` -> the package's
``voxel_keys`` (``stratified._voxel_grid``), timm ``DropPath`` -> ``stratified.DropPath``, ``torch_scatter.segment_csr`` -> the plain-torch
loop below (sequential sum / mean, first-wins max / min).  ``torch.sort(cluster)`` (v2m2:263) has no defined order among equal
elements: it is made stable for the call.

Cases (tests/ptv2_cases.py): ``map`` / ``interp`` x ``pe_multiplier`` off / on x train (drop path 0) / eval (drop path 0.3), two scenes of
2,048 + 1,600 points, a two-stage model with c / groups = 8.  Stored: the state-dict key list; the tables every case shares (per stage
cluster, idx_ptr, sort order, pooled coord and offset; every level's kNN tables) -- the script asserts that all cases AND the float64
runs produce the same tables, else the gradients would not be comparable --; per case logits (rows thinned) and loss; per train case
and stored gradient the float64 run's gradient (first rows), its scale, and the reference's own fp32 error against it.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (reference tree, oracle-backed pointops stub)
import ptv2_cases as pc  # noqa: E402

REF = mg.REF


def segment_csr(src, indptr, out=None, reduce="sum"):
    """torch_scatter.segment_csr along dim 0 for sum / mean / max / min, plain torch: a segment's rows are visited in order; the first
    row wins a tie of max / min (the gradient goes to that row through the gather)."""
    indptr = indptr.long()
    counts = indptr[1:] - indptr[:-1]
    first = indptr[:-1]
    kmax = int(counts.max())
    take = lambda k: src[(first + k).clamp(max=src.shape[0] - 1)]
    valid = lambda k: (k < counts).view(-1, *([1] * (src.dim() - 1)))
    if reduce in ("sum", "mean"):
        acc = take(0)
        for k in range(1, kmax):
            acc = acc + torch.where(valid(k), take(k), src.new_zeros(()))
        return acc / counts.to(src.dtype).view(-1, *([1] * (src.dim() - 1))) if reduce == "mean" else acc
    assert reduce in ("max", "min")
    best = take(0).detach().clone()
    arg = first.view(-1, *([1] * (src.dim() - 1))).expand_as(best).clone()
    for k in range(1, kmax):
        v = take(k).detach()
        better = valid(k) & ((v > best) if reduce == "max" else (v < best))
        best = torch.where(better, v, best)
        arg = torch.where(better, (first + k).clamp(max=src.shape[0] - 1).view(-1, *([1] * (src.dim() - 1))), arg)
    return src.gather(0, arg)


def load_reference():
    from pointcloudpdf_amd import point_transformer_v2 as ours
    from pointcloudpdf_amd import stratified

    mg.install_reference()

    def mod(name, **attrs):
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            sys.modules.setdefault(".".join(parts[:i]), types.ModuleType(".".join(parts[:i])))
            sys.modules[".".join(parts[:i])].__path__ = []
        for k, v in attrs.items():
            setattr(sys.modules[name], k, v)

    mod("timm.models.layers", DropPath=stratified.DropPath)
    mod("torch_geometric.nn.pool", voxel_grid=lambda pos, size, batch=None, start=None, end=None: ours.voxel_keys(pos, batch, size))
    mod("torch_scatter", segment_csr=segment_csr)

    def load(modname, rel):
        spec = importlib.util.spec_from_file_location(modname, os.path.join(REF, *rel.split("/")))
        m = importlib.util.module_from_spec(spec)
        sys.modules[modname] = m
        spec.loader.exec_module(m)
        return m

    misc = load("ref_models_utils_misc", "pointcept/models/utils/misc.py")
    utils = sys.modules["pointcept.models.utils"]
    utils.offset2batch, utils.batch2offset = misc.offset2batch, misc.batch2offset
    return load("ref_ptv2m2", "pointcept/models/point_transformer_v2/point_transformer_v2m2_base.py")


class _Recorder:
    """Collects what the reference's GridPool / BlockSequence compute from coordinates."""

    def __init__(self, ref):
        self.ref, self.rows = ref, {}

    def __enter__(self):
        ref, rows = self.ref, self.rows
        self._pool, self._knn, self._sort = ref.GridPool.forward, ref.pointops.knn_query, torch.sort
        rows.update(stages=[], knn={})

        def pool(mod, points, start=None):
            out, cluster = self._pool(mod, points, start)
            counts = torch.bincount(cluster)
            rows["stages"].append(dict(cluster=cluster.numpy().copy(), idx_ptr=np.concatenate([[0], np.cumsum(counts.numpy())]),
                                       sorted=torch.sort(cluster, stable=True)[1].numpy().copy(), coord=out[0].detach().numpy().copy(),
                                       offset=out[2].numpy().copy()))
            return out, cluster

        def knn(k, coord, offset, *a):
            idx, dist = self._knn(k, coord, offset, *a)
            if not a:
                rows["knn"].setdefault((coord.shape[0], int(k)), idx.numpy().copy())
            return idx, dist

        ref.GridPool.forward = pool
        ref.pointops.knn_query = knn
        torch.sort = lambda x, *a, **k: self._sort(x, *a, **({"stable": True} | k))   # (v2m2:263: undefined order among equal elements)
        return rows

    def __exit__(self, *exc):
        self.ref.GridPool.forward, self.ref.pointops.knn_query, torch.sort = self._pool, self._knn, self._sort
        return False


def tables(rows, sizes):
    out = {}
    for i, st in enumerate(rows["stages"]):
        out[f"cluster{i}"], out[f"idx_ptr{i}"], out[f"sorted{i}"] = st["cluster"].astype(np.int64), st["idx_ptr"].astype(np.int32), st["sorted"].astype(np.int32)
        out[f"coord{i + 1}"], out[f"offset{i + 1}"] = st["coord"], st["offset"].astype(np.int32)
    for level, ks in pc.LEVEL_NEIGHBOURS.items():
        for k in ks:
            out[f"knn{level}_{k}"] = pc.thin(rows["knn"][(sizes[level], k)])
    return out


def main():
    ref = load_reference()
    b = pc.batch()
    out, shared, shared64 = {}, None, None
    for case, (backend, pem, train, dpr) in pc.CASES.items():
        res = {}
        for dtype in (torch.float32, torch.float64):
            torch.manual_seed(0)
            model = pc.build(ref.PointTransformerV2, case, dtype)
            bb = dict(b, coord=b["coord"].to(dtype))
            with _Recorder(ref) as rows:
                res[dtype] = pc.run(model, bb, train)
            sizes = [b["coord"].shape[0]] + [st["coord"].shape[0] for st in rows["stages"]]
            t = tables(rows, sizes)
            if dtype == torch.float32:
                if shared is None:
                    shared = t
                assert all(np.array_equal(shared[k], t[k]) for k in shared), f"{case}: the tables differ between cases"
            else:   # the float64 run must share every cluster and kNN table (pooled coordinates agree to rounding)
                for k in shared:
                    if k.startswith("coord"):
                        assert np.abs(shared[k] - t[k]).max() < 1e-5, (case, k)
                    else:
                        assert np.array_equal(shared[k], t[k]), f"{case}: {k} differs in the float64 run: pick other seeds"
            if dtype == torch.float32:
                out["state_dict_keys_" + ("pem" if pem else "nopem")] = np.array(list(model.state_dict().keys()))
        r32, r64 = res[torch.float32], res[torch.float64]
        out[f"{case}_logits"] = pc.thin(r32["logits"].detach().numpy())
        out[f"{case}_loss"] = r32["loss"].detach().numpy()
        e_logits = np.abs(r32["logits"].detach().double().numpy() - r64["logits"].detach().numpy()).max() / np.abs(r64["logits"].detach().numpy()).max()
        print(case, "logits fp32 vs fp64 (max-rel)", f"{e_logits:.2e}", "loss", float(r32["loss"]), "pooled", sizes)
        if train:
            special = pc.zero_gradient_biases(model, ref.PointBatchNorm)
            g64 = r64["grads"]
            out[f"{case}_maxscale"] = np.array(max(float(np.abs(v).max()) for v in g64.values() if v is not None))
            for name in pc.grad_names(pem):
                a, t64 = pc.part(r32["grads"][name]).astype(np.float64), pc.part(g64[name])
                scale = float(np.abs(g64[name]).max())
                out[f"{case}_g64_{name}"], out[f"{case}_scale_{name}"] = t64, np.array(scale)
                if name in special:
                    scale = pc.block_scale(g64, special[name])
                    out[f"{case}_blockscale_{name}"] = np.array(scale)
                out[f"{case}_e32_{name}"] = np.array(np.abs(a - t64).max() / scale)
                print(f"   {name}: scale {float(np.abs(g64[name]).max()):.3e} reference fp32 error {float(out[f'{case}_e32_{name}']):.3e}"
                      + (" (against its block)" if name in special else ""))
    out.update(shared)
    path = os.path.join(mg.OUT, "model_ptv2_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

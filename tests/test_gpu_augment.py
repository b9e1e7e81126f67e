"""GPU suite: the device augmentation (csrc/augment.hip, pointcloudpdf_amd/augment.py) against numpy's Philox and the reference's own
transform classes with their recorded draws (tests/golden/ops_augment_ref.npz, made by tests/golden/make_golden_augment.py)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    z = np.load(os.path.join(GOLDEN, "ops_augment_ref.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


@pytest.fixture(scope="module")
def lists():
    with open(os.path.join(GOLDEN, "pdf_train_transforms.json")) as f:
        return json.load(f)


def test_philox_blocks_equal_numpy():
    from pointcloudpdf_amd import _native

    be = _native.hip_backend()
    for key in (0, 5, (1 << 64) + 7, 0xDEADBEEFCAFEF00D12345):
        got = be.philox4x64(1 << 20, key, 1, DEV).cpu().numpy().view(np.uint64)
        want = np.random.Philox(counter=0, key=key).random_raw(4 << 20).reshape(-1, 4)
        assert np.array_equal(got, want), key
    got = be.philox4x64(3, 9, (1 << 64) - 1, DEV).cpu().numpy().view(np.uint64)   # carry into the second counter word
    want = np.random.Philox(counter=(1 << 64) - 2, key=9).random_raw(12).reshape(-1, 4)
    assert np.array_equal(got, want)


def _case(z, meta, tag):
    m = meta[tag]
    scenes, records = [], []
    for s, names in enumerate(m["draws"]):
        d = {k.split("/")[-1]: z[k] for k in z.files if k.startswith(f"{tag}/in{s}/")}
        scenes.append(d)
        records.append([(nm, z[f"{tag}/draw{s}/{j}"]) for j, nm in enumerate(names)])
    return m["cfgs"], scenes, records


def _want(z, tag, s, k):
    """The reference's output array (the fixture omits an output equal to its input)."""
    key = f"{tag}/out{s}/{k}"
    return z[key] if key in z.files else z[f"{tag}/in{s}/{k}"]


def _ulps(a, b):
    """|a - b| in ulps of the row's largest magnitude, in the reference array's dtype: the error bound of a 3-term dot product, whose
    summation / FMA order inside BLAS is not ours to choose (a cancelling row differs by more ulps of its own small result)."""
    b = np.asarray(b)
    sp = np.spacing(np.abs(b).max(axis=-1, keepdims=True)).astype(np.float64)
    return np.abs(np.asarray(a, np.float64) - b.astype(np.float64)) / sp


def test_each_transform_with_recorded_draws(ref):
    """Every in-scope per-point transform alone, on float32 and float64 scenes, with the reference's recorded draws: bit-identical in
    the reference's dtype.  RandomRotate: within 2 fp64 ulps of the row (np.dot goes through BLAS).  ElasticDistortion: the blurred
    volume within 1 fp32 ulp of scipy's, the displacement within 1e-12, the coordinates within 1 ulp in the reference dtype."""
    from pointcloudpdf_amd import augment

    z, meta = ref
    tags = [t for t in meta if t.startswith("single")]
    assert len(tags) == 42
    for tag in tags:
        cfgs, scenes, records = _case(z, meta, tag)
        pipe = augment.Compose(cfgs)
        pipe.record_elastic = True
        out = pipe(scenes, [0], records=records, device=DEV)
        kind = cfgs[0]["type"]
        for k in ("coord", "color", "normal", "segment"):
            want = _want(z, tag, 0, k)
            got = out[k].cpu().numpy()
            assert got.shape == want.shape, (tag, k)
            if kind == "RandomRotate" and k in ("coord", "normal"):
                assert want.dtype == np.float64
                assert _ulps(got, want).max() <= 2.0, (tag, k)
            elif kind == "ElasticDistortion" and k == "coord":
                assert np.all(np.abs(got - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), tag
            else:
                assert np.array_equal(got.astype(want.dtype), want) and np.array_equal(got, want.astype(np.float64)), (tag, k)
        if kind == "ElasticDistortion":
            assert len(pipe.elastic_log) == 2
            for j, e in enumerate(pipe.elastic_log):
                vol = e["vol"].cpu().numpy().reshape(*e["dims"][0], 3)
                want_vol = z[f"{tag}/elastic0/{j}/vol"]
                assert vol.shape == want_vol.shape and want_vol.dtype == np.float32
                assert np.all(np.abs(vol - want_vol) <= np.spacing(np.abs(want_vol))), (tag, j)
                assert np.abs(e["disp"].cpu().numpy() - z[f"{tag}/elastic0/{j}/disp"]).max() <= 1e-12, (tag, j)


def _grid_parity(z, tag, coord, offset_host, grid):
    """Device GridSample (pdf_grid_hash_f64 for float64 rows) vs the reference GridSample's keys, inverse and count, scene by scene;
    a mismatching point would have to lie within a few fp64 ulps of a voxel face -- counted, and expected to be none."""
    from pointcloudpdf_amd import voxelize

    off = torch.tensor(np.asarray(offset_host, np.int32), device=DEV)
    g = voxelize.grid_sample(coord, off, grid, mode="train")
    key = g["key"].cpu().numpy().view(np.uint64)
    inv, count = g["inverse"].cpu().numpy(), g["count"].cpu().numpy()
    vo = [0] + g["voxel_offset"].cpu().tolist()
    c = coord.cpu().numpy()
    start, bad = 0, 0
    for s, e in enumerate(offset_host):
        wk, wi, wc = (z[f"{tag}/grid{s}/{k}"] for k in ("key", "inverse", "count"))
        miss = (key[start:e] != wk) | (inv[start:e] != wi)
        q = c[start:e] / grid
        near = np.abs(q - np.round(q)) <= 8 * np.spacing(np.abs(q))
        bad += int((miss & ~near.any(axis=1)).sum())
        assert not miss.any(), (tag, s, int(miss.sum()), int((miss & near.any(axis=1)).sum()))
        assert np.array_equal(count[vo[s]:vo[s + 1]], wc), (tag, s)
        start = e
    assert bad == 0
    return g


def test_chains_with_recorded_draws(ref):
    """The pre-GridSample part of the S3DIS PT / ST lists (float64 scenes) and of the ScanNet PT list (float32 scenes with normals,
    ElasticDistortion included) with the reference's draws; then GridSample keys, inverse and count on the device chain equal the
    reference GridSample's on the reference chain."""
    from pointcloudpdf_amd import augment

    z, meta = ref
    for tag in ("chain_s3dis_pt", "chain_s3dis_st", "chain_scannet_pt"):
        cfgs, scenes, records = _case(z, meta, tag)
        out = augment.Compose(cfgs)(scenes, [0] * len(scenes), records=records, device=DEV)
        off = out["offset_host"]
        start = 0
        for s, e in enumerate(off):
            for k in ("coord", "normal"):
                if k not in scenes[s]:
                    continue
                want = _want(z, tag, s, k)
                got = out[k].cpu().numpy()[start:e]
                if any(c["type"] == "ElasticDistortion" for c in cfgs) and k == "coord":
                    # RandomRotate's <= 2 ulps (BLAS) reach the elastic stages, whose sample moves by magnitude x the noise slope
                    # (up to ~2 / granularity x magnitude = 4 per stage here): bounded by 2 x (1 + 4)^2 = 50 ulps; seen: 10
                    assert _ulps(got, want).max() <= 50.0, (tag, k, _ulps(got, want).max())
                elif any(c["type"] in ("RandomRotate", "ElasticDistortion") for c in cfgs):
                    assert _ulps(got, want).max() <= 2.0, (tag, k, _ulps(got, want).max())
                else:
                    assert np.array_equal(got, want.astype(np.float64)), (tag, k)
            for k in ("color", "segment"):
                want = _want(z, tag, s, k)
                assert np.array_equal(out[k].cpu().numpy()[start:e], want), (tag, k)
            start = e
        _grid_parity(z, tag, out["coord"], off, meta[tag]["grid"])


def test_float64_grid_sample_on_millimetre_decimals(ref):
    """Raw float64 millimetre coordinates straight into GridSample at 0.04 m: the device keys / inverse / count equal the reference's,
    and the case matters -- the float32 path puts some of these points into another voxel."""
    z, meta = ref
    scenes = [z[f"grid_f64_mm/in{s}/coord"] for s in range(2)]
    coord = torch.from_numpy(np.concatenate(scenes)).to(DEV)
    off = list(np.cumsum([len(c) for c in scenes]))
    g = _grid_parity(z, "grid_f64_mm", coord, off, 0.04)
    from pointcloudpdf_amd import voxelize

    g32 = voxelize.grid_sample(coord.float(), torch.tensor(np.asarray(off, np.int32), device=DEV), 0.04, mode="train")
    assert int((g32["key"] != g["key"]).sum().item()) > 0


def _raw_scene(seed, n, dtype, normal=False):
    rng = np.random.default_rng(seed)
    d = dict(coord=np.round(rng.uniform(0, 3, (n, 3)), 3).astype(dtype), color=np.floor(rng.uniform(0, 256, (n, 3))).astype(dtype),
             segment=rng.integers(0, 13, n).astype(np.int64))
    if normal:
        v = rng.normal(size=(n, 3))
        d["normal"] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype)
    return d


def test_production_mode_is_deterministic_and_batch_independent(lists):
    """The whole S3DIS PT list (GridSample's kept point and SphereCrop's centre included) is a function of the scenes and their keys."""
    from pointcloudpdf_amd import augment

    cfgs = lists["s3dis/openseg-pt-v1-0-pointpdf-v1m1-base"]
    scenes = [_raw_scene(i, 3000 + 500 * i, np.float64) for i in range(3)]
    pipe = augment.Compose(cfgs)
    a = pipe(scenes, [11, 12, 13], device=DEV)
    b = pipe(scenes, [11, 12, 13], device=DEV)
    for k in ("coord", "grid_coord", "feat", "segment", "segment_known", "offset"):
        assert torch.equal(a[k], b[k]), k
    alone = pipe(scenes[1:2], [12], device=DEV)
    s0, s1 = a["offset_host"][0], a["offset_host"][1]
    for k in ("coord", "grid_coord", "feat", "segment"):
        assert torch.equal(alone[k], a[k][s0:s1]), k
    c = pipe(scenes, [21, 22, 23], device=DEV)
    assert c["offset_host"] != a["offset_host"] or not torch.equal(a["feat"], c["feat"])
    crop = augment.Compose([dict(type="SphereCrop", point_max=1000, mode="random")])
    assert torch.equal(crop(scenes, [1, 2, 3], device=DEV)["coord"], crop(scenes, [1, 2, 3], device=DEV)["coord"])


def test_production_statistics():
    """Flip rate, jitter clip and std, ChromaticJitter std, dropout count, ShufflePoint permutation."""
    from pointcloudpdf_amd import augment

    n, nsc = 4000, 64
    scenes = [dict(coord=np.zeros((n, 3)), color=np.full((n, 3), 128.0)) for _ in range(nsc)]
    out = augment.Compose([dict(type="RandomJitter", sigma=0.01, clip=0.05)])(scenes, list(range(nsc)), device=DEV)
    j = out["coord"].cpu().numpy()
    assert np.abs(j).max() <= 0.05 and abs(j.std() - 0.01) < 2e-4 and abs(j.mean()) < 2e-4
    out = augment.Compose([dict(type="ChromaticJitter", p=1, std=0.05)])(scenes, list(range(nsc)), device=DEV)
    cj = out["color"].cpu().numpy() - 128.0
    assert abs(cj.std() - 0.05 * 255) < 0.1
    pts = [dict(coord=np.tile([[1.0, 1.0, 1.0]], (8, 1))) for _ in range(2000)]
    out = augment.Compose([dict(type="RandomFlip", p=0.5)])(pts, list(range(2000)), device=DEV)
    fx = (out["coord"][::8, 0] < 0).float().mean().item()
    fy = (out["coord"][::8, 1] < 0).float().mean().item()
    assert 0.45 < fx < 0.55 and 0.45 < fy < 0.55
    one = [dict(coord=np.array([[1.0, 0.0, 0.0]])) for _ in range(4000)]
    out = augment.Compose([dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=1)])(one, list(range(4000)), device=DEV)
    ang = torch.atan2(out["coord"][:, 1], out["coord"][:, 0]).cpu().numpy()
    assert ang.min() < -0.95 * np.pi and ang.max() > 0.95 * np.pi and abs(ang.mean()) < 0.1
    out = augment.Compose([dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", center=[0, 0, 0], p=0.5)])(
        [dict(coord=np.array([[0.0, 1.0, 0.0]])) for _ in range(4000)], list(range(4000)), device=DEV)
    ang = torch.atan2(out["coord"][:, 2], out["coord"][:, 1]).cpu().numpy()
    assert np.abs(ang).max() <= np.pi / 64 + 1e-12 and 0.45 < (ang != 0).mean() < 0.55
    sc = [dict(coord=np.arange(3 * m, dtype=np.float64).reshape(m, 3)) for m in (1000, 999, 37)]
    out = augment.Compose([dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=1)])(sc, [1, 2, 3], device=DEV)
    assert out["offset_host"] == [800, 800 + 799, 800 + 799 + 29]
    out = augment.Compose([dict(type="ShufflePoint")])(sc, [1, 2, 3], device=DEV)
    ids = out["coord"][:, 0].cpu().numpy() / 3
    assert sorted(ids[:1000].tolist()) == list(range(1000)) and not np.array_equal(ids[:1000], np.arange(1000))


@pytest.mark.parametrize("name,in_ch,backbone,classes", [
    ("s3dis/openseg-pt-v1-0-pointpdf-v1m1-base", 6, "PointTransformer-Seg38", 13),
    ("s3dis/openseg-st-v1m1-0-origin-pointpdf-v1m1-base", 6, "ST-v1m1", 13),
    ("s3dis/incrseg-pt-v1-0-pointpdf-v1m1-base", 6, "incr", 13),
    ("scannet/openseg-pt-v1-0-pointpdf-v1m1-base", 9, "PointTransformer-Seg38", 20),
    ("scannet/openseg-st-v1m1-0-origin-pointpdf-v1m1-base", 6, "ST-v1m1", 20)])
def test_end_to_end_batch_trains(lists, name, in_ch, backbone, classes):
    """Raw synthetic scenes -> Compose(list) -> the Collect keys / dtypes / shapes -> one forward + backward with a finite loss."""
    from pointcloudpdf_amd import augment, engine, synthetic

    scannet = name.startswith("scannet")
    scenes = [_raw_scene(40 + i, 6000 + 1000 * i, np.float32 if scannet else np.float64, normal=scannet) for i in range(2)]
    cfgs = lists[name]
    collect = [c for c in cfgs if c["type"] == "Collect"][0]
    batch = augment.Compose(cfgs)(scenes, [5, 6], device=DEV)
    assert set(collect["keys"]) | {"feat", "offset"} <= set(batch)
    n = batch["coord"].shape[0]
    assert batch["coord"].dtype == torch.float32 and batch["feat"].shape == (n, in_ch) and batch["feat"].dtype == torch.float32
    assert batch["offset"][-1].item() == n == batch["offset_host"][-1] and batch["segment_known"].dtype == torch.int64
    if "grid_coord" in batch:
        assert batch["grid_coord"].dtype == torch.int64 and batch["grid_coord"].shape == (n, 3)
    rgb = batch["feat"][:, 3:6]
    assert (rgb.min() >= -1 and rgb.max() <= 1) if scannet else (rgb.min() >= 0 and rgb.max() <= 1)
    if backbone == "incr":
        m = engine.IncrSegStep(backbone="PointTransformer-Seg38").to(DEV).train()
        synthetic.fill_parameters_deterministic(m.teacher, seed=1)
        synthetic.fill_parameters_deterministic(m.student, seed=2)
        out = m(dict(coord=batch["coord"], feat=batch["feat"], offset=batch["offset"], offset_host=batch["offset_host"],
                     segment_incr=batch["segment_incr"]))
    else:
        m = engine.OpenSegStep(backbone=backbone, in_channels=in_ch, num_classes=classes).to(DEV).train()
        synthetic.fill_parameters_deterministic(m, seed=3)
        out = m(batch)
    assert torch.isfinite(out["loss"])
    out["loss"].backward()

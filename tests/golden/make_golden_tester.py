#!/usr/bin/env python3
"""Fixture of the precise tester (pointcloudpdf_amd/testing.py: TestPipeline / SceneTester) from the REFERENCE's own test pipeline.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_tester.py
pointcept/datasets/transform.py is imported in place and runs unmodified: per case the scene-level ``transform`` list, every
``aug_transform`` list, ``GridSample(mode="test")`` and ``Compose(post_transform)`` of ``DefaultDataset.prepare_test_data``
(datasets/defaults.py:96-129) on one small raw scene.  Writes tester_ref.npz (data only).

Stable argsort.  ``np.argsort(key)`` in GridSample is unstable, so WHICH point of a voxel lands in which fragment slot is undefined
upstream.  For the duration of the reference calls ``numpy.argsort`` defaults to ``kind="stable"`` here (original order inside a voxel),
which is what the device pipeline does; with it the reference's fragments equal ours index for index.

Size.  A fragment holds one row per voxel and a scene has ~11 fragments per augmentation, so the full arrays of every fragment would be
several MB.  Stored instead: a SHA-256 digest per fragment over the bytes of (index int64, coord f32,
feat f32, grid_coord int64) -- the comparisons are exact, so a digest checks no less -- ``index`` of every fragment of the first case
(int16; the voting tests need it) and the full arrays of ONE fragment of the other two cases.
The per-fragment logits / scores are rows of a stored table picked by a fixed rule (``logit_rows``), 3 * N(0, 1), K = 13.
The expected ``votes`` / ``pred`` / ``score`` are engines/test.py:206-251 restated with torch CPU ops: pred[idx] += softmax(logits), then
scatter_mean as sum / count.
"""
import hashlib
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

REF = os.environ.get("PDF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

GRID = 0.08
K = 13
TABLE_ROWS = 1024
AUGS = [[dict(type="RandomScale", scale=[1, 1])], [dict(type="RandomScale", scale=[0.9, 0.9])],
        [dict(type="RandomScale", scale=[1.1, 1.1]), dict(type="RandomFlip", p=1)]]
CASES = {
    "f32_center": dict(dtype=np.float32, normal=False, transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
                       post=dict(type="CenterShift", apply_z=False), keys=("coord", "color"), feat_keys=("coord", "color")),
    "f32_positive": dict(dtype=np.float32, normal=True, transform=[dict(type="PositiveShift"), dict(type="NormalizeColor", mode="zeroOne")],
                         post=dict(type="PositiveShift"), keys=("coord", "color", "normal"), feat_keys=("coord", "color", "normal")),
    "f64_center": dict(dtype=np.float64, normal=False, transform=[dict(type="CenterShift", apply_z=True), dict(type="NormalizeColor")],
                       post=dict(type="CenterShift", apply_z=False), keys=("coord", "color"), feat_keys=("coord", "color")),
}


def make_scene():
    """N ~ 6.8k points, about half of the 0.08 m voxels hold one point and the fullest ~11."""
    rng = np.random.default_rng(7)
    base = rng.uniform(0, 1, (3000, 3)) * np.array([4.0, 3.0, 2.5])
    third = np.arange(3000) % 3
    base[third == 0, 2] = 0.0          # floor
    base[third == 1, 0] = 0.0          # a wall
    base[third == 2, 1] = 0.0          # another wall
    parts = [base]
    for share in (0.6, 0.35, 0.2, 0.1, 0.05):
        pick = base[rng.random(3000) < share]
        parts.append(pick + rng.normal(0, 0.004, pick.shape))
    coord = np.concatenate(parts).astype(np.float32)
    n = coord.shape[0]
    color = np.floor(rng.uniform(0, 256, (n, 3))).astype(np.float32)
    v = rng.normal(size=(n, 3))
    normal = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    segment = rng.integers(0, K, n).astype(np.int64)
    segment[rng.random(n) < 0.02] = -1
    return dict(coord=coord, color=color, normal=normal, segment=segment)


def logit_rows(aug, frag, rows):
    """Rule picking the table row of fragment ``frag`` of augmentation ``aug`` for its rows 0 .. rows - 1 (restated in the tests)."""
    r = np.arange(rows, dtype=np.int64)
    return (r * 2654435761 + frag * 40503 + aug * 97) % TABLE_ROWS


class StableArgsort:
    def __enter__(self):
        self.orig = np.argsort

        def argsort(a, axis=-1, kind=None, order=None, **kw):
            return self.orig(a, axis=axis, kind="stable" if kind is None else kind, order=order, **kw)
        np.argsort = argsort

    def __exit__(self, *exc):
        np.argsort = self.orig


def main():
    spec = importlib.util.spec_from_file_location("ref_transform", os.path.join(REF, "pointcept", "datasets", "transform.py"))
    tr = importlib.util.module_from_spec(spec)
    sys.modules["ref_transform"] = tr
    spec.loader.exec_module(tr)
    import copy

    raw = make_scene()
    trng = np.random.default_rng(11)
    out = {f"scene/{k}": v for k, v in raw.items()}
    out["logit_table"] = (3.0 * trng.standard_normal((TABLE_ROWS, K))).astype(np.float32)
    out["score_table"] = trng.random(TABLE_ROWS).astype(np.float32)
    out["grid_size"] = np.array(GRID)
    info = []
    for tag, case in CASES.items():
        d = dict(coord=raw["coord"].astype(case["dtype"]), color=raw["color"].copy(), segment=raw["segment"].copy())
        if case["normal"]:
            d["normal"] = raw["normal"].copy()
        d = tr.Compose(case["transform"])(d)
        d.pop("segment")
        vox = tr.TRANSFORMS.build(dict(type="GridSample", grid_size=GRID, hash_type="fnv", mode="test", keys=case["keys"], return_grid_coord=True))
        post = tr.Compose([case["post"], dict(type="ToTensor"),
                           dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=case["feat_keys"])])
        n = raw["coord"].shape[0]
        votes, ssum, scnt = torch.zeros(n, K), torch.zeros(n), torch.zeros(n)
        for a, aug in enumerate(AUGS):
            np.random.seed(a)
            da = tr.Compose(aug)(copy.deepcopy(d))
            with StableArgsort():
                parts = vox(da)
            frags = [post(p) for p in parts]
            rows = frags[0]["index"].shape[0]
            assert n < 2 ** 15
            if tag == "f32_center":
                out[f"{tag}/aug{a}/index"] = np.stack([f["index"].numpy() for f in frags]).astype(np.int16)
            out[f"{tag}/aug{a}/shape"] = np.array([len(frags), rows])
            dig = []
            for f in frags:
                assert f["coord"].dtype == torch.float32 and f["feat"].dtype == torch.float32 and f["index"].dtype == torch.int64
                assert f["grid_coord"].dtype == torch.int64 and int(f["offset"][0]) == rows
                h = hashlib.sha256()
                for key in ("index", "coord", "feat", "grid_coord"):
                    h.update(np.ascontiguousarray(f[key].numpy()).tobytes())
                dig.append(np.frombuffer(h.digest(), dtype=np.uint8))
            out[f"{tag}/aug{a}/digest"] = np.stack(dig)
            if a == 2 and tag != "f32_center":   # the full arrays of one fragment: the last one (every voxel's slot is f % count)
                f = frags[-1]
                assert torch.equal(f["feat"][:, :3], f["coord"])
                out[f"{tag}/sample/index"], out[f"{tag}/sample/feat"] = f["index"].numpy().astype(np.int16), f["feat"].numpy()   # (coord = feat[:, :3])
                out[f"{tag}/sample/grid_coord"] = f["grid_coord"].numpy().astype(np.int16)
            info.append(f"{tag} aug{a}: V={rows} cmax={len(frags)}")
            if tag == "f32_center":     # engines/test.py:206-251 on the table-picked logits / scores
                for fi, f in enumerate(frags):
                    sel = logit_rows(a, fi, rows)
                    logits, score = torch.from_numpy(out["logit_table"][sel]), torch.from_numpy(out["score_table"][sel])
                    idx = f["index"]
                    votes[idx, :] += torch.softmax(logits, -1)
                    ssum.index_add_(0, idx, score)
                    scnt.index_add_(0, idx, torch.ones_like(score))
        if tag == "f32_center":
            top2 = votes.topk(2, dim=1)[0]
            margin = (top2[:, 0] - top2[:, 1]).numpy()
            info.append(f"votes: points with top-two margin < 1e-4: {int((margin < 1e-4).sum())} of {n}")
            out["votes"], out["pred"] = votes.numpy(), votes.max(1)[1].numpy().astype(np.int8)
            out["score"] = (ssum / scnt.clamp(min=1.0)).numpy()
    out["note"] = np.array("reference GridSample(mode='test') run with numpy.argsort defaulting to kind='stable' (upstream's order inside a "
                           "voxel is undefined); per-fragment digests are sha256 over index int64 | coord f32 | feat f32 | grid_coord int64; "
                           "logits / scores of fragment f, augmentation a, row r: table[(r * 2654435761 + f * 40503 + a * 97) % 1024]; "
                           + "; ".join(info))
    path = os.path.join(OUT, "tester_ref.npz")
    np.savez_compressed(path, **out)
    print("\n".join(info))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

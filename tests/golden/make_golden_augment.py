#!/usr/bin/env python3
"""Fixtures of the device augmentation (pointcloudpdf_amd/augment.py) from the REFERENCE's own transform classes.

Run in the build container only (needs the reference tree):   python tests/golden/make_golden_augment.py
pointcept/datasets/transform.py is imported in place and runs unmodified; np.random.{rand,randn,uniform,choice,shuffle} and
random.random are wrapped in a recorder, so every draw of a case is stored next to its input and output.  Writes
ops_augment_ref.npz (cases) and pdf_train_transforms.json (the PDF configs' train lists, settings only).
"""
import importlib.util
import json
import os
import random
import sys
import zlib

sys.dont_write_bytecode = True
import numpy as np
import scipy.interpolate

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("PDF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

CONFIGS = ["s3dis/openseg-pt-v1-0-pointpdf-v1m1-base", "s3dis/openseg-st-v1m1-0-origin-pointpdf-v1m1-base",
           "s3dis/incrseg-pt-v1-0-pointpdf-v1m1-base", "scannet/openseg-pt-v1-0-pointpdf-v1m1-base",
           "scannet/openseg-st-v1m1-0-origin-pointpdf-v1m1-base"]


def train_lists():
    out = {}
    for name in CONFIGS:
        text = open(os.path.join(REF, "configs", name + ".py")).read()
        # settings only: the label variables and the `data = dict(...)` block (other parts of some configs do not parse)
        head = [ln for ln in text.splitlines() if not ln[:1].isspace() and ln.split("=")[0].strip() in ("unknown_label", "incr_label_remap", "incr_label_select",
                                                                               "dataset_type", "data_root")]
        start = text.index("\ndata = dict(") + 1
        depth, end = 0, start
        for end in range(text.index("(", start), len(text)):
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            if depth == 0:
                break
        ns = {}
        exec(compile("\n".join(head) + "\n" + text[start:end + 1], name, "exec"), ns)
        out[name] = ns["data"]["train"]["transform"]
    return out


class Recorder:
    """Wraps numpy's / random's draws (and scipy's RegularGridInterpolator, to keep ElasticDistortion's blurred volume and sample)."""

    def __init__(self):
        self.log = []
        self.orig = {}
        self.elastic = []

    def __enter__(self):
        for name in ("rand", "randn", "uniform", "choice", "shuffle"):
            f = getattr(np.random, name)
            self.orig[name] = f

            def wrap(*a, _f=f, _n=name, **k):
                if _n == "shuffle":
                    _f(*a, **k)
                    self.log.append(("shuffle", np.array(a[0])))
                    return None
                v = _f(*a, **k)
                self.log.append((_n, np.array(v)))
                return v
            setattr(np.random, name, wrap)
        self.orig["random"] = random.random

        def rr():
            v = self.orig["random"]()
            self.log.append(("random", np.array(v)))
            return v
        random.random = rr
        rgi, rec = scipy.interpolate.RegularGridInterpolator, self

        class SpyRGI(rgi):
            def __call__(self, xi, *a, **k):
                v = super().__call__(xi, *a, **k)
                rec.elastic.append((np.array(self.values), np.array(v)))
                return v
        self.orig["rgi"] = rgi
        scipy.interpolate.RegularGridInterpolator = SpyRGI
        return self

    def __exit__(self, *exc):
        for name, f in self.orig.items():
            if name == "random":
                random.random = f
            elif name == "rgi":
                scipy.interpolate.RegularGridInterpolator = f
            else:
                setattr(np.random, name, f)


def scene(seed, n, dtype, normal=False, extent=4.0):
    rng = np.random.default_rng(seed)
    d = dict(coord=(np.round(rng.uniform(0, extent, (n, 3)), 3)).astype(dtype),
             color=np.floor(rng.uniform(0, 256, (n, 3))).astype(dtype),
             segment=rng.integers(0, 13, n).astype(np.int64))
    if normal:
        v = rng.normal(size=(n, 3))
        d["normal"] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(dtype)
    return d


SINGLE = [
    dict(type="CenterShift", apply_z=True), dict(type="CenterShift", apply_z=False), dict(type="PositiveShift"),
    dict(type="RandomRotate", angle=[-1, 1], axis="z", center=[0, 0, 0], p=1),
    dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="x", p=1), dict(type="RandomRotate", angle=[-1 / 64, 1 / 64], axis="y", p=1),
    dict(type="RandomScale", scale=[0.9, 1.1]), dict(type="RandomFlip", p=1), dict(type="RandomFlip", p=0),
    dict(type="RandomJitter", sigma=0.005, clip=0.02),
    dict(type="ChromaticAutoContrast", p=1, blend_factor=None), dict(type="ChromaticAutoContrast", p=0),
    dict(type="ChromaticTranslation", p=1, ratio=0.05), dict(type="ChromaticJitter", p=1, std=0.05),
    dict(type="HueSaturationTranslation", hue_max=0.5, saturation_max=0.2), dict(type="RandomColorDrop", p=1, color_augment=0.0),
    dict(type="NormalizeColor", mode="zeroOne"), dict(type="NormalizeColor"),
    dict(type="RandomDropout", dropout_ratio=0.2, dropout_application_ratio=1), dict(type="ShufflePoint"),
    dict(type="ElasticDistortion", distortion_params=[[0.2, 0.4], [0.8, 1.6]]),
]


def grid_ref(tr, coord, grid_size):
    """The reference GridSample's keys, inverse and count on one scene (its own class and hash; transform.py:813-824, 911-925)."""
    gs = tr.GridSample(grid_size=grid_size, hash_type="fnv", mode="train", keys=("coord",), return_inverse=True)
    d = gs(dict(coord=coord.copy()))
    grid = np.floor(coord / np.array(grid_size)).astype(int)
    key = gs.hash(grid - grid.min(0))
    _, count = np.unique(key, return_counts=True)
    return key, d["inverse"], count


def main():
    spec = importlib.util.spec_from_file_location("ref_transform", os.path.join(REF, "pointcept", "datasets", "transform.py"))
    tr = importlib.util.module_from_spec(spec)
    sys.modules["ref_transform"] = tr
    spec.loader.exec_module(tr)
    lists = train_lists()
    with open(os.path.join(OUT, "pdf_train_transforms.json"), "w") as f:
        json.dump(lists, f, indent=1, sort_keys=True)
    out, meta = {}, {}

    def run(tag, cfgs, scenes, grid=None):
        np.random.seed(zlib.crc32(tag.encode()))
        random.seed(zlib.crc32(tag.encode()))
        m = []
        for s, d in enumerate(scenes):
            for k, v in d.items():
                out[f"{tag}/in{s}/{k}"] = v
            d = {k: v.copy() for k, v in d.items()}
            with Recorder() as rec:
                for c in cfgs:
                    d = tr.TRANSFORMS.build(dict(c))(d)
            for k, v in d.items():   # (an output equal to its input, dtype included, is not stored: the test reads the input)
                src = scenes[s].get(k)
                if not (src is not None and src.dtype == v.dtype and src.shape == v.shape and np.array_equal(src, v)):
                    out[f"{tag}/out{s}/{k}"] = v
            for j, (name, v) in enumerate(rec.log):
                out[f"{tag}/draw{s}/{j}"] = v
            for j, (vol, val) in enumerate(rec.elastic):
                out[f"{tag}/elastic{s}/{j}/vol"], out[f"{tag}/elastic{s}/{j}/disp"] = vol, val
            if grid is not None:
                for k, v in zip(("key", "inverse", "count"), grid_ref(tr, d["coord"], grid)):
                    out[f"{tag}/grid{s}/{k}"] = v
            m.append([name for name, _ in rec.log])
        meta[tag] = dict(cfgs=cfgs, draws=m, grid=grid)

    for i, c in enumerate(SINGLE):
        for dt in (np.float32, np.float64):
            run(f"single{i}_{np.dtype(dt).name}", [c], [scene(100 + i, 150, dt, normal=True, extent=1.0)])
    pre = lambda name: [c for c in lists[name] if c["type"] not in ("GridSample",)][: [c["type"] for c in lists[name]].index("GridSample")]
    run("chain_s3dis_pt", pre("s3dis/openseg-pt-v1-0-pointpdf-v1m1-base"), [scene(7, 700, np.float64), scene(8, 900, np.float64)], 0.04)
    run("chain_s3dis_st", pre("s3dis/openseg-st-v1m1-0-origin-pointpdf-v1m1-base"), [scene(9, 600, np.float64), scene(10, 500, np.float64)],
        0.04)
    run("chain_scannet_pt", pre("scannet/openseg-pt-v1-0-pointpdf-v1m1-base"),
        [scene(11, 600, np.float32, normal=True, extent=1.5), scene(12, 500, np.float32, normal=True, extent=1.2)], 0.02)
    # float64 millimetre decimals straight into GridSample: many points sit on a 0.04 face, where float32 rounding changes the voxel
    run("grid_f64_mm", [], [dict(coord=scene(13, 2000, np.float64)["coord"]), dict(coord=scene(14, 1500, np.float64)["coord"])], 0.04)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "ops_augment_ref.npz"), **out)
    print({k: v.shape for k, v in list(out.items())[:5]}, len(out))


if __name__ == "__main__":
    main()

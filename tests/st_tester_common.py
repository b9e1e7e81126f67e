"""Shared by tests/test_st_tester_cpu.py and tests/test_gpu_st_tester.py: the tiny StratifiedTransformer of the fixture
tests/golden/tester_st_ref.npz (make_golden_st_tester.py), its scene and test section, and the comparison of window edge tables
scene by scene."""
import os

import numpy as np
import torch

import helpers
from pointcloudpdf_amd import stratified, synthetic
from pointcloudpdf_amd.registry import MODELS

K = 13
SEED = 21   # tests/golden/make_golden_st_tester.py: SEED
# tests/golden/make_golden_st_tester.py: ST_TINY -- the S3DIS recipe's backbone with one block pair per level and 48 channels
ST_TINY = dict(downsample_scale=8, depths=[2, 2, 2, 2], channels=[48, 48, 48, 48], num_heads=[3, 3, 3, 3],
               window_size=[0.16, 0.32, 0.64, 1.28], up_k=3, grid_sizes=[0.04, 0.08, 0.16, 0.32], quant_sizes=[0.01, 0.02, 0.04, 0.08],
               rel_query=True, rel_key=True, rel_value=True, drop_path_rate=0.3, num_layers=4, concat_xyz=True, num_classes=K, ratio=0.25,
               k=16, prev_grid_size=0.04, sigma=1.0, stem_transformer=True, kp_ball_radius=0.04 * 2.5, kp_max_neighbor=34)
VOTE_TOL = 1e-4   # the project's ST parity bar (test_stratified_model_matches_reference_classes_on_gpu: helpers.REL_TOL)


def st_section(augs=None):
    """The fixture's test section: no scene-level shift (the fixture's voxels are laid out on the raw coordinates), the ST recipes'
    voxelize / post_transform (configs/s3dis/openseg-st-v1m1-0-origin-msp.py, the section the config keeps as a comment)."""
    return dict(transform=[dict(type="NormalizeColor")], test_mode=True, test_cfg=dict(
        voxelize=dict(type="GridSample", grid_size=0.04, hash_type="fnv", mode="test", keys=("coord", "color"), return_grid_coord=True),
        crop=None,
        post_transform=[dict(type="CenterShift", apply_z=False), dict(type="ToTensor"),
                        dict(type="Collect", keys=("coord", "grid_coord", "index"), feat_keys=("coord", "color"))],
        aug_transform=augs or [[dict(type="RandomScale", scale=[1, 1])]]))


def load_ref(golden_dir):
    return np.load(os.path.join(golden_dir, "tester_st_ref.npz"))


def ref_scene(ref):
    return dict(coord=ref["scene/coord"], color=ref["scene/color"], segment=ref["scene/segment"], name="golden_st")


def tiny_model(device="cpu"):
    model = helpers.Wrap(MODELS.build(dict(type="ST-v1m1", **ST_TINY)))
    synthetic.fill_parameters_deterministic(model.backbone, seed=SEED)
    return model.to(device).eval()


def run_scene_tester(model, scene, device, fragments_per_batch, group=None, section=None):
    """-> dict(votes, pred, score, logits = the forward's outputs per batch, batches = (index, feat) per batch, keys seen)."""
    from pointcloudpdf_amd.testing import SceneTester, TestPipeline

    seen = dict(logits=[], batches=[], geometry=[])

    def forward(batch):
        seen["geometry"].append(batch.get("st_geometry"))
        logits = model({k: batch[k] for k in ("coord", "feat", "offset", "offset_host", "st_geometry") if k in batch})
        seen["logits"].append(logits)
        seen["batches"].append((batch["index"], batch["feat"]))
        return logits, -torch.softmax(logits, -1).max(-1)[0]

    tester = SceneTester(forward, K, TestPipeline(section or st_section()), fragments_per_batch=fragments_per_batch, group=group,
                         device=device, st_backbone=model.backbone)
    try:
        pred, score, votes = tester.run(scene, return_votes=True)
    finally:
        tester.close()
    return dict(votes=votes, pred=pred, score=score, **seen)


def check_votes_agree(votes_a, votes_b, tol=VOTE_TOL, cap=0.01):
    """|a - b| <= tol x max|vote|; arg-max equal wherever the top-two margin exceeds that bound, and at most ``cap`` of the points are
    excluded by the margin rule."""
    a, b = votes_a.detach().cpu().double(), votes_b.detach().cpu().double()
    bound = tol * float(b.abs().max())
    err = float((a - b).abs().max())
    print(f"votes: max |diff| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"votes differ by {err:.3e} > {bound:.3e}"
    top2 = b.topk(2, dim=1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > bound
    excluded = 1.0 - float(clear.double().mean())
    print(f"votes: {excluded:.4%} of the points excluded by the margin rule")
    assert excluded <= cap, f"{excluded:.3%} of the points have a top-two margin below the bound"
    assert torch.equal(a.argmax(1)[clear], b.argmax(1)[clear])


# ---- window edge tables, scene by scene ----------------------------------------------------------------------------------------------
def three_scenes(sizes, window_size, seed=0, device="cpu"):
    """Scenes of ``sizes`` points in a 1.1 x 0.9 x 0.5 m box; scenes 2 and 3 translated by 0.37 and 1.61 window sizes in x / y, so that
    their minima are no multiples of the window size away from the batch minimum.  -> xyz (n, 3) float32, offset int32, ends."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for s, n in enumerate(sizes):
        p = torch.rand(n, 3, generator=g) * torch.tensor([1.1, 0.9, 0.5])
        move = (0.0, 0.37, 1.61)[s] * window_size
        parts.append(p + torch.tensor([move, move, 0.0]))
    ends = np.cumsum(sizes).tolist()
    return torch.cat(parts).float().contiguous().to(device), torch.tensor(ends, dtype=torch.int32, device=device), ends


def key_subset(ends, device="cpu"):
    """Every 8th point of every scene (stands in for the FPS key subset) -> (ids in the batch, list of per-scene local ids)."""
    local = [torch.arange(0, z - a, 8, device=device) for a, z in zip([0] + ends[:-1], ends)]
    return torch.cat([l + a for l, a in zip(local, [0] + ends[:-1])]), local


def restrict(table, a, z):
    """Rows a .. z - 1 of a (index_0, index_1, offsets, n_max, rel_idx) table with row and key ids rebased to the scene."""
    i0, i1, off, _, rel = table
    e0, e1 = int(off[a]), int(off[z])
    o = (off[a:z + 1] - e0).cpu()
    return ((i0[e0:e1] - a).cpu(), (i1[e0:e1] - a).cpu(), o, int(torch.diff(o).max()) if z > a else 0, rel[e0:e1].cpu())


def tables_equal(x, y):
    return (torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3] and torch.equal(x[4], y[4]))


def single_scene_tables(layer, xyz, ends, local_keys):
    """Every scene collated alone as a batch of one through the default (batch-origin) path."""
    out = []
    for (a, z), ds in zip(zip([0] + ends[:-1], ends), local_keys):
        part = xyz[a:z].contiguous()
        out.append(layer.window_tables(part, torch.tensor([z - a], dtype=torch.int32, device=xyz.device), ds))
    return out

#!/usr/bin/env python3
"""Generate tests/golden/model_ptv3_ref.npz by running the REFERENCE's own Point Transformer V3 classes.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_ptv3.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py, models/utils/structure.py, models/utils/misc.py,
models/utils/serialization/, models/modules.py, models/point_prompt_training/prompt_driven_normalization.py and models/default.py, over
stand-ins written HERE for what the container lacks:
  * ``addict.Dict``: an attribute dict;
  * ``spconv.pytorch``: SparseConvTensor / SparseModule / SubMConv3d evaluated by DENSE torch convolutions on the bounding box
    (spunet_cases.subm_dense), plus ``spconv.modules.is_spconv_module`` -- the fixture pins the reference's wiring, not spconv;
  * ``torch_scatter.segment_csr`` (index_reduce / index_add over the segment ids), timm's ``DropPath``;
  * ``pointcept.models.builder`` (MODELS / MODULES registries with ``build_model``) and ``pointcept.models.losses.build_criteria``
    (cross entropy, ignore_index -1).

Stored (data only):
  1. codes, depth, orders and inverses of the four orders on ptv3_cases.code_batch();
  2. ``pad`` / ``unpad`` / ``cu_seqlens`` of the reference's ``get_padding_and_inverse`` for K = 48 and scenes of 30, 48, 49, 96, 101 rows;
  3. one ``SerializedPooling`` step (stride 2, no shuffle): pooling_inverse, pooled grid_coord / batch / codes / coord / feat;
  4. ``DefaultSegmentorV2`` over ptv3_cases.MODEL_KW with CE: rpe off / on, train (drop_path 0, shuffle_orders with a fixed CPU seed) and
     eval (drop_path 0.3), in fp32 and float64: state-dict keys and shapes, thinned logits, loss, thinned float64 gradients of
     ptv3_cases.GRAD_NAMES with the reference run's own fp32 error.  The seed is stepped until the fp32 gradients are within KINK_FREE of
     the float64 run's, judged by the reference run alone."""
import importlib
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
import torch.nn as nn  # noqa: E402

import make_golden as mg  # noqa: E402  (where the reference tree lives)
import ptv3_cases as pc  # noqa: E402
import spunet_cases as sc  # noqa: E402

REF = mg.REF
# A flipped arg-max of the segment max moves a gradient by its whole contribution (1e-3 and more of the tensor's scale); the rounding noise
# of the reference's own fp32 run of this model (softmax, LayerNorm, GELU chains) is 1.0e-5 .. 1.8e-5 for every one of 16 seeds.
KINK_FREE = 5e-5


class Dict(dict):
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape=None, batch_size=None):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size)


class SparseModule(nn.Module):
    pass


class SubMConv3d(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__()
        k = kernel_size
        self.weight = nn.Parameter(torch.zeros(out_channels, k, k, k, in_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

    def forward(self, x):
        return x.replace_feature(sc.subm_dense(x.features, self.weight, self.bias, x.indices))


def segment_csr(src, indptr, reduce="sum"):
    counts = torch.diff(indptr)
    ids = torch.repeat_interleave(torch.arange(counts.shape[0]), counts)
    out = src.new_zeros((counts.shape[0],) + tuple(src.shape[1:]))
    if reduce in ("sum", "mean"):
        out = out.index_add(0, ids, src)
        return out / counts.to(src.dtype).view(-1, *([1] * (src.dim() - 1))) if reduce == "mean" else out
    return out.index_reduce(0, ids, src, {"max": "amax", "min": "amin"}[reduce], include_self=False)


class DropPath(nn.Module):
    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return x * mask


class Registry:
    def __init__(self):
        self.classes = {}

    def register_module(self, name=None):
        def deco(cls):
            self.classes[name if isinstance(name, str) else cls.__name__] = cls
            return cls
        return deco

    def build(self, cfg):
        cfg = dict(cfg)
        return self.classes[cfg.pop("type")](**cfg)


def load_reference():
    def module(name, path=None, **attrs):
        m = types.ModuleType(name)
        m.__path__ = [] if path is None else [path]
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    module("addict", Dict=Dict)
    module("spconv")
    sp = module("spconv.pytorch", SparseConvTensor=SparseConvTensor, SparseModule=SparseModule, SubMConv3d=SubMConv3d)
    sp.modules = module("spconv.pytorch.modules", is_spconv_module=lambda m: isinstance(m, SparseModule))
    sys.modules["spconv"].pytorch = sp
    module("torch_scatter", segment_csr=segment_csr)
    module("timm")
    module("timm.models")
    module("timm.models.layers", DropPath=DropPath)
    models_dir = os.path.join(REF, "pointcept", "models")
    module("pointcept", os.path.join(REF, "pointcept"))
    module("pointcept.models", models_dir)
    MODELS, MODULES = Registry(), Registry()
    module("pointcept.models.builder", MODELS=MODELS, MODULES=MODULES, build_model=MODELS.build)
    module("pointcept.models.losses",
           build_criteria=lambda cfg: (lambda pred, target: nn.functional.cross_entropy(pred, target, ignore_index=-1)))
    utils = module("pointcept.models.utils", os.path.join(models_dir, "utils"))
    misc = importlib.import_module("pointcept.models.utils.misc")
    utils.offset2batch, utils.offset2bincount, utils.batch2offset = misc.offset2batch, misc.offset2bincount, misc.batch2offset
    ppt = module("pointcept.models.point_prompt_training", os.path.join(models_dir, "point_prompt_training"))
    importlib.import_module("pointcept.models.modules")
    ppt.PDNorm = importlib.import_module("pointcept.models.point_prompt_training.prompt_driven_normalization").PDNorm
    v3 = importlib.import_module("pointcept.models.point_transformer_v3.point_transformer_v3m1_base")
    default = importlib.import_module("pointcept.models.default")
    structure = importlib.import_module("pointcept.models.utils.structure")
    return v3, default, structure


# ---------------------------------------------------------------------------------------------------------------------------------------
def part_codes(structure, out):
    grid, offset = pc.code_batch()
    point = structure.Point(grid_coord=torch.from_numpy(grid), offset=torch.from_numpy(offset), feat=torch.zeros(grid.shape[0], 1))
    point.serialization(order=list(pc.ORDERS), shuffle_orders=False)
    assert int(grid.max()) >= 256
    out.update(c_grid_coord=grid, c_offset=offset, c_depth=np.int64(point.serialized_depth), c_code=point.serialized_code.numpy(),
               c_order=point.serialized_order.numpy(), c_inverse=point.serialized_inverse.numpy())


def part_padding(v3, structure, out):
    attn = v3.SerializedAttention(channels=32, num_heads=2, patch_size=pc.PAD_K, enable_flash=False)
    attn.patch_size = pc.PAD_K
    offset = torch.cumsum(torch.tensor(pc.PAD_SIZES), 0)
    point = structure.Point(offset=offset, feat=torch.zeros(int(offset[-1]), 1))
    pad, unpad, cu = attn.get_padding_and_inverse(point)
    out.update(p_pad=pad.numpy(), p_unpad=unpad.numpy(), p_cu_seqlens=cu.numpy())


def part_pooling(v3, structure, out):
    grid, offset, coord, feat = pc.pool_batch()
    pool = v3.SerializedPooling(32, 64, stride=2, shuffle_orders=False).double()
    pool.norm = pool.act = None
    pc.named_weights(pool, 0)
    point = structure.Point(grid_coord=torch.from_numpy(grid), coord=torch.from_numpy(coord).double(), offset=torch.from_numpy(offset),
                            feat=torch.from_numpy(feat).double())
    point.serialization(order=list(pc.ORDERS), shuffle_orders=False)
    with torch.no_grad():
        low = pool(point)
    out.update(s_coord=coord, s_feat=feat, s_cluster=low.pooling_inverse.numpy(), s_grid_coord=low.grid_coord.numpy(),
               s_batch=low.batch.numpy(), s_code=low.serialized_code.numpy(), s_order=low.serialized_order.numpy(),
               s_pooled_coord=low.coord.numpy(), s_pooled_feat=low.feat.numpy()[::pc.POOL_THIN], s_depth=np.int64(low.serialized_depth))


def run(default, case, seed, dtype, batch):
    grid, coord, feat, offset, segment = batch
    rpe, train, dpr, shuffle = pc.MODEL_CASES[case]
    torch.manual_seed(0)
    model = default.DefaultSegmentorV2(backbone=dict(type="PT-v3m1", enable_rpe=rpe, drop_path=dpr, shuffle_orders=shuffle, **pc.MODEL_KW),
                                       criteria=None, **pc.SEG_KW).to(dtype)
    pc.named_weights(model, seed)
    model.train(train)
    data = dict(grid_coord=torch.from_numpy(grid), coord=torch.from_numpy(coord).to(dtype), feat=torch.from_numpy(feat).to(dtype),
                offset=torch.from_numpy(offset), segment=torch.from_numpy(segment))
    torch.manual_seed(pc.SHUFFLE_SEED)
    if train:
        got = {}
        h = model.seg_head.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o))
        res = model(data)
        h.remove()
        names = pc.GRAD_NAMES + (pc.RPE_GRAD_NAMES if rpe else [])
        params = dict(model.named_parameters())
        grads = torch.autograd.grad(res["loss"], [params[k] for k in names])
        return dict(model=model, logits=got["logits"].detach(), loss=res["loss"].detach(), grads=[g.detach() for g in grads])
    with torch.no_grad():
        res = model(data)
    return dict(model=model, logits=res["seg_logits"], loss=res["loss"], grads=[])


def rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def main():
    v3, default, structure = load_reference()
    out = {}
    part_codes(structure, out)
    part_padding(v3, structure, out)
    part_pooling(v3, structure, out)
    batch = pc.scene_batch()
    seed = 0
    while True:
        worst = 0.0
        runs = {}
        for case in ("train", "train_rpe"):
            lo, hi = run(default, case, seed, torch.float32, batch), run(default, case, seed, torch.float64, batch)
            runs[case] = (lo, hi)
            worst = max([worst] + [rel(a, b) for a, b in zip(lo["grads"], hi["grads"])])
        print(f"seed {seed}: the reference's fp32 gradients are {worst:.2e} off its float64 run", flush=True)
        if worst <= KINK_FREE:
            break
        seed += 1
        assert seed < 16, "no kink-free seed among 16"
    for case in ("eval", "eval_rpe"):
        runs[case] = (run(default, case, seed, torch.float32, batch), run(default, case, seed, torch.float64, batch))
    grid, coord, feat, offset, segment = batch
    n = grid.shape[0]
    rows = np.arange(0, n, max(1, n // pc.KEEP_ROWS))
    out.update(seed=np.int64(seed), m_grid_coord=grid, m_coord=coord, m_feat=feat, m_offset=offset, m_segment=segment, m_rows=rows)
    for case, (lo, hi) in runs.items():
        sd = hi["model"].state_dict()
        out[f"{case}_keys"] = np.array(list(sd.keys()))
        out[f"{case}_shapes"] = np.array([list(v.shape) + [-1] * (5 - v.dim()) for v in sd.values()])
        out[f"{case}_logits"] = hi["logits"][rows].numpy()
        out[f"{case}_loss"] = hi["loss"].numpy()
        out[f"{case}_err_logits"] = rel(lo["logits"], hi["logits"])
        out[f"{case}_err_loss"] = rel(lo["loss"], hi["loss"])
        for i, (a, b) in enumerate(zip(lo["grads"], hi["grads"])):
            out[f"{case}_grad_{i}"] = pc.thin_grad(b.numpy())
            out[f"{case}_grad_err_{i}"] = np.float64(rel(a, b))
            out[f"{case}_grad_max_{i}"] = np.float64(b.abs().max())
        print(case, "fp32 vs float64: logits", out[f"{case}_err_logits"], "loss", out[f"{case}_err_loss"])
    path = os.path.join(HERE, "model_ptv3_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/model_spunet_ref.npz by running the REFERENCE's own ``SpUNetBase``.

Run in the build container only (needs the reference tree, like make_golden.py):   python tests/golden/make_golden_spunet.py

Executed from the reference (imported in place, never copied; bytecode writing disabled):
pointcept/models/sparse_unet/spconv_unet_v1m1_base.py, over stand-ins written HERE for what the container lacks:
  * ``spconv.pytorch``: SparseConvTensor / SparseModule / SparseSequential / SubMConv3d / SparseConv3d / SparseInverseConv3d / Identity
    whose layers evaluate the definitions of pointcloudpdf_amd/sparse_conv.py by DENSE torch convolutions on the bounding box
    (spunet_cases.subm_dense / down_dense / inverse_dense) -- so the fixture pins the reference's wiring (skips, concatenation order, key
    sharing, BatchNorm settings), not spconv itself, which is unpinned;
  * ``torch_geometric.utils.scatter`` (mean / sum over dim 0), timm's ``trunc_normal_`` (torch's), ``pointcept.models.builder`` (a
    registry that registers nothing) and ``pointcept.models.utils.offset2batch``.

The run: 2 scenes of about 1,500 voxels in a 24^3 box (four halvings still leave sites), spunet_cases.MODEL_KW (every width occurs),
name-keyed deterministic weights (spunet_cases.named_weights), train and eval modes in fp32 and float64.  Stored: state-dict keys and
shapes, thinned logits, the CE loss, thinned float64 gradients of spunet_cases.GRAD_NAMES with the reference run's own fp32 error, and the
BatchNorm buffers of three norms after one training forward.  The seed is stepped until the fp32 run's gradients are within KINK_FREE of
the float64 run's (no activation on a ReLU kink), judged by the reference run alone."""
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
import spunet_cases as sc  # noqa: E402

REF = mg.REF
KINK_FREE = 1e-5
GRAD_KEEP = 4096
BUFFERS = ["conv_input.1.running_mean", "conv_input.1.running_var", "enc.3.block0.bn2.running_var", "dec.0.block0.proj.1.running_mean"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# stand-in for spconv.pytorch: the definitions, evaluated densely
# ---------------------------------------------------------------------------------------------------------------------------------------
class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape=None, batch_size=None, keys=None):
        self.features, self.indices, self.spatial_shape, self.batch_size = features, indices, spatial_shape, batch_size
        self.keys = {} if keys is None else keys

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.keys)


class SparseModule(nn.Module):
    pass


class SparseSequential(SparseModule):
    def __init__(self, *args):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], dict):
            for k, m in args[0].items():
                self.add_module(k, m)
        else:
            for i, m in enumerate(args):
                self.add_module(str(i), m)

    def forward(self, x):
        for m in self._modules.values():
            x = m(x) if isinstance(m, SparseModule) else x.replace_feature(m(x.features))
        return x


class _Conv(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__()
        k = kernel_size
        self.weight = nn.Parameter(torch.zeros(out_channels, k, k, k, in_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self.indice_key, self.kernel_size, self.stride = indice_key, k, stride


class SubMConv3d(_Conv):
    def forward(self, x):
        return x.replace_feature(sc.subm_dense(x.features, self.weight, self.bias, x.indices))


class SparseConv3d(_Conv):
    def forward(self, x):
        assert self.kernel_size == 2 and self.stride == 2
        parent, _, coarse, _ = sc.down_brute(x.indices)   # (the model's max + 96 shape never truncates)
        keys = dict(x.keys)
        keys[self.indice_key] = (x.indices, parent)
        return SparseConvTensor(sc.down_dense(x.features, self.weight, self.bias, x.indices, coarse), coarse, None, x.batch_size, keys)


class SparseInverseConv3d(_Conv):
    def forward(self, x):
        fine, parent = x.keys[self.indice_key]
        return SparseConvTensor(sc.inverse_dense(x.features, self.weight, self.bias, fine, x.indices, parent), fine, None, x.batch_size, x.keys)


class Identity(nn.Identity):
    pass


def scatter(src, index, dim=0, reduce="sum"):
    n = int(index.max()) + 1
    out = src.new_zeros((n,) + tuple(src.shape[1:])).index_add(0, index, src)
    if reduce == "mean":
        out = out / torch.bincount(index, minlength=n).clamp(min=1).to(src.dtype).view(-1, *([1] * (src.dim() - 1)))
    return out


def load_reference():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class _Registry:
        @staticmethod
        def register_module(*a, **k):
            return lambda cls: cls

    module("spconv")
    module("spconv.pytorch", SparseConvTensor=SparseConvTensor, SparseModule=SparseModule, SparseSequential=SparseSequential,
           SubMConv3d=SubMConv3d, SparseConv3d=SparseConv3d, SparseInverseConv3d=SparseInverseConv3d, Identity=Identity)
    sys.modules["spconv"].pytorch = sys.modules["spconv.pytorch"]
    module("torch_geometric")
    module("torch_geometric.utils", scatter=scatter)
    module("timm")
    module("timm.models")
    module("timm.models.layers", trunc_normal_=nn.init.trunc_normal_)
    for name in ("pointcept", "pointcept.models"):
        if name not in sys.modules:
            module(name)
    module("pointcept.models.builder", MODELS=_Registry())
    module("pointcept.models.utils", offset2batch=lambda offset: torch.searchsorted(offset.long(), torch.arange(int(offset[-1])), right=True))
    spec = importlib.util.spec_from_file_location("ref_spunet", os.path.join(REF, "pointcept/models/sparse_unet/spconv_unet_v1m1_base.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_spunet"] = mod
    spec.loader.exec_module(mod)
    return mod


def scene_batch(seed=7):
    rng = np.random.default_rng(seed)
    coords, sizes = [], (1500, 1400)
    for n in sizes:
        cells = rng.permutation(24 ** 3)[:n]
        coords.append(np.stack([cells // 576, (cells // 24) % 24, cells % 24], 1))
    grid = np.concatenate(coords).astype(np.int32)
    n = grid.shape[0]
    feat = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    segment = rng.integers(0, 13, n).astype(np.int64)
    segment[rng.permutation(n)[: n // 20]] = -1
    return grid, feat, np.cumsum(sizes).astype(np.int32), segment


def run(ref, seed, dtype, grid, feat, offset, segment):
    torch.manual_seed(0)
    model = ref.SpUNetBase(**sc.MODEL_KW).to(dtype)
    sc.named_weights(model, seed)
    data = dict(grid_coord=torch.from_numpy(grid), feat=torch.from_numpy(feat).to(dtype), offset=torch.from_numpy(offset))
    model.train()
    logits = model(data)
    loss = nn.functional.cross_entropy(logits, torch.from_numpy(segment), ignore_index=-1)
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(loss, [params[k] for k in sc.GRAD_NAMES])
    buffers = {k: v.detach().clone() for k, v in model.state_dict().items() if k in BUFFERS}
    model2 = ref.SpUNetBase(**sc.MODEL_KW).to(dtype)
    sc.named_weights(model2, seed)
    model2.eval()
    with torch.no_grad():
        ev = model2(data)
    return dict(model=model, train=logits.detach(), loss=loss.detach(), grads=[g.detach() for g in grads], buffers=buffers, eval=ev)


def rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def main():
    ref = load_reference()
    grid, feat, offset, segment = scene_batch()
    seed = 0
    while True:
        lo = run(ref, seed, torch.float32, grid, feat, offset, segment)
        hi = run(ref, seed, torch.float64, grid, feat, offset, segment)
        err_grads = [rel(a, b) for a, b in zip(lo["grads"], hi["grads"])]
        print(f"seed {seed}: the reference's fp32 gradients are {max(err_grads):.2e} off its float64 run", flush=True)
        if max(err_grads) <= KINK_FREE:
            break
        seed += 1
        assert seed < 16, "no kink-free seed among 16"
    sd = hi["model"].state_dict()
    n = grid.shape[0]
    rows = np.arange(0, n, max(1, n // sc.KEEP_ROWS))
    out = dict(seed=np.int64(seed), keys=np.array(list(sd.keys())), shapes=np.array([list(v.shape) + [-1] * (5 - v.dim()) for v in sd.values()]),
               grid_coord=grid, feat=feat, offset=offset, segment=segment, rows=rows, grad_names=np.array(sc.GRAD_NAMES),
               train_logits=hi["train"][rows].numpy(), eval_logits=hi["eval"][rows].numpy(), loss=hi["loss"].numpy(),
               err_train_logits=rel(lo["train"], hi["train"]), err_eval_logits=rel(lo["eval"], hi["eval"]), err_loss=rel(lo["loss"], hi["loss"]),
               err_grads=np.array(err_grads), buffer_names=np.array(BUFFERS))
    for i, g in enumerate(hi["grads"]):
        stride = max(1, g.numel() // GRAD_KEEP)
        out[f"grad_{i}"] = g.reshape(-1)[::stride].numpy()
        out[f"grad_stride_{i}"] = np.int64(stride)
        out[f"grad_max_{i}"] = np.float64(g.abs().max())
    for i, k in enumerate(BUFFERS):
        out[f"buffer_{i}"] = hi["buffers"][k].numpy()
    path = os.path.join(HERE, "model_spunet_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

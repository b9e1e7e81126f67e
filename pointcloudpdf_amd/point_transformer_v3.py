"""PT-v3m1 -- pointcept/models/point_transformer_v3/point_transformer_v3m1_base.py mirrored class by class (``RPE``,
``SerializedAttention``, ``MLP``, ``Block``, ``SerializedPooling``, ``SerializedUnpooling``, ``Embedding``, ``PointTransformerV3``), with
its supports: ``Point`` (models/utils/structure.py; an attribute dict with ``serialization()`` / ``sparsify()``, ``octreetization`` left
out), ``PointModule`` / ``PointSequential`` (models/modules.py), ``PDNorm`` (point_prompt_training/prompt_driven_normalization.py, plain
torch) and the serialization codes (models/utils/serialization/).  Constructor arguments, submodule names and ``state_dict`` keys are the
reference's: a reference checkpoint loads with ``strict=True``.  The convolutions (``Block.cpe``, the stem) are this package's
sparse_conv.py -- spconv does not exist for this platform, so their arithmetic is unpinned (sparse_conv.py's contract).

Serialization (coordinate-only, exact integers).  ``encode`` yields ``batch << 3 depth | curve(grid_coord)`` for the curves ``z``,
``z-trans``, ``hilbert``, ``hilbert-trans``, bit-identical to the reference's table look-ups; orders are stable sorts (duplicated sites
keep row order), inverses a scatter; ``depth = int(grid_coord.max()).bit_length()`` is the one host read, with the reference's asserts
(depth <= 16, 63 bits).  ``shuffle_orders`` draws ``torch.randperm(k)`` from torch's CPU generator where the reference does: once in
``serialization``, then once per ``SerializedPooling`` in encoder order.  All of it -- every level's codes, orders, inverses, depth,
pooling tables (``cluster`` = the reference's ``pooling_inverse``, ``idx_ptr``, ``sorted``, head rows), the per-level ``SpGeometry`` and
the patch tables -- depends on the coordinates and those draws alone: ``PointTransformerV3.make_geometry(grid_coord, offset)`` builds a
``PTv3Geometry`` ahead of the forward (it makes the draws; a geometry serves ONE forward) and the forward takes it from
``data_dict["ptv3_geometry"]``; without the key it builds the same object itself, bit-identically.  With the geometry handed in the
forward performs no host read.  Device tensors run csrc/serialization.hip; host tensors take the torch composition, which follows the
reference line by line and is the kernels' oracle.

Patch layout (derived from ``get_padding_and_inverse``).  A scene of ``n`` points in serialized order, ``J = ceil(n / K)``,
``r = n % K``: if ``n <= K`` the scene is one patch of ``n`` rows; otherwise patch ``j < J - 1`` covers the positions
``[j K, (j + 1) K)``, and, when ``r != 0``, the last patch holds its own ``r`` rows followed by the last ``K - r`` rows of the patch
before it -- as a set the positions ``[n - K, n)`` -- of which only the ``r`` own rows keep their output (``inverse =
unpad[serialized_inverse]``).  The keys and values at ``[n - K, (J - 1) K)`` therefore serve two patches.  Softmax attention does not
depend on the order of the keys, so ``serial_attention`` -- one autograd node over csrc/serial_attention.hip on the (N, 3C) rows of the
qkv Linear in ORIGINAL order -- needs no ``pad`` / ``unpad`` array and no gathered copy, only per level a small table that maps query
chunks to key windows (and, for the backward, key chunks to their one or two query windows); it never forms a K x K tensor, saves
``out`` and the rows' log-sum-exp, and its backward recomputes the probabilities (no float atomics, bit-reproducible, every gradient
element written once).  The HIP class is fp32 device tensors with head width 16, C <= 512, any K >= 1 and no attention dropout
(``pdf_serial_attn_supported``); other head widths, ``enable_rpe=True``, ``attn_drop > 0`` in training, host tensors and 16-bit inputs
take the composition, the reference's non-flash branch (``RPE`` keeps the reference's ``int((4 * patch_size) ** (1 / 3) * 2)``: 15, not
16, at patch_size 128).

``enable_flash=True`` is accepted although ``flash_attn`` does not exist here: it selects the flash branch's LAYOUT (fixed K, the padding
rule above, a short scene as one short sequence; the index tables are pinned by the fixture) computed by the node above in fp32 -- the
reference's ``.half()`` is not imitated, so this branch's ARITHMETIC is unpinned.  The reference's three asserts on the flag stay.
With ``enable_flash=False`` the patch size is ``min(smallest scene, patch_size)`` per level, resolved when the geometry is made.
(The reference caches ``pad`` / ``unpad`` on the Point under one key whatever the patch size; the tables here are kept per patch size.)

Left for later: RPE inside the kernel, 16-bit operands, the 512-wide cpe as a HIP pass, ``cls_mode``'s pooling head, PPT."""
import math
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from . import dense
from . import sparse_conv as spconv
from .dense import _amp_bwd, _amp_fwd
from .point_transformer_v2 import _SegMax, _segment_rows, segment_max_torch, segment_mean_torch
from .registry import MODELS

FORCE_TORCH = False   # module-wide switch: serialization, pooling partition and attention take the composition (tools/ptv3_bench.py's other side)

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
QROWS = 64            # rows per table entry (csrc/serial_attention.hip: ROWS)


def _be():
    from . import _native

    return _native.hip_backend()


def _hip(t):
    return t.is_cuda and not FORCE_TORCH


# ---------------------------------------------------------------------------------------------------------------------------------------
# Serialization codes (models/utils/serialization/{default,z_order,hilbert}.py), the composition
# ---------------------------------------------------------------------------------------------------------------------------------------
def _interleave3(x, y, z, depth):
    key = torch.zeros_like(x)
    for i in range(depth):
        m = 1 << i
        key = key | ((x & m) << (2 * i + 2)) | ((y & m) << (2 * i + 1)) | ((z & m) << (2 * i))
    return key


def z_order_encode(grid_coord, depth=16):
    """z_order.py:66-101: bit i of x / y / z at 3 i + 2 / 3 i + 1 / 3 i (the reference's two 8-bit tables spell the same bits out)."""
    mask = (1 << depth) - 1
    x, y, z = (grid_coord[:, i].long() & mask for i in range(3))
    return _interleave3(x, y, z, depth)


def hilbert_encode(grid_coord, depth=16):
    """hilbert.py:91-198 (Skilling's transform) on integers: per bit from the top and per axis, invert the lower bits of axis 0 where the
    bit is on, exchange them with the axis where it is off; interleave; Gray -> binary over the 3 depth bits."""
    mask = (1 << depth) - 1
    X = [grid_coord[:, i].long() & mask for i in range(3)]
    for bit in range(depth):
        q = 1 << (depth - 1 - bit)
        lower = q - 1
        for d in range(3):
            on = (X[d] & q) != 0
            if d == 0:
                X[0] = torch.where(on, X[0] ^ lower, X[0])
            else:
                t = torch.where(on, torch.zeros_like(X[0]), (X[0] ^ X[d]) & lower)
                X[0] = torch.where(on, X[0] ^ lower, X[0] ^ t)
                X[d] = X[d] ^ t
    h = _interleave3(X[0], X[1], X[2], depth)
    for sh in (1, 2, 4, 8, 16, 32):
        h = h ^ (h >> sh)
    return h


@torch.no_grad()
def encode(grid_coord, batch=None, depth=16, order="z"):
    """default.py:8-24."""
    assert order in {"z", "z-trans", "hilbert", "hilbert-trans"}
    if order == "z":
        code = z_order_encode(grid_coord, depth=depth)
    elif order == "z-trans":
        code = z_order_encode(grid_coord[:, [1, 0, 2]], depth=depth)
    elif order == "hilbert":
        code = hilbert_encode(grid_coord, depth=depth)
    else:
        code = hilbert_encode(grid_coord[:, [1, 0, 2]], depth=depth)
    if batch is not None:
        code = batch.long() << depth * 3 | code
    return code


def offset2batch(offset, n=None):
    """models/utils/misc.py without its host read (repeat_interleave): the scene of every row."""
    n = int(n) if n is not None else int(offset[-1])
    return torch.searchsorted(offset.long().contiguous(), torch.arange(n, device=offset.device), right=True)


def batch2offset(batch):
    return torch.cumsum(batch.bincount(), dim=0).long()


def offset2bincount(offset):
    return torch.diff(offset, prepend=torch.tensor([0], device=offset.device, dtype=torch.long))


def serialize_codes(grid_coord, batch, depth, orders):
    """(k, n) int64 codes of the named curves."""
    if _hip(grid_coord) and grid_coord.shape[0] > 0 and len(orders) <= 8:
        return _be().serial_codes(grid_coord.int().contiguous(), batch.long().contiguous(), depth, list(orders))
    return torch.stack([encode(grid_coord, batch, depth, order=o) for o in orders])


def order_and_inverse(code):
    """structure.py:85-92 with the stable sort: equal codes (duplicated sites) keep row order."""
    if _hip(code) and code.shape[1] > 0:
        return _be().serial_sort(code.contiguous())
    order = torch.sort(code, dim=1, stable=True)[1]
    inverse = torch.zeros_like(order).scatter_(dim=1, index=order,
                                               src=torch.arange(0, code.shape[1], device=order.device).repeat(code.shape[0], 1))
    return order, inverse


def pool_partition_torch(code0):
    """point_transformer_v3m1_base.py:385-396 -> (cluster, sorted, idx_ptr, head): the composition and the oracle of
    pdf_serial_pool_partition (``torch.sort(cluster)`` as a stable sort: a cluster's rows in ascending row index)."""
    _, cluster, counts = torch.unique(code0, sorted=True, return_inverse=True, return_counts=True)
    indices = torch.sort(cluster, stable=True)[1]
    idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)])
    head = indices[idx_ptr[:-1]]
    return cluster, indices.int(), idx_ptr.int(), head


def pool_partition(code0, order0, shift):
    """The partition of one ``SerializedPooling`` from the level's first code row and its order (``code0 >> shift`` is sorted by it)."""
    if _hip(code0) and code0.shape[0] > 0:
        cluster, srt, idx_ptr, head, _ = _be().serial_pool_partition(code0.contiguous(), order0.contiguous(), shift)
        return cluster, srt, idx_ptr, head
    return pool_partition_torch(code0 >> shift)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Patch tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def padding_and_inverse(offset, patch_size):
    """``SerializedAttention.get_padding_and_inverse`` (:115-170) on host tensors -> (pad, unpad, cu_seqlens)."""
    offset = offset.long().cpu()
    bincount = offset2bincount(offset)
    bincount_pad = torch.div(bincount + patch_size - 1, patch_size, rounding_mode="trunc") * patch_size
    mask_pad = bincount > patch_size
    bincount_pad = ~mask_pad * bincount + mask_pad * bincount_pad
    _offset = nn.functional.pad(offset, (1, 0))
    _offset_pad = nn.functional.pad(torch.cumsum(bincount_pad, dim=0), (1, 0))
    pad = torch.arange(_offset_pad[-1])
    unpad = torch.arange(_offset[-1])
    cu_seqlens = []
    for i in range(len(offset)):
        unpad[_offset[i]:_offset[i + 1]] += _offset_pad[i] - _offset[i]
        if bincount[i] != bincount_pad[i]:
            pad[_offset_pad[i + 1] - patch_size + (bincount[i] % patch_size):_offset_pad[i + 1]] = pad[
                _offset_pad[i + 1] - 2 * patch_size + (bincount[i] % patch_size):_offset_pad[i + 1] - patch_size]
        pad[_offset_pad[i]:_offset_pad[i + 1]] -= _offset_pad[i] - _offset[i]
        cu_seqlens.append(torch.arange(_offset_pad[i], _offset_pad[i + 1], step=patch_size, dtype=torch.int32))
    cu_seqlens = nn.functional.pad(torch.concat(cu_seqlens), (0, 1), value=_offset_pad[-1])
    return pad, unpad, cu_seqlens


def patch_windows(sizes, patch_size):
    """The layout rule of the module docstring: [(q_start, q_len, k_start, k_len)] per patch, positions in the batch's serialized order."""
    out, o, K = [], 0, int(patch_size)
    for n in sizes:
        n = int(n)
        if n <= K:
            if n:
                out.append((o, n, o, n))
        else:
            J, r = -(-n // K), n % K
            for j in range(J - 1):
                out.append((o + j * K, K, o + j * K, K))
            out.append((o + (J - 1) * K, r, o + n - K, K) if r else (o + (J - 1) * K, K, o + (J - 1) * K, K))
        o += n
    return out


def attention_tables(sizes, patch_size):
    """(qtab (nq, 4), ktab (nk, 8)) int32 host tensors of csrc/serial_attention.hip (include/pdfops.h)."""
    K = int(patch_size)
    qtab, ktab, o = [], [], 0
    for (q0, ql, k0, kl) in patch_windows(sizes, K):
        for a in range(0, ql, QROWS):
            qtab.append((q0 + a, min(QROWS, ql - a), k0, kl))
    for n in sizes:
        n = int(n)
        wins = patch_windows([n], K)
        shared = len(wins) > 1 and n % K != 0
        for j, (q0, ql, _, _) in enumerate(wins):
            # the keys a patch OWNS are its own rows; the patch before the last one lends its tail to the last patch's queries
            qb = (o + wins[-1][0], wins[-1][1], o + n - K) if shared and j == len(wins) - 2 else (0, 0, 0)
            for a in range(0, ql, QROWS):
                ktab.append((o + q0 + a, min(QROWS, ql - a), o + q0, ql, qb[0], qb[1], qb[2], 0))
        o += n
    return (torch.tensor(qtab, dtype=torch.int32).reshape(-1, 4), torch.tensor(ktab, dtype=torch.int32).reshape(-1, 8))


class PatchTables:
    """Per (level, patch size): the reference's pad / unpad / cu_seqlens, and the device tables of the HIP node."""

    def __init__(self, sizes, patch_size, device):
        self.patch_size = int(patch_size)
        self.sizes = [int(s) for s in sizes]
        offset = torch.cumsum(torch.tensor(self.sizes, dtype=torch.long), 0)
        pad, unpad, cu = padding_and_inverse(offset, self.patch_size)
        self.seqs = [(int(a), int(b - a)) for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]   # (start, length) in the padded order
        self.pad, self.unpad, self.cu_seqlens = pad.to(device), unpad.to(device), cu.to(device)
        self.qtab = self.ktab = None
        if device.type == "cuda":
            q, k = attention_tables(self.sizes, self.patch_size)
            self.qtab, self.ktab = q.to(device), k.to(device)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
class PTv3Level:
    def __init__(self, grid_coord, batch, offset, sizes, depth, code, order, inverse, subm_sizes):
        self.grid_coord, self.batch, self.offset, self.sizes, self.depth = grid_coord, batch, offset, sizes, depth
        self.code, self.order, self.inverse = code, order, inverse
        self.n = int(grid_coord.shape[0])
        self.pool = None       # (cluster, sorted, idx_ptr, head, pooling_depth) towards the next level
        self._patch = {}
        indices = torch.cat([batch.unsqueeze(-1).int(), grid_coord.int()], dim=1).contiguous()
        self.sp = spconv.SpGeometry.build(indices, 1, [tuple(subm_sizes)], None)   # (k = 3 for the cpe; k = 5 for the stem at level 0)

    def patch(self, patch_size):
        K = int(patch_size)
        if K not in self._patch:
            self._patch[K] = PatchTables(self.sizes, K, self.grid_coord.device)
        return self._patch[K]

    @property
    def min_size(self):
        return min(self.sizes)


class PTv3Geometry:
    """Everything of one forward that depends on the coordinates (and the ``shuffle_orders`` draws) alone; ``levels[l]``: PTv3Level."""

    def __init__(self, levels):
        self.levels = levels


def _shuffle(code, order, inverse):
    perm = torch.randperm(code.shape[0])
    return code[perm], order[perm], inverse[perm]


def build_geometry(grid_coord, offset, orders, strides, shuffle_orders, patch_sizes=None, enable_flash=True, batch=None):
    """``Point.serialization`` + the coordinate part of every ``SerializedPooling`` (:372-412), level by level.  ``patch_sizes[l]``: the
    patch sizes the blocks of level l use (their tables are built here; others on first use)."""
    grid_coord = grid_coord.int()
    offset = offset.long()
    n = grid_coord.shape[0]
    if batch is None:
        batch = offset2batch(offset, n)
    depth = int(grid_coord.max()).bit_length()
    assert depth * 3 + len(offset).bit_length() <= 63
    assert depth <= 16
    code = serialize_codes(grid_coord, batch, depth, orders)
    order, inverse = order_and_inverse(code)
    if shuffle_orders:
        code, order, inverse = _shuffle(code, order, inverse)
    sizes = offset2bincount(offset).tolist()
    levels = [PTv3Level(grid_coord, batch, offset, sizes, depth, code, order, inverse, (5, 3))]
    for stride in strides:
        lv = levels[-1]
        pd = (math.ceil(stride) - 1).bit_length()
        if pd > lv.depth:
            pd = 0
        cluster, srt, idx_ptr, head = pool_partition(lv.code[0], lv.order[0], pd * 3)
        lv.pool = (cluster, srt, idx_ptr, head, pd)
        code = (lv.code >> pd * 3)[:, head]
        order, inverse = order_and_inverse(code)
        if shuffle_orders:
            code, order, inverse = _shuffle(code, order, inverse)
        b = lv.batch[head]
        off = batch2offset(b)
        levels.append(PTv3Level(lv.grid_coord[head] >> pd, b, off, offset2bincount(off).tolist(), lv.depth - pd, code, order, inverse, (3,)))
    for l, lv in enumerate(levels):
        for K in (patch_sizes[l] if patch_sizes is not None else ()):
            lv.patch(K if enable_flash else min(lv.min_size, K))
    return PTv3Geometry(levels)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Point, PointModule, PointSequential, PDNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
class Dict(dict):
    """The part of ``addict.Dict`` the reference uses: keys as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        del self[name]


class Point(Dict):
    """models/utils/structure.py: ``coord``, ``grid_coord``, ``feat``, ``offset`` / ``batch`` and what ``serialization`` / ``sparsify`` add
    (``serialized_depth`` / ``_code`` / ``_order`` / ``_inverse``, ``sparse_shape``, ``sparse_conv_feat``).  ``ptv3_geometry`` /
    ``ptv3_level`` are this package's additions: the prebuilt tables and the level this point set lives on."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if "batch" not in self.keys() and "offset" in self.keys():
            self["batch"] = offset2batch(self.offset, self["feat"].shape[0] if "feat" in self.keys() else None)
        elif "offset" not in self.keys() and "batch" in self.keys():
            self["offset"] = batch2offset(self.batch)

    def _grid_coord(self):
        if "grid_coord" not in self.keys():
            assert {"grid_size", "coord"}.issubset(self.keys())
            self["grid_coord"] = torch.div(self.coord - self.coord.min(0)[0], self.grid_size, rounding_mode="trunc").int()

    def serialization(self, order="z", depth=None, shuffle_orders=False):
        assert "batch" in self.keys()
        self._grid_coord()
        geom = self.get("ptv3_geometry")
        if geom is None:
            if depth is not None:
                raise NotImplementedError("Point.serialization: an explicit depth is not provided")
            geom = build_geometry(self.grid_coord, self.offset, [order] if isinstance(order, str) else order, (), shuffle_orders,
                                  batch=self.batch)
            self["ptv3_geometry"] = geom
        lv = geom.levels[self.get("ptv3_level", 0)]
        self["ptv3_level"] = self.get("ptv3_level", 0)
        self["serialized_depth"] = lv.depth
        self["serialized_code"] = lv.code
        self["serialized_order"] = lv.order
        self["serialized_inverse"] = lv.inverse

    def sparsify(self, pad=96):
        assert {"feat", "batch"}.issubset(self.keys())
        self._grid_coord()
        geom = self.get("ptv3_geometry")
        if geom is not None:
            lv = geom.levels[self.get("ptv3_level", 0)]
            sp, indices = lv.sp, lv.sp.indices0
        else:
            indices = torch.cat([self.batch.unsqueeze(-1).int(), self.grid_coord.int()], dim=1).contiguous()
            sp = None
        # (the reference's sparse_shape = max(grid_coord) + pad only bounds spconv's hash; sparse_conv.py is unbounded, and no host read)
        self["sparse_conv_feat"] = spconv.SparseConvTensor(features=self.feat, indices=indices, spatial_shape=None,
                                                           batch_size=int(self.offset.shape[0]), geometry=sp)


class PointModule(nn.Module):
    """models/modules.py: every subclass takes a ``Point`` in ``PointSequential``."""


class PointSequential(PointModule):
    """models/modules.py:17-83; a ``sparse_conv.SparseModule`` is routed as the reference routes a spconv module.  On the device
    ``nn.Linear`` and ``nn.BatchNorm1d`` over a Point's features run as the package's own nodes (dense.linear, dense.bn_act)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], OrderedDict):
            for key, module in args[0].items():
                self.add_module(key, module)
        else:
            for idx, module in enumerate(args):
                self.add_module(str(idx), module)
        for name, module in kwargs.items():
            if name in self._modules:
                raise ValueError("name exists.")
            self.add_module(name, module)

    def __getitem__(self, idx):
        if not (-len(self) <= idx < len(self)):
            raise IndexError("index {} is out of range".format(idx))
        if idx < 0:
            idx += len(self)
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        if name is None:
            name = str(len(self._modules))
            if name in self._modules:
                raise KeyError("name exists")
        self.add_module(name, module)

    def forward(self, input):
        for k, module in self._modules.items():
            if isinstance(module, PointModule):
                input = module(input)
            elif isinstance(module, spconv.SparseModule):
                if isinstance(input, Point):
                    input.sparse_conv_feat = module(input.sparse_conv_feat)
                    input.feat = input.sparse_conv_feat.features
                else:
                    input = module(input)
            else:
                if isinstance(input, Point):
                    input.feat = _apply(module, input.feat)
                    if "sparse_conv_feat" in input.keys():
                        input.sparse_conv_feat = input.sparse_conv_feat.replace_feature(input.feat)
                elif isinstance(input, spconv.SparseConvTensor):
                    if input.indices.shape[0] != 0:
                        input = input.replace_feature(_apply(module, input.features))
                else:
                    input = module(input)
        return input


def _apply(module, x):
    if x.is_cuda and x.dim() == 2 and not FORCE_TORCH:
        if type(module) is nn.Linear:
            return dense.linear(module, x.contiguous())
        if type(module) is nn.BatchNorm1d:
            return dense.bn_act(module, x.contiguous(), relu=False)
    return module(x)


class PDNorm(PointModule):
    """prompt_driven_normalization.py (plain torch): one norm per condition, optional context modulation."""

    def __init__(self, num_features, norm_layer, context_channels=256, conditions=("ScanNet", "S3DIS", "Structured3D"), decouple=True,
                 adaptive=False):
        super().__init__()
        self.conditions = conditions
        self.decouple = decouple
        self.adaptive = adaptive
        if self.decouple:
            self.norm = nn.ModuleList([norm_layer(num_features) for _ in conditions])
        else:
            self.norm = norm_layer
        if self.adaptive:
            self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(context_channels, 2 * num_features, bias=True))

    def forward(self, point):
        assert {"feat", "condition"}.issubset(point.keys())
        condition = point.condition if isinstance(point.condition, str) else point.condition[0]
        if self.decouple:
            assert condition in self.conditions
            norm = self.norm[self.conditions.index(condition)]
        else:
            norm = self.norm
        point.feat = norm(point.feat)
        if self.adaptive:
            assert "context" in point.keys()
            shift, scale = self.modulation(point.context).chunk(2, dim=1)
            point.feat = point.feat * (1.0 + scale) + shift
        return point


class DropPath(nn.Module):
    """timm's stochastic depth per row (``scale_by_keep``)."""

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# Patch attention
# ---------------------------------------------------------------------------------------------------------------------------------------
class _SerialAttnFn(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, qkv, order, qtab, ktab, heads, scale):
        out, lse = _be().serial_attn_forward(qkv, order, qtab, heads, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (order, qtab, ktab, heads, scale)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        qkv, out, lse = ctx.saved_tensors
        order, qtab, ktab, heads, scale = ctx.cfg
        return _be().serial_attn_backward(qkv, out, lse, g.contiguous(), order, qtab, ktab, heads, scale), None, None, None, None, None


def attention_supported(qkv, heads, patch_size):
    """Does ``serial_attention`` run the HIP node on these rows (fp32 device rows inside ``pdf_serial_attn_supported``)?"""
    return bool(_hip(qkv) and qkv.dtype == torch.float32 and qkv.dim() == 2 and qkv.shape[0] > 0
                and _be().serial_attn_supported(qkv.shape[1] // 3, heads, patch_size))


def attention_torch(qkv, tables, order, inverse, heads, scale, bias=None, upcast_attention=True, upcast_softmax=True, drop=None):
    """The reference's non-flash branch (:184-206, :216) over the padded order; sequences shorter than the patch size (the flash
    layout's short scenes) one by one.  ``bias``: (patches, H, K, K) relative-position term or None."""
    K, C = tables.patch_size, qkv.shape[1] // 3
    H = heads
    rows = qkv[order[tables.pad]]
    inv = tables.unpad[inverse]

    def attend(x, k):   # x (P k, 3 C) -> (P k, C)
        q, kk, v = x.reshape(-1, k, 3, H, C // H).permute(2, 0, 3, 1, 4).unbind(dim=0)
        if upcast_attention:
            q, kk = q.float(), kk.float()
        attn = (q * scale) @ kk.transpose(-2, -1)
        if bias is not None:
            attn = attn + bias
        if upcast_softmax:
            attn = attn.float()
        attn = torch.softmax(attn, dim=-1)
        if drop is not None:
            attn = drop(attn)
        return (attn.to(x.dtype) @ v).transpose(1, 2).reshape(-1, C)

    if all(ln == K for _, ln in tables.seqs):
        feat = attend(rows, K)
    else:
        assert bias is None
        parts, a = [], 0
        seqs = tables.seqs
        while a < len(seqs):   # runs of equal length in one product
            b = a
            while b < len(seqs) and seqs[b][1] == seqs[a][1]:
                b += 1
            parts.append(attend(rows[seqs[a][0]:seqs[b - 1][0] + seqs[b - 1][1]], seqs[a][1]))
            a = b
        feat = torch.cat(parts)
    return feat[inv]


def serial_attention(qkv, level, order_index, heads, patch_size, scale):
    """``softmax(scale q k^T) v`` per head inside every patch of ``level``'s serialized order ``order_index``: (N, 3C) rows of the qkv
    Linear in original order -> (N, C) in original order (the chain ``[order]``, reshape, attention, ``[inverse]`` as one node)."""
    tables = level.patch(patch_size)
    if attention_supported(qkv, heads, patch_size) and tables.qtab is not None:
        q = qkv.contiguous()
        if q.data_ptr() % 16:
            q = q.clone()
        return _SerialAttnFn.apply(q, level.order[order_index].contiguous(), tables.qtab, tables.ktab, int(heads), float(scale))
    return attention_torch(qkv, tables, level.order[order_index], level.inverse[order_index], heads, scale)


class RPE(nn.Module):
    def __init__(self, patch_size, num_heads):
        super().__init__()
        self.patch_size = patch_size
        self.num_heads = num_heads
        self.pos_bnd = int((4 * patch_size) ** (1 / 3) * 2)
        self.rpe_num = 2 * self.pos_bnd + 1
        self.rpe_table = nn.Parameter(torch.zeros(3 * self.rpe_num, num_heads))
        nn.init.trunc_normal_(self.rpe_table, std=0.02)

    def forward(self, coord):
        idx = (coord.clamp(-self.pos_bnd, self.pos_bnd) + self.pos_bnd + torch.arange(3, device=coord.device) * self.rpe_num)
        out = self.rpe_table.index_select(0, idx.reshape(-1))
        out = out.view(idx.shape + (-1,)).sum(3)
        return out.permute(0, 3, 1, 2)   # (N, K, K, H) -> (N, H, K, K)


class SerializedAttention(PointModule):
    def __init__(self, channels, num_heads, patch_size, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0, order_index=0,
                 enable_rpe=False, enable_flash=True, upcast_attention=True, upcast_softmax=True):
        super().__init__()
        assert channels % num_heads == 0
        self.channels = channels
        self.num_heads = num_heads
        self.scale = qk_scale or (channels // num_heads) ** -0.5
        self.order_index = order_index
        self.upcast_attention = upcast_attention
        self.upcast_softmax = upcast_softmax
        self.enable_rpe = enable_rpe
        self.enable_flash = enable_flash
        if enable_flash:
            assert enable_rpe is False, "Set enable_rpe to False when enable Flash Attention"
            assert upcast_attention is False, "Set upcast_attention to False when enable Flash Attention"
            assert upcast_softmax is False, "Set upcast_softmax to False when enable Flash Attention"
            # (flash_attn does not exist for this platform: the flag selects the flash branch's layout, computed in fp32)
            self.patch_size = patch_size
            self.attn_drop = attn_drop
        else:
            # the patch size is set to min(patch_size_max, smallest scene) per forward: no mask
            self.patch_size_max = patch_size
            self.patch_size = 0
            self.attn_drop = nn.Dropout(attn_drop)

        self.qkv = nn.Linear(channels, channels * 3, bias=qkv_bias)
        self.proj = nn.Linear(channels, channels)
        self.proj_drop = nn.Dropout(proj_drop)
        self.softmax = nn.Softmax(dim=-1)
        self.rpe = RPE(patch_size, num_heads) if self.enable_rpe else None

    @torch.no_grad()
    def get_rel_pos(self, point, order):
        K = self.patch_size
        rel_pos_key = f"rel_pos_{self.order_index}"
        if rel_pos_key not in point.keys():
            grid_coord = point.grid_coord[order]
            grid_coord = grid_coord.reshape(-1, K, 3)
            point[rel_pos_key] = grid_coord.unsqueeze(2) - grid_coord.unsqueeze(1)
        return point[rel_pos_key]

    def _level(self, point):
        return point.ptv3_geometry.levels[point.get("ptv3_level", 0)]

    def get_padding_and_inverse(self, point):
        t = self._level(point).patch(self.patch_size)
        return t.pad, t.unpad, t.cu_seqlens

    def _drop_p(self):
        p = self.attn_drop if self.enable_flash else self.attn_drop.p
        return p if self.training else 0.0

    def forward(self, point):
        level = self._level(point)
        if not self.enable_flash:
            self.patch_size = min(level.min_size, self.patch_size_max)
        H, K = self.num_heads, self.patch_size
        qkv = _apply(self.qkv, point.feat)
        if self.rpe is None and self._drop_p() == 0.0 and attention_supported(qkv, H, K):
            feat = serial_attention(qkv, level, self.order_index, H, K, self.scale)
        else:
            tables = level.patch(K)
            order = level.order[self.order_index]
            bias = self.rpe(self.get_rel_pos(point, order[tables.pad])) if self.enable_rpe else None
            drop = None
            if self._drop_p() > 0.0:
                drop = self.attn_drop if not self.enable_flash else partial(nn.functional.dropout, p=self.attn_drop, training=True)
            feat = attention_torch(qkv, tables, order, level.inverse[self.order_index], H, self.scale, bias, self.upcast_attention,
                                   self.upcast_softmax, drop)
        feat = _apply(self.proj, feat)
        feat = self.proj_drop(feat)
        point.feat = feat
        return point


class MLP(nn.Module):
    def __init__(self, in_channels, hidden_channels=None, out_channels=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        out_channels = out_channels or in_channels
        hidden_channels = hidden_channels or in_channels
        self.fc1 = nn.Linear(in_channels, hidden_channels)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_channels, out_channels)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        x = _apply(self.fc1, x)
        x = self.act(x)
        x = self.drop(x)
        x = _apply(self.fc2, x)
        x = self.drop(x)
        return x


class Block(PointModule):
    def __init__(self, channels, num_heads, patch_size=48, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0,
                 drop_path=0.0, norm_layer=nn.LayerNorm, act_layer=nn.GELU, pre_norm=True, order_index=0, cpe_indice_key=None,
                 enable_rpe=False, enable_flash=True, upcast_attention=True, upcast_softmax=True):
        super().__init__()
        self.channels = channels
        self.pre_norm = pre_norm
        self.cpe = PointSequential(
            spconv.SubMConv3d(channels, channels, kernel_size=3, bias=True, indice_key=cpe_indice_key),
            nn.Linear(channels, channels),
            norm_layer(channels),
        )
        self.norm1 = PointSequential(norm_layer(channels))
        self.attn = SerializedAttention(channels=channels, patch_size=patch_size, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                        attn_drop=attn_drop, proj_drop=proj_drop, order_index=order_index, enable_rpe=enable_rpe,
                                        enable_flash=enable_flash, upcast_attention=upcast_attention, upcast_softmax=upcast_softmax)
        self.norm2 = PointSequential(norm_layer(channels))
        self.mlp = PointSequential(MLP(in_channels=channels, hidden_channels=int(channels * mlp_ratio), out_channels=channels,
                                       act_layer=act_layer, drop=proj_drop))
        self.drop_path = PointSequential(DropPath(drop_path) if drop_path > 0.0 else nn.Identity())

    def forward(self, point):
        shortcut = point.feat
        point = self.cpe(point)
        point.feat = shortcut + point.feat
        shortcut = point.feat
        if self.pre_norm:
            point = self.norm1(point)
        point = self.drop_path(self.attn(point))
        point.feat = shortcut + point.feat
        if not self.pre_norm:
            point = self.norm1(point)

        shortcut = point.feat
        if self.pre_norm:
            point = self.norm2(point)
        point = self.drop_path(self.mlp(point))
        point.feat = shortcut + point.feat
        if not self.pre_norm:
            point = self.norm2(point)
        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
        return point


def segment_reduce(x, cluster, idx_ptr, srt, reduce):
    """``torch_scatter.segment_csr(x[indices], idx_ptr, reduce)`` over a partition whose ``sorted`` lists a cluster's rows in ascending row
    index; max on fp32 device rows is csrc/grid_pool.hip's node (the first row wins a tie), the rest the sequential composition."""
    if reduce == "max":
        if _hip(x) and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0:
            return _SegMax.apply(x.contiguous(), cluster, idx_ptr, srt)[0]
        return segment_max_torch(x, idx_ptr, srt)
    if reduce == "min":
        return -segment_max_torch(-x, idx_ptr, srt)
    if reduce == "mean":
        return segment_mean_torch(x, idx_ptr, srt)
    assert reduce == "sum"
    rows, valid = _segment_rows(idx_ptr, srt)
    acc = x.new_zeros(rows.shape[1], x.shape[1])
    for k in range(rows.shape[0]):
        acc = acc + torch.where(valid[k].unsqueeze(1), x[rows[k]], x.new_zeros(()))
    return acc


def segment_coord_mean(coord, idx_ptr, srt):
    if _hip(coord) and coord.dtype == torch.float32 and coord.shape[0] > 0 and coord.shape[1] == 3:
        return _be().grid_pool_mean(coord.contiguous(), idx_ptr, srt)
    return segment_mean_torch(coord, idx_ptr, srt)


class SerializedPooling(PointModule):
    def __init__(self, in_channels, out_channels, stride=2, norm_layer=None, act_layer=None, reduce="max", shuffle_orders=True,
                 traceable=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        assert stride == 2 ** (math.ceil(stride) - 1).bit_length()  # 2, 4, 8
        self.stride = stride
        assert reduce in ["sum", "mean", "min", "max"]
        self.reduce = reduce
        self.shuffle_orders = shuffle_orders
        self.traceable = traceable

        self.proj = nn.Linear(in_channels, out_channels)
        if norm_layer is not None:
            self.norm = PointSequential(norm_layer(out_channels))
        if act_layer is not None:
            self.act = PointSequential(act_layer())

    def forward(self, point):
        assert {"serialized_code", "serialized_order", "serialized_inverse", "serialized_depth"}.issubset(
            point.keys()), "Run point.serialization() point cloud before SerializedPooling"
        geom, l = point.ptv3_geometry, point.get("ptv3_level", 0)
        if len(geom.levels) <= l + 1 or geom.levels[l].pool is None:
            raise RuntimeError("SerializedPooling: the geometry holds no level below this one (build it with the model's make_geometry)")
        cluster, srt, idx_ptr, head, pooling_depth = geom.levels[l].pool
        nxt = geom.levels[l + 1]
        point_dict = Dict(
            feat=segment_reduce(_apply(self.proj, point.feat), cluster, idx_ptr, srt, self.reduce),
            coord=segment_coord_mean(point.coord, idx_ptr, srt),
            grid_coord=nxt.grid_coord,
            serialized_code=nxt.code,
            serialized_order=nxt.order,
            serialized_inverse=nxt.inverse,
            serialized_depth=nxt.depth,
            batch=nxt.batch,
            offset=nxt.offset,
            ptv3_geometry=geom,
            ptv3_level=l + 1,
        )
        if "condition" in point.keys():
            point_dict["condition"] = point.condition
        if "context" in point.keys():
            point_dict["context"] = point.context
        if self.traceable:
            point_dict["pooling_inverse"] = cluster
            point_dict["pooling_parent"] = point
        point = Point(point_dict)
        if getattr(self, "norm", None) is not None:
            point = self.norm(point)
        if getattr(self, "act", None) is not None:
            point = self.act(point)
        point.sparsify()
        return point


class SerializedUnpooling(PointModule):
    def __init__(self, in_channels, skip_channels, out_channels, norm_layer=None, act_layer=None, traceable=False):
        super().__init__()
        self.proj = PointSequential(nn.Linear(in_channels, out_channels))
        self.proj_skip = PointSequential(nn.Linear(skip_channels, out_channels))
        if norm_layer is not None:
            self.proj.add(norm_layer(out_channels))
            self.proj_skip.add(norm_layer(out_channels))
        if act_layer is not None:
            self.proj.add(act_layer())
            self.proj_skip.add(act_layer())
        self.traceable = traceable

    def forward(self, point):
        assert "pooling_parent" in point.keys()
        assert "pooling_inverse" in point.keys()
        parent = point.pop("pooling_parent")
        inverse = point.pop("pooling_inverse")
        point = self.proj(point)
        parent = self.proj_skip(parent)
        parent.feat = parent.feat + point.feat[inverse]
        if self.traceable:
            parent["unpooling_parent"] = point
        return parent


class Embedding(PointModule):
    def __init__(self, in_channels, embed_channels, norm_layer=None, act_layer=None):
        super().__init__()
        self.in_channels = in_channels
        self.embed_channels = embed_channels
        self.stem = PointSequential(conv=spconv.SubMConv3d(in_channels, embed_channels, kernel_size=5, padding=1, bias=False,
                                                           indice_key="stem"))
        if norm_layer is not None:
            self.stem.add(norm_layer(embed_channels), name="norm")
        if act_layer is not None:
            self.stem.add(act_layer(), name="act")

    def forward(self, point):
        return self.stem(point)


@MODELS.register_module("PT-v3m1")
class PointTransformerV3(PointModule):
    def __init__(self, in_channels=6, order=("z", "z_trans"), stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2),
                 enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32), enc_patch_size=(48, 48, 48, 48, 48),
                 dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256), dec_num_head=(4, 4, 8, 16), dec_patch_size=(48, 48, 48, 48),
                 mlp_ratio=4, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0, drop_path=0.3, pre_norm=True,
                 shuffle_orders=True, enable_rpe=False, enable_flash=True, upcast_attention=True, upcast_softmax=True, cls_mode=False,
                 pdnorm_bn=False, pdnorm_ln=False, pdnorm_decouple=True, pdnorm_adaptive=False, pdnorm_affine=True,
                 pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D")):
        super().__init__()
        self.num_stages = len(enc_depths)
        self.order = [order] if isinstance(order, str) else order
        self.cls_mode = cls_mode
        self.shuffle_orders = shuffle_orders
        self.stride = tuple(stride)
        self.enable_flash = enable_flash

        assert self.num_stages == len(stride) + 1
        assert self.num_stages == len(enc_depths)
        assert self.num_stages == len(enc_channels)
        assert self.num_stages == len(enc_num_head)
        assert self.num_stages == len(enc_patch_size)
        assert self.cls_mode or self.num_stages == len(dec_depths) + 1
        assert self.cls_mode or self.num_stages == len(dec_channels) + 1
        assert self.cls_mode or self.num_stages == len(dec_num_head) + 1
        assert self.cls_mode or self.num_stages == len(dec_patch_size) + 1
        self.patch_sizes = [sorted({enc_patch_size[s]} | (set() if cls_mode or s >= len(dec_patch_size) else {dec_patch_size[s]}))
                            for s in range(self.num_stages)]

        if pdnorm_bn:
            bn_layer = partial(PDNorm, norm_layer=partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01, affine=pdnorm_affine),
                               conditions=pdnorm_conditions, decouple=pdnorm_decouple, adaptive=pdnorm_adaptive)
        else:
            bn_layer = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        if pdnorm_ln:
            ln_layer = partial(PDNorm, norm_layer=partial(nn.LayerNorm, elementwise_affine=pdnorm_affine), conditions=pdnorm_conditions,
                               decouple=pdnorm_decouple, adaptive=pdnorm_adaptive)
        else:
            ln_layer = dense.LayerNorm   # (nn.LayerNorm's parameters and keys; one HIP pass per direction on fp32 device rows)
        act_layer = nn.GELU

        self.embedding = Embedding(in_channels=in_channels, embed_channels=enc_channels[0], norm_layer=bn_layer, act_layer=act_layer)

        enc_drop_path = [x.item() for x in torch.linspace(0, drop_path, sum(enc_depths))]
        self.enc = PointSequential()
        for s in range(self.num_stages):
            enc_drop_path_ = enc_drop_path[sum(enc_depths[:s]):sum(enc_depths[:s + 1])]
            enc = PointSequential()
            if s > 0:
                enc.add(SerializedPooling(in_channels=enc_channels[s - 1], out_channels=enc_channels[s], stride=stride[s - 1],
                                          norm_layer=bn_layer, act_layer=act_layer), name="down")
            for i in range(enc_depths[s]):
                enc.add(Block(channels=enc_channels[s], num_heads=enc_num_head[s], patch_size=enc_patch_size[s], mlp_ratio=mlp_ratio,
                              qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop, drop_path=enc_drop_path_[i],
                              norm_layer=ln_layer, act_layer=act_layer, pre_norm=pre_norm, order_index=i % len(self.order),
                              cpe_indice_key=f"stage{s}", enable_rpe=enable_rpe, enable_flash=enable_flash,
                              upcast_attention=upcast_attention, upcast_softmax=upcast_softmax), name=f"block{i}")
            if len(enc) != 0:
                self.enc.add(module=enc, name=f"enc{s}")

        if not self.cls_mode:
            dec_drop_path = [x.item() for x in torch.linspace(0, drop_path, sum(dec_depths))]
            self.dec = PointSequential()
            dec_channels = list(dec_channels) + [enc_channels[-1]]
            for s in reversed(range(self.num_stages - 1)):
                dec_drop_path_ = dec_drop_path[sum(dec_depths[:s]):sum(dec_depths[:s + 1])]
                dec_drop_path_.reverse()
                dec = PointSequential()
                dec.add(SerializedUnpooling(in_channels=dec_channels[s + 1], skip_channels=enc_channels[s], out_channels=dec_channels[s],
                                            norm_layer=bn_layer, act_layer=act_layer), name="up")
                for i in range(dec_depths[s]):
                    dec.add(Block(channels=dec_channels[s], num_heads=dec_num_head[s], patch_size=dec_patch_size[s], mlp_ratio=mlp_ratio,
                                  qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop,
                                  drop_path=dec_drop_path_[i], norm_layer=ln_layer, act_layer=act_layer, pre_norm=pre_norm,
                                  order_index=i % len(self.order), cpe_indice_key=f"stage{s}", enable_rpe=enable_rpe,
                                  enable_flash=enable_flash, upcast_attention=upcast_attention, upcast_softmax=upcast_softmax),
                            name=f"block{i}")
                self.dec.add(module=dec, name=f"dec{s}")

    def make_geometry(self, grid_coord, offset):
        """The batch's ``PTv3Geometry`` (makes the ``shuffle_orders`` draws): hand it in as ``data_dict["ptv3_geometry"]``."""
        return build_geometry(grid_coord, offset, list(self.order), self.stride, self.shuffle_orders, self.patch_sizes, self.enable_flash)

    @dense.fp32_path
    def forward(self, data_dict):
        point = Point(data_dict)
        point._grid_coord()
        if point.get("ptv3_geometry") is None:
            point["ptv3_geometry"] = self.make_geometry(point.grid_coord, point.offset)
        elif point.ptv3_geometry.levels[0].n != point.feat.shape[0]:
            raise ValueError(f"PT-v3m1: ptv3_geometry of {point.ptv3_geometry.levels[0].n} points for a batch of {point.feat.shape[0]}")
        point["ptv3_level"] = 0
        point.serialization(order=self.order, shuffle_orders=self.shuffle_orders)
        point.sparsify()

        point = self.embedding(point)
        point = self.enc(point)
        if not self.cls_mode:
            point = self.dec(point)
        return point

"""PointTransformer-V2 mode 2 (``PT-v2m2``) on HIP passes for grid pooling and grouped vector attention.

Mirrors pointcept/models/point_transformer_v2/point_transformer_v2m2_base.py class by class (cited as ``v2m2:LINE``): same constructor
arguments and defaults, same submodule tree and ``state_dict`` keys (``patch_embed.proj.0``, ``enc_stages.{i}.down.fc``,
``...blocks.blocks.{j}.attn.linear_q.0``, ``weight_encoding.{0,1.norm,3}``, ``dec_stages.{i}.up.proj.0``, ``seg_head.{0,1.norm,3}``),
same forward contract (``data_dict`` with ``coord`` / ``feat`` / ``offset`` -> logits ``(N, num_classes)``), so reference checkpoints load.

What runs where
  * partition pooling / unpooling: csrc/grid_pool.hip (keys, stable sort, run boundaries, segment mean / max, gathers);
  * the attention core: csrc/gva.hip -- two autograd nodes, ``gva_relation`` and ``gva_attend``, each with a hand-written backward;
  * kNN, the masked relative coordinates, 3-NN interpolation: the ``pointops`` kernels;
  * Linear / BatchNorm / ReLU stacks: the ``dense`` helpers where they apply, torch otherwise.  The two position MLPs and
    ``weight_encoding`` stay compositions: their train-mode BatchNorm needs statistics over all n*s rows.
CPU tensors, other dtypes, shapes outside the fused class (``c / groups != 8``, ``s > 64``), an explicit ``start=`` of ``GridPool`` and
attention dropout in train mode take the torch compositions in this file (``*_torch``); they are the kernels' oracle in the tests.

Everything the hierarchy is made of -- clusters, pooled coordinates, kNN tables -- depends on coordinates only: ``make_geometry`` computes
it ahead of the forward (``data_dict["ptv2_geometry"]``); without it the forward computes the same object itself.

Third-party pieces the reference imports and this image lacks (unversioned, hence parity unpinned) are restated from their documented
behaviour: ``torch_geometric.nn.pool.voxel_grid`` (``stratified._voxel_grid``), ``torch_scatter.segment_csr`` (sequential mean, first-wins
max: ``segment_mean_torch`` / ``segment_max_torch``) and timm's ``DropPath`` (``stratified.DropPath``).  The order inside
``torch.sort(cluster)`` (v2m2:263) is undefined upstream; here it is the stable order.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.utils.checkpoint import checkpoint

from . import _native, dense
from .pointops import _ops as _p1_ops
from .registry import MODELS
from .stratified import DropPath, _Linear, _voxel_grid, offset2batch, scene_bounds

_amp_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")

HIP_NODES = True   # module-wide switch of the HIP passes (tests and tools/ptv2_bench.py compare both paths)


def _hip(*tensors):
    """The HIP passes apply: every given tensor is a contiguous float32 tensor on the device."""
    return HIP_NODES and all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)


# ------------------------------------------------------------------------------------------------------------------
# Partition pooling (v2m2:244-269, :308-309)
# ------------------------------------------------------------------------------------------------------------------
class Partition:
    """One pooling stage: ``cluster`` (n) int64 = what ``GridPool`` returns, ``idx_ptr`` (m + 1) int32, ``sorted`` (n) int32 = the stable
    sort order of ``cluster``, pooled ``coord`` (m, 3) and ``offset`` (scenes) int32."""

    __slots__ = ("cluster", "idx_ptr", "sorted", "coord", "offset", "m")

    def __init__(self, cluster, idx_ptr, srt, coord, offset):
        self.cluster, self.idx_ptr, self.sorted, self.coord, self.offset, self.m = cluster, idx_ptr, srt, coord, offset, int(idx_ptr.shape[0]) - 1

    @property
    def counts(self):
        return torch.diff(self.idx_ptr)


def voxel_keys(pos, batch, size):
    """``voxel_grid(pos, size, batch, start=0)`` (v2m2:257-259): the int64 cell id; float division by ``size`` in ``pos``'s dtype."""
    size3 = torch.full((3,), float(size), dtype=pos.dtype, device=pos.device)
    return _voxel_grid(pos, batch, size3, start=pos.new_zeros(3))


def _segment_rows(idx_ptr, srt):
    """(rows (kmax, m): the k-th fine row of every segment (clamped), valid (kmax, m)) -- one host read (the longest segment)."""
    counts = torch.diff(idx_ptr.long())
    kmax = int(counts.max()) if counts.numel() else 0
    k = torch.arange(kmax, device=idx_ptr.device).unsqueeze(1)
    valid = k < counts.unsqueeze(0)
    at = (idx_ptr[:-1].long().unsqueeze(0) + k).clamp_(max=max(int(srt.shape[0]) - 1, 0))
    return srt.long()[at], valid


def segment_mean_torch(x, idx_ptr, srt):
    """``segment_csr(x[sorted], idx_ptr, reduce="mean")`` as a sequential loop: the segment's rows added in ascending sorted position, one
    division by the count."""
    rows, valid = _segment_rows(idx_ptr, srt)
    acc = x.new_zeros(rows.shape[1], x.shape[1])
    for k in range(rows.shape[0]):
        acc = acc + torch.where(valid[k].unsqueeze(1), x[rows[k]], x.new_zeros(()))
    return acc / torch.diff(idx_ptr.long()).to(x.dtype).unsqueeze(1)


def segment_argmax_torch(x, idx_ptr, srt):
    """(m, c) int64: the fine row that holds every segment's maximum; the first row in sorted position wins a tie."""
    rows, valid = _segment_rows(idx_ptr, srt)
    xd = x.detach()
    best = xd[rows[0]].clone()
    arg = rows[0].unsqueeze(1).expand_as(best).clone()
    for k in range(1, rows.shape[0]):
        v = xd[rows[k]]
        better = valid[k].unsqueeze(1) & (v > best)
        best = torch.where(better, v, best)
        arg = torch.where(better, rows[k].unsqueeze(1), arg)
    return arg


def segment_max_torch(x, idx_ptr, srt):
    """``segment_csr(x[sorted], idx_ptr, reduce="max")``; differentiable through the gather of the arg-max rows."""
    return x.gather(0, segment_argmax_torch(x, idx_ptr, srt))


def grid_partition_torch(coord, offset, grid_size, start=None):
    """v2m2:246-268 with the stable sort: the composition (and the oracle of csrc/grid_pool.hip)."""
    n = coord.shape[0]
    batch = offset2batch(offset, n)
    if start is None:
        start = scene_bounds(coord, offset)[0].to(coord.dtype)
    key = voxel_keys(coord - start[batch], batch, grid_size)
    _, cluster, counts = torch.unique(key, sorted=True, return_inverse=True, return_counts=True)
    srt = torch.sort(cluster, stable=True)[1].int()
    idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).int()
    return _finish_partition(coord, offset, cluster, idx_ptr, srt, segment_mean_torch(coord, idx_ptr, srt))


def _finish_partition(coord, offset, cluster, idx_ptr, srt, pooled):
    # batch[idx_ptr[:-1]] + batch2offset (v2m2:267-268): clusters are ordered scene by scene, so a scene ends where the cluster starts do
    new_offset = torch.searchsorted(idx_ptr[:-1].contiguous(), offset.to(idx_ptr.dtype).contiguous()).int()
    return Partition(cluster, idx_ptr, srt, pooled, new_offset)


def grid_partition(coord, offset, grid_size, start=None):
    """The partition of one ``GridPool`` and its pooled coordinates.  An explicit ``start`` takes the composition."""
    if start is None and _hip(coord) and coord.shape[0] > 0:
        be = _native.hip_backend()
        cluster, srt, idx_ptr, _ = be.grid_pool_partition(coord, offset, grid_size)
        return _finish_partition(coord, offset, cluster, idx_ptr, srt, be.grid_pool_mean(coord, idx_ptr, srt))
    return grid_partition_torch(coord, offset, grid_size, start)


class _SegMax(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, feat, cluster, idx_ptr, srt):
        out, arg = _native.hip_backend().grid_pool_max(feat, idx_ptr, srt)
        ctx.save_for_backward(cluster, arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @_amp_bwd
    def backward(ctx, g, _garg):
        cluster, arg = ctx.saved_tensors
        return _native.hip_backend().grid_pool_max_backward(g.contiguous(), cluster, arg), None, None, None


def segment_max(feat, part):
    """Pooled features of a partition: segment max, the first row in point order wins a tie."""
    if _hip(feat) and part.m > 0:
        return _SegMax.apply(feat, part.cluster, part.idx_ptr, part.sorted)[0]
    return segment_max_torch(feat, part.idx_ptr, part.sorted)


class _MapUnpoolTorch(Function):
    """``x[cluster]`` whose backward is the segmented row sum in the association of ``pdf_seg_sum_rows``: a segment's rows in ascending
    sorted position, even and odd positions in two chains that are added at the end (index_add's order is not fixed on the device)."""

    @staticmethod
    def forward(ctx, x, cluster, idx_ptr, srt):
        ctx.save_for_backward(idx_ptr, srt)
        return x[cluster]

    @staticmethod
    def backward(ctx, g):
        idx_ptr, srt = ctx.saved_tensors
        rows, valid = _segment_rows(idx_ptr, srt)
        acc = [g.new_zeros(rows.shape[1], g.shape[1]) for _ in range(2)]
        for k in range(rows.shape[0]):
            acc[k & 1] = acc[k & 1] + torch.where(valid[k].unsqueeze(1), g[rows[k]], g.new_zeros(()))
        return acc[0] + acc[1], None, None, None


class _MapUnpool(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, cluster, idx_ptr, srt):
        ctx.save_for_backward(idx_ptr, srt)
        return _native.hip_backend().grid_unpool_forward(x, cluster)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        idx_ptr, srt = ctx.saved_tensors
        return _native.hip_backend().grid_unpool_backward(g.contiguous(), idx_ptr, srt), None, None, None


def map_unpool_torch(x, part):
    return _MapUnpoolTorch.apply(x, part.cluster, part.idx_ptr, part.sorted)


def map_unpool(x, part):
    """Map unpooling (v2m2:308-309): a row gather by ``cluster``; backward = segmented row sums in a fixed order."""
    if _hip(x) and x.shape[0] > 0:
        return _MapUnpool.apply(x, part.cluster, part.idx_ptr, part.sorted)
    return map_unpool_torch(x, part)


# ------------------------------------------------------------------------------------------------------------------
# Grouped vector attention core (v2m2:109-129)
# ------------------------------------------------------------------------------------------------------------------
def _gather_rows_zero(x, idx):
    """x[idx] with a zero row for idx < 0 (pointops.grouping, grouping.py:36-60)."""
    xp = torch.cat([x, x.new_zeros(1, x.shape[1])], 0)
    return xp[torch.where(idx < 0, x.shape[0], idx.long())]


def gva_relation_torch(query, key, idx, pem=None, peb=None):
    """rel[n,s,:] = (key[idx[n,s]] - query[n]) * pem[n,s] + peb[n,s]  (v2m2:109-118)."""
    rel = _gather_rows_zero(key, idx) - query.unsqueeze(1)
    if pem is not None:
        rel = rel * pem
    if peb is not None:
        rel = rel + peb
    return rel


def gva_attend_torch(logits, value, peb, idx, attn_drop=None):
    """v2m2:119-128: softmax over the neighbours, the mask AFTER it (no renormalisation), grouped weighted sum of value[idx] + peb."""
    n, s, g = logits.shape
    v = _gather_rows_zero(value, idx)
    if peb is not None:
        v = v + peb
    w = torch.softmax(logits, dim=1)
    if attn_drop is not None:
        w = attn_drop(w)
    mask = torch.sign(idx + 1)
    w = torch.einsum("n s g, n s -> n s g", w, mask.to(w.dtype))
    out = torch.einsum("n s g i, n s g -> n g i", v.view(n, s, g, -1), w)
    return out.reshape(n, -1)


class _GvaRelation(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, query, key, idx, pem, peb):
        ctx.save_for_backward(query, key, idx, pem)
        ctx.has = (pem is not None, peb is not None)
        return _native.hip_backend().gva_relation_forward(query, key, idx, pem, peb)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        query, key, idx, pem = ctx.saved_tensors
        has_pem, has_peb = ctx.has
        g = g.contiguous()
        need = ctx.needs_input_grad
        gq, gk, gp = _native.hip_backend().gva_relation_backward(g, query, key, idx, pem if has_pem else None, need[0], need[1],
                                                                 has_pem and need[3])
        return gq, gk, None, gp, (g if has_peb and need[4] else None)


class _GvaAttend(Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, logits, value, peb, idx):
        out, p = _native.hip_backend().gva_attend_forward(logits, value, peb, idx)
        ctx.save_for_backward(p, value, peb, idx)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        p, value, peb, idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        gl, gv, gp = _native.hip_backend().gva_attend_backward(g.contiguous(), p, value, peb, idx, need[1], peb is not None and need[2])
        return gl, gv, gp, None


def gva_relation(query, key, idx, pem=None, peb=None):
    """The relation node; the grouped (n, s, c) key is never materialised on the HIP path."""
    if _hip(query, key, pem, peb) and idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and query.shape[0] > 0:
        return _GvaRelation.apply(query, key, idx, pem, peb)
    return gva_relation_torch(query, key, idx, pem, peb)


def gva_attend(logits, value, peb, idx):
    """The attend node (fused class: c = 8 * groups, s <= 64; anything else takes the composition)."""
    if (_hip(logits, value, peb) and idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and value.shape[0] > 0
            and value.shape[1] % logits.shape[2] == 0
            and _native.hip_backend().gva_supported(value.shape[1], logits.shape[2], idx.shape[1])):
        return _GvaAttend.apply(logits, value, peb, idx)
    return gva_attend_torch(logits, value, peb, idx)


def relative_positions(coord, idx):
    """pos (n, s, 3) = (coord[idx] - coord[n]) * [idx >= 0]: the first three columns of ``pointops.grouping(..., with_xyz=True)``."""
    if _hip(coord):
        return _p1_ops.grouping(idx, coord, coord, with_xyz=True)[:, :, 0:3].contiguous()
    mask = torch.sign(idx + 1).unsqueeze(-1).to(coord.dtype)
    return (_gather_rows_zero(coord, idx) - coord.unsqueeze(1)) * mask


# ------------------------------------------------------------------------------------------------------------------
# Coordinate-only geometry
# ------------------------------------------------------------------------------------------------------------------
class PTv2Geometry:
    """Everything of a batch's hierarchy that depends on coordinates only.  ``coords[l]`` / ``offsets[l]``: level l (0 = the input points);
    ``stages[i]``: the ``Partition`` from level i to level i + 1; ``knn(l, k)`` / ``pos(l, k)``: the kNN table of level l (with its inverse
    table attached for the backward gathers) and the masked relative coordinates; ``interp(i)``: the 3-NN interpolation tables from level
    i + 1 onto level i."""

    def __init__(self, coord, offset, offset_host=None, grid_sizes=(), neighbours=(), interp=False):
        coord, offset = coord.contiguous(), offset.int()
        self.coords, self.offsets, self.stages = [coord], [offset], []
        self.offset_host = offset_host
        self._knn, self._pos, self._interp = {}, {}, {}
        for size in grid_sizes:
            part = grid_partition(self.coords[-1], self.offsets[-1], size)
            self.stages.append(part)
            self.coords.append(part.coord)
            self.offsets.append(part.offset)
        for level, ks in enumerate(neighbours):
            for k in sorted(set(ks)):
                self.knn(level, k)
                self.pos(level, k)
        if interp:
            for i in range(len(self.stages)):
                self.interp(i)

    def knn(self, level, k):
        key = (level, int(k))
        if key not in self._knn:
            c = self.coords[level]
            idx = _p1_ops.knn_query(int(k), c, self.offsets[level])[0]
            if idx.dtype == torch.int32 and idx.is_contiguous():
                _native.inverse_table(idx, c.shape[0])
            self._knn[key] = idx
        return self._knn[key]

    def pos(self, level, k):
        key = (level, int(k))
        if key not in self._pos:
            self._pos[key] = relative_positions(self.coords[level], self.knn(level, k))
        return self._pos[key]

    def tables(self, level, k):
        """(kNN table, relative coordinates) of a level: what a ``BlockSequence`` on that level takes."""
        return self.knn(level, k), self.pos(level, k)

    def interp(self, i):
        if i not in self._interp:
            self._interp[i] = _p1_ops._interp_tables(self.coords[i + 1], self.coords[i], self.offsets[i + 1], self.offsets[i], 3)
            idx = self._interp[i][0]
            if idx.dtype == torch.int32 and idx.is_contiguous():
                _native.inverse_table(idx, self.coords[i + 1].shape[0])
        return self._interp[i]


# ------------------------------------------------------------------------------------------------------------------
# Modules
# ------------------------------------------------------------------------------------------------------------------
class PointBatchNorm(nn.Module):
    """v2m2:26-45.  An (n, s, c) input is BatchNorm over the n*s rows: on the device it runs on the (n*s, c) view, no transposed copies.
    Host tensors keep the reference's formulation (two transposed copies around ``BatchNorm1d`` on (n, c, s)): the statistics are then
    summed in the reference's order, and the composition's fp32 forward is the reference's bit for bit (PT-v2m2)."""

    def __init__(self, embed_channels):
        super().__init__()
        self.norm = nn.BatchNorm1d(embed_channels)

    def forward(self, input, relu=False, residual=None):
        if input.dim() == 3:
            n, s, c = input.shape
            if not input.is_cuda:
                y = self.norm(input.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()
                return F.relu(y) if relu else y
            return self.forward(input.reshape(n * s, c), relu).view(n, s, c)
        if input.dim() != 2:
            raise NotImplementedError
        if relu or residual is not None:
            return dense.bn_act(self.norm, input, residual=residual, relu=relu)
        return self.norm(input)


def _lin_bn_relu(lin, pbn, x):
    """relu(bn(lin(x))) on (rows, k): the fused Linear -> BatchNorm -> ReLU node where it applies, else Linear + the BatchNorm / ReLU pass."""
    if dense.linbn_ok(lin, pbn.norm, x):
        return dense.linear_bn_act(lin, pbn.norm, x, True)
    return pbn(lin(x), relu=True)


def _mlp(seq, x):
    """Linear -> PointBatchNorm -> ReLU -> Linear on the (rows, k) view of x (host tensors: on x as it is, see PointBatchNorm)."""
    if x.dim() == 3 and not x.is_cuda:
        return seq[3](seq[1](seq[0](x), relu=True))
    rows = x.reshape(-1, x.shape[-1])
    return seq[3](_lin_bn_relu(seq[0], seq[1], rows)).view(*x.shape[:-1], -1)


def _linear_norm_relu(cin, cout, bias=True):
    return nn.Sequential(_Linear(cin, cout, bias=bias), PointBatchNorm(cout), nn.ReLU(inplace=True))


def _two_layer(cin, mid, cout):
    return nn.Sequential(_Linear(cin, mid), PointBatchNorm(mid), nn.ReLU(inplace=True), _Linear(mid, cout))


class GroupedVectorAttention(nn.Module):
    """v2m2:48-129.  ``pos``: the masked relative coordinates of ``reference_index`` when the caller has them (they depend on coordinates
    only; every block of a level shares them)."""

    def __init__(self, embed_channels, groups, attn_drop_rate=0.0, qkv_bias=True, pe_multiplier=False, pe_bias=True):
        super().__init__()
        if embed_channels % groups:
            raise ValueError(f"GroupedVectorAttention: {embed_channels} channels do not split into {groups} groups")
        c = self.embed_channels = embed_channels
        self.groups, self.attn_drop_rate, self.qkv_bias = groups, attn_drop_rate, qkv_bias
        self.pe_multiplier, self.pe_bias = pe_multiplier, pe_bias
        self.linear_q, self.linear_k = _linear_norm_relu(c, c, qkv_bias), _linear_norm_relu(c, c, qkv_bias)
        self.linear_v = _Linear(c, c, bias=qkv_bias)
        if pe_multiplier:
            self.linear_p_multiplier = _two_layer(3, c, c)
        if pe_bias:
            self.linear_p_bias = _two_layer(3, c, c)
        self.weight_encoding = _two_layer(c, groups, groups)
        self.softmax = nn.Softmax(dim=1)       # (parameter-free members of the reference's tree; the nodes below do their work)
        self.attn_drop = nn.Dropout(attn_drop_rate)

    def forward(self, feat, coord, reference_index, pos=None):
        query = _lin_bn_relu(self.linear_q[0], self.linear_q[1], feat)
        key = _lin_bn_relu(self.linear_k[0], self.linear_k[1], feat)
        value = self.linear_v(feat)
        if pos is None:
            pos = relative_positions(coord, reference_index)
        pem = _mlp(self.linear_p_multiplier, pos) if self.pe_multiplier else None
        peb = _mlp(self.linear_p_bias, pos) if self.pe_bias else None
        relation_qk = gva_relation(query, key, reference_index, pem, peb)
        weight = _mlp(self.weight_encoding, relation_qk)
        if self.attn_drop_rate > 0.0 and self.training:
            return gva_attend_torch(weight, value, peb, reference_index, self.attn_drop)
        return gva_attend(weight, value, peb, reference_index)


class Block(nn.Module):
    """v2m2:132-177"""

    def __init__(self, embed_channels, groups, qkv_bias=True, pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.0,
                 enable_checkpoint=False):
        super().__init__()
        c = embed_channels
        self.attn = GroupedVectorAttention(c, groups, attn_drop_rate=attn_drop_rate, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier,
                                           pe_bias=pe_bias)
        self.fc1, self.fc3 = _Linear(c, c, bias=False), _Linear(c, c, bias=False)
        self.norm1, self.norm2, self.norm3 = PointBatchNorm(c), PointBatchNorm(c), PointBatchNorm(c)
        self.act = nn.ReLU(inplace=True)
        self.enable_checkpoint = enable_checkpoint
        self.drop_path = DropPath(drop_path_rate) if drop_path_rate > 0.0 else nn.Identity()

    def forward(self, points, reference_index, pos=None):
        coord, feat, offset = points
        identity = feat
        feat = _lin_bn_relu(self.fc1, self.norm1, feat)
        if pos is None:
            pos = relative_positions(coord, reference_index)
        if not self.enable_checkpoint:
            feat = self.attn(feat, coord, reference_index, pos)
        else:
            feat = checkpoint(self.attn, feat, coord, reference_index, pos, use_reentrant=False)
        feat = self.norm2(feat, relu=True)
        feat = self.fc3(feat)
        if isinstance(self.drop_path, nn.Identity) or not self.training:
            feat = self.norm3(feat, relu=True, residual=identity)     # act(identity + norm3(fc3(feat)))
        else:
            feat = self.act(identity + self.drop_path(self.norm3(feat)))
        return [coord, feat, offset]


class BlockSequence(nn.Module):
    """v2m2:180-226.  ``tables``: (kNN table, relative coordinates) of the points for ``neighbours`` (``PTv2Geometry.tables``); without them
    the sequence queries the table itself, as the reference does."""

    def __init__(self, depth, embed_channels, groups, neighbours=16, qkv_bias=True, pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0,
                 drop_path_rate=0.0, enable_checkpoint=False):
        super().__init__()
        if isinstance(drop_path_rate, list):   # one rate per block; a float: the same for all; anything else (0, None): none
            if len(drop_path_rate) != depth:
                raise ValueError(f"BlockSequence: {len(drop_path_rate)} drop path rates for {depth} blocks")
            rates = drop_path_rate
        else:
            rates = [drop_path_rate if isinstance(drop_path_rate, float) else 0.0] * depth
        self.neighbours = neighbours
        self.blocks = nn.ModuleList(Block(embed_channels, groups, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier, pe_bias=pe_bias,
                                          attn_drop_rate=attn_drop_rate, drop_path_rate=rate, enable_checkpoint=enable_checkpoint)
                                    for rate in rates)

    def forward(self, points, tables=None):
        coord, _, offset = points
        if tables is None:
            reference_index, _ = _p1_ops.knn_query(self.neighbours, coord.contiguous(), offset)
            tables = reference_index, relative_positions(coord.contiguous(), reference_index)
        for block in self.blocks:
            points = block(points, *tables)
        return points


class GridPool(nn.Module):
    """Partition-based pooling, v2m2:229-269: ``forward`` returns ``([coord, feat, offset], cluster)``.  ``partition``: the stage's
    ``Partition`` when the caller has it (``PTv2Geometry.stages``); an explicit ``start`` takes the composition."""

    def __init__(self, in_channels, out_channels, grid_size, bias=False):
        super().__init__()
        self.in_channels, self.out_channels, self.grid_size = in_channels, out_channels, grid_size
        self.fc = _Linear(in_channels, out_channels, bias=bias)
        self.norm = PointBatchNorm(out_channels)
        self.act = nn.ReLU(inplace=True)

    def forward(self, points, start=None, partition=None):
        coord, feat, offset = points
        feat = _lin_bn_relu(self.fc, self.norm, feat)
        if partition is None or start is not None:
            partition = grid_partition(coord.contiguous(), offset, self.grid_size, start)
        return [partition.coord, segment_max(feat, partition), partition.offset], partition.cluster


class UnpoolWithSkip(nn.Module):
    """Map / interpolation unpooling with skip connection, v2m2:272-316.  ``cluster``: what ``GridPool`` returned, or the stage's
    ``Partition`` (the map backward then runs as segmented sums in a fixed order); ``interp``: the 3-NN tables (idx, weight) when the
    caller has them."""

    def __init__(self, in_channels, skip_channels, out_channels, bias=True, skip=True, backend="map"):
        super().__init__()
        if backend not in ("map", "interp"):
            raise ValueError(f"UnpoolWithSkip: backend {backend!r} (map / interp)")
        self.in_channels, self.skip_channels, self.out_channels = in_channels, skip_channels, out_channels
        self.skip, self.backend = skip, backend
        self.proj = _linear_norm_relu(in_channels, out_channels, bias)
        self.proj_skip = _linear_norm_relu(skip_channels, out_channels, bias)

    def forward(self, points, skip_points, cluster=None, interp=None):
        coord, feat, offset = points
        skip_coord, skip_feat, skip_offset = skip_points
        feat = _lin_bn_relu(self.proj[0], self.proj[1], feat)
        if self.backend == "map" and cluster is not None:
            feat = map_unpool(feat, cluster) if isinstance(cluster, Partition) else feat[cluster]
        elif interp is not None and feat.dtype == torch.float32:
            feat = _p1_ops._InterpolateIdx.apply(feat.contiguous(), *interp)
        else:
            feat = _p1_ops.interpolation(coord.contiguous(), skip_coord.contiguous(), feat.contiguous(), offset, skip_offset)
        if self.skip:
            feat = feat + _lin_bn_relu(self.proj_skip[0], self.proj_skip[1], skip_feat)
        return [skip_coord, feat, skip_offset]


class Encoder(nn.Module):
    """v2m2:319-358"""

    def __init__(self, depth, in_channels, embed_channels, groups, grid_size=None, neighbours=16, qkv_bias=True, pe_multiplier=False,
                 pe_bias=True, attn_drop_rate=None, drop_path_rate=None, enable_checkpoint=False):
        super().__init__()
        self.down = GridPool(in_channels, embed_channels, grid_size)
        self.blocks = BlockSequence(depth, embed_channels, groups, neighbours=neighbours, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier,
                                    pe_bias=pe_bias, attn_drop_rate=attn_drop_rate or 0.0,
                                    drop_path_rate=0.0 if drop_path_rate is None else drop_path_rate, enable_checkpoint=enable_checkpoint)

    def forward(self, points, partition=None, tables=None):
        points, cluster = self.down(points, partition=partition)
        return self.blocks(points, tables), cluster


class Decoder(nn.Module):
    """v2m2:361-402"""

    def __init__(self, in_channels, skip_channels, embed_channels, groups, depth, neighbours=16, qkv_bias=True, pe_multiplier=False,
                 pe_bias=True, attn_drop_rate=None, drop_path_rate=None, enable_checkpoint=False, unpool_backend="map"):
        super().__init__()
        self.up = UnpoolWithSkip(in_channels, skip_channels, embed_channels, backend=unpool_backend)
        self.blocks = BlockSequence(depth, embed_channels, groups, neighbours=neighbours, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier,
                                    pe_bias=pe_bias, attn_drop_rate=attn_drop_rate or 0.0,
                                    drop_path_rate=0.0 if drop_path_rate is None else drop_path_rate, enable_checkpoint=enable_checkpoint)

    def forward(self, points, skip_points, cluster, tables=None, interp=None):
        return self.blocks(self.up(points, skip_points, cluster, interp), tables)


class GVAPatchEmbed(nn.Module):
    """v2m2:405-444"""

    def __init__(self, depth, in_channels, embed_channels, groups, neighbours=16, qkv_bias=True, pe_multiplier=False, pe_bias=True,
                 attn_drop_rate=0.0, drop_path_rate=0.0, enable_checkpoint=False):
        super().__init__()
        self.in_channels, self.embed_channels = in_channels, embed_channels
        self.proj = _linear_norm_relu(in_channels, embed_channels, bias=False)
        self.blocks = BlockSequence(depth, embed_channels, groups, neighbours=neighbours, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier,
                                    pe_bias=pe_bias, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
                                    enable_checkpoint=enable_checkpoint)

    def forward(self, points, tables=None):
        coord, feat, offset = points
        return self.blocks([coord, _lin_bn_relu(self.proj[0], self.proj[1], feat), offset], tables)


@MODELS.register_module("PT-v2m2")
class PointTransformerV2(nn.Module):
    """v2m2:447-576"""

    def __init__(self, in_channels, num_classes, patch_embed_depth=1, patch_embed_channels=48, patch_embed_groups=6, patch_embed_neighbours=8,
                 enc_depths=(2, 2, 6, 2), enc_channels=(96, 192, 384, 512), enc_groups=(12, 24, 48, 64), enc_neighbours=(16, 16, 16, 16),
                 dec_depths=(1, 1, 1, 1), dec_channels=(48, 96, 192, 384), dec_groups=(6, 12, 24, 48), dec_neighbours=(16, 16, 16, 16),
                 grid_sizes=(0.06, 0.12, 0.24, 0.48), attn_qkv_bias=True, pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0,
                 drop_path_rate=0, enable_checkpoint=False, unpool_backend="map"):
        super().__init__()
        stages = self.num_stages = len(enc_depths)
        per_stage = dict(dec_depths=dec_depths, enc_channels=enc_channels, dec_channels=dec_channels, enc_groups=enc_groups,
                         dec_groups=dec_groups, enc_neighbours=enc_neighbours, dec_neighbours=dec_neighbours, grid_sizes=grid_sizes)
        for name, seq in per_stage.items():
            if len(seq) != stages:
                raise ValueError(f"PT-v2m2: {name} has {len(seq)} entries for {stages} stages")
        self.in_channels, self.num_classes = in_channels, num_classes
        attn = dict(qkv_bias=attn_qkv_bias, pe_multiplier=pe_multiplier, pe_bias=pe_bias, attn_drop_rate=attn_drop_rate,
                    enable_checkpoint=enable_checkpoint)
        self.patch_embed = GVAPatchEmbed(patch_embed_depth, in_channels, patch_embed_channels, patch_embed_groups,
                                         neighbours=patch_embed_neighbours, **attn)
        # stochastic depth: one linear ramp over the encoder blocks, one over the decoder blocks
        ramp = lambda depths: [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        enc_rates, dec_rates = ramp(enc_depths), ramp(dec_depths)
        enc_c = [patch_embed_channels] + list(enc_channels)      # width of level i
        dec_c = list(dec_channels) + [enc_c[-1]]                 # width of the decoder's output on level i
        self.enc_stages, self.dec_stages = nn.ModuleList(), nn.ModuleList()
        for i in range(stages):
            e0, d0 = sum(enc_depths[:i]), sum(dec_depths[:i])
            self.enc_stages.append(Encoder(enc_depths[i], enc_c[i], enc_c[i + 1], enc_groups[i], grid_size=grid_sizes[i],
                                           neighbours=enc_neighbours[i], drop_path_rate=enc_rates[e0:e0 + enc_depths[i]], **attn))
            self.dec_stages.append(Decoder(dec_c[i + 1], enc_c[i], dec_c[i], dec_groups[i], dec_depths[i], neighbours=dec_neighbours[i],
                                           drop_path_rate=dec_rates[d0:d0 + dec_depths[i]], unpool_backend=unpool_backend, **attn))
        self.seg_head = _two_layer(dec_c[0], dec_c[0], num_classes) if num_classes > 0 else nn.Identity()
        # the tables every level is asked for: the patch embedding and decoder 0 run on level 0, encoder i on level i + 1, decoder i on level i
        neighbours = [set() for _ in range(stages + 1)]
        neighbours[0].add(patch_embed_neighbours)
        for i in range(stages):
            neighbours[i + 1].add(enc_neighbours[i])
            neighbours[i].add(dec_neighbours[i])
        self.geometry_cfg = dict(grid_sizes=tuple(grid_sizes), neighbours=[sorted(s) for s in neighbours], interp=unpool_backend == "interp")

    def make_geometry(self, coord, offset, offset_host=None):
        """The batch's ``PTv2Geometry``: pass it as ``data_dict["ptv2_geometry"]``, or let the forward compute the same object."""
        return PTv2Geometry(coord, offset, offset_host, **self.geometry_cfg)

    @dense.fp32_path
    def forward(self, data_dict):
        coord = data_dict["coord"].contiguous()
        feat = data_dict["feat"]
        offset = data_dict["offset"].int()
        geom = data_dict.get("ptv2_geometry")
        if geom is None:
            geom = self.make_geometry(coord, offset, data_dict.get("offset_host"))
        elif geom.coords[0].shape[0] != coord.shape[0]:
            raise ValueError(f"PT-v2m2: ptv2_geometry of {geom.coords[0].shape[0]} points for a batch of {coord.shape[0]}")
        use_interp = self.geometry_cfg["interp"]
        points = self.patch_embed([coord, feat, offset], geom.tables(0, self.patch_embed.blocks.neighbours))
        skips = [points]
        for i, enc in enumerate(self.enc_stages):
            points, _ = enc(points, geom.stages[i], geom.tables(i + 1, enc.blocks.neighbours))
            skips.append(points)
        points = skips.pop()
        for i in reversed(range(self.num_stages)):
            dec = self.dec_stages[i]
            points = dec(points, skips.pop(), geom.stages[i], geom.tables(i, dec.blocks.neighbours), geom.interp(i) if use_interp else None)
        feat = points[1]
        if isinstance(self.seg_head, nn.Identity):
            return feat
        return self.seg_head[3](_lin_bn_relu(self.seg_head[0], self.seg_head[1], feat))

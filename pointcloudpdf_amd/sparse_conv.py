"""Sparse 3-D convolutions with spconv 2.x's module interface -- ``SparseConvTensor``, ``SubMConv3d``, ``SparseConv3d``,
``SparseInverseConv3d``, ``SparseSequential`` -- over csrc/sparse_conv.hip.  spconv itself does not exist for this platform, so its
arithmetic is NOT pinned; the definitions below are this package's contract (checked against dense ``conv3d`` / ``conv_transpose3d`` in
float64 by tests/spunet_cases.py).

Sites: ``indices (N, 4)`` int32 ``[batch, d0, d1, d2]`` with ``features (N, C)``.  Weights ``(C_out, k, k, k, C_in)``; the offset
``o in [0, k)^3`` has the flat index ``(o0 k + o1) k + o2``.

* ``SubMConv3d(k odd)``: output sites = input sites in input order; ``out[i] = bias + sum_o W[o] x[site at coord_i + o - k // 2]`` of the
  same batch, absent sites contribute nothing.  ``padding`` is accepted and ignored (the kernel is always centred); ``k = 1`` is a Linear
  layer over the features.
* ``SparseConv3d(k=2, stride=2, padding=0)``: output sites = the distinct ``(batch, coord // 2)`` in ascending ``(batch, d0, d1, d2)``
  order; ``out[p] = sum_o W[o] x[site at 2 p + o]``.  A ``spatial_shape`` on the input drops output sites outside ``shape // 2`` (their
  inputs then have no parent); the default is unbounded.
* ``SparseInverseConv3d(k=2, indice_key)``: output sites = the input sites of the ``SparseConv3d`` with that key, in their order;
  ``out[i] = W[o_i] x[parent(i)]``, ``o_i = coord_i - 2 coord_parent`` (a row without a parent gets the bias alone).
* Duplicated sites (Mix3D): every row gets an output, and a lookup of a duplicated coordinate finds the LOWEST row.  The mirror identity
  of the neighbour table that the HIP input gradient relies on does not hold among duplicates, so the operators that touch a level with
  duplicated sites take the composition.
* Limits: coordinates in [0, 65536), batch index in [0, 32768), < 2^31 - 2 sites (key = batch << 48 | d0 << 32 | d1 << 16 | d2).  A
  violation raises ``RuntimeError``; it never yields a wrong table.

The geometry (``SpGeometry``) is coordinate-only: neighbour tables per (level, kernel size), and per stride-2 step parent / code /
children / code buckets.  It is shared by level and kernel size, not by ``indice_key`` string; the key only tells an inverse convolution
which step to undo.  On the device all requested levels are built in one submission with ONE host read (counts + status).

fp32 device tensors in ``pdf_spconv_supported(k, C_in, C_out)`` -- widths that are multiples of 32 up to 384 with k <= 3, and the stem's
C_in <= 16 -> 32 | 64 with k <= 5 -- run one autograd node per convolution with a hand-written backward: the gather-convolution (SubM
forward, SubM input gradient through the mirrored table, strided forward over the children table, inverse input gradient), the
selected-weight product over the code buckets (inverse forward, strided input gradient) and the slab-reduced weight gradient.  Other
shapes, host tensors and other dtypes take the torch composition (per-offset gather, product, ``index_add``).  Under ``torch.autocast``
the passes run in fp32: 16-bit operands are not provided."""
import math

import torch
import torch.nn as nn

from . import dense
from .dense import _amp_bwd, _amp_fwd

FORCE_TORCH = False   # module-wide switch: every operator and the geometry take the composition (tools/spconv_bench.py's other side)

MAX_COORD, MAX_BATCH = 1 << 16, 1 << 15
_STATUS = {1: "a negative coordinate or batch index", 2: f"a coordinate >= {MAX_COORD} or a batch index >= {MAX_BATCH}"}


def _be():
    from . import _native

    return _native.hip_backend()


def _on_device(t):
    return t.is_cuda and not FORCE_TORCH


def _pack(b, d0, d1, d2):
    return (b.long() << 48) | (d0.long() << 32) | (d1.long() << 16) | d2.long()


def offsets_of(ks):
    """(k^3, 3) offsets in flat-index order."""
    r = torch.arange(ks)
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Step:
    """One stride-2 step between level l (fine) and l + 1 (coarse)."""

    def __init__(self, parent, code, children, truncated, bucket=None):
        self.parent, self.code, self.children, self.truncated = parent, code, children, truncated
        self.bucket = bucket   # (perm, tile_code, rows) on the device path
        self._pairs = None


class SpGeometry:
    """Tables of a site set and its stride-2 pyramid.  ``levels[l]``: dict(indices, n, nbr={ksize: table}, order, skey)."""

    def __init__(self, indices, spatial_shape=None):
        if indices.dim() != 2 or indices.shape[1] != 4:
            raise ValueError(f"indices must be (N, 4) [batch, d0, d1, d2], got {tuple(indices.shape)}")
        self.indices0 = indices.int().contiguous()
        self.shapes = [None if spatial_shape is None else [int(v) for v in spatial_shape]]
        self.levels, self.steps, self.key_level, self._pairs = [], [], {}, {}
        self.has_duplicates = False
        self.hip = _on_device(indices)

    # -- construction -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def build(cls, indices, levels=1, subm_sizes=None, spatial_shape=None):
        """Everything at once: ``levels`` levels, level l with the neighbour tables of the kernel sizes ``subm_sizes[l]``."""
        g = cls(indices, spatial_shape)
        subm_sizes = [tuple(s) for s in (subm_sizes or [()] * levels)]
        for l in range(1, levels):
            g.shapes.append(None if g.shapes[-1] is None else [v // 2 for v in g.shapes[-1]])
        if g.indices0.shape[0] == 0:
            raise RuntimeError("sparse convolution geometry: no sites")
        if g.hip:
            status, lv, steps = _be().spconv_geometry(g.indices0, levels, subm_sizes, [g.shapes[l + 1] for l in range(levels - 1)])
            g._raise(status)
            g.has_duplicates = bool(status & 4)
            g.levels = lv
            g.steps = [_Step(s["parent"], s["code"], s["children"], s["truncated"], (s["bucket_perm"], s["tile_code"], s["bucket_rows"]))
                       for s in steps]
        else:
            g._level0_torch()
            for l in range(levels):
                for ks in subm_sizes[l]:
                    g.subm(l, ks)
                if l < levels - 1:
                    g._down_torch(l)
        return g

    def _raise(self, status):
        for bit, what in _STATUS.items():
            if status & bit:
                raise RuntimeError(f"sparse convolution geometry: {what} (coordinates must lie in [0, {MAX_COORD}), batch in [0, {MAX_BATCH}))")

    def _level0_torch(self):
        idx = self.indices0
        status = (1 if bool((idx < 0).any()) else 0) | (2 if bool((idx[:, 1:] >= MAX_COORD).any() or (idx[:, 0] >= MAX_BATCH).any()) else 0)
        self._raise(status)
        key = _pack(*idx.unbind(1))
        skey, order = torch.sort(key, stable=True)
        self.has_duplicates = bool((skey[1:] == skey[:-1]).any())
        self.levels = [dict(indices=idx, n=idx.shape[0], nbr={}, order=order.int(), skey=skey)]

    def _ensure(self, level):
        if not self.levels:
            if self.hip:
                built = SpGeometry.build(self.indices0, 1, [()], self.shapes[0])
                self.levels, self.has_duplicates = built.levels, built.has_duplicates
            else:
                self._level0_torch()
        while len(self.levels) <= level:
            self.down(len(self.levels) - 1)

    def subm(self, level, ks):
        """(N_l, ks^3) int32 neighbour table of level ``level``."""
        self._ensure(level)
        lv = self.levels[level]
        if ks not in lv["nbr"]:
            if ks % 2 != 1:
                raise ValueError(f"SubMConv3d: kernel_size {ks} must be odd")
            if self.hip:
                import ctypes

                n = lv["n"]
                tbl = torch.empty((n, ks ** 3), dtype=torch.int32, device=lv["indices"].device)
                cnt = torch.tensor([n], dtype=torch.int32, device=tbl.device)
                if n:
                    _be()._call("spconv_subm_table", n, cnt, lv["indices"].contiguous(), lv["skey"],
                                lv["order"] if lv["order"] is not None else ctypes.c_void_p(None), int(ks), tbl)
                lv["nbr"][ks] = tbl
            else:
                idx = lv["indices"].long()
                off = offsets_of(ks).to(idx.device) - ks // 2
                c = idx[:, None, 1:] + off[None]                                                # (n, K, 3)
                ok = ((c >= 0) & (c < MAX_COORD)).all(-1)
                key = _pack(idx[:, None, 0].expand(-1, off.shape[0]), *c.clamp(0, MAX_COORD - 1).unbind(-1))
                pos = torch.searchsorted(lv["skey"], key.reshape(-1)).view(key.shape)
                posc = pos.clamp(max=max(lv["n"] - 1, 0))
                found = ok & (pos < lv["n"]) & (lv["skey"][posc] == key)
                rows = posc if lv["order"] is None else lv["order"].long()[posc]
                lv["nbr"][ks] = torch.where(found, rows, torch.full_like(rows, -1)).int()
        return lv["nbr"][ks]

    def _down_torch(self, level):
        lv = self.levels[level]
        idx = lv["indices"].long()
        n = idx.shape[0]
        lim = self.shapes[level + 1] if len(self.shapes) > level + 1 else None
        pc = idx[:, 1:] >> 1
        valid = torch.ones(n, dtype=torch.bool, device=idx.device)
        if lim is not None:
            valid = (pc < torch.tensor(lim, device=idx.device)).all(1)
        pk = _pack(idx[:, 0], *pc.unbind(1))
        ckey = torch.unique(pk[valid])                                                          # ascending = (batch, d0, d1, d2) order
        m = ckey.shape[0]
        parent = torch.where(valid, torch.searchsorted(ckey, pk), torch.full_like(pk, -1))
        code = torch.where(valid, ((idx[:, 1] & 1) << 2) | ((idx[:, 2] & 1) << 1) | (idx[:, 3] & 1), torch.zeros_like(pk))
        big = torch.full((m * 8,), n, dtype=torch.long, device=idx.device)
        rows = torch.arange(n, device=idx.device)
        big.scatter_reduce_(0, (parent * 8 + code)[valid], rows[valid], "amin")
        children = torch.where(big == n, torch.full_like(big, -1), big).view(m, 8)
        cidx = torch.stack([ckey >> 48, (ckey >> 32) & 0xffff, (ckey >> 16) & 0xffff, ckey & 0xffff], 1).int()
        self.steps.append(_Step(parent.int(), code.int(), children.int(), lim is not None))
        self.levels.append(dict(indices=cidx, n=m, nbr={}, order=None, skey=ckey))

    def down(self, level):
        """The step level -> level + 1 (built on demand: one more host read; ``build`` makes all levels with one)."""
        self._ensure(level)
        if len(self.steps) <= level:
            assert len(self.steps) == level
            while len(self.shapes) <= level + 1:
                self.shapes.append(None if self.shapes[-1] is None else [v // 2 for v in self.shapes[-1]])
            if self.hip:
                lv = self.levels[level]
                sub = SpGeometry.build(lv["indices"].contiguous(), 2, [(), ()], self.shapes[level])
                self.steps.append(sub.steps[0])
                self.levels.append(sub.levels[1])
            else:
                self._down_torch(level)
        return self.steps[level]

    # -- pair lists of the composition (prebuilt once per table) -----------------------------------------------------------------------------
    def pairs(self, tag, tbl):
        """[(k, out_rows, in_rows)] of a (rows, K) table, the offsets without any pair left out."""
        if tag not in self._pairs:
            out = []
            for k in range(tbl.shape[1]):
                rows = torch.nonzero(tbl[:, k] >= 0).squeeze(1)
                if rows.numel():
                    out.append((k, rows, tbl[rows, k].long()))
            self._pairs[tag] = out
        return self._pairs[tag]

    def code_pairs(self, level):
        st = self.steps[level]
        if st._pairs is None:
            st._pairs = []
            for o in range(8):
                rows = torch.nonzero((st.code == o) & (st.parent >= 0)).squeeze(1)
                if rows.numel():
                    st._pairs.append((o, rows, st.parent[rows].long()))
        return st._pairs

    def dup_at(self, level):
        return self.has_duplicates and level == 0


class SparseConvTensor:
    """spconv's container: ``features (N, C)``, ``indices (N, 4)`` int32, ``spatial_shape``, ``batch_size``.  ``geometry`` / ``level`` are
    this package's additions (the tables travel with the tensor)."""

    def __init__(self, features, indices, spatial_shape=None, batch_size=None, geometry=None, level=0):
        self.features = features
        self.indices = indices
        self.spatial_shape = None if spatial_shape is None else list(spatial_shape)
        self.batch_size = batch_size
        self.geometry = geometry if geometry is not None else SpGeometry(indices, spatial_shape)
        self.level = level
        if features.shape[0] != indices.shape[0]:
            raise ValueError(f"SparseConvTensor: {features.shape[0]} feature rows for {indices.shape[0]} sites")

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.geometry, self.level)

    def at_level(self, features, level):
        g = self.geometry
        g._ensure(level)
        return SparseConvTensor(features, g.levels[level]["indices"], g.shapes[level] if len(g.shapes) > level else None,
                                self.batch_size, g, level)



# ---------------------------------------------------------------------------------------------------------------------------------------
# Compositions (spconv's "native" algorithm: per-offset gather, product, index_add)
# ---------------------------------------------------------------------------------------------------------------------------------------
def table_conv_torch(x, weight, bias, pairs, out_rows):
    """out[r] = bias + sum_k W[:, k, :] x[tbl[r, k]] from the table's pair lists; weight (C_out, K, C_in)."""
    out = x.new_zeros((out_rows, weight.shape[0]))
    for k, rows, src in pairs:
        out = out.index_add(0, rows, x.index_select(0, src) @ weight[:, k, :].t())
    return out if bias is None else out + bias


def code_conv_torch(x, weight, bias, code_pairs, out_rows):
    """out[i] = bias + W[:, code_i, :] x[parent_i] (rows without a parent: the bias alone)."""
    out = x.new_zeros((out_rows, weight.shape[0]))
    for o, rows, src in code_pairs:
        out = out.index_add(0, rows, x.index_select(0, src) @ weight[:, o, :].t())
    return out if bias is None else out + bias


# ---------------------------------------------------------------------------------------------------------------------------------------
# Fused nodes (csrc/sparse_conv.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------
class _SubMFn(torch.autograd.Function):
    @staticmethod
    @_amp_fwd
    def forward(ctx, x, weight, bias, tbl, perm, small):
        be = _be()
        w3 = weight.detach().reshape(weight.shape[0], -1, weight.shape[-1])
        b = None if bias is None else bias.detach()
        out = be.spconv_small_forward(x, tbl, w3, b) if small else be.spconv_gather(x, tbl, w3, b, x.shape[0], False, perm=perm)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (tbl, perm, small, bias is not None)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        tbl, perm, small, has_bias = ctx.cfg
        be = _be()
        g = g.contiguous()
        w3 = weight.detach().reshape(weight.shape[0], -1, weight.shape[-1])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            # nbr[i, k] = j  <=>  nbr[j, K - 1 - k] = i: the same table, mirrored, with W transposed -- no inverse table, no atomics
            gx = be.spconv_small_dgrad(g, tbl, w3) if small else be.spconv_gather(g, tbl, w3, None, x.shape[0], True, mirror=True, perm=perm)
        if ctx.needs_input_grad[1]:
            gw = be.spconv_wgrad(x, g, tbl, w3.shape, False).view_as(weight)
        if has_bias and ctx.needs_input_grad[2]:
            gb = be.spconv_colsum(g)
        return gx, gw, gb, None, None, None


class _DownFn(torch.autograd.Function):
    """Strided forward over the children table; its input gradient is the selected-weight product over the code buckets."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, weight, bias, step, n_coarse):
        w3 = weight.detach().reshape(weight.shape[0], 8, weight.shape[-1])
        out = _be().spconv_gather(x, step.children, w3, None if bias is None else bias.detach(), n_coarse, False)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (step, bias is not None)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        step, has_bias = ctx.cfg
        be = _be()
        g = g.contiguous()
        w3 = weight.detach().reshape(weight.shape[0], 8, weight.shape[-1])
        gx = gw = gb = None
        perm, tile_code, rows = step.bucket
        if ctx.needs_input_grad[0]:
            gx = be.spconv_gather(g, step.parent, w3, None, x.shape[0], True, perm=perm, tile_k=tile_code, rows=rows, zero=step.truncated)
        if ctx.needs_input_grad[1]:
            gw = be.spconv_wgrad(x, g, step.children, w3.shape, False).view_as(weight)
        if has_bias and ctx.needs_input_grad[2]:
            gb = be.spconv_colsum(g)
        return gx, gw, gb, None, None


class _InverseFn(torch.autograd.Function):
    """Selected-weight product forward; the input gradient gathers over the children table."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, weight, bias, step, n_fine):
        w3 = weight.detach().reshape(weight.shape[0], 8, weight.shape[-1])
        perm, tile_code, rows = step.bucket
        out = _be().spconv_gather(x, step.parent, w3, None if bias is None else bias.detach(), n_fine, False, perm=perm, tile_k=tile_code,
                                  rows=rows, zero=step.truncated)
        if step.truncated and bias is not None:
            out = torch.where((step.parent >= 0).unsqueeze(1), out, bias.detach().expand_as(out))
        ctx.save_for_backward(x, weight)
        ctx.cfg = (step, bias is not None)
        return out

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        step, has_bias = ctx.cfg
        be = _be()
        g = g.contiguous()
        w3 = weight.detach().reshape(weight.shape[0], 8, weight.shape[-1])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = be.spconv_gather(g, step.children, w3, None, x.shape[0], True)
        if ctx.needs_input_grad[1]:
            gw = be.spconv_wgrad(g, x, step.children, w3.shape, True).view_as(weight)
        if has_bias and ctx.needs_input_grad[2]:
            gb = be.spconv_colsum(g)
        return gx, gw, gb, None, None


def _hip_class(x, weight, ks, geometry, level):
    """0: the composition; 1 / 2: the HIP class (include/pdfops.h: pdf_spconv_supported)."""
    if FORCE_TORCH or not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and geometry.hip) or x.shape[0] == 0:
        return 0
    if geometry.dup_at(level):
        return 0
    return _be().spconv_supported(ks, weight.shape[-1], weight.shape[0])


@dense.fp32_path
def subm_conv(x, weight, bias, geometry, level):
    """SubMConv3d on features x (N_l, C_in) of ``geometry``'s level ``level``; weight (C_out, k, k, k, C_in)."""
    ks = weight.shape[1]
    if ks == 1:
        return _linear1(weight, bias, x)
    tbl = geometry.subm(level, ks)
    cls = _hip_class(x, weight, ks, geometry, level)
    if cls:
        order = geometry.levels[level]["order"]   # key-sorted walk: tiles of neighbouring sites skip empty offsets and keep the gathers in L2
        return _SubMFn.apply(x.contiguous(), weight, bias, tbl, order, cls == 2)
    return table_conv_torch(x, weight.reshape(weight.shape[0], -1, weight.shape[-1]), bias, geometry.pairs(("subm", level, ks), tbl), x.shape[0])


@dense.fp32_path
def down_conv(x, weight, bias, geometry, level):
    """SparseConv3d(k=2, stride=2) from level ``level`` to ``level + 1``."""
    step = geometry.down(level)
    m = geometry.levels[level + 1]["n"]
    if _hip_class(x, weight, 2, geometry, level) == 1 and m > 0:
        return _DownFn.apply(x.contiguous(), weight, bias, step, m)
    return table_conv_torch(x, weight.reshape(weight.shape[0], 8, weight.shape[-1]), bias, geometry.pairs(("down", level), step.children), m)


@dense.fp32_path
def inverse_conv(x, weight, bias, geometry, level):
    """SparseInverseConv3d(k=2) from level ``level + 1`` back to ``level``."""
    step = geometry.down(level)
    n = geometry.levels[level]["n"]
    if _hip_class(x, weight, 2, geometry, level) == 1:
        return _InverseFn.apply(x.contiguous(), weight, bias, step, n)
    return code_conv_torch(x, weight.reshape(weight.shape[0], 8, weight.shape[-1]), bias, geometry.code_pairs(level), n)


class _Linear1:
    """A kernel-size-1 SubM convolution is a Linear layer over the features (dense.linear: the package's own matrix-core products)."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight.reshape(weight.shape[0], weight.shape[-1]), bias

    def __call__(self, x):
        return torch.nn.functional.linear(x, self.weight, self.bias)


def _linear1(weight, bias, x):
    lin = _Linear1(weight, bias)
    return lin(x) if FORCE_TORCH or not x.is_cuda else dense.linear(lin, x.contiguous())


# ---------------------------------------------------------------------------------------------------------------------------------------
# Modules (spconv's constructor arguments, parameter names and shapes)
# ---------------------------------------------------------------------------------------------------------------------------------------
class SparseModule(nn.Module):
    """Marker: a module that takes and returns a ``SparseConvTensor``."""


class _SparseConv(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1, bias=True, indice_key=None,
                 algo=None, fp32_accum=None, name=None):
        super().__init__()
        ks = kernel_size if isinstance(kernel_size, int) else kernel_size[0]
        if not isinstance(kernel_size, int) and len(set(kernel_size)) != 1:
            raise NotImplementedError("sparse convolutions: cubic kernels only")
        if dilation != 1 or groups != 1:
            raise NotImplementedError("sparse convolutions: dilation and groups are not provided")
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding = in_channels, out_channels, ks, stride, padding
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(out_channels, ks, ks, ks, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size ** 3
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, indice_key={self.indice_key}"


class SubMConv3d(_SparseConv):
    def forward(self, x):
        if self.kernel_size % 2 != 1:
            raise ValueError("SubMConv3d: kernel_size must be odd")
        return x.replace_feature(subm_conv(x.features, self.weight, self.bias, x.geometry, x.level))


class SparseConv3d(_SparseConv):
    def forward(self, x):
        if self.kernel_size != 2 or self.stride != 2 or self.padding != 0:
            raise NotImplementedError("SparseConv3d: only kernel_size=2, stride=2, padding=0 is provided")
        out = down_conv(x.features, self.weight, self.bias, x.geometry, x.level)
        if self.indice_key is not None:
            x.geometry.key_level[self.indice_key] = x.level
        return x.at_level(out, x.level + 1)


class SparseInverseConv3d(_SparseConv):
    def forward(self, x):
        if self.kernel_size != 2:
            raise NotImplementedError("SparseInverseConv3d: only kernel_size=2 is provided")
        level = x.geometry.key_level.get(self.indice_key)
        if level is None:
            raise KeyError(f"SparseInverseConv3d: no SparseConv3d with indice_key={self.indice_key!r} has run on this tensor's geometry")
        if level + 1 != x.level:
            raise ValueError(f"SparseInverseConv3d({self.indice_key!r}): the input is at level {x.level}, the key's output at {level + 1}")
        return x.at_level(inverse_conv(x.features, self.weight, self.bias, x.geometry, level), level)


class Identity(nn.Identity):
    pass


class SparseSequential(SparseModule):
    """spconv's container: sparse modules take the tensor, every other module its features.  ``BatchNorm1d`` (+ a following ``ReLU``) runs
    as the package's fused BatchNorm node (dense.bn_act)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if len(args) == 1 and isinstance(args[0], dict):
            for k, m in args[0].items():
                self.add_module(k, m)
        else:
            for i, m in enumerate(args):
                self.add_module(str(i), m)
        for k, m in kwargs.items():
            self.add_module(k, m)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def forward(self, x):
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(m, nn.BatchNorm1d) and isinstance(x, SparseConvTensor):
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                x = x.replace_feature(dense.bn_act(m, x.features.contiguous(), relu=relu))
                i += int(relu)
            elif isinstance(x, SparseConvTensor):
                if x.features.shape[0] != 0 or not isinstance(m, nn.Identity):
                    x = x.replace_feature(m(x.features))
            else:
                x = m(x)
            i += 1
        return x

"""Seeded cases of the sparse-convolution tests (test_spunet_cpu.py, test_gpu_spunet.py): site sets, a brute-force table builder (a Python
dict of coordinates) and the dense float64 oracle -- ``conv3d``, ``conv3d(stride=2)`` and ``conv_transpose3d(stride=2)`` on the bounding
box, read out at the sites.  spconv is not pinned (it does not exist for this platform); the oracle pins the definitions of
pointcloudpdf_amd/sparse_conv.py.

Tolerance of an operator result against the float64 truth, elementwise: ``gamma_n * S`` with ``gamma_n = n u / (1 - n u)``, ``u = 2^-24``,
``n`` the number of terms of the sum and ``S`` the same convolution applied to ``|x|`` and ``|W|`` in float64 -- the a-priori bound of an
fp32 dot product in any summation order; nothing measured enters it."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24

# (C_in, C_out, kernel size of the SubM layer); the strided / inverse layers use (C_in, C_out) of the k = 3 rows
WIDTHS = [(32, 32, 3), (64, 64, 3), (128, 96, 3), (192, 128, 3), (384, 256, 3), (6, 32, 5), (9, 32, 5), (24, 40, 3)]
UNSUPPORTED = (24, 40, 3)


def gamma(n):
    return n * U / (1 - n * U)


def _distinct(rng, n, extent, batch=0):
    cells = rng.permutation(extent ** 3)[:n]
    c = np.stack([cells // (extent * extent), (cells // extent) % extent, cells % extent], 1)
    return np.concatenate([np.full((n, 1), batch), c], 1)


def site_sets():
    """name -> (indices (N, 4) int32, spatial_shape or None)"""
    rng = np.random.default_rng(20261020)
    out = {"one": (np.array([[0, 3, 4, 5]]), None)}
    for n in (63, 64, 65, 257):
        out[f"n{n}"] = (_distinct(rng, n, 8), None)
    out["dense500"] = (np.concatenate([_distinct(rng, 250, 10, 0), _distinct(rng, 250, 10, 1)]), None)   # 25 % of a 10^3 box: all 27 offsets
    twin = _distinct(rng, 100, 6)
    out["twin"] = (np.concatenate([twin, twin + np.array([[1, 0, 0, 0]])]), None)                         # equal coordinates, two scenes
    # sites at coordinate 0 (an offset of -1 must find nothing) next to a scene that ends at the largest coordinate of every axis
    org = np.concatenate([np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]), _distinct(rng, 40, 5, 0) + np.array([[0, 0, 0, 0]]),
                          np.array([[1, 4, 4, 4], [1, 4, 4, 3], [1, 0, 0, 0]]), _distinct(rng, 30, 5, 1)])
    out["origin"] = (np.unique(org, axis=0)[rng.permutation(len(np.unique(org, axis=0)))], None)
    d = _distinct(rng, 90, 6)
    out["dups"] = (np.concatenate([d, d[rng.permutation(90)[:30]]])[rng.permutation(120)], None)
    out["odd_trunc"] = (_distinct(rng, 120, 7), (7, 7, 7))                                               # shape // 2 = 3 drops coarse coordinate 3
    return {k: (torch.from_numpy(v.astype(np.int32)), s) for k, (v, s) in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# brute force: a dict of coordinates
# ---------------------------------------------------------------------------------------------------------------------------------------
def _lowest(indices):
    where = {}
    for i, row in enumerate(indices.tolist()):
        where.setdefault(tuple(row), i)
    return where


def subm_table_brute(indices, ks):
    where = _lowest(indices)
    h = ks // 2
    tbl = np.full((indices.shape[0], ks ** 3), -1, dtype=np.int32)
    for i, (b, x, y, z) in enumerate(indices.tolist()):
        for o0 in range(ks):
            for o1 in range(ks):
                for o2 in range(ks):
                    tbl[i, (o0 * ks + o1) * ks + o2] = where.get((b, x + o0 - h, y + o1 - h, z + o2 - h), -1)
    return torch.from_numpy(tbl)


def down_brute(indices, spatial_shape=None):
    """-> parent (N), code (N), coarse indices (M, 4) ascending, children (M, 8)"""
    lim = None if spatial_shape is None else [v // 2 for v in spatial_shape]
    rows = indices.tolist()
    keep = lambda p: lim is None or all(p[1 + a] < lim[a] for a in range(3))
    par = [(b, x // 2, y // 2, z // 2) for b, x, y, z in rows]
    coarse = sorted({p for p in par if keep(p)})
    rank = {p: j for j, p in enumerate(coarse)}
    parent = np.array([rank.get(p, -1) if keep(p) else -1 for p in par], dtype=np.int32)
    code = np.array([((x & 1) << 2) | ((y & 1) << 1) | (z & 1) if parent[i] >= 0 else 0 for i, (b, x, y, z) in enumerate(rows)], dtype=np.int32)
    children = np.full((len(coarse), 8), -1, dtype=np.int32)
    for i in reversed(range(len(rows))):
        if parent[i] >= 0:
            children[parent[i], code[i]] = i
    return (torch.from_numpy(parent), torch.from_numpy(code), torch.tensor(coarse, dtype=torch.int32).view(-1, 4), torch.from_numpy(children))


# ---------------------------------------------------------------------------------------------------------------------------------------
# dense float64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
def _first_rows(indices):
    where = _lowest(indices)
    return torch.tensor(sorted(where.values()))


def _dense(x, indices, extent, batches):
    """(B, C, E, E, E) with the features of the LOWEST row of every site."""
    keep = _first_rows(indices)
    idx = indices[keep].long()
    vol = x.new_zeros((batches, extent, extent, extent, x.shape[1]))
    vol = vol.index_put((idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]), x[keep])
    return vol.permute(0, 4, 1, 2, 3)


def _read(vol, indices):
    idx = indices.long()
    return vol.permute(0, 2, 3, 4, 1)[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]


def _box(indices):
    return int(indices[:, 0].max()) + 1, (int(indices[:, 1:].max()) + 2) // 2 * 2   # batches, an even extent


def subm_dense(x, weight, bias, indices):
    """weight (C_out, k, k, k, C_in); x float64 (N, C_in) -> (N, C_out)"""
    b, e = _box(indices)
    ks = weight.shape[1]
    y = F.conv3d(_dense(x, indices, e, b), weight.permute(0, 4, 1, 2, 3), bias, padding=ks // 2)
    return _read(y, indices)


def down_dense(x, weight, bias, indices, coarse):
    b, e = _box(indices)
    y = F.conv3d(_dense(x, indices, e, b), weight.permute(0, 4, 1, 2, 3), bias, stride=2)
    return _read(y, coarse)


def inverse_dense(x, weight, bias, indices, coarse, parent):
    """x (M, C_in) on the coarse sites -> (N, C_out) on the fine sites; rows without a parent get the bias alone."""
    b, e = _box(indices)
    y = F.conv_transpose3d(_dense(x, coarse, e // 2, b), weight.permute(4, 0, 1, 2, 3), None, stride=2)
    out = _read(y, indices) * (parent >= 0).to(x.dtype).unsqueeze(1)
    return out if bias is None else out + bias


def draw(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().double()   # fp32-representable: no input rounding


def oracle(kind, indices, spatial_shape, cin, cout, ks, seed, bias=True):
    """Inputs (float64), truth and bound of one operator: dict(x, w, b, g, out, gx, gw, gb, tol_out, tol_gx, tol_gw, tol_gb)."""
    parent, code, coarse, children = down_brute(indices, spatial_shape)
    n, m = indices.shape[0], coarse.shape[0]
    k = ks if kind == "subm" else 2
    rows_in, rows_out = (n, n) if kind == "subm" else (n, m) if kind == "down" else (m, n)
    x = draw((rows_in, cin), seed).requires_grad_()
    w = draw((cout, k, k, k, cin), seed + 1, 0.2).requires_grad_()
    b = draw((cout,), seed + 2).requires_grad_() if bias else None
    g = draw((rows_out, cout), seed + 3)

    def run(x_, w_, b_):
        if kind == "subm":
            return subm_dense(x_, w_, b_, indices)
        if kind == "down":
            return down_dense(x_, w_, b_, indices, coarse)
        return inverse_dense(x_, w_, b_, indices, coarse, parent)

    out = run(x, w, b)
    grads = torch.autograd.grad(out, [x, w] + ([b] if bias else []), g)
    # the bounds: the same sums over magnitudes
    xa, wa, ga = x.detach().abs().requires_grad_(), w.detach().abs().requires_grad_(), g.abs()
    ba = None if b is None else b.detach().abs().requires_grad_()
    s_out = run(xa, wa, ba)
    s_grads = torch.autograd.grad(s_out, [xa, wa] + ([ba] if bias else []), ga)
    K = k ** 3
    terms_out = (K if kind != "inverse" else 1) * cin + (1 if bias else 0)
    terms_gx = (K if kind != "down" else 1) * cout
    res = dict(x=x.detach(), w=w.detach(), b=None if b is None else b.detach(), g=g, out=out.detach(), gx=grads[0], gw=grads[1],
               gb=grads[2] if bias else None, tol_out=gamma(terms_out) * s_out.detach(), tol_gx=gamma(terms_gx) * s_grads[0],
               tol_gw=gamma(max(rows_out, 1)) * s_grads[1], tol_gb=gamma(max(rows_out, 1)) * s_grads[2] if bias else None,
               parent=parent, code=code, coarse=coarse, children=children)
    return res


def check(name, got, want, tol):
    """|got - want| <= tol elementwise (no element excluded); prints the measured worst ratio for the record."""
    got = got.detach().double().cpu()
    err = (got - want).abs()
    worst = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, worst err / bound {worst:.3f}")
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert bool((err <= tol).all()), f"{name}: {int((err > tol).sum())} elements outside the fp32 bound (worst ratio {worst:.3g})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# model fixture (tests/golden/make_golden_spunet.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
MODEL_KW = dict(in_channels=6, num_classes=13, channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(1,) * 8)
GRAD_NAMES = ["conv_input.0.weight", "down.1.0.weight", "enc.2.block0.conv1.weight", "up.3.0.weight", "up.0.0.weight",
              "dec.1.block0.proj.0.weight", "dec.0.block0.conv2.weight", "final.weight", "final.bias"]
KEEP_ROWS = 400   # logits rows kept in the fixture (every 1 of N // KEEP_ROWS)


def named_weights(model, seed):
    """Name-keyed deterministic parameters (make_golden.py's scheme): every tensor from a generator seeded by its name."""
    import zlib

    with torch.no_grad():
        for name, p in model.state_dict().items():
            if not p.dtype.is_floating_point:
                continue
            g = torch.Generator().manual_seed((zlib.crc32(name.encode()) + seed) % (2 ** 31))
            v = torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1
            if name.endswith("running_var"):
                v = 0.5 + v.abs()
            elif name.endswith("running_mean"):
                v = 0.1 * v
            elif p.dim() == 1 and name.endswith("weight"):
                v = 1.0 + 0.2 * v                      # BatchNorm scales
            elif p.dim() == 1:
                v = 0.1 * v
            else:
                fan = p[0].numel()
                v = v * (3.0 / fan) ** 0.5 * 1.4
            p.copy_(v.float().to(p.dtype))   # fp32-representable in every dtype

"""Shared by test_msc_cpu.py, test_gpu_msc.py and golden/make_golden_msc.py: the fixture's model arguments and stand-ins, what the
reference's cross masks and pair matching compute, written independently as loops, the float64 compositions of the two loss nodes and the tolerance rules.

Tolerances -- nothing measured goes into them.

* kernels against their float64 composition (the a-priori rule of DESIGN 8n): elementwise ``|result - truth64| <= gamma_n * S`` with
  ``gamma_n = n u / (1 - n u)``, ``u = 2^-24`` and ``S`` the same expression evaluated over absolute values.
  InfoNCE: ``n = 2 P + 8 C + 64`` -- the P-term sum enters once directly and once through ``lse``, the C-term dot product enters the
  exponent scaled by ``1 / t <= 4``, again twice, and 64 covers ``exp``, the normalisation and the divisions.  For the loss
  ``S = mean_i(|lse_i| + |s_ii| / t)``; for a gradient element ``S = sum_j |G_ij| |b^_jc|`` pushed through the adjoint of the normalisation
  with absolute values and added over the pairs that point at the row; for ``pos_sim`` / ``neg_sim`` the means of ``sum_c |a^_ic| |b^_jc|``.
  Reconstruction: ``n = N_masked + 2 C + 16``; ``S`` is the first-order propagation of the absolute values through the head, the norm and
  the quotient (``recon_truth``: every difference becomes a sum, every intermediate carries the scale of its own rounding).
* the model against the fixture: ``max(2 x the reference fp32 run's own error against its float64 run, 24 fp32 ulps of the tensor's
  largest magnitude)`` (``pointgroup_cases.bound``, restated)."""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_msc_ref.npz")
ULP = 2.0 ** -23
U = 2.0 ** -24
FLOOR_ULP = 24

IN_CHANNELS = 6
WIDTH = 32
BACKBONE = dict(type="MSC-test-MLP", in_channels=IN_CHANNELS, out_channels=WIDTH)
RUNS = {   # run A: the randperm cut fires, view 1 is mixed, both heads; run B: pairs below the cap, no mixing, the color head alone
    "a": dict(backbone=BACKBONE, backbone_in_channels=IN_CHANNELS, backbone_out_channels=WIDTH, mask_grid_size=0.1, mask_rate=0.4,
              view1_mix_prob=1, view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=512, nce_t=0.4,
              reconstruct_color=True, reconstruct_normal=True),
    "b": dict(backbone=BACKBONE, backbone_in_channels=IN_CHANNELS, backbone_out_channels=WIDTH, mask_grid_size=0.1, mask_rate=0.4,
              view1_mix_prob=0, view2_mix_prob=0, matching_max_k=8, matching_max_radius=0.03, matching_max_pair=8192, nce_t=0.4,
              reconstruct_color=True, reconstruct_normal=False),
}
INPUT_KEYS = [f"view{v}_{k}" for v in (1, 2) for k in ("origin_coord", "coord", "offset", "color", "normal")]


class TinyBackbone(nn.Module):
    """The fixture's backbone: a per-point MLP with a BatchNorm over ``data_dict["feat"]`` plus the mean of its output over the rows of
    the point's scene (``offset``), so that view mixing -- which only changes the offsets the backbone sees -- is visible."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin1 = nn.Linear(in_channels, out_channels)
        self.bn = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        self.lin2 = nn.Linear(out_channels, out_channels)

    def forward(self, data_dict):
        x = self.lin2(torch.relu(self.bn(self.lin1(data_dict["feat"]))))
        ends = data_dict["offset"].tolist()
        return torch.cat([x[s:e] + x[s:e].mean(dim=0, keepdim=True) for s, e in zip([0] + ends[:-1], ends)])


def register_backbone():
    from pointcloudpdf_amd.registry import MODELS

    if "MSC-test-MLP" not in MODELS:
        MODELS.register_module("MSC-test-MLP")(TinyBackbone)


def bound(theirs, ref64):
    ref64 = torch.as_tensor(ref64)
    return max(2.0 * float(theirs), FLOOR_ULP * ULP * float(ref64.abs().max()) if ref64.numel() else 0.0)


def err(value, ref64):
    value, ref64 = torch.as_tensor(value).double().cpu(), torch.as_tensor(ref64).double()
    return float((value - ref64).abs().max()) if ref64.numel() else 0.0


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- stand-ins for what the reference imports -----------------------------------------------------------------------------------------
def voxel_grid(pos, size, batch=None, start=None, end=None):
    """torch_geometric.nn.pool.voxel_grid -> torch_cluster.grid_cluster as a formula: the batch index becomes a 4th coordinate of cell
    size 1; cluster = sum_d floor((pos_d - start_d) / size_d) * prod_{e<d} (floor((end_e - start_e) / size_e) + 1)."""
    pos4 = torch.cat([pos, batch.unsqueeze(-1).to(pos.dtype)], dim=-1)
    size4 = torch.cat([torch.as_tensor(size, dtype=pos.dtype, device=pos.device).reshape(-1).expand(pos.shape[1]), pos.new_ones(1)])
    start4 = pos4.min(0).values if start is None else torch.cat([torch.as_tensor(start, dtype=pos.dtype, device=pos.device).reshape(-1).expand(pos.shape[1]),
                                                                 pos.new_zeros(1)])
    end4 = pos4.max(0).values
    cell = torch.floor((pos4 - start4) / size4).long()
    num = (torch.floor((end4 - start4) / size4).long() + 1).clamp(min=1)   # (as stratified._voxel_grid: an axis whose cells are all below the start counts once)
    stride = torch.cumprod(torch.cat([num.new_ones(1), num[:-1]]), 0)
    return (cell * stride).sum(-1)


def knn_query(nsample, xyz, offset, new_xyz, new_offset):
    """pointops.knn_query by brute force: per scene the ``nsample`` nearest rows of ``xyz`` (ascending distance) -> (idx, distance)."""
    idx = torch.full((new_xyz.shape[0], nsample), -1, dtype=torch.int32, device=xyz.device)
    dst = torch.full((new_xyz.shape[0], nsample), 1e10, dtype=torch.float32, device=xyz.device)
    s0 = q0 = 0
    for s1, q1 in zip(offset.tolist(), new_offset.tolist()):
        d2 = ((new_xyz[q0:q1, None, :] - xyz[None, s0:s1, :]) ** 2).sum(-1)
        k = min(nsample, s1 - s0)
        if q1 > q0 and k > 0:
            val, arg = torch.topk(d2, k, dim=1, largest=False, sorted=True)
            idx[q0:q1, :k] = (arg + s0).int()
            dst[q0:q1, :k] = torch.sqrt(val)
        s0, q0 = s1, q1
    return idx, dst


def offset2batch(offset):
    return torch.searchsorted(offset.long(), torch.arange(int(offset[-1]), device=offset.device), right=True)


# ---- what the reference's two index stages compute, written independently as loops (the tests' oracle) ---------------------------------
def ref_cross_masks(view1_origin_coord, view1_offset, view2_origin_coord, view2_offset, mask_grid_size, mask_rate, randperm=torch.randperm):
    """``generate_cross_masks`` (masked_scene_contrast_v1m1_base.py:69-141) as a dictionary over patches: a patch is a value of the
    ``voxel_grid`` id (``start = 0``, cell size 1, the scene as the slowest coordinate) over the cells of both views; the patches in
    ascending id take the tags of the permutation (1 on its first m entries, 2 on the next m); a view-1 point is masked where its patch
    has tag 1, a view-2 point where it has tag 2."""
    assert mask_rate <= 0.5
    cells, scenes = [], []
    for origin, offset in ((view1_origin_coord, view1_offset), (view2_origin_coord, view2_offset)):
        cells.append(torch.floor(origin.div(mask_grid_size)).cpu().numpy().astype(np.int64))
        ends = offset.cpu().numpy().astype(np.int64)
        scenes.append(np.searchsorted(ends, np.arange(origin.shape[0]), side="right"))
    cell, scene = np.concatenate(cells), np.concatenate(scenes)
    num = np.maximum(cell.max(axis=0) + 1, 1)
    ids = (cell[:, 0] + num[0] * (cell[:, 1] + num[1] * (cell[:, 2] + num[2] * scene))).tolist()
    patches = sorted(set(ids))
    order = randperm(len(patches)).tolist()
    m = int(len(patches) * mask_rate)
    tag = {patches[p]: (1 if at < m else 2 if at < 2 * m else 0) for at, p in enumerate(order)}
    n1 = view1_origin_coord.shape[0]
    dev = view1_origin_coord.device
    return (torch.tensor([tag[i] == 1 for i in ids[:n1]], dtype=torch.bool, device=dev),
            torch.tensor([tag[i] == 2 for i in ids[n1:]], dtype=torch.bool, device=dev))


def ref_match_pairs(view1_coord, view1_offset, view2_coord, view2_offset, max_k, max_radius, max_pair, randint=torch.randint,
                    randperm=torch.randperm):
    """``match_contrastive_pair`` (:143-172) query by query: the neighbours closer than the radius in ascending-k order, one draw per
    query that has any, the neighbour at position c - 1 - (draw % c); more than ``max_pair`` pairs: the permutation's first entries."""
    index, distance = knn_query(max_k, view2_coord.float(), view2_offset.int(), view1_coord.float(), view1_offset.int())
    inside = (distance < max_radius).cpu().numpy()
    index = index.cpu().numpy()
    found = []
    for q in range(index.shape[0]):
        near = [int(index[q, j]) for j in range(max_k) if inside[q, j]]
        if near:
            found.append((q, near))
    draw = randint(max(len(near) for _, near in found), (len(found),), device=view1_coord.device).tolist()
    pairs = [(q, near[len(near) - 1 - d % len(near)]) for (q, near), d in zip(found, draw)]
    if len(pairs) > max_pair:
        pairs = [pairs[i] for i in randperm(len(pairs))[:max_pair].tolist()]
    return torch.tensor(pairs, dtype=torch.int64, device=view1_coord.device).reshape(-1, 2)


# ---- recording / replaying draws ---------------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps torch.randperm / torch.randint / random.random for the duration of a reference run and keeps (name, value) in order."""

    def __init__(self):
        self.seq = []

    def __enter__(self):
        import random

        self._saved = (torch.randperm, torch.randint, random.random)
        randperm, randint, rnd = self._saved

        def rec_randperm(*a, **k):
            v = randperm(*a, **k)
            self.seq.append(("randperm", v.clone()))
            return v

        def rec_randint(*a, **k):
            v = randint(*a, **k)
            self.seq.append(("randint", v.clone()))
            return v

        def rec_random():
            v = rnd()
            self.seq.append(("random", v))
            return v

        torch.randperm, torch.randint, random.random = rec_randperm, rec_randint, rec_random
        return self

    def __exit__(self, *exc):
        import random

        torch.randperm, torch.randint, random.random = self._saved
        return False


def draws_of(golden, run):
    """The fixture's recorded draws of a run as the (name, value) list ``RecordedDraws`` takes."""
    names = [str(n) for n in golden[f"{run}_draw_names"]]
    return [(n, golden[f"{run}_draw_{i}"]) for i, n in enumerate(names)]


def inputs_of(golden, device="cpu", dtype=torch.float32):
    out = {}
    for k in INPUT_KEYS:
        t = torch.from_numpy(golden[f"in_{k}"])
        # (geometry stays fp32 in every run: masks and pairs are those of the fp32 run)
        out[k] = t.to(device) if k.endswith("offset") or k.endswith("origin_coord") else t.to(device=device, dtype=dtype)
    for v in (1, 2):
        out[f"view{v}_feat"] = torch.cat([out[f"view{v}_color"], out[f"view{v}_normal"]], dim=1)   # feat = [color | normal]
    return out


def load_weights(golden, run, model):
    keys = [str(k) for k in golden[f"{run}_keys"]]
    model.load_state_dict({k: torch.from_numpy(golden[f"{run}_weight_{i}"]) for i, k in enumerate(keys)}, strict=True)
    return keys


# ---- float64 truth and S of the InfoNCE node -------------------------------------------------------------------------------------------------
def nce_truth(feat1, feat2, match, t):
    """float64 composition (the reference's lines) on the device of the inputs -> dict of truth values and of the S of every output."""
    f1 = feat1.detach().double().requires_grad_(True)
    f2 = feat2.detach().double().requires_grad_(True)
    m0, m1 = match[:, 0], match[:, 1]
    P = match.shape[0]
    a, b = f1[m0], f2[m1]
    na, nb = torch.norm(a, p=2, dim=1, keepdim=True), torch.norm(b, p=2, dim=1, keepdim=True)
    ah, bh = a / (na + 1e-7), b / (nb + 1e-7)
    sim = ah @ bh.t()
    pos = torch.diagonal(sim).mean()
    neg = sim.mean(dim=-1).mean() - pos / P
    lse = torch.logsumexp(sim / t, dim=1)
    loss = (lse - torch.diagonal(sim) / t).mean()
    g1, g2 = torch.autograd.grad(loss, [f1, f2])
    with torch.no_grad():
        G = (torch.softmax(sim / t, dim=1) - torch.eye(P, dtype=sim.dtype, device=sim.device)).abs() / (P * t)
        abs_sim = ah.abs() @ bh.abs().t()

        def through_adjoint(d_abs, x, n, index, rows):
            den = n + 1e-7
            s = d_abs / den + torch.where(n > 0, x.abs() * (x.abs() * d_abs).sum(1, keepdim=True) / (n.clamp(min=1e-300) * den * den), torch.zeros_like(x))
            return torch.zeros(rows, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, index, s)

        S = dict(loss=float((lse.abs() + torch.diagonal(sim).abs() / t).mean()),
                 pos_sim=float(torch.diagonal(abs_sim).mean()),
                 neg_sim=float(abs_sim.mean() + torch.diagonal(abs_sim).mean() / P),
                 g1=through_adjoint(G @ bh.abs(), a, na, m0, f1.shape[0]),
                 g2=through_adjoint(G.t() @ ah.abs(), b, nb, m1, f2.shape[0]))
    truth = dict(loss=float(loss.detach()), pos_sim=float(pos.detach()), neg_sim=float(neg.detach()), g1=g1, g2=g2)
    return truth, S


def nce_worst_ratio(got, truth, S, P, C):
    """max over every output element of |got - truth| / (gamma_n S); an element with S == 0 must be exact."""
    g = gamma(2 * P + 8 * C + 64)
    worst = 0.0
    for k in ("loss", "pos_sim", "neg_sim"):
        e = abs(float(got[k]) - truth[k])
        worst = max(worst, e / (g * S[k]) if S[k] > 0 else (0.0 if e == 0 else float("inf")))
    for k in ("g1", "g2"):
        e = (got[k].double() - truth[k]).abs()
        ratio = torch.where(S[k] > 0, e / (g * S[k]).clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
    return worst


def nce_case(P, C, n1, n2, seed, repeats=True, zero_rows=True, scaled=True, device="cpu"):
    """fp32-representable inputs: distinct view-1 rows, view-2 rows that repeat, one all-zero feature row on each side, rows scaled by
    1e3 and by 1e-3."""
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((n1, C)).astype(np.float32)
    f2 = (0.5 * rng.standard_normal((n2, C))).astype(np.float32)
    m0 = rng.permutation(n1)[:P]
    m1 = rng.integers(0, n2, P)
    if repeats and P >= 3:
        m1[P // 2] = m1[0]
        m1[P - 1] = m1[0]
    f2[m1] += f1[m0] * 0.7           # matched rows correlate (a repeated row keeps the last write: still plain fp32 data)
    if zero_rows and P >= 2:
        f1[m0[1]] = 0
        f2[m1[P // 3]] = 0
    if scaled and P >= 5:
        f1[m0[2]] *= np.float32(1e3)
        f1[m0[3]] *= np.float32(1e-3)
        f2[m1[4]] *= np.float32(1e3)
        f2[m1[2]] *= np.float32(1e-3)
    match = torch.from_numpy(np.stack([m0, m1], 1).astype(np.int64))
    return torch.from_numpy(f1).to(device), torch.from_numpy(f2).to(device), match.to(device)


# ---- float64 truth and S of the reconstruction node --------------------------------------------------------------------------------------------
def recon_truth(kind, f1, f2, m1, m2, w, b, t1, t2):
    """float64 composition of one head over both views -> truth and S (loss, g1, g2, gw, gb; gradients of the loss itself)."""
    f = torch.cat([f1, f2]).detach().double().requires_grad_(True)
    w64, b64 = w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
    mask = torch.cat([m1, m2])
    tgt = torch.cat([t1, t2]).double()
    count = int(mask.sum())
    pred = f[mask] @ w64.t() + b64
    tm = tgt[mask]
    if kind == "color":
        total = ((pred - tm) ** 2).sum()
    else:
        total = (pred / (torch.norm(pred, p=2, dim=1, keepdim=True) + 1e-10) * tm).sum()
    loss = total / count if count else total * float("nan")
    if count:
        gf, gw, gb = torch.autograd.grad(loss, [f, w64, b64])
    else:
        gf, gw, gb = torch.zeros_like(f), torch.zeros_like(w64), torch.zeros_like(b64)
    with torch.no_grad():
        fa = f[mask].abs()
        pbar = fa @ w64.abs().t() + b64.abs()                      # the scale of a prediction's rounding
        p = pred
        if kind == "color":
            s_e = pbar + tm.abs()
            s_term = (s_e ** 2).sum(1)
            s_d = 2 * s_e                                           # (d term / d pred = 2 (pred - target), over absolute values)
        else:
            n = torch.norm(p, dim=1, keepdim=True)
            den = n + 1e-10
            pos = n > 0
            nz = n.clamp(min=1e-300)
            s_n = torch.where(pos, (p.abs() * pbar).sum(1, keepdim=True) / nz, torch.norm(pbar, dim=1, keepdim=True))
            s_q = pbar / den + p.abs() * s_n / den ** 2
            s_term = (s_q * tm.abs()).sum(1)
            dot = (p * tm).sum(1, keepdim=True)
            s_dot = (pbar * tm.abs()).sum(1, keepdim=True)
            kappa = dot / (nz * den ** 2)
            s_kappa = s_dot / (nz * den ** 2) + dot.abs() * s_n * (1 / (nz ** 2 * den ** 2) + 2 / (nz * den ** 3))
            s_d = tm.abs() / den + tm.abs() * s_n / den ** 2 + torch.where(pos, pbar * kappa.abs() + p.abs() * s_kappa, torch.zeros_like(p))
        scale = 1.0 / count if count else 0.0
        s_gf = torch.zeros_like(f)
        s_gf[mask] = scale * (s_d @ w64.abs())
        S = dict(loss=float(s_term.sum() * scale), gf=s_gf, gw=scale * (s_d.t() @ fa), gb=scale * s_d.sum(0))
    return dict(loss=float(loss.detach()), gf=gf, gw=gw, gb=gb, count=count), S


def recon_worst_ratio(got, truth, S, C):
    g = gamma(truth["count"] + 2 * C + 16)
    e = abs(float(got["loss"]) - truth["loss"])
    worst = e / (g * S["loss"]) if S["loss"] > 0 else (0.0 if e == 0 else float("inf"))
    for k in ("gf", "gw", "gb"):
        e = (got[k].double() - truth[k]).abs()
        ratio = torch.where(S[k] > 0, e / (g * S[k]).clamp(min=1e-300), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))))
        worst = max(worst, float(ratio.max()) if ratio.numel() else 0.0)
    return worst

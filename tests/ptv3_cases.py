"""Shared by test_ptv3_cpu.py, test_gpu_ptv3.py and tests/golden/make_golden_ptv3.py: the fixture's inputs and model configuration, the
attention cases of the GPU test and their references.

Tolerances (nothing measured enters them):
* model logits / loss: 1e-6 relative on the host (the composition is the reference's arithmetic in the same order up to the spconv
  stand-in), ``helpers.REL_TOL`` on the device;
* model gradients -- the rule of tests/ptv2_cases.py: max |ours - reference float64| / max |reference| <= max(2 x the reference's own
  fp32 error, REL_TOL);
* attention node against the float64 composition -- the rule of tests/criteria_cases.py: error <= max(2 x the fp32 composition's own
  error, FLOOR_ULP ulps of the largest magnitude of the result)."""
import numpy as np
import torch

import spunet_cases as sc

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
MODEL_KW = dict(in_channels=6, order=ORDERS, stride=(2, 2), enc_depths=(1, 1, 2), enc_channels=(32, 64, 128), enc_num_head=(2, 4, 8),
                enc_patch_size=(48, 48, 48), dec_depths=(1, 1), dec_channels=(64, 64), dec_num_head=(4, 4), dec_patch_size=(48, 48),
                enable_flash=False, upcast_attention=True, upcast_softmax=True)
SEG_KW = dict(num_classes=13, backbone_out_channels=64)
# name -> (enable_rpe, train, drop_path, shuffle_orders)
MODEL_CASES = {"train": (False, True, 0.0, True), "train_rpe": (True, True, 0.0, True), "eval": (False, False, 0.3, True),
               "eval_rpe": (True, False, 0.3, True)}
SHUFFLE_SEED = 20261020   # torch's CPU generator before every forward
GRAD_NAMES = ["backbone.embedding.stem.conv.weight", "backbone.enc.enc0.block0.attn.qkv.weight", "backbone.enc.enc0.block0.cpe.0.weight",
              "backbone.enc.enc1.down.proj.weight", "backbone.enc.enc2.block1.attn.qkv.bias", "backbone.enc.enc2.block1.mlp.0.fc1.weight",
              "backbone.dec.dec1.up.proj_skip.0.weight", "backbone.dec.dec0.block0.attn.proj.weight", "backbone.dec.dec0.block0.norm1.0.weight",
              "seg_head.weight", "seg_head.bias"]
RPE_GRAD_NAMES = ["backbone.enc.enc0.block0.attn.rpe.rpe_table", "backbone.enc.enc2.block0.attn.rpe.rpe_table"]
KEEP_ROWS = 400
GRAD_KEEP = 1024
POOL_THIN = 8        # pooled feature rows kept in the fixture (every 8th)
PAD_K, PAD_SIZES = 48, (30, 48, 49, 96, 101)

named_weights = sc.named_weights


def _recipe(num_classes, patch, rpe, flash):
    """The `model` section of a reference ``semseg-pt-v3m1-*`` config (settings only)."""
    return dict(type="DefaultSegmentorV2", num_classes=num_classes, backbone_out_channels=64,
                backbone=dict(type="PT-v3m1", in_channels=6, order=("z", "z-trans", "hilbert", "hilbert-trans"), stride=(2, 2, 2, 2),
                              enc_depths=(2, 2, 2, 6, 2), enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
                              enc_patch_size=(patch,) * 5, dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
                              dec_num_head=(4, 4, 8, 16), dec_patch_size=(patch,) * 4, mlp_ratio=4, qkv_bias=True, qk_scale=None,
                              attn_drop=0.0, proj_drop=0.0, drop_path=0.3, shuffle_orders=True, pre_norm=True, enable_rpe=rpe,
                              enable_flash=flash, upcast_attention=not flash, upcast_softmax=not flash, cls_mode=False, pdnorm_bn=False,
                              pdnorm_ln=False, pdnorm_decouple=True, pdnorm_adaptive=False, pdnorm_affine=True,
                              pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D")),
                criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                          dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)])


RECIPES = {"scannet/semseg-pt-v3m1-0-base": _recipe(20, 1024, False, True), "s3dis/semseg-pt-v3m1-0-rpe": _recipe(13, 128, True, False)}


def code_batch():
    """Two scenes with distinct grid coordinates; the second one reaches past 256 (the reference's second table byte)."""
    rng = np.random.default_rng(31)
    a = rng.permutation(40 ** 3)[:700]
    a = np.stack([a // 1600, (a // 40) % 40, a % 40], 1)
    b = rng.permutation(60 ** 3)[:500]
    b = np.stack([b // 3600, (b // 60) % 60, b % 60], 1) * np.array([[7, 5, 6]]) + np.array([[3, 0, 1]])   # up to 416
    return np.concatenate([a, b]).astype(np.int32), np.array([700, 1200], dtype=np.int64)


def pool_batch():
    """Sites, float coordinates and features of the SerializedPooling step of the fixture."""
    rng = np.random.default_rng(32)
    grid, offset = code_batch()
    n = grid.shape[0]
    coord = (grid + rng.uniform(0, 1, (n, 3))).astype(np.float32) * np.float32(0.05)
    feat = rng.uniform(-1, 1, (n, 32)).astype(np.float32)
    return grid, offset, coord, feat


def scene_batch(seed=7):
    rng = np.random.default_rng(seed)
    coords, sizes = [], (2000, 1600)
    for n in sizes:
        cells = rng.permutation(24 ** 3)[:n]
        coords.append(np.stack([cells // 576, (cells // 24) % 24, cells % 24], 1))
    grid = np.concatenate(coords).astype(np.int32)
    n = grid.shape[0]
    coord = (grid + rng.uniform(0, 1, (n, 3))).astype(np.float32) * np.float32(0.05)
    feat = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    segment = rng.integers(0, 13, n).astype(np.int64)
    segment[rng.permutation(n)[: n // 20]] = -1
    return grid, coord, feat, np.cumsum(sizes).astype(np.int64), segment


def thin_grad(g):
    g = np.asarray(g).reshape(-1)
    return g[::max(1, g.size // GRAD_KEEP)]


def build_model(case, seed, dtype=torch.float32, device="cpu"):
    import pointcloudpdf_amd  # noqa: F401
    from pointcloudpdf_amd import point_transformer_v3, segmentor  # noqa: F401
    from pointcloudpdf_amd.registry import MODELS

    rpe, train, dpr, shuffle = MODEL_CASES[case]
    model = MODELS.build(dict(type="DefaultSegmentorV2", backbone=dict(type="PT-v3m1", enable_rpe=rpe, drop_path=dpr, shuffle_orders=shuffle,
                                                                         **MODEL_KW),
                              criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)], **SEG_KW))
    model = model.to(dtype)
    named_weights(model, seed)
    model.train(train)
    return model.to(device)


def model_data(g, dtype=torch.float32, device="cpu"):
    return dict(grid_coord=torch.from_numpy(g["m_grid_coord"]).to(device), coord=torch.from_numpy(g["m_coord"]).to(dtype).to(device),
                feat=torch.from_numpy(g["m_feat"]).to(dtype).to(device), offset=torch.from_numpy(g["m_offset"]).to(device),
                segment=torch.from_numpy(g["m_segment"]).to(device))


def run_model(model, data, train, geometry=None):
    data = dict(data)
    torch.manual_seed(SHUFFLE_SEED)
    if geometry == "ahead":
        data["ptv3_geometry"] = model.backbone.make_geometry(data["grid_coord"], data["offset"])
    if train:
        model.zero_grad(set_to_none=True)
        # (train mode returns the loss alone; the logits are taken where the criteria receive them)
        feats, criteria = {}, model.criteria
        model.criteria = lambda pred, target: (feats.__setitem__("logits", pred), criteria(pred, target))[1]
        try:
            out = model(data)
        finally:
            model.criteria = criteria
        out["loss"].backward()
        return dict(logits=feats["logits"].detach(), loss=out["loss"].detach(),
                    grads={k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None})
    with torch.no_grad():
        out = model(data)
    return dict(logits=out["seg_logits"], loss=out["loss"])


def check_model(case, out, g, tol, rel_tol_grad):
    from helpers import max_rel

    rows = g["m_rows"]
    rep = {"logits": max_rel(out["logits"].detach().cpu().numpy()[rows], g[f"{case}_logits"]),
           "loss": max_rel(out["loss"].detach().cpu().numpy(), g[f"{case}_loss"])}
    print(case, "logits", f"{rep['logits']:.3e}", "loss", f"{rep['loss']:.3e}")
    fails = [k for k in ("logits", "loss") if rep[k] > tol]
    if MODEL_CASES[case][1]:
        names = GRAD_NAMES + (RPE_GRAD_NAMES if MODEL_CASES[case][0] else [])
        for i, name in enumerate(names):
            truth, ref_err, scale = g[f"{case}_grad_{i}"], float(g[f"{case}_grad_err_{i}"]), float(g[f"{case}_grad_max_{i}"])
            err = float(np.abs(thin_grad(out["grads"][name]).astype(np.float64) - truth).max() / (scale + 1e-300))
            bound = max(2.0 * ref_err, rel_tol_grad)
            print(f"  {name}: error {err:.3e} (reference {ref_err:.3e}, bound {bound:.3e})")
            if err > bound:
                fails.append(name)
    assert not fails, (case, fails)


# ---------------------------------------------------------------------------------------------------------------------------------------
# attention cases of the GPU test
# ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (K, scene sizes, scale on q)
ATTN_CASES = {"k48": (48, (30, 48, 49, 96, 101), 1.0), "k128": (128, (300, 128), 1.0), "k1024": (1024, (2500, 700), 1.0),
              "k40": (40, (97,), 1.0), "k48_q30": (48, (30, 48, 49, 96, 101), 30.0)}
ATTN_WIDTHS = [(32, 2), (64, 4), (512, 32)]


class AttnLevel:
    """What ``serial_attention`` needs of a geometry level: a random permutation per scene as the order, and the patch tables."""

    def __init__(self, sizes, seed, device):
        from pointcloudpdf_amd import point_transformer_v3 as v3

        g = torch.Generator().manual_seed(seed)
        order, o = [], 0
        for n in sizes:
            order.append(torch.randperm(n, generator=g) + o)
            o += n
        order = torch.cat(order)
        inverse = torch.empty_like(order)
        inverse[order] = torch.arange(o)
        self.order, self.inverse = order.unsqueeze(0).to(device), inverse.unsqueeze(0).to(device)
        self.sizes, self.n, self._v3, self._t, self.device = list(sizes), o, v3, {}, torch.device(device)

    def patch(self, K):
        if K not in self._t:
            self._t[K] = self._v3.PatchTables(self.sizes, K, self.device)
        return self._t[K]


def attn_inputs(n, c, qscale, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((n, 3 * c), generator=g, dtype=torch.float64).float()
    qkv[:, :c] *= qscale
    gout = torch.randn((n, c), generator=g, dtype=torch.float64).float()
    return qkv, gout


def attn_composition(qkv, gout, level, heads, K, scale):
    """The reference's non-flash branch in qkv's dtype -> (out, grad_qkv)."""
    from pointcloudpdf_amd import point_transformer_v3 as v3

    x = qkv.detach().clone().requires_grad_()
    out = v3.attention_torch(x, level.patch(K), level.order[0], level.inverse[0], heads, scale, upcast_attention=False,
                             upcast_softmax=False)   # (`.float()` would round a float64 evaluation to fp32; a no-op for fp32 rows)
    (grad,) = torch.autograd.grad(out, x, gout.to(out.dtype))
    return out.detach(), grad


def attn_patchwise(qkv, level, heads, K, scale):
    """Every patch of the layout rule gathered and computed on its own (float64): the kept rows in original order."""
    from pointcloudpdf_amd import point_transformer_v3 as v3

    c = qkv.shape[1] // 3
    out = torch.zeros((qkv.shape[0], c), dtype=torch.float64)
    order = level.order[0].cpu()
    x = qkv.double().cpu()
    for (q0, ql, k0, kl) in v3.patch_windows(level.sizes, K):
        qr, kr = order[q0:q0 + ql], order[k0:k0 + kl]
        q = x[qr, :c].reshape(ql, heads, -1).transpose(0, 1)
        k = x[kr, c:2 * c].reshape(kl, heads, -1).transpose(0, 1)
        v = x[kr, 2 * c:].reshape(kl, heads, -1).transpose(0, 1)
        p = torch.softmax((q * scale) @ k.transpose(1, 2), dim=-1)
        out[qr] = (p @ v).transpose(0, 1).reshape(ql, c)
    return out

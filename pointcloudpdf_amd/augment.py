"""Training augmentation on the device: a PDF config's ``data.train.transform`` list (pointcept/datasets/transform.py) applied to a
whole batch of raw scenes, ending in the batch upstream's ``Collect`` + ``collate_fn`` would give.

    pipe = augment.Compose(cfg.data.train.transform)
    batch = pipe(scenes, keys)        # scenes: list of dicts (numpy arrays or device tensors), keys: one 64-bit key per scene

* Per-point work runs in csrc/augment.hip.  The list is cut into segments at every op that reads a data-dependent reduction (the
  bounding box of CenterShift / PositiveShift / RandomRotate(center=None), the colour range of ChromaticAutoContrast); a segment is one
  bounds pass (when its first op needs one) and one fused point pass over every point of every scene.  RandomDropout, GridSample,
  SphereCrop and ShufflePoint are gathers between segments (device sorts: plumbing).
* Precision: NumPy's dtype per scene and array is tracked on the host and carried into every op row (csrc/augment.hip, head comment):
  results equal NumPy's in the reference's dtype, given the same draws.
* Draws: per-scene scalars come from numpy's Philox keyed by the scene key, on the host; per-point values (jitter, colour noise, dropout
  and shuffle keys) are Philox4x64-10 in the kernels, keyed by (scene key, stream of the step).  A scene's augmentation therefore does not
  depend on the batch it is in, and no draw needs a device -> host read.  Tests pass ``records`` (the reference's own draws) instead.
* ElasticDistortion: per stage one bounds pass whose result is read back (the noise-volume sizes and upstream's np.linspace axes are
  made on the host from it), the noise volume (float32 normals), six blur passes and one trilinear sampling pass on the device.
* GridSample's kept point per voxel and SphereCrop's random centre also derive from the scene keys, so the whole batch is a function of
  the scenes and their keys.
"""
import numpy as np
import torch

from . import _native, data_path, voxelize
from .registry import Registry

TRANSFORMS = Registry("transforms")

_M64 = (1 << 64) - 1
# csrc/augment.hip op codes and row slots
OP_CENTER, OP_ROTATE, OP_SCALE, OP_FLIP, OP_JITTER, OP_AUTOCONTRAST, OP_CTRANS, OP_CJITTER, OP_HST, OP_CDROP, OP_POSSHIFT, OP_NORMCOLOR = range(1, 13)
ROW = 16
R_FIRED, R_STREAM, R_REC, R_NF32, R_KF32, R_CF32, R_CODE = 0, 10, 11, 12, 13, 14, 15


class SceneDraws:
    """Per-scene scalar draws from numpy's Philox keyed by the scene key; per-point arrays come from the kernels (``points`` -> None)."""

    def __init__(self, key):
        self.key = int(key) & _M64
        self.rng = np.random.Generator(np.random.Philox(key=self.key))

    def random(self):
        return float(self.rng.random())

    def rand(self, *shape):
        return float(self.rng.random()) if not shape else self.rng.random(shape)

    def uniform(self, lo, hi, size=None):
        return lo + (hi - lo) * (self.rand() if size is None else self.rng.random(size))

    def randint(self, n):
        return int(self.rng.integers(n))

    def points(self, kind, n):
        return None


class RecordedDraws:
    """The draws one scene's reference run made, in order: a list of (name, value) with name in random / rand / randn / uniform /
    choice / shuffle (tests/golden/make_golden_augment.py records them)."""

    def __init__(self, seq):
        self.seq = list(seq)
        self.pos = 0

    def _next(self, name):
        if self.pos >= len(self.seq):
            raise RuntimeError(f"recorded draws exhausted at {name}")
        got, val = self.seq[self.pos]
        if got != name:
            raise RuntimeError(f"recorded draw {self.pos} is {got}, the pipeline asks for {name}")
        self.pos += 1
        return val

    def random(self):
        return float(self._next("random"))

    def rand(self, *shape):
        v = self._next("rand")
        return float(v) if not shape else np.asarray(v, dtype=np.float64).reshape(shape)

    def uniform(self, lo, hi, size=None):
        v = self._next("uniform")
        return float(v) if size is None else np.asarray(v, dtype=np.float64).reshape(size)

    def randint(self, n):
        return int(self._next("randint"))

    def points(self, kind, n):
        return np.asarray(self._next(kind))


class _Scene:
    """Host state of one scene while the list runs: its point count and NumPy's current dtype of each array."""

    def __init__(self, n, cf, kf, nf, draws, key):
        self.n, self.cf, self.kf, self.nf, self.draws, self.key = n, cf, kf, nf, draws, key


class _PointOp:
    code = 0
    bounds = False          # reads the scene's bounds at the start of its segment

    def row(self, sc, rec):
        """-> the op's parameter row for scene ``sc`` (draws consumed here, in list order); ``rec``: list the recorded per-point arrays go to."""
        raise NotImplementedError

    def _row(self, sc, fired=True):
        r = np.zeros(ROW)
        r[R_CODE], r[R_FIRED], r[R_REC] = self.code, 1.0 if fired else 0.0, -1
        r[R_CF32], r[R_KF32], r[R_NF32] = sc.cf, sc.kf, sc.nf
        return r


@TRANSFORMS.register_module()
class CenterShift(_PointOp):
    code, bounds = OP_CENTER, True

    def __init__(self, apply_z=True):
        self.apply_z = apply_z

    def row(self, sc, rec):
        r = self._row(sc)
        r[1] = 1.0 if self.apply_z else 0.0
        return r


@TRANSFORMS.register_module()
class PositiveShift(_PointOp):
    code, bounds = OP_POSSHIFT, True

    def row(self, sc, rec):
        return self._row(sc)


@TRANSFORMS.register_module()
class RandomRotate(_PointOp):
    code = OP_ROTATE

    def __init__(self, angle=None, center=None, axis="z", always_apply=False, p=0.5):
        self.angle = [-1, 1] if angle is None else angle
        self.axis = axis
        self.p = p if not always_apply else 1
        self.center = center
        self.bounds = center is None
        if axis not in ("x", "y", "z"):
            raise NotImplementedError(f"RandomRotate: axis {axis!r}")

    def row(self, sc, rec):
        if sc.draws.random() > self.p:
            return self._row(sc, fired=False)
        angle = sc.draws.uniform(self.angle[0], self.angle[1]) * np.pi
        r = self._row(sc)
        r[1], r[2], r[3] = np.cos(angle), np.sin(angle), "xyz".index(self.axis)
        r[4] = 1.0 if self.center is None else 0.0
        if self.center is not None:
            r[5:8] = [float(c) for c in self.center]
        sc.cf = sc.nf = False          # np.dot with the float64 matrix
        return r


@TRANSFORMS.register_module()
class RandomScale(_PointOp):
    code = OP_SCALE

    def __init__(self, scale=None, anisotropic=False):
        self.scale = scale if scale is not None else [0.95, 1.05]
        self.anisotropic = anisotropic

    def row(self, sc, rec):
        s = np.asarray(sc.draws.uniform(self.scale[0], self.scale[1], 3 if self.anisotropic else 1), dtype=np.float64).reshape(-1)
        r = self._row(sc)
        r[1:4] = s if s.size == 3 else s[0]
        return r


@TRANSFORMS.register_module()
class RandomFlip(_PointOp):
    code = OP_FLIP

    def __init__(self, p=0.5):
        self.p = p

    def row(self, sc, rec):
        r = self._row(sc)
        r[1] = 1.0 if sc.draws.rand() < self.p else 0.0
        r[2] = 1.0 if sc.draws.rand() < self.p else 0.0
        return r


class _NoiseOp(_PointOp):
    def _noise(self, sc, r, rec, stream):
        r[R_STREAM] = stream
        arr = sc.draws.points("randn", sc.n)
        if arr is not None:
            rec.append((sc, arr))
            r[R_REC] = -2              # resolved to the recorded array's index when the segment is packed


@TRANSFORMS.register_module()
class RandomJitter(_NoiseOp):
    code = OP_JITTER

    def __init__(self, sigma=0.01, clip=0.05):
        assert clip > 0
        self.sigma, self.clip = sigma, clip

    def row(self, sc, rec):
        r = self._row(sc)
        r[1], r[2] = self.sigma, self.clip
        self._noise(sc, r, rec, self.stream)
        return r


@TRANSFORMS.register_module()
class ChromaticAutoContrast(_PointOp):
    code, bounds = OP_AUTOCONTRAST, True

    def __init__(self, p=0.2, blend_factor=None):
        self.p, self.blend_factor = p, blend_factor

    def row(self, sc, rec):
        if not sc.has_color or not sc.draws.rand() < self.p:
            return self._row(sc, fired=False)
        r = self._row(sc)
        r[1] = sc.draws.rand() if self.blend_factor is None else self.blend_factor
        return r


@TRANSFORMS.register_module()
class ChromaticTranslation(_PointOp):
    code = OP_CTRANS

    def __init__(self, p=0.95, ratio=0.05):
        self.p, self.ratio = p, ratio

    def row(self, sc, rec):
        if not sc.has_color or not sc.draws.rand() < self.p:
            return self._row(sc, fired=False)
        r = self._row(sc)
        r[1:4] = ((sc.draws.rand(1, 3) - 0.5) * 255 * 2 * self.ratio).reshape(3)
        return r


@TRANSFORMS.register_module()
class ChromaticJitter(_NoiseOp):
    code = OP_CJITTER

    def __init__(self, p=0.95, std=0.005):
        self.p, self.std = p, std

    def row(self, sc, rec):
        if not sc.has_color or not sc.draws.rand() < self.p:
            return self._row(sc, fired=False)
        r = self._row(sc)
        r[1] = self.std * 255
        self._noise(sc, r, rec, self.stream)
        return r


@TRANSFORMS.register_module()
class HueSaturationTranslation(_PointOp):
    code = OP_HST

    def __init__(self, hue_max=0.5, saturation_max=0.2):
        self.hue_max, self.saturation_max = hue_max, saturation_max

    def row(self, sc, rec):
        if not sc.has_color:
            return self._row(sc, fired=False)
        r = self._row(sc)
        r[1] = (sc.draws.rand() - 0.5) * 2 * self.hue_max
        r[2] = 1 + (sc.draws.rand() - 0.5) * 2 * self.saturation_max
        return r


@TRANSFORMS.register_module()
class RandomColorDrop(_PointOp):
    code = OP_CDROP

    def __init__(self, p=0.2, color_augment=0.0):
        self.p, self.color_augment = p, color_augment

    def row(self, sc, rec):
        if not sc.has_color or not sc.draws.rand() < self.p:
            return self._row(sc, fired=False)
        r = self._row(sc)
        r[1] = self.color_augment
        return r


@TRANSFORMS.register_module()
class NormalizeColor(_PointOp):
    code = OP_NORMCOLOR

    def __init__(self, mode="zeroCenter"):
        if mode not in ("zeroCenter", "zeroOne"):
            raise NotImplementedError(f"NormalizeColor: mode {mode!r}")
        self.mode = mode

    def row(self, sc, rec):
        r = self._row(sc, fired=sc.has_color)
        r[1] = 1.0 if self.mode == "zeroOne" else 0.0
        return r


@TRANSFORMS.register_module()
class ElasticDistortion:
    def __init__(self, distortion_params=None):
        self.distortion_params = [[0.2, 0.4], [0.8, 1.6]] if distortion_params is None else distortion_params


@TRANSFORMS.register_module()
class RandomDropout:
    def __init__(self, dropout_ratio=0.2, dropout_application_ratio=0.5):
        self.dropout_ratio, self.dropout_application_ratio = dropout_ratio, dropout_application_ratio


@TRANSFORMS.register_module()
class GridSample:
    def __init__(self, grid_size=0.05, hash_type="fnv", mode="train", keys=("coord", "color", "normal", "segment"), return_inverse=False,
                 return_grid_coord=False, return_min_coord=False, return_displacement=False, project_displacement=False):
        if hash_type != "fnv" or mode != "train" or return_displacement or return_inverse:
            raise NotImplementedError("GridSample: the PDF train lists use hash_type='fnv', mode='train', grid / min coords only")
        self.grid_size, self.keys = grid_size, tuple(keys)
        self.return_grid_coord, self.return_min_coord = return_grid_coord, return_min_coord


@TRANSFORMS.register_module()
class SphereCrop:
    def __init__(self, point_max=80000, sample_rate=None, mode="random"):
        self.point_max, self.sample_rate, self.mode = point_max, sample_rate, mode


@TRANSFORMS.register_module()
class ShufflePoint:
    pass


@TRANSFORMS.register_module()
class MaskLabel:
    def __init__(self, mask_label=None, mask_to=-1):
        self.mask_label, self.mask_to = mask_label, mask_to


@TRANSFORMS.register_module()
class RemapLabel:
    def __init__(self, remap_dict=None, remap_select=None, ignore_index=-1):
        # (a config read back from JSON carries the label keys as strings)
        self.remap_dict = {int(k): int(v) for k, v in (remap_dict or {}).items()}
        self.remap_select, self.ignore_index = remap_select, ignore_index


@TRANSFORMS.register_module()
class Copy:
    """transform.py:53-68.  A scene-level op of the TEST pipeline (testing.TestPipeline applies it); ``Compose`` refuses it."""
    test_only = True

    def __init__(self, keys_dict=None):
        self.keys_dict = dict(coord="origin_coord", segment="origin_segment") if keys_dict is None else dict(keys_dict)


@TRANSFORMS.register_module()
class RandomRotateTargetAngle:
    """transform.py:264-300.  Test-time augmentation op (testing.TestPipeline applies it when it is deterministic); ``Compose`` refuses it."""
    test_only = True

    def __init__(self, angle=(1 / 2, 1, 3 / 2), center=None, axis="z", always_apply=False, p=0.75):
        self.angle = [angle] if not hasattr(angle, "__len__") else list(angle)
        self.center, self.axis = center, axis
        self.p = p if not always_apply else 1
        if axis not in ("x", "y", "z"):
            raise NotImplementedError(f"RandomRotateTargetAngle: axis {axis!r}")


@TRANSFORMS.register_module()
class ToTensor:
    pass


@TRANSFORMS.register_module()
class Collect:
    def __init__(self, keys, offset_keys_dict=None, **kwargs):
        self.keys = [keys] if isinstance(keys, str) else list(keys)
        self.offset_keys = dict(offset="coord") if offset_keys_dict is None else dict(offset_keys_dict)
        self.kwargs = {k.replace("_keys", ""): list(v) for k, v in kwargs.items()}


_ROWS = ("coord", "color", "normal")


class Compose:
    """``Compose(cfg.data.train.transform)(scenes, keys, records=None)`` -> the collated batch (see the module docstring)."""

    def __init__(self, cfg_list):
        self.record_elastic = False   # tests: keep every ElasticDistortion stage's blurred volume and displacement in self.elastic_log
        self.elastic_log = []
        self.transforms = []
        for i, cfg in enumerate(cfg_list):
            cfg = dict(cfg)
            name = cfg.get("type")
            if name not in TRANSFORMS or getattr(TRANSFORMS.get(name), "test_only", False):
                raise KeyError(f"augment.Compose: transform type {name!r} is not supported on the device")
            t = TRANSFORMS.build(cfg)
            t.stream = 16 * (i + 1)
            self.transforms.append(t)

    # -- plumbing ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _upload(scenes, device):
        data, flags = {}, []
        for key in _ROWS + ("segment",):
            parts = [s[key] for s in scenes if key in s]
            if not parts:
                continue
            if len(parts) != len(scenes):
                raise ValueError(f"augment.Compose: {key!r} present in some scenes only")
            host = [p for p in parts if not isinstance(p, torch.Tensor)]
            if host:   # one host -> device copy per array per batch
                cat = np.concatenate([np.asarray(p) if not isinstance(p, torch.Tensor) else p.cpu().numpy() for p in parts])
                t = torch.from_numpy(np.ascontiguousarray(cat)).to(device, non_blocking=False)
            else:
                t = torch.cat([p.to(device) for p in parts])
            data[key] = t.to(torch.float64).contiguous() if key in _ROWS else t.to(torch.int64).contiguous()
        for s in scenes:
            f = {}
            for key in _ROWS:
                if key in s:
                    f[key] = (s[key].dtype == torch.float32) if isinstance(s[key], torch.Tensor) else (np.asarray(s[key]).dtype == np.float32)
            flags.append(f)
        return data, flags

    def _starts(self, sizes, device):
        return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), device=device)

    def _flush(self, ops, data, scenes, sizes, be):
        if not ops:
            return
        rec = []
        tab = np.zeros((len(scenes), 1 + len(ops), ROW))
        for s, sc in enumerate(scenes):
            tab[s, 0, 0] = np.array([sc.key], dtype=np.uint64).view(np.float64)[0]
            for o, op in enumerate(ops):
                first = len(rec)
                r = op.row(sc, rec)
                if r[R_REC] == -2:
                    r[R_REC] = first
                tab[s, 1 + o] = r
        dev = data["coord"].device
        n = data["coord"].shape[0]
        starts = self._starts(sizes, dev)
        rec_t = None
        if rec:   # recorded per-point arrays: (k, n, 3), zero outside the scene that owns each
            full = np.zeros((len(rec), n, 3))
            off = np.concatenate([[0], np.cumsum(sizes)])
            idx = {id(sc): i for i, sc in enumerate(scenes)}
            for k, (sc, arr) in enumerate(rec):
                s = idx[id(sc)]
                full[k, off[s]:off[s + 1]] = arr
            rec_t = torch.from_numpy(full).to(dev)
        bounds = be.aug_bounds(starts, data["coord"], data.get("color")) if ops[0].bounds else None
        be.aug_points(starts, torch.from_numpy(tab).to(dev), bounds, rec_t, data["coord"], data.get("color"), data.get("normal"))
        ops.clear()

    def _voxel_pick(self, g, vsizes, scenes, stream, be):
        """GridSample train mode's kept point per voxel (transform.py:826-830): a Philox key per voxel (scene key, stream; counter =
        the voxel's rank in its scene) modulo the voxel's count, instead of np.random.randint."""
        dev = g["count"].device
        count = g["count"]
        vstart = torch.cumsum(count, 0) - count
        skeys = torch.tensor(np.array([sc.key for sc in scenes], dtype=np.uint64).view(np.int64), device=dev)
        keys = be.aug_keys(self._starts(vsizes, dev), int(sum(vsizes)), skeys, stream)
        dice = torch.remainder((keys >> 11) & ((1 << 53) - 1), count)     # the key's top 53 bits, non-negative
        return g["order"][vstart + dice]

    def _elastic(self, stream, gran, mag, fired, data, scenes, sizes, be):
        """One (granularity, magnitude) stage of ElasticDistortion (transform.py:734-776) for every scene where the step fired."""
        dev = data["coord"].device
        starts = self._starts(sizes, dev)
        bounds = be.aug_bounds(starts, data["coord"]).cpu().numpy()     # read back once per stage: the noise-volume sizes
        dims, axes, noises = [], [], []
        fired = [f and sc.n > 0 for f, sc in zip(fired, scenes)]
        for s, sc in enumerate(scenes):
            if not fired[s]:
                dims.append((0, 0, 0))
                continue
            T = np.float32 if sc.cf else np.float64
            cmin, cmax = bounds[s, :3].astype(T), bounds[s, 3:6].astype(T)
            noise_dim = ((cmax - cmin) // gran).astype(int) + 3       # (coords - coords_min).max(0): rounding is monotone
            ax = [np.linspace(d_min, d_max, d) for d_min, d_max, d in zip(cmin - gran, cmin + gran * (noise_dim - 2), noise_dim)]
            dims.append(tuple(int(d) for d in noise_dim))
            axes.extend(np.asarray(a, dtype=np.float64) for a in ax)
            rec = sc.draws.points("randn", None)
            if rec is not None:
                if rec.shape != (*dims[-1], 3):
                    raise RuntimeError(f"ElasticDistortion: recorded noise {rec.shape}, volume {dims[-1]}")
                noises.append(rec.astype(np.float32).reshape(-1, 3))
        vox = [a * b * c for a, b, c in dims]
        b = len(scenes)
        vinfo = np.concatenate([np.concatenate([[0], np.cumsum(vox)]), np.asarray(dims, dtype=np.int64).reshape(-1),
                                np.concatenate([[0], np.cumsum([sum(d) for d in dims])])]).astype(np.int64)
        params = np.array([[1.0 if f else 0.0, 1.0 if sc.cf else 0.0] for f, sc in zip(fired, scenes)])
        skeys = np.array([sc.key for sc in scenes], dtype=np.uint64).view(np.int64)
        host = [vinfo, np.concatenate(axes), params, skeys]
        vinfo_t, axes_t, params_t, skeys_t = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
        noise_t = torch.from_numpy(np.concatenate(noises)).to(dev) if noises else None
        vol, disp = be.aug_elastic_stage(starts, data["coord"], vinfo_t, int(sum(vox)), axes_t, params_t, mag, skeys_t, stream, noise_t,
                                         keep_disp=self.record_elastic)
        if self.record_elastic:
            self.elastic_log.append(dict(vol=vol, disp=disp, dims=dims))

    @staticmethod
    def _gather(data, idx):
        return {k: v[idx] for k, v in data.items()}

    def _random_order(self, data, sizes, scenes, stream, kind, be, fired=None):
        """Per scene: global point indices in a random order -- the scene's points sorted by their random keys, or the recorded
        choice / permutation (only for the scenes where the step fired)."""
        dev = data["coord"].device
        fired = [True] * len(scenes) if fired is None else fired
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if isinstance(scenes[0].draws, RecordedDraws):
            return [torch.from_numpy(np.asarray(sc.draws.points(kind, sc.n), dtype=np.int64) + off[s]).to(dev) if f else None
                    for s, (sc, f) in enumerate(zip(scenes, fired))]
        n = int(off[-1])
        skeys = torch.tensor(np.array([sc.key for sc in scenes], dtype=np.uint64).view(np.int64), device=dev)
        keys = be.aug_keys(self._starts(sizes, dev), n, skeys, stream) ^ voxelize._SIGN      # unsigned order under a signed sort
        scene = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev), output_size=n)
        o1 = torch.sort(keys, stable=True)[1]
        order = o1[torch.sort(scene[o1], stable=True)[1]]
        return [order[off[s]:off[s + 1]] for s in range(len(sizes))]

    # -- the list ----------------------------------------------------------------------------------------------------------------------
    def __call__(self, scenes, keys, records=None, generator=None, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        data, flags = self._upload(scenes, dev)
        be = _native.backend_for(data["coord"])
        sizes = [int(np.asarray(s["coord"]).shape[0]) if not isinstance(s["coord"], torch.Tensor) else int(s["coord"].shape[0]) for s in scenes]
        st = []
        for i, (f, k) in enumerate(zip(flags, keys)):
            d = RecordedDraws(records[i]) if records is not None else SceneDraws(k)
            sc = _Scene(sizes[i], f.get("coord", False), f.get("color", False), f.get("normal", False), d, int(k) & _M64)
            sc.has_color = "color" in data
            st.append(sc)
        ops, out = [], None
        for t in self.transforms:
            if isinstance(t, _PointOp):
                if t.bounds and ops:
                    self._flush(ops, data, st, sizes, be)
                ops.append(t)
                continue
            self._flush(ops, data, st, sizes, be)
            if isinstance(t, ElasticDistortion):
                if t.distortion_params is not None:
                    fired = [sc.draws.random() < 0.95 for sc in st]
                    if any(fired):
                        for k, (gran, mag) in enumerate(t.distortion_params):
                            self._elastic(t.stream + k, float(gran), float(mag), fired, data, st, sizes, be)
            elif isinstance(t, RandomDropout):
                fired = [sc.draws.random() < t.dropout_application_ratio for sc in st]
                if any(fired):
                    per = self._random_order(data, sizes, st, t.stream, "choice", be, fired)
                    keep = []
                    off = np.concatenate([[0], np.cumsum(sizes)])
                    for s, sc in enumerate(st):
                        if fired[s]:
                            m = int(sc.n * (1 - t.dropout_ratio))
                            keep.append(per[s][:m])
                            sc.n = m
                        else:
                            keep.append(torch.arange(int(off[s]), int(off[s + 1]), device=dev))
                    data = self._gather(data, torch.cat(keep))
                    sizes = [sc.n for sc in st]
            elif isinstance(t, GridSample):
                coord_off = torch.tensor(np.cumsum(sizes).astype(np.int32), device=dev)
                g = voxelize.grid_sample(data["coord"], coord_off, t.grid_size, mode="train", generator=generator,
                                         offset_host=[int(v) for v in np.cumsum(sizes)])
                vsizes = [int(v) for v in torch.diff(g["voxel_offset"].long(), prepend=g["voxel_offset"].new_zeros(1).long()).tolist()]
                idx = self._voxel_pick(g, vsizes, st, t.stream, be) if generator is None else g["idx_unique"]
                new = {k: v[idx] for k, v in data.items() if k in t.keys or k not in _ROWS + ("segment",)}
                if t.return_grid_coord:
                    new["grid_coord"] = g["grid_coord"][idx]
                data = new
                sizes = vsizes
                for sc, n in zip(st, sizes):
                    sc.n = n
            elif isinstance(t, SphereCrop):
                limits = [int(t.sample_rate * n) if t.sample_rate is not None else int(t.point_max) for n in sizes]
                centers = None
                if t.mode == "random" and generator is None:   # transform.py:997-999, drawn from the scene key
                    starts = np.concatenate([[0], np.cumsum(sizes)])
                    centers = [int(starts[s]) + (sc.draws.randint(n) if n > lim else 0) for s, (sc, n, lim) in enumerate(zip(st, sizes, limits))]
                data, new_off, _ = data_path.sphere_crop(data, [int(v) for v in np.cumsum(sizes)], t.point_max, t.sample_rate, t.mode,
                                                         generator=generator, centers=centers)
                sizes = [min(n, lim) for n, lim in zip(sizes, limits)]
                for sc, n in zip(st, sizes):
                    sc.n = n
            elif isinstance(t, ShufflePoint):
                per = self._random_order(data, sizes, st, t.stream, "shuffle", be)
                data = self._gather(data, torch.cat(per))
            elif isinstance(t, MaskLabel):
                if "segment" in data:
                    data["segment_known"] = data_path.mask_label(data["segment"], t.mask_label, t.mask_to)
            elif isinstance(t, RemapLabel):
                if "segment" in data:
                    data["segment_incr_remap"], data["segment_incr"] = data_path.remap_label(data["segment"], t.remap_dict, t.remap_select,
                                                                                             t.ignore_index)
            elif isinstance(t, ToTensor):
                pass
            elif isinstance(t, Collect):
                out = self._collect(t, data, sizes, dev)
        self._flush(ops, data, st, sizes, be)
        if out is None:
            out = dict(data)
            out["offset"] = torch.tensor(np.cumsum(sizes).astype(np.int32), device=dev)
        out["offset_host"] = [int(v) for v in np.cumsum(sizes)]
        return out

    @staticmethod
    def _collect(t, data, sizes, dev):
        """Collect (transform.py:26-50) + collate_fn: ToTensor's casts (floating -> float32, integer -> int64), offsets cumulative."""
        def cast(v):
            return v.float() if v.is_floating_point() else (v.long() if v.dtype != torch.bool else v)

        out = {k: cast(data[k]) for k in t.keys}
        for name in t.offset_keys:
            out[name] = torch.tensor(np.cumsum(sizes).astype(np.int32), device=dev)
        for name, keys in t.kwargs.items():
            out[name] = torch.cat([cast(data[k]).float() for k in keys], dim=1)
        return out

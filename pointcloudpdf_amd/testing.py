"""Test-time fragment voting (pointcept/engines/test.py:189-253).

The reference's tester splits a scene into GridSample "test" fragments (one point per voxel each), runs the segmentor and the
recognizer on every fragment, adds the softmax of the logits into a per-point vote, and averages the recognizer scores per point
with ``torch_scatter.scatter_mean`` (absent here and on the GPU box).  ``FragmentVoter`` keeps the same three accumulators on the
device and folds one fragment per call with a single kernel (``pdf_vote_accumulate``); ``result()`` returns what the tester
derives from them: ``pred = votes.argmax(1)``, ``score = sum / count`` (0 where a point was never visited -- scatter_mean's
convention).  ``fragment_inference`` is that loop, one fragment per forward.  The second half of the module is the tester proper:
``TestPipeline`` / ``SceneTester`` / ``OpenSegTester`` / ``IncrSegTester`` run a reference ``cfg.data.test`` dict on raw scenes with batched
fragments, look-ahead geometry (PT-v1's ``pdf_geometry``, or the StratifiedTransformer's ``st_geometry`` with one window origin per
fragment) and an ordered, atomic-free batched vote (csrc/fragments.hip)."""
import logging
import os

import numpy as np
import torch

from . import _native


class FragmentVoter:
    def __init__(self, num_points, num_classes, device):
        self.pred = torch.zeros(num_points, num_classes, dtype=torch.float32, device=device)   # test.py:207
        self.score_sum = torch.zeros(num_points, dtype=torch.float32, device=device)
        self.score_cnt = torch.zeros(num_points, dtype=torch.float32, device=device)

    @torch.no_grad()
    def add(self, seg_logits, index, score=None):
        """seg_logits (n, classes) of one fragment, index (n) its point ids in the full scene (distinct), score (n) or None."""
        be = _native.backend_for(seg_logits)
        be.vote_accumulate(seg_logits.float().contiguous(), None if score is None else score.float().contiguous(),
                           index.long().contiguous(), self.pred, self.score_sum, self.score_cnt)

    @torch.no_grad()
    def result(self):
        pred = self.pred.max(1)[1]                                            # test.py:242
        score = self.score_sum / self.score_cnt.clamp(min=1.0)               # scatter_mean (test.py:243-251)
        return pred, score


@torch.no_grad()
def fragment_inference(segmentor, recognizer_score_fn, data, fragments, num_classes):
    """Run ``segmentor`` (and ``recognizer_score_fn``) over GridSample test fragments of ONE scene and vote.

    data: dict with coord (N,3), feat (N,C) of the full scene on the device; fragments: list of (n_i,) index tensors
    (``voxelize.grid_sample(..., mode="test")["fragments"]``).  ``segmentor(input_dict)`` must return ``{"seg_logits": (n, K)}``
    (models/default.py:55-62); ``recognizer_score_fn(input_dict, seg_logits)`` returns per-point scores or None."""
    n = data["coord"].shape[0]
    voter = FragmentVoter(n, num_classes, data["coord"].device)
    for idx in fragments:
        part = dict(coord=data["coord"][idx].contiguous(), feat=data["feat"][idx].contiguous(),
                    offset=torch.tensor([idx.shape[0]], dtype=torch.int32, device=idx.device), offset_host=[int(idx.shape[0])])
        logits = segmentor(part)["seg_logits"]
        score = recognizer_score_fn(part, logits) if recognizer_score_fn is not None else None
        voter.add(logits, idx, score)
    return voter.result()


# ================================================================================================================================
# The precise tester (tools/test.py of the reference: OpenSegTester / IncrSegTester, pointcept/engines/test.py:126-510, 513-895) on
# device tensors: the reference's ``cfg.data.test`` dict as is, fragments built G at a time by one kernel, their geometry computed one
# group ahead (engine.GroupedGeometryLoader), votes folded per batch without atomics in the reference's summation order.
#
# Every norm on the path is BatchNorm in eval mode and every geometric op works per scene segment, so a batch of G fragments is G
# independent forwards: the reference's ``fragment_batch_size = 1`` is a choice, not a requirement.  For PT-v1 that holds as the model
# stands.  The StratifiedTransformer's window partition starts at the minimum over the whole collated batch (right for a training batch),
# and CenterShift(apply_z=False) moves every fragment's x/y minimum elsewhere: there the tester hands the model a geometry whose
# partitions start at every fragment's OWN minimum (``st_backbone=``, StratifiedGeometry(window_origin="scene")), which makes the batch
# G independent forwards again.
#
# Dtypes follow NumPy (>= 2) step by step: a float32 scene stays float32 through the shifts, ``coord *= scale`` multiplies in float64
# and rounds back to the array's dtype, RandomRotateTargetAngle promotes to float64 (np.dot with the float64 matrix), and a fragment's
# shift is one subtraction in the coordinates' dtype followed by ToTensor's rounding to float32.
# Host tensors run a torch-op composition of the same steps (``_host_*`` below): that is how the host logic is tested without a GPU.
# ================================================================================================================================
from . import augment, data_path, evaluator, voxelize  # noqa: E402

_LOG = logging.getLogger(__name__)
_CODE_POS, _CODE_IGNORE = 1, 2          # OpenSegTester's all-points labels: 0 = negative, 1 = positive (unknown class), 2 = ignored
_MAX_FUSED_ROWS = 2 ** 31 - 1           # rows of one pdf_openset_metrics call stay below this

_FNV_OFFSET = 14695981039346656037 - (1 << 64)      # the uint64 constants of fnv_hash_vec as int64 bit patterns (int64 products wrap)
_FNV_PRIME = 1099511628211


def _host_grid_hash(coord, offset, gs, min_grid):
    """``pdf_grid_hash`` / ``pdf_grid_hash_f64`` with torch ops (transform.py:815-821, 911-925): floor(coord / grid) in float64,
    scene-relative, FNV key (multiply, then xor) -- for host tensors."""
    g = torch.tensor(gs, dtype=torch.float64, device=coord.device)
    scene = torch.bucketize(torch.arange(coord.shape[0], device=coord.device), offset.long(), right=True)
    grid = torch.floor(coord.double() / g).long() - min_grid[scene]
    h = torch.full((coord.shape[0],), _FNV_OFFSET, dtype=torch.int64, device=coord.device)
    for a in range(3):
        h = (h * _FNV_PRIME) ^ grid[:, a]
    return grid, h


def _table(coord, grid_size):
    off = torch.tensor([coord.shape[0]], dtype=torch.int32, device=coord.device)
    return voxelize.fragment_table(coord.contiguous(), off, grid_size, offset_host=[int(coord.shape[0])],
                                   hash_fn=None if coord.is_cuda else _host_grid_hash)


def _shift_of(op, mn, mx):
    """The vector PositiveShift / CenterShift subtract, from the bounds (.., 3) of the coordinates (transform.py:139-165)."""
    if isinstance(op, augment.PositiveShift):
        return mn
    half = (mn + mx) / 2
    z = mn[..., 2] if op.apply_z else torch.zeros_like(mn[..., 2])
    return torch.stack([half[..., 0], half[..., 1], z], -1)


class TestPipeline:
    """``TestPipeline(cfg.data.test)``: the reference's test-split dict (datasets/defaults.py:23-129) parsed once.

    * ``transform``: scene-level CenterShift / PositiveShift / NormalizeColor / Copy and GridSample(mode="train", return_inverse=True)
      (-> ``inverse`` / ``origin_segment``: predictions are mapped back to the full-resolution scene).
    * ``test_cfg.voxelize``: GridSample(mode="test", hash_type="fnv"); ``test_cfg.crop`` must be None;
      ``test_cfg.post_transform``: one shift, ToTensor, Collect(keys, feat_keys); ``test_cfg.aug_transform``: lists of deterministic
      ops -- RandomScale with scale[0] == scale[1], RandomFlip(p = 0 | 1), RandomRotateTargetAngle with one angle and p = 1.
    """
    __test__ = False   # (not a pytest class)

    def __init__(self, cfg_data_test, generator=None):
        cfg = dict(cfg_data_test)
        test_cfg = cfg.get("test_cfg")
        if test_cfg is None:
            raise ValueError("TestPipeline: the dict has no test_cfg (expected cfg.data.test of a reference config)")
        test_cfg = dict(test_cfg)
        self.generator = generator
        self.scene_ops = [self._scene_op(c) for c in (cfg.get("transform") or [])]
        if test_cfg.get("crop") is not None:
            raise NotImplementedError("TestPipeline: test_cfg.crop must be None -- data_path.sphere_crop has no sliding 'all' mode "
                                      "(SphereCrop(mode='all'), transform.py:958-994)")
        vox = dict(test_cfg.get("voxelize") or {})
        if vox.pop("type", None) != "GridSample" or vox.get("mode") != "test" or vox.get("hash_type", "fnv") != "fnv":
            raise NotImplementedError("TestPipeline: test_cfg.voxelize must be GridSample(mode='test', hash_type='fnv')")
        for k in ("return_inverse", "return_min_coord", "return_displacement"):
            if vox.get(k):
                raise NotImplementedError(f"TestPipeline: test_cfg.voxelize.{k}")
        self.grid_size = vox.get("grid_size", 0.05)
        self.voxel_keys = tuple(vox.get("keys", ("coord", "color", "normal", "segment")))
        self.return_grid_coord = bool(vox.get("return_grid_coord", False))
        post = [augment.TRANSFORMS.build(dict(c)) for c in test_cfg.get("post_transform") or []]
        if (len(post) != 3 or not isinstance(post[0], (augment.CenterShift, augment.PositiveShift)) or not isinstance(post[1], augment.ToTensor)
                or not isinstance(post[2], augment.Collect)):
            raise NotImplementedError("TestPipeline: test_cfg.post_transform must be [CenterShift | PositiveShift, ToTensor, Collect]")
        self.post_shift, collect = post[0], post[2]
        self.keys = list(collect.keys)
        extra = set(collect.kwargs) - {"feat"}
        if extra or "feat" not in collect.kwargs or set(collect.offset_keys.items()) != {("offset", "coord")}:
            raise NotImplementedError("TestPipeline: Collect must have feat_keys and offset_keys_dict=dict(offset='coord') only")
        self.feat_keys = list(collect.kwargs["feat"])
        for k in self.feat_keys:
            if k not in ("coord", "color", "normal") or k not in self.voxel_keys:
                raise ValueError(f"TestPipeline: feat key {k!r} must be coord / color / normal and listed in voxelize.keys")
        if not 1 <= len(self.feat_keys) <= 4:
            raise ValueError("TestPipeline: 1..4 feat_keys")
        for k in self.keys:
            if k not in ("coord", "grid_coord", "index", "segment") or (k == "grid_coord" and not self.return_grid_coord):
                raise ValueError(f"TestPipeline: Collect key {k!r} is not produced by the test pipeline")
        self.augs = [[self._aug_op(c) for c in lst] for lst in test_cfg.get("aug_transform") or [[]]]

    @staticmethod
    def _scene_op(c):
        c = dict(c)
        if c.get("type") == "GridSample":
            if c.get("mode", "train") != "train" or c.get("hash_type", "fnv") != "fnv" or not c.get("return_inverse", False):
                raise NotImplementedError("TestPipeline: a scene-level GridSample must be mode='train', hash_type='fnv', return_inverse=True")
            for k in ("return_grid_coord", "return_min_coord", "return_displacement"):
                if c.get(k):
                    raise NotImplementedError(f"TestPipeline: scene-level GridSample.{k}")
            return c
        op = augment.TRANSFORMS.build(c)
        if not isinstance(op, (augment.CenterShift, augment.PositiveShift, augment.NormalizeColor, augment.Copy)):
            raise NotImplementedError(f"TestPipeline: scene-level transform {c.get('type')!r}")
        return op

    @staticmethod
    def _aug_op(c):
        op = augment.TRANSFORMS.build(dict(c))
        if isinstance(op, augment.RandomScale):
            if op.anisotropic or float(op.scale[0]) != float(op.scale[1]):
                raise ValueError(f"TestPipeline: RandomScale(scale={list(op.scale)}, anisotropic={op.anisotropic}) is not deterministic")
        elif isinstance(op, augment.RandomFlip):
            if op.p not in (0, 1):
                raise ValueError(f"TestPipeline: RandomFlip(p={op.p}) is not deterministic")
        elif isinstance(op, augment.RandomRotateTargetAngle):
            if len(op.angle) != 1 or op.p != 1:
                raise ValueError(f"TestPipeline: RandomRotateTargetAngle(angle={op.angle}, p={op.p}) is not deterministic")
        else:
            raise ValueError(f"TestPipeline: test-time augmentation {c.get('type')!r} (RandomScale / RandomFlip / RandomRotateTargetAngle)")
        return op

    # -- scene level -------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _tensor(v, device):
        return (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(device)

    def prepare(self, scene, device):
        """Raw scene dict (coord, color, normal?, segment; numpy or tensors) -> the scene state after ``transform`` on ``device``: coord in
        its own float dtype, color / normal, segment int64 (+ inverse, origin_segment after a scene-level GridSample)."""
        st = {}
        for k in ("coord", "color", "normal"):
            if k in scene and scene[k] is not None:
                t = self._tensor(scene[k], device)
                st[k] = t if t.dtype in (torch.float32, torch.float64) else t.double()   # (uint8 colour / 127.5 is float64 in NumPy)
        seg = scene.get("segment")
        st["segment"] = (self._tensor(seg, device).long().reshape(-1) if seg is not None
                         else torch.full((st["coord"].shape[0],), -1, dtype=torch.long, device=device))
        for op in self.scene_ops:
            if isinstance(op, dict):
                st = self._scene_grid_sample(st, op)
            elif isinstance(op, augment.Copy):
                for src, dst in op.keys_dict.items():
                    st[dst] = st[src].clone()
            elif isinstance(op, augment.NormalizeColor):
                if "color" in st:
                    # a (1,) tensor divisor: torch's device kernels turn division by a SCALAR into a product with its reciprocal
                    div = st["color"].new_full((1,), 255.0 if op.mode == "zeroOne" else 127.5)
                    st["color"] = st["color"] / div if op.mode == "zeroOne" else st["color"] / div - 1
            else:
                c = st["coord"]
                st["coord"] = c - _shift_of(op, c.amin(0), c.amax(0))
        if "origin_segment" in st and "inverse" not in st:
            raise ValueError("TestPipeline: origin_segment without inverse (Copy without GridSample(return_inverse=True))")
        return st

    def _scene_grid_sample(self, st, c):
        """GridSample(mode="train", return_inverse=True) of the scene list (transform.py:813-857): one random point per voxel kept."""
        t = _table(st["coord"], c.get("grid_size", 0.05))
        # drawn on the generator's own device (a CPU generator serves a device scene, and gives it the host path's draw), then moved
        dev = st["coord"].device if self.generator is None else self.generator.device
        dice = torch.randint(0, max(t["cmax"], 1), (t["count"].shape[0],), generator=self.generator, device=dev).to(st["coord"].device) % t["count"]
        idx = t["order"][t["vstart"] + dice]
        keys = tuple(c.get("keys", ("coord", "color", "normal", "segment")))
        out = {k: (v[idx] if k in keys else v) for k, v in st.items()}
        out["inverse"] = t["inverse"]
        return out

    def augmented(self, st, ops):
        """-> (coord, normal) of the scene after one ``aug_transform`` list (transform.py:264-334)."""
        coord, normal = st["coord"], st.get("normal")
        for op in ops:
            if isinstance(op, augment.RandomScale):
                coord = (coord.double() * float(op.scale[0])).to(coord.dtype)      # in-place `*=` with a float64 array: float64 product, one rounding
            elif isinstance(op, augment.RandomFlip):
                if op.p == 1:
                    sign = coord.new_tensor([-1.0, -1.0, 1.0])
                    coord = coord * sign
                    normal = normal * sign.to(normal.dtype) if normal is not None else None
            else:
                angle = float(op.angle[0]) * np.pi
                co, si = float(np.cos(angle)), float(np.sin(angle))
                rot = {"x": [[1, 0, 0], [0, co, -si], [0, si, co]], "y": [[co, 0, si], [0, 1, 0], [-si, 0, co]],
                       "z": [[co, -si, 0], [si, co, 0], [0, 0, 1]]}[op.axis]
                rot_t = torch.tensor(rot, dtype=torch.float64, device=coord.device).t()
                center = ((coord.amin(0) + coord.amax(0)) / 2 if op.center is None
                          else torch.tensor([float(v) for v in op.center], dtype=torch.float64, device=coord.device))
                coord = (coord - center.to(coord.dtype) if op.center is None else (coord.double() - center).to(coord.dtype))
                coord = coord.double() @ rot_t + center.double()
                normal = normal.double() @ rot_t if normal is not None else None
        return coord, normal

    # -- fragments ---------------------------------------------------------------------------------------------------------------------
    def batches(self, st, fragments_per_batch, with_segment=False):
        """Generator over the collated fragment batches of the scene, every augmentation in list order, ``fragments_per_batch`` fragments
        at a time (the last batch of an augmentation may be shorter).  A batch: coord, feat, offset, offset_host, index[, grid_coord,
        segment] and ``fragment`` = dict(table, f0, g, aug)."""
        g_max = max(int(fragments_per_batch), 1)
        f32 = {}
        for a, ops in enumerate(self.augs):
            coord, normal = self.augmented(st, ops)
            coord = coord.contiguous()
            table = _table(coord, self.grid_size)
            if table["count"].shape[0] == 0:
                continue
            segs = []
            for k in self.feat_keys:
                if k == "coord":
                    segs.append(None)
                elif k == "normal":
                    segs.append(normal.float().contiguous())
                else:
                    if k not in f32:
                        f32[k] = st[k].float().contiguous()
                    segs.append(f32[k])
            for f0 in range(0, table["cmax"], g_max):
                g = min(g_max, table["cmax"] - f0)
                make = self._device_batch if coord.is_cuda else self._host_batch
                batch = make(coord, table, f0, g, segs)
                if "grid_coord" not in self.keys:
                    batch.pop("grid_coord", None)
                if with_segment or "segment" in self.keys:
                    batch["segment"] = st["segment"][batch["index"]]
                v = int(table["count"].shape[0])
                batch["offset_host"] = [(k + 1) * v for k in range(g)]
                batch["fragment"] = dict(table=table, f0=f0, g=g, aug=a)
                yield batch

    def _device_batch(self, coord, table, f0, g, segs):
        be = _native.backend_for(coord)
        bounds = be.fragment_bounds(coord, table, f0, g).to(coord.dtype)      # (exact: the bounds are values of coord's dtype)
        shift = _shift_of(self.post_shift, bounds[:, :3], bounds[:, 3:]).contiguous()
        return be.fragment_gather(coord, table, f0, g, shift, segs, table["grid_coord"] if self.return_grid_coord else None)

    def _host_batch(self, coord, table, f0, g, segs):
        """``pdf_fragment_bounds`` + ``pdf_fragment_gather`` with torch ops."""
        v = table["count"].shape[0]
        idx = torch.stack([table["order"][table["vstart"] + f % table["count"]] for f in range(f0, f0 + g)])   # (g, v)
        c = coord[idx]                                                                                         # (g, v, 3)
        shift = _shift_of(self.post_shift, c.amin(1), c.amax(1))
        out_coord = (c - shift[:, None, :]).float().reshape(g * v, 3)
        index = idx.reshape(-1)
        feat = torch.cat([out_coord if s is None else s[index] for s in segs], 1)
        out = dict(index=index, coord=out_coord, feat=feat, offset=(torch.arange(1, g + 1, dtype=torch.int32) * v).to(coord.device))
        if self.return_grid_coord:
            out["grid_coord"] = table["grid_coord"][index]
        return out


class SceneTester:
    """Votes one scene: ``SceneTester(forward_fn, num_classes, pipeline).run(scene) -> (pred (N), score (N) | None)``.

    ``forward_fn(batch) -> (seg_logits (rows, num_classes), score (rows) | None)`` sees a collated batch of ``fragments_per_batch``
    fragments with ``batch["pdf_geometry"]`` attached -- computed ``group`` batches ahead on a side stream by
    ``engine.GroupedGeometryLoader`` (``group=0``: inline, the serial path).  Batches are generated lazily, one group ahead of use.
    Every batch is folded with ``pdf_fragment_vote``: no atomics, a point's fragments in ascending order, so the result is
    bit-reproducible and bit-identical to feeding the fragments one at a time through ``FragmentVoter.add``."""

    def __init__(self, forward_fn, num_classes, pipeline, fragments_per_batch=4, group=None, prefetch_plan=None, with_segment=False,
                 device=None, st_backbone=None, own_geometry=False):
        """``group``: batches per look-ahead pre-pass; default 12, or as many as ``GroupedGeometryLoader.MAX_SCENES`` fragments allow.
        ``st_backbone``: the forward's ``stratified.StratifiedTransformer`` (anything with ``make_geometry`` / ``layers_by_level``): the
        batches then carry ``batch["st_geometry"]`` instead -- FPS chain, neighbour tables and window partitions with one origin per
        fragment -- from a ``StratifiedPrefetcher(st_backbone, window_origin="scene")`` one group ahead, or inline with ``group=0``.
        ``own_geometry``: the forward builds its geometry itself (PT-v2m2): the fragment batches reach it as they are -- no loader, no
        PT-v1 pre-pass, no ``pdf_geometry`` attached."""
        from . import engine

        if st_backbone is not None and not (hasattr(st_backbone, "make_geometry") and hasattr(st_backbone, "layers_by_level")):
            raise TypeError("SceneTester: st_backbone must be a StratifiedTransformer (make_geometry / layers_by_level)")
        self.st_backbone = st_backbone
        self.own_geometry = bool(own_geometry)
        if self.own_geometry and st_backbone is not None:
            raise ValueError("SceneTester: own_geometry and st_backbone exclude each other")

        self.forward_fn, self.num_classes, self.pipeline = forward_fn, int(num_classes), pipeline
        self.fragments_per_batch = max(int(fragments_per_batch), 1)
        if group is None:
            group = max(min(12, engine.GroupedGeometryLoader.MAX_SCENES // self.fragments_per_batch), 1)
        self.group = max(int(group), 0)
        if self.group * self.fragments_per_batch > engine.GroupedGeometryLoader.MAX_SCENES:
            raise ValueError(f"SceneTester: group x fragments_per_batch = {self.group * self.fragments_per_batch} exceeds "
                             f"GroupedGeometryLoader.MAX_SCENES = {engine.GroupedGeometryLoader.MAX_SCENES}")
        self.with_segment = with_segment
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.plan = dict(prefetch_plan or {})
        self._loader, self._prefetcher = None, None
        if st_backbone is not None and self.group > 0 and not st_backbone.geometry_cfg.get("stem_transformer", True):
            _LOG.info("SceneTester: StratifiedGeometry.precompute_group covers stem_transformer=True only: geometry inline (group=0)")
            self.group = 0

    def _st_inline(self, batches):
        """The look-ahead's geometry, computed per batch on the consumer's stream (``group=0``, and every host-tensor run)."""
        bb = self.st_backbone
        for batch in batches:
            geom = bb.make_geometry(batch["coord"], batch["offset"], batch.get("offset_host"), window_origin="scene")
            yield dict(batch, st_geometry=geom.precompute(bb.layers_by_level()))

    def _loaded(self, batches):
        if self.own_geometry:
            return batches
        if self.st_backbone is not None and (self.device.type != "cuda" or self.group == 0):
            return self._st_inline(batches)
        if self.device.type != "cuda":
            return batches
        if self._loader is None:   # one loader (its side streams and their allocator pools) for every scene this tester sees
            from . import engine

            if self.st_backbone is not None:
                from .stratified import StratifiedPrefetcher

                self._prefetcher = StratifiedPrefetcher(self.st_backbone, window_origin="scene")
                self._loader = engine.GroupedGeometryLoader(None, group=self.group, prefetcher=self._prefetcher, key="st_geometry")
            else:
                self._loader = engine.GroupedGeometryLoader(None, group=self.group, **self.plan)
        self._loader.loader = batches
        return self._loader

    def close(self):
        """Joins the look-ahead's worker thread and drops its side stream (also done when the tester is dropped)."""
        pf, self._prefetcher, self._loader = self._prefetcher, None, None
        if pf is not None:
            pf.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown: the pool's module may be gone)
            pass

    @torch.no_grad()
    def vote(self, st):
        """Scene state (``pipeline.prepare``) -> (votes (N, K), score_sum (N), score_cnt (N), scored)."""
        n, dev = st["coord"].shape[0], st["coord"].device
        votes = torch.zeros(n, self.num_classes, dtype=torch.float32, device=dev)
        ssum, scnt = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        scored = False
        for batch in self._loaded(self.pipeline.batches(st, self.fragments_per_batch, self.with_segment)):
            logits, score = self.forward_fn(batch)
            frag = batch["fragment"]
            logits = logits.float().contiguous()
            score = None if score is None else score.float().reshape(-1).contiguous()
            scored = scored or score is not None
            if logits.is_cuda:
                _native.backend_for(logits).fragment_vote(logits, score, frag["table"], frag["f0"], frag["g"], votes, ssum, scnt)
            else:
                _host_vote(logits, score, batch["index"], frag["g"], votes, ssum, scnt)
        return votes, ssum, scnt, scored

    @torch.no_grad()
    def run(self, scene, return_votes=False):
        st = self.pipeline.prepare(scene, self.device)
        votes, ssum, scnt, scored = self.vote(st)
        pred = votes.max(1)[1]                                                      # test.py:241
        score = ssum / scnt.clamp(min=1.0) if scored else None                      # scatter_mean (test.py:242-251)
        if "inverse" in st:                                                         # test.py:254-257
            pred = pred[st["inverse"]]
            score = score[st["inverse"]] if score is not None else None
        return (pred, score, votes) if return_votes else (pred, score)


def _host_vote(logits, score, index, g, votes, ssum, scnt):
    """``pdf_fragment_vote`` with torch ops: the batch's fragments one after the other (test.py:225-230)."""
    v = index.shape[0] // g
    for k in range(g):
        rows = slice(k * v, (k + 1) * v)
        votes[index[rows], :] += torch.softmax(logits[rows], -1)
        if score is not None:
            ssum.index_add_(0, index[rows], score[rows])
            scnt.index_add_(0, index[rows], torch.ones_like(score[rows]))


_BATCH_KEYS = ("coord", "feat", "offset", "offset_host", "grid_coord", "pdf_geometry", "st_geometry")


def _cfg_get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def _st_backbone(model):
    """The segmentor's backbone when it is a StratifiedTransformer (window partitions per fragment: ``make_geometry`` /
    ``layers_by_level``), else None.  (PT-v2m2 has a ``make_geometry`` too; its partition starts at every scene's own minimum, so a batch
    of fragments is independent forwards: ``SceneTester(own_geometry=True)`` hands the batches to the forward without any pre-pass.)"""
    bb = getattr(model, "backbone", None)
    return bb if bb is not None and hasattr(bb, "make_geometry") and hasattr(bb, "layers_by_level") else None


class _TesterBase:
    """What the two testers share: the scene loop, the result files and the class histograms (test.py:189-266, 572-634)."""

    def __init__(self, cfg, num_classes, forward_fn, with_segment, st_backbone=None, own_geometry=False):
        data = _cfg_get(cfg, "data")
        self.cfg = cfg
        self.ignore_index = int(_cfg_get(data, "ignore_index", -1))
        self.dim_pred = int(num_classes)
        self.pipeline = TestPipeline(_cfg_get(data, "test"))
        opts = {k: _cfg_get(cfg, k) for k in ("fragments_per_batch", "group", "prefetch_plan") if _cfg_get(cfg, k) is not None}
        self.scene_tester = SceneTester(forward_fn, self.dim_pred, self.pipeline, with_segment=with_segment, device=_cfg_get(cfg, "device"),
                                        st_backbone=st_backbone, own_geometry=own_geometry, **opts)

    def close(self):
        self.scene_tester.close()

    def _labels(self, st):
        return st["segment"]

    def _scene(self, scene, result_dir, need_score):
        """-> (name, pred, score, segment) on the full-resolution scene as tensors on the tester's device.  Host copies are made for the
        result files only; results reloaded from them are uploaded."""
        name = scene.get("name", "scene")
        dev = self.scene_tester.device
        st = self.pipeline.prepare(scene, dev)
        pred_path = os.path.join(result_dir, f"{name}_pred.npy") if result_dir else None
        score_path = os.path.join(result_dir, f"{name}_score.npy") if result_dir else None
        if pred_path and os.path.isfile(pred_path) and (not need_score or os.path.isfile(score_path)):   # test.py:195-204
            pred = torch.from_numpy(np.load(pred_path)).to(dev)
            score = torch.from_numpy(np.load(score_path)).to(dev) if need_score else None
        else:
            votes, ssum, scnt, scored = self.scene_tester.vote(st)
            pred = votes.max(1)[1]
            score = ssum / scnt.clamp(min=1.0) if scored else None
            if pred_path:
                np.save(pred_path, pred.cpu().numpy())
                if need_score and score is not None:
                    np.save(score_path, score.cpu().numpy())
        segment = self._labels(st)
        if "inverse" in st:   # test.py:254-257 (the score follows the prediction back to the full-resolution scene)
            inv = st["inverse"]
            pred, score = pred[inv], (score[inv] if score is not None else None)
            segment = self._origin_labels(st)
        return name, pred.long().contiguous(), (None if score is None else score.float().contiguous()), segment.long().contiguous()

    def _origin_labels(self, st):
        return st["origin_segment"]

    def _metrics(self, pred, score, segment, unknown_label=()):
        """``evaluator.openset_metrics`` of one scene, read back at once -> (intersection, union, target (K) float64, record (4))."""
        hist, rec = evaluator.openset_metrics(pred, score, segment, self.dim_pred, unknown_label, self.ignore_index)
        flat = torch.cat([hist.reshape(-1).double(), rec]).cpu().numpy()
        h = flat[:-4].reshape(3, -1)
        return h[0], h[1], h[2], flat[-4:]

    @staticmethod
    def _result_dir(save_path):
        if save_path is None:
            return None
        d = os.path.join(save_path, "result")
        os.makedirs(d, exist_ok=True)
        return d


class OpenSegTester(_TesterBase):
    """``OpenSegTester(step_or_models, cfg).test(scenes, save_path=None)`` -- engines/test.py:126-445 on raw scenes.

    ``step_or_models``: an ``engine.OpenSegStep``, or ``(segmentor, recognizer)`` with a ``MaxProbability`` or ``PointPdf-v1m1``
    recognizer (a PointPdf-v1m1 must carry its ``model_hooks``); modules are put in eval mode.  ``cfg``: the reference config
    (dict or attribute access): ``data.num_classes``, ``data.ignore_index``, ``data.test``, ``unknown_label``; optional
    ``fragments_per_batch`` / ``group`` / ``prefetch_plan`` / ``device``.

    The reference's tester reads ``recognizer(input_dict)["score"]``, while ``PointPdfV1.forward`` returns ``score`` only when the dict
    has a ``segment`` key (pointpdf_v1m1_base.py:109-116): as shipped, the reference raises ``KeyError`` for PointPdf-v1m1 with Collect
    keys that hold no ``segment``.  Here the fragment's labels are passed to the recognizer so that the evaluator's branch runs; the
    segmentor does not see them (no loss is computed).

    Returns one dict: mIoU / mAcc / allAcc over the known classes, iou_class / acc_class, aupr / auroc (mean over the scenes that hold
    unknown points), all_aupr / all_auroc (over all points), and ``scenes``: the per-scene and running figures of the reference's log."""

    def __init__(self, step_or_models, cfg):
        from . import recognizer as rec_mod

        if isinstance(step_or_models, (tuple, list)):
            model, rec = step_or_models
            hooks = getattr(rec, "model_hooks", None)
        else:
            model, rec, hooks = step_or_models.model, step_or_models.recognizer, step_or_models.hooks
            step_or_models.eval()
        model.eval()
        if isinstance(rec, torch.nn.Module):
            rec.eval()
        is_msp = isinstance(rec, rec_mod.MaxProbability)
        if not is_msp and hooks is None:
            raise ValueError("OpenSegTester: the recognizer needs its model_hooks (engine.OpenSegStep sets them)")

        def forward(batch):
            d = {k: batch[k] for k in _BATCH_KEYS if k in batch}
            if is_msp:
                logits = model(d)["seg_logits"]
                return logits, -rec.prob_func(logits)
            with hooks:
                logits = model(d)["seg_logits"]
                score = rec(dict(d, segment=batch["segment"]))["score"]
            return logits, score.reshape(-1)

        data = _cfg_get(cfg, "data")
        bb = getattr(model, "backbone", None)
        super().__init__(cfg, int(_cfg_get(data, "num_classes")), forward, with_segment=not is_msp, st_backbone=_st_backbone(model),
                         own_geometry=hasattr(bb, "make_geometry") and _st_backbone(model) is None)
        self.unknown_label = [int(v) for v in _cfg_get(cfg, "unknown_label", [])]
        self.mask_known = np.ones(self.dim_pred, dtype=bool)
        self.mask_known[self.unknown_label] = False
        dev = self.scene_tester.device
        if dev.type == "cuda":   # the byte masks of the per-scene and the all-points call, uploaded once
            self._unknown = evaluator.unknown_mask(self.dim_pred, self.unknown_label, dev)
            self._unknown_code = evaluator.unknown_mask(2, [_CODE_POS], dev)
        else:
            self._unknown, self._unknown_code = self.unknown_label, [_CODE_POS]

    def _codes(self, segment):
        """One byte per point for the all-points figures: negative / positive / ignored."""
        unknown = torch.as_tensor(self.unknown_label, dtype=segment.dtype, device=segment.device)
        code = torch.isin(segment, unknown).to(torch.uint8) * _CODE_POS
        return torch.where(segment == self.ignore_index, torch.full_like(code, _CODE_IGNORE), code)

    def test(self, scenes, save_path=None):
        result_dir = self._result_dir(save_path)
        k = self.mask_known
        isum, usum, tsum = (np.zeros(self.dim_pred) for _ in range(3))
        auprs, aurocs, per_scene, all_score, all_code = [], [], {}, [], []
        for scene in scenes:
            name, pred, score, segment = self._scene(scene, result_dir, need_score=True)
            i, u, t, record = self._metrics(pred, score, segment, self._unknown)
            isum, usum, tsum = isum + i, usum + u, tsum + t
            cls = (u != 0) & k                                                         # test.py:268-279
            rec = dict(intersection=i, union=u, target=t,
                       mIoU=float(np.mean((i / (u + 1e-10))[cls])), allAcc=float(sum(i[cls]) / (sum(t[cls]) + 1e-10)),
                       running_mIoU=float(np.mean(isum[cls] / (usum[cls] + 1e-10))), running_mAcc=float(np.mean(isum[cls] / (tsum[cls] + 1e-10))))
            aupr, auroc = (float(record[0]), float(record[1])) if record[2] > 0 else (None, None)
            if aupr is not None:                                                       # test.py:281-294
                auprs.append(aupr); aurocs.append(auroc)
            rec.update(aupr=aupr, auroc=auroc)
            per_scene[name] = rec
            all_score.append(score); all_code.append(self._codes(segment))             # 5 bytes per point stay on the device
        iou_class, acc_class = isum / (usum + 1e-10), isum / (tsum + 1e-10)             # test.py:405-411
        out = dict(mIoU=float(np.mean(iou_class[k])), mAcc=float(np.mean(acc_class[k])), allAcc=float(sum(isum[k]) / (sum(tsum[k]) + 1e-10)),
                   iou_class=iou_class, acc_class=acc_class, intersection=isum, union=usum, target=tsum,
                   aupr=float(np.mean(auprs)) if auprs else float("nan"), auroc=float(np.mean(aurocs)) if aurocs else float("nan"), scenes=per_scene)
        if all_score:                                                                   # test.py:419-427
            a, r = self._all_points(all_score, all_code)
            out.update(all_aupr=float("nan") if a is None else a, all_auroc=float("nan") if r is None else r)
        return out

    def _all_points(self, scores, codes):
        """AUPR / AUROC over every point of the split: one ``openset_metrics`` call over the concatenation (labels = the codes)."""
        total = sum(int(c.shape[0]) for c in codes)
        if total >= _MAX_FUSED_ROWS and codes[0].is_cuda:
            _LOG.warning("OpenSegTester: %d points exceed one device pass (2^31 - 2 rows); all-points AUPR / AUROC on the host", total)
            scores, codes = [s.cpu() for s in scores], [c.cpu() for c in codes]
        score, code = torch.cat(scores), torch.cat(codes).long()
        unknown = self._unknown_code if code.is_cuda else [_CODE_POS]
        _, rec = evaluator.openset_metrics(code, score, code, 2, unknown, _CODE_IGNORE)
        rec = rec.cpu().numpy()
        return (float(rec[0]), float(rec[1])) if rec[2] > 0 else (None, None)


class IncrSegTester(_TesterBase):
    """``IncrSegTester(step, cfg).test(scenes, save_path=None)`` -- engines/test.py:513-840: the student of an ``engine.IncrSegStep``
    (``num_classes + len(incr_label_remap)`` logits) voted over the fragments, the scene's labels remapped with
    ``data_path.remap_label`` (``RemapLabel(cfg.incr_label_remap)``, test.py:576-577), metrics over the known / incremental / remapped
    class sets.  ``cfg``: ``data.num_classes``, ``data.ignore_index``, ``data.test``, ``incr_label_remap``, ``incr_label_select``."""

    def __init__(self, step, cfg):
        learner = getattr(step, "learner", step)
        if isinstance(learner, torch.nn.Module) and any(hasattr(m, "make_geometry") and hasattr(m, "layers_by_level") for m in learner.modules()):
            raise NotImplementedError("IncrSegTester: a StratifiedTransformer learner -- the incremental stage is PointTransformer-V1 only "
                                      "(the reference has no ST incremental recipe); use OpenSegTester for ST-v1m1")
        learner.eval()

        def forward(batch):
            return learner({k: batch[k] for k in _BATCH_KEYS if k in batch})["seg_logits"], None

        data = _cfg_get(cfg, "data")
        remap = _cfg_get(cfg, "incr_label_remap") or getattr(step, "incr_label_remap", None)
        self.remap = {int(a): int(b) for a, b in dict(remap).items()}
        masks = evaluator.IncrSegEvaluator(int(_cfg_get(data, "num_classes")), self.remap, _cfg_get(cfg, "incr_label_select"),
                                           int(_cfg_get(data, "ignore_index", -1)))
        self.base_num_classes, self.mask_known = masks.base_num_classes, masks.mask_known
        self.incr_label_idx, self.mask_incr_remap, self.map_reverse = masks.incr_label_idx, masks.mask_incr_remap, masks.map_reverse
        super().__init__(cfg, masks.num_classes, forward, with_segment=False)

    def _labels(self, st):
        return data_path.remap_label(st["segment"], self.remap, ignore_index=self.ignore_index)[0]

    def _origin_labels(self, st):
        return data_path.remap_label(st["origin_segment"], self.remap, ignore_index=self.ignore_index)[0]

    def test(self, scenes, save_path=None):
        result_dir = self._result_dir(save_path)
        b, k, idx, r = self.base_num_classes, self.mask_known, self.incr_label_idx, self.mask_incr_remap
        isum, usum, tsum = (np.zeros(self.dim_pred) for _ in range(3))
        per_scene = {}
        for scene in scenes:
            name, pred, _, segment = self._scene(scene, result_dir, need_score=False)
            i, u, t, _ = self._metrics(pred, None, segment)
            isum, usum, tsum = isum + i, usum + u, tsum + t
            mask = u != 0                                                              # test.py:636-698
            iou = i / (u + 1e-10)
            mk = mask[:b] & k
            rec = dict(intersection=i, union=u, target=t,
                       mIoU_known=float(np.mean(iou[:b][mk])), allAcc_known=float(sum(i[:b][mk]) / (sum(t[:b][mk]) + 1e-10)),
                       running_mIoU_known=float(np.mean(isum[:b][k] / (usum[:b][k] + 1e-10))),
                       running_mAcc_known=float(np.mean(isum[:b][k] / (tsum[:b][k] + 1e-10))))
            incr_valid = bool(mask[b:].any())
            im = np.array(idx)[mask[b:b + len(idx)]]
            rec.update(mIoU_incr=float(np.mean(iou[im])) if incr_valid else -1.0,
                       allAcc_incr=float(sum(i[im]) / (sum(t[im]) + 1e-10)) if incr_valid else -1.0,
                       running_mIoU_incr=float(np.mean(isum[idx] / (usum[idx] + 1e-10))), running_mAcc_incr=float(np.mean(isum[idx] / (tsum[idx] + 1e-10))),
                       mIoU_remap=float(np.mean(iou[mask & r])), allAcc_remap=float(sum(i[mask & r]) / (sum(t[mask & r]) + 1e-10)),
                       running_mIoU_remap=float(np.mean(isum[r] / (usum[r] + 1e-10))), running_mAcc_remap=float(np.mean(isum[r] / (tsum[r] + 1e-10))))
            per_scene[name] = rec
        iou_class, acc_class = isum / (usum + 1e-10), isum / (tsum + 1e-10)             # test.py:794-814
        out = dict(iou_class=iou_class, acc_class=acc_class, intersection=isum, union=usum, target=tsum, scenes=per_scene)
        for tag, sel in (("known", lambda x: x[:b][k]), ("incr", lambda x: x[idx]), ("remap", lambda x: x[r])):
            out[f"mIoU_{tag}"] = float(np.mean(sel(iou_class)))
            out[f"mAcc_{tag}"] = float(np.mean(sel(acc_class)))
            out[f"allAcc_{tag}"] = float(sum(sel(isum)) / (sum(sel(tsum)) + 1e-10))
        return out

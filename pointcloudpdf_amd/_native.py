"""ctypes binding of the C ABI declared in include/pdfops.h.

``CBackend`` turns torch tensors into raw pointers + sizes and calls the C entry points.  The
product instance (``hip_backend()``) binds ``libpdfops.so`` (prefix ``pdf_``, device pointers, a
trailing hipStream_t).  There is NO CPU fallback in this package: if the library is missing or a
tensor is not on a ROCm device the call raises.  (The test-only oracle binds its own library
through the same class from ``oracle/``; nothing here imports it.)
"""
import ctypes
import os
import threading

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDFOPS_DIST_FMA=1|2: the library whose geometry kernels (kNN, ball query, FPS) evaluate the squared distance as an explicit FMA
# chain -- the arithmetic an `nvcc -O2` build of libs/pointops most likely runs (csrc/pdfops_common.h: pdf_sqdist3).
# Default: the as-written IEEE fp32 expression.
DIST_FMA = int(os.environ.get("PDFOPS_DIST_FMA", "0") or 0)
if DIST_FMA not in (0, 1, 2):
    raise RuntimeError(f"PDFOPS_DIST_FMA={DIST_FMA}: expected 0 (as written), 1 or 2 (csrc/pdfops_common.h)")


def library_path(dist_fma=0):
    return os.path.join(_HERE, "lib", "libpdfops.so" if not dist_fma else f"libpdfops_fma{int(dist_fma)}.so")


LIB_PATH = library_path(DIST_FMA)
ABI_VERSION = 22  # include/pdfops.h: PDF_ABI_VERSION (the rows of _abi.ENTRIES are THIS version's parameter lists)

c_int = ctypes.c_int
c_void_p = ctypes.c_void_p


class PdfOpsError(RuntimeError):
    pass


# default since round 3: the complete GPU suite (315 tests, incl. the 10-evaluation bit-reproducibility test) passes with it on;
# PDFOPS_RAW_STREAM=0 goes back through torch.cuda.current_stream()
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None) if os.environ.get("PDFOPS_RAW_STREAM", "1") != "0" else None


def raw_stream():
    """hipStream_t (as an integer) of torch's current stream on the current device.  ``torch.cuda.current_stream().cuda_stream`` builds a
    Stream object per call (~12 us; ~60 calls per training step); the raw accessor torch's own code generators use takes < 1 us."""
    dev = torch.cuda.current_device()
    return _RAW_STREAM(dev) if _RAW_STREAM is not None else torch.cuda.current_stream().cuda_stream


def cu_masked_stream(first_cu, n_cus, device=None):
    """A torch stream whose kernels run only on ``n_cus`` compute units starting at logical CU ``first_cu`` (hipExtStreamCreateWithCUMask).
    MI355X numbering, measured with tools/probes/cu_mask_probe.hip: mask bit i = CU (i // 8) of XCD (i % 8) -- consecutive bits go round
    the eight XCDs, so [first_cu, first_cu + n_cus) with both multiples of 8 takes the same CUs out of every XCD (a mask that leaves an XCD
    without any CU is not honoured: that XCD then runs on all of its CUs).  The stream is a BLOCKING stream in HIP's sense (the call has no
    flags): it synchronises implicitly with the legacy default stream, so nothing of a loop that uses it may run on that stream
    (engine.TrainStep(stream=...) keeps the whole step on its own stream).  The handle lives as long as the process."""
    if first_cu % 8 or n_cus % 8 or n_cus < 8:
        raise PdfOpsError("cu_masked_stream: first_cu and n_cus must be multiples of 8 (one CU of every XCD per step of 8)")
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    if first_cu + n_cus > total:
        raise PdfOpsError(f"cu_masked_stream: CUs [{first_cu}, {first_cu + n_cus}) of {total}")
    hip = ctypes.CDLL("libamdhip64.so")
    words = (total + 31) // 32
    mask = (ctypes.c_uint32 * words)()
    for cu in range(first_cu, first_cu + n_cus):
        mask[cu // 32] |= 1 << (cu % 32)
    handle = ctypes.c_void_p()
    with torch.cuda.device(dev):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(handle), ctypes.c_uint32(words), mask)
    if rc != 0:
        raise PdfOpsError(f"hipExtStreamCreateWithCUMask returned hipError {rc}")
    return torch.cuda.ExternalStream(handle.value, device=torch.device("cuda", dev))


def require_current_device(*tensors):
    """Every launch goes onto torch's current stream of the CURRENT device (the reference relies on
    ``torch.cuda.set_device(local_rank)`` the same way, engines/launch.py:131).  A tensor that lives on another GPU would be
    handed to a stream of the wrong device -- a fault, or a kernel unordered against the tensor's own stream -- so that is an
    error here, raised before anything is enqueued.  The public ``pointops`` ops switch devices themselves (CBackend._call)."""
    cur = None
    for t in tensors:
        if t is None or not t.is_cuda:
            continue
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise PdfOpsError(f"pointcloudpdf_amd: tensor on {t.device} but the current device is cuda:{cur}; call "
                              "torch.cuda.set_device(...) or wrap the call in torch.cuda.device(...)")


# ------------------------------------------------------------------------------------------------------------------
# Inverse neighbour tables (csrc/seg_gather.hip): entry ids of a table idx (m, nsample) grouped by destination row.
# Plumbing only (one stable device sort + one binary search per table); built once per table -- by the geometry pre-pass on
# its side stream for the tables the model uses, lazily here for any other idx tensor -- and cached on the idx tensor object.
# ------------------------------------------------------------------------------------------------------------------
_INV = "_pdf_inverse"


def attach_inverse(idx, n, table):
    setattr(idx, _INV, (idx.data_ptr(), idx._version, int(n), table))
    return table


def inverse_table(idx, n):
    """-> (inv_off (n + 1) int32, inv_entry int32, entry_base int) for idx (m, nsample) int32 with values in [-1, n)."""
    cached = getattr(idx, _INV, None)
    if cached is not None and cached[0] == idx.data_ptr() and cached[1] == idx._version and cached[2] == int(n):
        return cached[3]
    flat = idx.reshape(-1)
    vals, perm = torch.sort(flat, stable=True)        # ascending destination, ascending entry id inside a destination; -1 first
    off = torch.searchsorted(vals, torch.arange(int(n) + 1, device=idx.device, dtype=vals.dtype), out_int32=True)
    return attach_inverse(idx, n, (off, perm.to(torch.int32), 0))


_CSC = "_pdf_window_csc"
_WORDER = "_pdf_window_order"   # on the CSR offsets of a window edge table: the queries sorted by fine-window key (int32 permutation)


def window_order_of(offsets):
    """The visiting order ``HipBackend.window_edges`` left on a table's CSR offsets (queries window by window), or None."""
    tag = getattr(offsets, _WORDER, None)
    if tag is not None and tag[0] == offsets.data_ptr() and tag[1] == offsets._version and tag[2].shape[0] == offsets.shape[0] - 1:
        return tag[2]
    return None


def window_csc(index1, offsets, rel_idx=None, n_keys=None):
    """The window-attention edge list grouped by KEY (csrc/window_attention_bwd.hip): for index1 (M) int32 = key of every edge and the
    CSR offsets (N + 1) of the queries -> (key_off (N + 1) int32, key_edge (M) int32: edge ids grouped by key in ascending order,
    key_q (M) int32: the query of those edges[, key_rel (M, 3) int32: their rel_idx rows]).  Coordinate-only, so the pre-pass of a
    window partition builds it once (stratified.BasicLayer.window_tables) and every block / step reuses it: cached on ``index1``."""
    cache = getattr(index1, _CSC, None)
    if cache is None or cache["key"] != (index1.data_ptr(), index1._version, offsets.data_ptr(), offsets._version):
        n, m = offsets.shape[0] - 1, index1.shape[0]
        nk = n if n_keys is None else int(n_keys)
        vals, perm = torch.sort(index1, stable=True)
        key_off = torch.searchsorted(vals, torch.arange(nk + 1, device=index1.device, dtype=vals.dtype), out_int32=True)
        counts = (offsets[1:] - offsets[:-1]).long()
        index0 = torch.repeat_interleave(torch.arange(n, device=index1.device, dtype=torch.int32), counts, output_size=m)
        cache = {"key": (index1.data_ptr(), index1._version, offsets.data_ptr(), offsets._version),
                 "base": (key_off, perm.to(torch.int32), index0[perm].contiguous()), "perm": perm, "rel": {}}
        # Visiting order of the KEY-side row passes: the rows by key are long (a down-sampled point is a key of every query of its coarse
        # window: ~10x the entries) or short; owners that share a workgroup walk their rows in lockstep, so equal lengths belong together:
        # longest first, window by window inside a length (the window order of the table when the edge builder left one).  Level 0 of
        # config 5: grad_k 305 -> 152 us, grad_v 106 -> 59 us per call (tools/probes/wa_bwd_probe.py).
        if nk == n:
            wo = window_order_of(offsets)
            base = wo.long() if wo is not None else torch.arange(nk, device=index1.device)
            klen = (key_off[1:] - key_off[:-1]).index_select(0, base)
            cache["order"] = base.index_select(0, torch.sort(klen, descending=True, stable=True)[1]).to(torch.int32)
        setattr(index1, _CSC, cache)
    if rel_idx is None:
        return cache["base"]
    rk = (rel_idx.data_ptr(), rel_idx._version)
    if rk not in cache["rel"]:
        cache["rel"] = {rk: rel_idx[cache["perm"]].contiguous()}   # (one table per edge list in practice; a new one replaces the old)
    return cache["base"] + (cache["rel"][rk],)


def window_key_order(index1):
    """The key-side visiting order ``window_csc`` cached on ``index1`` (longest rows first, window by window), or None."""
    cache = getattr(index1, _CSC, None)
    return cache.get("order") if cache is not None and cache["key"][:2] == (index1.data_ptr(), index1._version) else None


_ORD = "_pdf_order"


def attach_order(idx, order, src_order=None):
    """Remember a visiting order of the QUERIES of a neighbour table (a permutation of its rows: the Morton order of the query points,
    Geometry.order) on the idx tensor; the forward gathers then walk the queries in that order (csrc/gather_ops.hip, *_ord kernels).
    ``src_order``: the same for the SOURCE rows (the destinations of the backward's segmented gathers)."""
    setattr(idx, _ORD, (idx.data_ptr(), idx._version, order, src_order))
    return idx


def src_order_of(idx, n):
    tag = getattr(idx, _ORD, None)
    if tag is not None and tag[0] == idx.data_ptr() and tag[1] == idx._version and tag[3] is not None and tag[3].shape[0] == n:
        return tag[3]
    return None


def order_of(idx):
    tag = getattr(idx, _ORD, None)
    if tag is not None and tag[0] == idx.data_ptr() and tag[1] == idx._version and tag[2].shape[0] == idx.shape[0]:
        return tag[2]
    return None


_MOM = "_pdf_moments"


def attach_moments(idx, moments):
    """Remember the batch's relative-coordinate sums of a SELF neighbour table (9 doubles on the device: csrc/geom_moments.hip) on
    its idx tensor; the fused layer's forward then takes the geometry branch's BatchNorm statistics from them."""
    setattr(idx, _MOM, (idx.data_ptr(), idx._version, moments))
    return idx


def moments_of(idx):
    tag = getattr(idx, _MOM, None)
    if tag is not None and tag[0] == idx.data_ptr() and tag[1] == idx._version:
        return tag[2]
    return None


def _check(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


class CBackend:
    """Calls a C library that implements the pdfops ABI on tensors of one device kind."""

    # the reference kernels ACCUMULATE into interpolation / aggregation / subtraction outputs, so its wrappers pre-zero them
    # (interpolation.py:39, aggregation.py:21); a backend whose kernels overwrite those outputs skips the fill
    overwrites_outputs = False

    def __init__(self, lib, prefix, device_type, use_stream, extra_protos=(), proto_overrides=None):
        """Binds the reference launchers and the short names in ``extra_protos`` (None: every row of the table) from ``_abi.ENTRIES``;
        ``proto_overrides``: short name -> the kinds of a launcher whose parameter list differs in ``lib``."""
        self.lib = lib
        self.prefix = prefix
        self.device_type = device_type
        self.use_stream = use_stream
        names = None if extra_protos is None else _abi.REFERENCE_OPS + tuple(extra_protos)
        self._fn = _abi.bind(lib, names, prefix, use_stream, proto_overrides)

    # -- plumbing -------------------------------------------------------------------------------
    def _ptr(self, t):
        if t.device.type != self.device_type:
            raise PdfOpsError(
                f"pointcloudpdf_amd: tensor on '{t.device}' but this backend runs on '{self.device_type}' "
                "(the HIP path has no CPU fallback)"
            )
        return t.data_ptr()

    def _launch(self, name, *args, unsupported_ok=False):
        """The one launch path: ``args`` are raw already (ints, floats, None, ``data_ptr()`` integers, ctypes arrays; the prototype
        converts them), the current stream is appended, a non-zero status raises.  No per-argument work and no device check: a
        caller that takes tensors of any device goes through ``_call``, one that must not calls ``require_current_device`` first.
        ``unsupported_ok``: PDF_ERR_UNSUPPORTED (-3) is returned instead, for the callers that have another path for the shape."""
        rc = self._fn[name](*args, raw_stream()) if self.use_stream else self._fn[name](*args)
        if rc != 0 and not (unsupported_ok and rc == -3):
            raise PdfOpsError(f"{self.prefix}{name} failed with status {rc}")
        return rc

    def _call(self, name, *args):
        """``_launch`` on tensors: every tensor becomes its pointer, and the launch goes to the tensors' device."""
        conv, dev = [], None
        for a in args:
            if isinstance(a, torch.Tensor):
                conv.append(self._ptr(a))
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise PdfOpsError(f"{self.prefix}{name}: tensors on different devices ({dev}, {a.device})")
            else:
                conv.append(a)
        if self.use_stream and dev is not None and dev.index != torch.cuda.current_device():
            # the stream must belong to the tensors' device (and per-device kernel attributes are set for the current one)
            with torch.cuda.device(dev):
                self._launch(name, *conv)
        else:
            self._launch(name, *conv)

    def _new(self, like, shape, dtype, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=like.device)

    # -- reference ops ----------------------------------------------------------------------------
    def knn_query(self, nsample, xyz, new_xyz, offset, new_offset):
        """-> idx (m, nsample) int32, dist2 (m, nsample) f32 (squared).  knn_query_cuda, query.py:19-23."""
        _check(xyz, torch.float32, "xyz"); _check(new_xyz, torch.float32, "new_xyz")
        _check(offset, torch.int32, "offset"); _check(new_offset, torch.int32, "new_offset")
        if not 1 <= nsample <= 128:
            raise ValueError("nsample must be in 1..128")
        m = new_xyz.shape[0]
        idx = self._new(xyz, (m, nsample), torch.int32)
        dist2 = self._new(xyz, (m, nsample), torch.float32)
        if self.use_stream:
            self._call("knn_query", m, nsample, xyz, new_xyz, offset, new_offset, offset.shape[0], idx, dist2)
        else:
            self._call("knn_query", m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2)
        return idx, dist2

    def ball_query(self, nsample, max_radius, min_radius, xyz, new_xyz, offset, new_offset, order=None):
        """-> idx (m, nsample) int32, dist2 (m, nsample) f32.  ball_query_cuda / random_ball_query_cuda (``order`` given),
        query.py:48-64, 96-111."""
        _check(xyz, torch.float32, "xyz"); _check(new_xyz, torch.float32, "new_xyz")
        _check(offset, torch.int32, "offset"); _check(new_offset, torch.int32, "new_offset")
        if not min_radius < max_radius:
            raise ValueError("min_radius must be below max_radius")
        if not 1 <= nsample <= 2048:
            raise ValueError("nsample must be in 1..2048")
        m = new_xyz.shape[0]
        idx = self._new(xyz, (m, nsample), torch.int32)
        dist2 = self._new(xyz, (m, nsample), torch.float32)
        head = [m, nsample, float(min_radius), float(max_radius)]
        name = "ball_query"
        if order is not None:
            _check(order, torch.int32, "order")
            head.append(order)
            name = "random_ball_query"
        tail = [offset.shape[0], idx, dist2] if self.use_stream else [idx, dist2]
        self._call(name, *head, xyz, new_xyz, offset, new_offset, *tail)
        return idx, dist2

    def farthest_point_sampling(self, xyz, offset, new_offset, n_max, m_total):
        """-> idx (m_total,) int32.  farthest_point_sampling_cuda, sampling.py:18-22."""
        _check(xyz, torch.float32, "xyz")
        _check(offset, torch.int32, "offset"); _check(new_offset, torch.int32, "new_offset")
        idx = self._new(xyz, (m_total,), torch.int32, zero=True)
        tmp = torch.full((xyz.shape[0],), 1e10, dtype=torch.float32, device=xyz.device)
        self._call("farthest_point_sampling", offset.shape[0], int(n_max), xyz, offset, new_offset, tmp, idx)
        return idx

    def grouping_forward(self, input, idx):
        _check(input, torch.float32, "input"); _check(idx, torch.int32, "idx")
        m, ns = idx.shape
        c = input.shape[1]
        out = self._new(input, (m, ns, c), torch.float32)
        self._call("grouping_forward", m, ns, c, input, idx, out)
        return out

    def grouping_backward(self, grad_output, idx, n):
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx")
        m, ns, c = grad_output.shape
        gi = self._new(grad_output, (n, c), torch.float32, zero=True)
        self._call("grouping_backward", m, ns, c, grad_output, idx, gi)
        return gi

    def interpolation_forward(self, input, idx, weight):
        _check(input, torch.float32, "input"); _check(idx, torch.int32, "idx"); _check(weight, torch.float32, "weight")
        n, k = idx.shape
        c = input.shape[1]
        out = self._new(input, (n, c), torch.float32, zero=not self.overwrites_outputs)
        self._call("interpolation_forward", n, c, k, input, idx, weight, out)
        return out

    def interpolation_backward(self, grad_output, idx, weight, m):
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx"); _check(weight, torch.float32, "weight")
        n, c = grad_output.shape
        k = idx.shape[1]
        gi = self._new(grad_output, (m, c), torch.float32, zero=True)
        self._call("interpolation_backward", n, c, k, grad_output, idx, weight, gi)
        return gi

    def subtraction_forward(self, input1, input2, idx):
        _check(input1, torch.float32, "input1"); _check(input2, torch.float32, "input2"); _check(idx, torch.int32, "idx")
        n, c = input1.shape
        ns = idx.shape[-1]
        out = self._new(input1, (n, ns, c), torch.float32, zero=not self.overwrites_outputs)
        self._call("subtraction_forward", n, ns, c, input1, input2, idx, out)
        return out

    def subtraction_backward(self, idx, grad_output, n2=None):
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx")
        n, ns, c = grad_output.shape
        g1 = self._new(grad_output, (n, c), torch.float32, zero=True)
        g2 = self._new(grad_output, (n if n2 is None else n2, c), torch.float32, zero=True)
        self._call("subtraction_backward", n, ns, c, idx, grad_output, g1, g2)
        return g1, g2

    def aggregation_forward(self, input, position, weight, idx):
        for t, nm in ((input, "input"), (position, "position"), (weight, "weight")):
            _check(t, torch.float32, nm)
        _check(idx, torch.int32, "idx")
        n, ns, c = position.shape
        w_c = weight.shape[-1]
        out = self._new(input, (n, c), torch.float32, zero=not self.overwrites_outputs)
        self._call("aggregation_forward", n, ns, c, w_c, input, position, weight, idx, out)
        return out

    def aggregation_backward(self, input, position, weight, idx, grad_output):
        _check(grad_output, torch.float32, "grad_output")
        n, ns, c = position.shape
        w_c = weight.shape[-1]
        gi = self._new(input, tuple(input.shape), torch.float32, zero=True)
        gp = self._new(input, (n, ns, c), torch.float32, zero=not self.overwrites_outputs)
        gw = self._new(input, (n, ns, w_c), torch.float32, zero=True)
        self._call("aggregation_backward", n, ns, c, w_c, input, position, weight, idx, grad_output, gi, gp, gw)
        return gi, gp, gw

    def attention_relation_step_forward(self, query, key, weight, index_target, index_refer):
        for t, nm in ((query, "query"), (key, "key"), (weight, "weight")):
            _check(t, torch.float32, nm)
        _check(index_target, torch.int32, "index_target"); _check(index_refer, torch.int32, "index_refer")
        _, g, c = query.shape
        m = index_target.shape[0]
        out = self._new(query, (m, g), torch.float32, zero=True)
        self._call("attention_relation_step_forward", m, g, c, query, key, weight, index_target, index_refer, out)
        return out

    def attention_relation_step_backward(self, query, key, weight, index_target, index_refer, grad_output):
        _check(grad_output, torch.float32, "grad_output")
        n, g, c = query.shape
        m = index_target.shape[0]
        gq = self._new(query, (n, g, c), torch.float32, zero=True)
        gk = self._new(query, tuple(key.shape), torch.float32, zero=True)
        gw = self._new(query, (c,), torch.float32, zero=True)
        self._call("attention_relation_step_backward", m, g, c, query, gq, key, gk, weight, gw,
                   index_target, index_refer, grad_output)
        return gq, gk, gw

    def attention_fusion_step_forward(self, weight, value, index_target, index_refer):
        _check(weight, torch.float32, "weight"); _check(value, torch.float32, "value")
        _check(index_target, torch.int32, "index_target"); _check(index_refer, torch.int32, "index_refer")
        n, g, c = value.shape
        m = index_refer.shape[0]
        out = self._new(value, (n, g, c), torch.float32, zero=True)
        self._call("attention_fusion_step_forward", m, g, c, weight, value, index_target, index_refer, out)
        return out

    def attention_fusion_step_backward(self, weight, value, index_target, index_refer, grad_output):
        _check(grad_output, torch.float32, "grad_output")
        n, g, c = value.shape
        m = index_target.shape[0]
        gw = self._new(value, (m, g), torch.float32, zero=True)
        gv = self._new(value, (n, g, c), torch.float32, zero=True)
        self._call("attention_fusion_step_backward", m, g, c, weight, gw, value, gv, index_target, index_refer, grad_output)
        return gw, gv


    # -- libs/pointops2 window attention ---------------------------------------------------------------
    def attention_step1_v2(self, q, k, index1, offsets, n_max):
        """-> attn (M, h).  AttentionStep1_v2.forward, libs/pointops2/functions/pointops.py:170-199."""
        _check(q, torch.float32, "q"); _check(k, torch.float32, "k")
        _check(index1, torch.int32, "index1"); _check(offsets, torch.int32, "index0_offsets")
        n, h, d = q.shape
        m = index1.shape[0]
        if offsets.shape[0] != n + 1:
            raise ValueError("index0_offsets must have N + 1 entries")
        attn = self._new(q, (m, h), torch.float32)
        self._call("attention_step1_forward_v2", n, m, h, h * d, int(n_max), q, k, offsets, index1, attn)
        return attn

    def attention_step1_v2_backward(self, grad_out, q, k, index1, offsets, n_max):
        _check(grad_out, torch.float32, "grad_output")
        n, h, d = q.shape
        m = index1.shape[0]
        gq = self._new(q, tuple(q.shape), torch.float32)
        gk = self._new(q, tuple(k.shape), torch.float32, zero=True)
        self._call("attention_step1_backward_v2", n, m, h, h * d, int(n_max), grad_out, offsets, index1, q, k, gq, gk)
        return gq, gk

    def dot_prod_with_idx_v3(self, q, offsets, n_max, k, index_k, table_q, table_k, rel_idx):
        """-> out (M, h).  DotProdWithIdx_v3.forward, pointops.py:632-676."""
        for t, nm in ((q, "q"), (k, "k"), (table_q, "table_q"), (table_k, "table_k")):
            _check(t, torch.float32, nm)
        for t, nm in ((offsets, "index_q_offsets"), (index_k, "index_k"), (rel_idx, "rel_idx")):
            _check(t, torch.int32, nm)
        n, h, d = q.shape
        m = index_k.shape[0]
        if offsets.shape[0] != n + 1 or table_q.shape != table_k.shape or tuple(table_q.shape[1:]) != (h, d, 3):
            raise ValueError("dot_prod_with_idx_v3: inconsistent shapes")
        out = self._new(q, (m, h), torch.float32)
        if self.use_stream:   # HIP: per-head kernels with the table slabs in LDS (table length instead of n_max)
            self._call("dot_prod_with_idx_forward_v3_l", n, m, h, d, int(table_q.shape[0]), q, offsets, k, index_k, table_q, table_k, rel_idx, out)
        else:
            self._call("dot_prod_with_idx_forward_v3", n, m, h, d, int(n_max), q, offsets, k, index_k, table_q, table_k, rel_idx, out)
        return out

    def dot_prod_with_idx_v3_backward(self, grad_out, q, offsets, n_max, k, index_k, table_q, table_k, rel_idx):
        _check(grad_out, torch.float32, "grad_output")
        n, h, d = q.shape
        m = index_k.shape[0]
        gq = self._new(q, tuple(q.shape), torch.float32)
        gk = self._new(q, tuple(k.shape), torch.float32, zero=True)
        gtq = self._new(q, tuple(table_q.shape), torch.float32, zero=True)
        gtk = self._new(q, tuple(table_k.shape), torch.float32, zero=True)
        name, x = ("dot_prod_with_idx_backward_v3_l", int(table_q.shape[0])) if self.use_stream else ("dot_prod_with_idx_backward_v3", int(n_max))
        self._call(name, n, m, h, d, x, grad_out, q, offsets, k, index_k, table_q, table_k, rel_idx, gq, gk, gtq, gtk)
        return gq, gk, gtq, gtk

    def attention_step2_with_rel_pos_value_v2(self, attn, v, offsets, n_max, index1, table, rel_idx):
        """-> out (N, h, d).  AttentionStep2WithRelPosValue_v2.forward, pointops.py:854-895."""
        for t, nm in ((attn, "attn"), (v, "v"), (table, "table")):
            _check(t, torch.float32, nm)
        for t, nm in ((offsets, "index0_offsets"), (index1, "index1"), (rel_idx, "rel_idx")):
            _check(t, torch.int32, nm)
        m, h = attn.shape
        n, _, d = v.shape
        if offsets.shape[0] != n + 1 or tuple(table.shape[1:]) != (h, d, 3):
            raise ValueError("attention_step2_with_rel_pos_value_v2: inconsistent shapes")
        out = self._new(v, (n, h, d), torch.float32)
        self._call("attention_step2_with_rel_pos_value_forward_v2", n, m, h, d, int(n_max), attn, v, offsets, index1, table, rel_idx, out)
        return out

    def attention_step2_with_rel_pos_value_v2_backward(self, grad_out, attn, v, offsets, n_max, index1, table, rel_idx):
        _check(grad_out, torch.float32, "grad_output")
        m, h = attn.shape
        n, _, d = v.shape
        ga = self._new(v, (m, h), torch.float32, zero=True)
        gv = self._new(v, (n, h, d), torch.float32, zero=True)
        gt = self._new(v, tuple(table.shape), torch.float32, zero=True)
        name, x = (("attention_step2_with_rel_pos_value_backward_v2_l", int(table.shape[0])) if self.use_stream
                   else ("attention_step2_with_rel_pos_value_backward_v2", int(n_max)))
        self._call(name, n, m, h, d, x, grad_out, offsets, index1, attn, v, table, rel_idx, ga, gv, gt)
        return ga, gv, gt


    def segment_softmax(self, x, offsets):
        """-> y (M, h): softmax over the edges of every query, per head (scatter_softmax for a CSR-ordered index)."""
        _check(x, torch.float32, "src"); _check(offsets, torch.int32, "index0_offsets")
        m, h = x.shape
        if h > 64:
            raise ValueError("segment_softmax: at most 64 heads")
        y = self._new(x, (m, h), torch.float32)
        self._call("segment_softmax_forward", offsets.shape[0] - 1, m, h, offsets, x, y)
        return y

    def segment_softmax_backward(self, y, grad_y, offsets):
        _check(grad_y, torch.float32, "grad_output")
        m, h = y.shape
        gx = self._new(y, (m, h), torch.float32)
        self._call("segment_softmax_backward", offsets.shape[0] - 1, m, h, offsets, y, grad_y, gx)
        return gx


class HipBackend(CBackend):
    """libpdfops.so on the current ROCm device; adds the fused entry points."""

    overwrites_outputs = True

    def __init__(self, lib):
        _abi.bind(lib, ("abi_version",))   # first, alone: a stale library may lack a symbol that a later row names
        got = int(lib.pdf_abi_version())
        if got != ABI_VERSION:   # parameter lists differ between versions: calling through would hand shifted arguments to the kernels
            raise PdfOpsError(f"libpdfops ABI {got} != {ABI_VERSION} expected by pointcloudpdf_amd/_native.py (include/pdfops.h: PDF_ABI_VERSION): "
                              "stale library -- rebuild with `python -m pointcloudpdf_amd.build --force`")
        super().__init__(lib, "pdf_", "cuda", True, extra_protos=None)
        self.CopySeg = _abi.PdfCopySeg
        self.collect_fps_stats = False  # debug: keep the work counters of the last bucketed FPS call (forces a sync)
        self.last_fps_stats = None
        self.fps_mode = os.environ.get("PDFOPS_FPS", "bucketed")  # "bucketed" | "plain"
        self.knn_mode = os.environ.get("PDFOPS_KNN", "grid")      # "grid" | "scan"

    KNN_GRID_MAX_SCENES = 64
    # scatter-adds of the gather family as segmented gathers over inverse tables (PDFOPS_INVERSE=0: the atomic kernels, for A/B runs)
    use_inverse = os.environ.get("PDFOPS_INVERSE", "1") != "0"
    # reduced-precision variant (the reference trains under AMP, engines/train.py:343-356): the fused PointTransformerLayer keeps the
    # row arrays only it reads -- H (saved), G2 / Wsm / GR (backward scratch) -- as bfloat16; sums, products, statistics, parameters and
    # every tensor that crosses the layer boundary stay fp32.  Set per process (PDFOPS_STORAGE=bf16) or with set_storage().
    storage_bf16 = os.environ.get("PDFOPS_STORAGE", "f32") == "bf16"

    def set_storage(self, kind):
        if kind not in ("f32", "bf16"):
            raise ValueError("storage: 'f32' or 'bf16'")
        self.storage_bf16 = kind == "bf16"

    # forward gathers: queries visited in the order attached to the idx tensor (Geometry: Morton order of the query level), if any
    def grouping_forward(self, input, idx):
        _check(input, torch.float32, "input"); _check(idx, torch.int32, "idx")
        m, ns = idx.shape
        c = input.shape[1]
        out = self._new(input, (m, ns, c), torch.float32)
        self._call("grouping_forward_ordered", m, ns, c, input, idx, order_of(idx), out)
        return out

    def interpolation_forward(self, input, idx, weight):
        _check(input, torch.float32, "input"); _check(idx, torch.int32, "idx"); _check(weight, torch.float32, "weight")
        n, k = idx.shape
        c = input.shape[1]
        out = self._new(input, (n, c), torch.float32)
        self._call("interpolation_forward_ordered", n, c, k, input, idx, weight, order_of(idx), out)
        return out

    def subtraction_forward(self, input1, input2, idx):
        _check(input1, torch.float32, "input1"); _check(input2, torch.float32, "input2"); _check(idx, torch.int32, "idx")
        n, c = input1.shape
        ns = idx.shape[-1]
        out = self._new(input1, (n, ns, c), torch.float32)
        self._call("subtraction_forward_ordered", n, ns, c, input1, input2, idx, order_of(idx), out)
        return out

    def aggregation_forward(self, input, position, weight, idx):
        for t, nm in ((input, "input"), (position, "position"), (weight, "weight")):
            _check(t, torch.float32, nm)
        _check(idx, torch.int32, "idx")
        n, ns, c = position.shape
        out = self._new(input, (n, c), torch.float32)
        self._call("aggregation_forward_ordered", n, ns, c, weight.shape[-1], input, position, weight, idx, order_of(idx), out)
        return out

    def grouping_backward(self, grad_output, idx, n):
        if not self.use_inverse:
            return super().grouping_backward(grad_output, idx, n)
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx")
        m, ns, c = grad_output.shape
        if grad_output.numel() == 0 or n == 0:
            return self._new(grad_output, (n, c), torch.float32, zero=True)
        off, ent, base = inverse_table(idx, n)
        gi = self._new(grad_output, (n, c), torch.float32)
        self._call("seg_sum_rows", n, c, grad_output, off, ent, base, 1.0, gi)
        return gi

    def interpolation_backward(self, grad_output, idx, weight, m):
        if not self.use_inverse:
            return super().interpolation_backward(grad_output, idx, weight, m)
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx"); _check(weight, torch.float32, "weight")
        n, c = grad_output.shape
        if grad_output.numel() == 0 or m == 0:
            return self._new(grad_output, (m, c), torch.float32, zero=True)
        off, ent, base = inverse_table(idx, m)
        gi = self._new(grad_output, (m, c), torch.float32)
        self._call("seg_sum_weighted_ordered", m, c, idx.shape[1], 1, grad_output, weight, off, ent, base, src_order_of(idx, m), gi)
        return gi

    def subtraction_backward(self, idx, grad_output, n2=None):
        if not self.use_inverse:
            return super().subtraction_backward(idx, grad_output, n2)
        _check(grad_output, torch.float32, "grad_output"); _check(idx, torch.int32, "idx")
        n, ns, c = grad_output.shape
        n2 = n if n2 is None else n2
        if grad_output.numel() == 0 or n2 == 0:
            return super().subtraction_backward(idx, grad_output, n2)
        off, ent, base = inverse_table(idx, n2)
        g2 = self._new(grad_output, (n2, c), torch.float32)
        if n == n2 and c % 4 == 0 and self.fuse_own_rows:   # self table: both sums in one walk over the gradient (csrc/seg_gather.hip)
            g1 = self._new(grad_output, (n, c), torch.float32)
            self._call("seg_sum_rows_own", n2, c, ns, grad_output, off, ent, base, -1.0, src_order_of(idx, n2), g2, g1)
            return g1, g2
        g1 = self._new(grad_output, (n, c), torch.float32, zero=True)
        self._call("subtraction_backward", n, ns, c, idx, grad_output, g1, None)       # row sums only
        self._call("seg_sum_rows", n2, c, grad_output, off, ent, base, -1.0, g2)
        return g1, g2

    fuse_own_rows = os.environ.get("PDFOPS_FUSE_OWN_ROWS", "1") != "0"   # 0: two passes over the gradient (rounds 2-3; A/B runs)

    def aggregation_backward(self, input, position, weight, idx, grad_output):
        if not self.use_inverse:
            return super().aggregation_backward(input, position, weight, idx, grad_output)
        _check(grad_output, torch.float32, "grad_output")
        n, ns, c = position.shape
        w_c = weight.shape[-1]
        if position.numel() == 0 or input.shape[0] == 0:
            return super().aggregation_backward(input, position, weight, idx, grad_output)
        off, ent, base = inverse_table(idx, input.shape[0])
        gi = self._new(input, tuple(input.shape), torch.float32)
        gp = self._new(input, (n, ns, c), torch.float32)
        gw = self._new(input, (n, ns, w_c), torch.float32, zero=True)
        self._call("aggregation_backward", n, ns, c, w_c, input, position, weight, idx, grad_output, None, gp, gw)
        self._call("seg_sum_weighted_ordered", input.shape[0], c, ns, w_c, grad_output, weight, off, ent, base, src_order_of(idx, input.shape[0]), gi)
        return gi, gp, gw

    def knn_grid(self, xyz, offset, m_max):
        """The uniform grid over the source points ``xyz`` (csrc/knn_grid.hip) as a workspace tensor that ``knn_query(..., grid=)`` takes for
        any query set of up to ``m_max`` points and nsample 3 / 8 / 16; None where the grid path does not apply."""
        n, b = xyz.shape[0], offset.shape[0]
        if self.knn_mode == "scan" or b > self.KNN_GRID_MAX_SCENES or n < 1:
            return None
        _check(xyz, torch.float32, "xyz"); _check(offset, torch.int32, "offset")
        require_current_device(xyz, offset)
        nbytes = int(self.lib.pdf_knn_workspace_bytes(b, n, int(max(m_max, n))))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        self._launch("knn_grid_build", n, self._ptr(xyz), self._ptr(offset), b, self._ptr(ws), nbytes)
        return ws

    def knn_query(self, nsample, xyz, new_xyz, offset, new_offset, grid=None):
        if grid is not None and self.lib.pdf_knn_grid_supported(int(nsample)) and new_xyz.shape[0] > 0:
            _check(new_xyz, torch.float32, "new_xyz"); _check(new_offset, torch.int32, "new_offset")
            require_current_device(xyz, new_xyz, offset, new_offset)
            n, m, b = xyz.shape[0], new_xyz.shape[0], offset.shape[0]
            if int(self.lib.pdf_knn_workspace_bytes(b, n, m)) > grid.numel():
                raise PdfOpsError("knn_query: the grid workspace was built for fewer queries")
            idx = self._new(xyz, (m, nsample), torch.int32)
            dist2 = self._new(xyz, (m, nsample), torch.float32)
            self._launch("knn_query_grid", m, int(nsample), n, self._ptr(xyz), self._ptr(new_xyz), self._ptr(offset), self._ptr(new_offset), b,
                         self._ptr(idx), self._ptr(dist2), self._ptr(grid), grid.numel())
            return idx, dist2
        if self.knn_mode == "scan" or not self.lib.pdf_knn_grid_supported(int(nsample)):
            return super().knn_query(nsample, xyz, new_xyz, offset, new_offset)
        _check(xyz, torch.float32, "xyz"); _check(new_xyz, torch.float32, "new_xyz")
        _check(offset, torch.int32, "offset"); _check(new_offset, torch.int32, "new_offset")
        n, m, b = xyz.shape[0], new_xyz.shape[0], offset.shape[0]
        if b > self.KNN_GRID_MAX_SCENES:   # the grid workspace holds <= 64 scenes; beyond, the C side scans anyway (no workspace)
            return super().knn_query(nsample, xyz, new_xyz, offset, new_offset)
        require_current_device(xyz, new_xyz, offset, new_offset)
        idx = self._new(xyz, (m, nsample), torch.int32)
        dist2 = self._new(xyz, (m, nsample), torch.float32)
        nbytes = int(self.lib.pdf_knn_workspace_bytes(b, n, m))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        self._launch("knn_query_ws", m, int(nsample), n, self._ptr(xyz), self._ptr(new_xyz), self._ptr(offset),
                     self._ptr(new_offset), b, self._ptr(idx), self._ptr(dist2), self._ptr(ws), nbytes)
        return idx, dist2

    def scene_morton_keys(self, xyz, offset):
        """-> keys (n,) int64: scene << 30 | Morton code on the scene's own bounding box (include/pdfops.h: pdf_scene_morton_keys)."""
        _check(xyz, torch.float32, "xyz"); _check(offset, torch.int32, "offset")
        require_current_device(xyz, offset)
        n, b = xyz.shape[0], offset.shape[0]
        keys = torch.empty((n,), dtype=torch.int64, device=xyz.device)
        bounds = torch.empty((4 * b,), dtype=torch.float32, device=xyz.device)
        self._launch("scene_morton_keys", n, b, self._ptr(xyz), self._ptr(offset), self._ptr(bounds), self._ptr(keys))
        return keys

    def knn_query_counted(self, nsample, xyz, new_xyz, offset, new_offset):
        """Measurement aid: the grid kNN with its kernel counting the candidate distances it evaluates -> (idx, dist2, evaluated pairs)
        (one host read-back).  tools/ops_roofline.py prices the kernel against the fp32 vector peak with this count."""
        n, m, b = xyz.shape[0], new_xyz.shape[0], offset.shape[0]
        require_current_device(xyz, new_xyz, offset, new_offset)
        idx = self._new(xyz, (m, nsample), torch.int32)
        dist2 = self._new(xyz, (m, nsample), torch.float32)
        nbytes = int(self.lib.pdf_knn_workspace_bytes(b, n, m))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        pairs = torch.zeros((1,), dtype=torch.int64, device=xyz.device)
        self._launch("knn_query_ws_counted", m, int(nsample), n, self._ptr(xyz), self._ptr(new_xyz), self._ptr(offset),
                     self._ptr(new_offset), b, self._ptr(idx), self._ptr(dist2), self._ptr(ws), nbytes, self._ptr(pairs))
        return idx, dist2, int(pairs.item())

    def farthest_point_sampling(self, xyz, offset, new_offset, n_max, m_total):
        if self.fps_mode == "plain":
            return super().farthest_point_sampling(xyz, offset, new_offset, n_max, m_total)
        _check(xyz, torch.float32, "xyz")
        _check(offset, torch.int32, "offset"); _check(new_offset, torch.int32, "new_offset")
        b, n_total = offset.shape[0], xyz.shape[0]
        idx = self._new(xyz, (m_total,), torch.int32, zero=True)
        nbytes = int(self.lib.pdf_fps_workspace_bytes(b, n_total))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        self._call("farthest_point_sampling_bucketed", b, int(n_max), n_total, xyz, offset, new_offset, ws, nbytes, idx)
        if self.collect_fps_stats:
            o = int(self.lib.pdf_fps_stats_offset(b, n_total))
            self.last_fps_stats = ws[o:o + 16 * b].view(torch.int32).view(b, 4).cpu()
        return idx

    # -- fused PointTransformerLayer -----------------------------------------------------------------
    def pt_layer_supported(self, nsample, c):
        return bool(self.lib.pdf_pt_layer_supported(int(nsample), int(c)))

    @staticmethod
    def _ptr_array(tensors):
        return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])

    def pt_layer_forward(self, xq, xk, xv, p, idx, weights, bn_params, bn_buffers, training, eps, momentum):
        """-> out (N,C), ctx tensors (bn scale/shift, saved mean/rstd, H).  See include/pdfops.h."""
        n, c = xq.shape
        k = idx.shape[1]
        cs = c // 8
        for t in (xq, xk, xv, p, *weights, *bn_params):
            _check(t, torch.float32, "pt_layer tensor")
        _check(idx, torch.int32, "idx")
        require_current_device(xq, xk, xv, p, idx)
        bn = self._new(xq, (2 * (3 + c + cs),), torch.float32)
        saved = self._new(xq, (2 * (3 + c + cs),), torch.float32)
        H = self._new(xq, (n, k, cs), torch.float32)
        partial = self._new(xq, (int(self.lib.pdf_pt_layer_partial_floats(n, k, c)),), torch.float32)
        out = self._new(xq, (n, c), torch.float32)
        self._launch(
            "pt_layer_forward", n, k, c, self._ptr(xq), self._ptr(xk), self._ptr(xv), self._ptr(p), self._ptr(idx),
            self._ptr_array(weights), self._ptr_array(bn_params), self._ptr_array(bn_buffers), int(bool(training)),
            eps, momentum, self._ptr(bn), self._ptr(saved), self._ptr(H),
            self._ptr(partial), self._ptr(out), self.layer_flags(self.storage_bf16), self._order_ptr(idx))
        return out, bn, saved, H

    # visiting order of the points in the fused layer passes (PDFOPS_LAYER_ORDER=0: storage order, for A/B runs)
    layer_order = os.environ.get("PDFOPS_LAYER_ORDER", "0") == "1"     # measured: no gain (22.3 vs 22.1 ms per step), the passes are not
    layer_chunked = os.environ.get("PDFOPS_LAYER_CHUNKED", "0") == "1"  # bound by where their rows come from -- both off by default

    def layer_flags(self, bf16):
        """the `storage_bf16` argument of the layer entry points: bit 0 = bfloat16 row arrays, bit 1 = chunked point walk"""
        return int(bool(bf16)) | (2 if self.layer_chunked else 0) | (4 if self.layer_order else 0)

    use_moments = os.environ.get("PDFOPS_BNP_MOMENTS", "1") != "0"   # 0: the layer's own first statistics pass (P1) instead

    def _moments_ptr(self, idx):
        m = moments_of(idx) if self.use_moments else None
        return None if m is None else m.data_ptr()

    def knn_rel_moments(self, nsample, xyz, offset, idx, new_xyz=None):
        """Per-scene sums (b, 9) float64 of rel = xyz[idx] - new_xyz over the rows of a kNN table (csrc/geom_moments.hip); ``offset`` =
        scene ends of the QUERIES; ``new_xyz`` None = a self table."""
        q = xyz if new_xyz is None else new_xyz
        _check(xyz, torch.float32, "xyz"); _check(q, torch.float32, "new_xyz"); _check(offset, torch.int32, "offset"); _check(idx, torch.int32, "idx")
        out = torch.empty((offset.shape[0], 9), dtype=torch.float64, device=xyz.device)
        ws = torch.empty((max(int(self.lib.pdf_knn_rel_moments_ws_doubles(int(offset.shape[0]), int(q.shape[0]))), 1),), dtype=torch.float64, device=xyz.device)
        require_current_device(xyz, q, offset, idx)
        self._launch("knn_rel_moments_q", int(offset.shape[0]), int(q.shape[0]), int(nsample), xyz.data_ptr(), q.data_ptr(), offset.data_ptr(),
                     idx.data_ptr(), out.data_ptr(), ws.data_ptr())
        return out

    def _order_ptr(self, idx):
        o = order_of(idx)   # (always handed over: the g_xv gather visits its destinations in this order; the passes only with bit 2)
        return None if o is None else o.data_ptr()

    def pt_layer_backward(self, xq, xk, xv, p, idx, weights, bn, saved, H, gout, storage_bf16=None):
        n, c = xq.shape
        k = idx.shape[1]
        cs = c // 8
        _check(gout, torch.float32, "gout")
        require_current_device(xq, gout)
        gxq = self._new(xq, (n, c), torch.float32)
        gxk = self._new(xq, (n, c), torch.float32)
        gxv = self._new(xq, (n, c), torch.float32)
        G2 = self._new(xq, (n * k * cs,), torch.float32)
        G3 = self._new(xq, (n * k * 3,), torch.float32)
        Wsm = self._new(xq, (n * k * cs,), torch.float32)
        GR = self._new(xq, (n * k * c,), torch.float32)
        inv_off, inv_entry, entry_base = inverse_table(idx, n)
        partial = self._new(xq, (int(self.lib.pdf_pt_layer_bwd_partial_floats(n, k, c)),), torch.float32)
        nsum = int(self.lib.pdf_pt_layer_bwd_sums_floats(c))
        sums = self._new(xq, (nsum + 2 * (3 + c + cs),), torch.float32)
        self._launch(
            "pt_layer_backward", n, k, c, self._ptr(xq), self._ptr(xk), self._ptr(xv), self._ptr(p), self._ptr(idx),
            self._ptr_array(weights), self._ptr(bn), self._ptr(saved), self._ptr(H), self._ptr(gout),
            self._ptr(gxq), self._ptr(gxk), self._ptr(gxv), self._ptr(G2), self._ptr(G3), self._ptr(Wsm), self._ptr(GR),
            self._ptr(inv_off), self._ptr(inv_entry), int(entry_base), self._ptr(partial),
            self._ptr(sums), self.layer_flags(self.storage_bf16 if storage_bf16 is None else storage_bf16), self._order_ptr(idx),
            self._moments_ptr(idx))
        # unpack the parameter-gradient sections (layout: csrc/fused_layer.hip, pdf_pt_layer_backward)
        o1 = 0
        o2 = o1 + 3 * cs + cs * cs
        o3 = o2 + 2 * c + cs + cs * c
        o4 = o3 + 8 + 4 * c
        g = dict(
            beta2=sums[o1:o1 + cs], gamma2=sums[o1 + cs:o1 + 2 * cs], bw2=sums[o1 + 2 * cs:o1 + 3 * cs],
            Ww2=sums[o1 + 3 * cs:o2].view(cs, cs),
            beta1=sums[o2:o2 + c], gamma1=sums[o2 + c:o2 + 2 * c], bw1=sums[o2 + 2 * c:o2 + 2 * c + cs],
            Ww1=sums[o2 + 2 * c + cs:o3].view(cs, c),
            betap=sums[o3:o3 + 3], gammap=sums[o3 + 3:o3 + 6], bp2=sums[o3 + 8:o3 + 8 + c],
            Wp2=sums[o3 + 8 + c:o4].view(c, 3),
            bp1=sums[o4:o4 + 3], Wp1=sums[o4 + 3:o4 + 12].view(3, 3),
        )
        return gxq, gxk, gxv, g

    # -- dense per-point Linear on the matrix cores (csrc/rowlin.hip) ---------------------------------------
    # -- libs/pointops2 window attention, backward: atomic-free segmented sums (csrc/window_attention_bwd.hip) ---------------------
    # False: the fp32-atomic launchers of csrc/window_attention.hip for every shape (the independent implementation the tests compare
    # against; other shapes take them anyway)
    wa_atomic_free = True

    def _wa_ok(self, d, L, *tensors):
        return self.wa_atomic_free and d == 16 and L <= 64 and all(t.data_ptr() % 16 == 0 for t in tensors)

    def _wa_rows(self, n, h, d, L, seg_off, seg_edge, other, rel, w, X, table, out, ldx=None, xscale=1.0, ldo=None, oscale=1.0, order=None):
        """pdf_wa_segment_rows[_ordered]; X / out may be column slices of wider rows (ldx / ldo = their row strides in floats); ``order``:
        visiting order of the owners (int32 permutation) or None."""
        c = h * d
        if order is not None and (order.shape[0] != n or order.dtype != torch.int32):
            order = None
        self._call("wa_segment_rows_ordered", n, h, d, L, seg_off, seg_edge, other, rel, w, X, c if ldx is None else int(ldx), float(xscale), table, out,
                   c if ldo is None else int(ldo), float(oscale), order)

    def _wa_permute(self, w, edge):
        """w (M, h) float32 -> w[edge] (torch's index_select takes 25-95 us for these 12-96-byte rows; this is one pass at copy speed)"""
        w = w.contiguous()
        _check(w, torch.float32, "edge scalars"); _check(edge, torch.int32, "edge ids")
        out = torch.empty((edge.shape[0], w.shape[1]), dtype=torch.float32, device=w.device)
        self._call("wa_permute_edges", int(edge.shape[0]), int(w.shape[1]), w, edge, out)
        return out

    def _wa_table_grad(self, n, h, d, L, seg_off, seg_edge, rel, w, x, like, ldx=None, xscale=1.0):
        g = torch.empty((L, h, d, 3), dtype=torch.float32, device=like.device)
        ws = torch.empty((max(int(self.lib.pdf_wa_table_grad_ws_floats(n, h, L)), 1),), dtype=torch.float32, device=like.device)
        self._call("wa_table_grad", n, h, d, L, seg_off, seg_edge, rel, w, x, h * d if ldx is None else int(ldx), float(xscale), ws, g)
        return g

    def attention_step1_v2_backward(self, grad_out, q, k, index1, offsets, n_max):
        n, h, d = q.shape
        if index1.shape[0] == 0 or not self._wa_ok(d, 1, q, k):
            return super().attention_step1_v2_backward(grad_out, q, k, index1, offsets, n_max)
        _check(grad_out, torch.float32, "grad_output")
        key_off, key_edge, key_q = window_csc(index1, offsets, n_keys=k.shape[0])
        gq, gk = torch.empty_like(q), torch.empty_like(k)
        self._wa_rows(n, h, d, 0, offsets, None, index1, None, grad_out, k, None, gq)                      # grad_q = sum g k[index1]
        self._wa_rows(k.shape[0], h, d, 0, key_off, key_edge, key_q, None, grad_out, q, None, gk)          # grad_k = sum g q[query]
        return gq, gk

    def dot_prod_with_idx_v3_backward(self, grad_out, q, offsets, n_max, k, index_k, table_q, table_k, rel_idx):
        n, h, d = q.shape
        L = int(table_q.shape[0])
        if index_k.shape[0] == 0 or not self._wa_ok(d, L, q, k):
            return super().dot_prod_with_idx_v3_backward(grad_out, q, offsets, n_max, k, index_k, table_q, table_k, rel_idx)
        _check(grad_out, torch.float32, "grad_output")
        nk = k.shape[0]
        key_off, key_edge, _key_q, key_rel = window_csc(index_k, offsets, rel_idx, n_keys=nk)
        g_key = self._wa_permute(grad_out, key_edge)   # (the edge scalars in key order, once: two kernels read them sequentially)
        gq, gk = torch.empty_like(q), torch.empty_like(k)
        self._wa_rows(n, h, d, L, offsets, None, None, rel_idx, grad_out, None, table_q, gq)               # grad_q = sum g T_q
        self._wa_rows(nk, h, d, L, key_off, None, None, key_rel, g_key, None, table_k, gk)                 # grad_k = sum g T_k
        gtq = self._wa_table_grad(n, h, d, L, offsets, None, rel_idx, grad_out, q, q)
        gtk = self._wa_table_grad(nk, h, d, L, key_off, None, key_rel, g_key, k, q)
        return gq, gk, gtq, gtk

    def attention_step2_with_rel_pos_value_v2(self, attn, v, offsets, n_max, index1, table, rel_idx):
        """out[q] = sum over the query's edges of attn * (v[index1] + T): the same segmented pass as the backward's row sums (lane = (query,
        16-byte piece), 8 edges in flight) instead of the lane-per-channel walk of csrc/window_attention.hip (235 -> 120 us per call)."""
        m, h = attn.shape
        n, _, d = v.shape
        L = int(table.shape[0])
        if m == 0 or offsets.shape[0] != n + 1 or not self._wa_ok(d, L, v):
            return super().attention_step2_with_rel_pos_value_v2(attn, v, offsets, n_max, index1, table, rel_idx)
        for t, nm in ((attn, "attn"), (v, "v"), (table, "table")):
            _check(t, torch.float32, nm)
        for t, nm in ((offsets, "index0_offsets"), (index1, "index1"), (rel_idx, "rel_idx")):
            _check(t, torch.int32, nm)
        if tuple(table.shape[1:]) != (h, d, 3):
            raise ValueError("attention_step2_with_rel_pos_value_v2: inconsistent shapes")
        out = torch.empty((n, h, d), dtype=torch.float32, device=v.device)
        self._wa_rows(n, h, d, L, offsets, None, index1, rel_idx, attn, v, table, out)
        return out

    def window_keys(self, xyz, ends, lo, hi, window_size, parity, per_scene=False):
        """(kf, kc, wk) int64 per point of one window partition (csrc/window_edges.hip we::k_keys; what stratified.window_keys composes from
        ~45 torch ops): xyz (N, 3), ends (scenes) int32 scene ends, lo / hi (3) float32 = per-axis minimum / maximum of xyz.
        ``per_scene``: lo / hi (scenes, 3) (``scene_bounds``), every scene partitioned from its own origin (we::k_keys_scene; what
        stratified.window_keys_scene composes)."""
        n, scenes = int(xyz.shape[0]), int(ends.shape[0])
        if tuple(lo.shape) != ((scenes, 3) if per_scene else (3,)) or lo.shape != hi.shape:
            raise ValueError(f"window_keys: lo / hi of shape {tuple(lo.shape)} / {tuple(hi.shape)} for {scenes} scenes, per_scene={per_scene}")
        out = torch.empty((3, n), dtype=torch.int64, device=xyz.device)
        self._call("window_keys_scene" if per_scene else "window_keys", n, xyz.contiguous(), ends.int().contiguous(), scenes,
                   lo.float().contiguous(), hi.float().contiguous(), float(window_size), int(parity), out[0], out[1], out[2])
        return out[0], out[1], out[2]

    def scene_bounds(self, xyz, ends):
        """(lo, hi) (scenes, 3) float32: per-axis minimum / maximum of every scene's rows of xyz (N, 3) float32 -- one launch, no host
        read (csrc/window_edges.hip we::k_scene_bounds); ends (scenes) int32 ascending scene ends, the last one = N."""
        _check(xyz, torch.float32, "xyz")
        scenes = int(ends.shape[0])
        out = torch.empty((2, scenes, 3), dtype=torch.float32, device=xyz.device)
        self._call("scene_bounds", int(xyz.shape[0]), xyz.contiguous(), ends.int().contiguous(), scenes, out[0], out[1])
        return out[0], out[1]

    def window_edges(self, xyz, kf, kc, wk, downsample_idx, c2w, qs, vmax):
        """The CSR-by-query edge table of one window partition (csrc/window_edges.hip; stratified_transformer_v1m1_origin.py:45-127 + the
        sort by query of :468-536 + :282-292).  kf / kc / wk (N) int64: fine-window key, coarse-window key, packed fine-window cell of every
        point; downsample_idx: the FPS key subset.  -> index_0 (E) int64 ascending, index_1 (E) int32, offsets (N + 1) int32, n_max (int),
        rel_idx (E, 3) int32, flag (1) int32 device tensor (non-zero: a quantised offset left [0, vmax] -- the caller asserts).
        Two point-sized stable sorts (torch / rocPRIM), two launches, ONE host read (edge count + longest row)."""
        n, dev = int(xyz.shape[0]), xyz.device
        i32 = dict(dtype=torch.int32, device=dev)
        kf, kc, wk = kf.contiguous(), kc.contiguous(), wk.contiguous()
        kf_sorted, order_f = torch.sort(kf, stable=True)
        ds = torch.sort(downsample_idx.long())[0]
        kcd_sorted, perm = torch.sort(kc[ds], stable=True)
        order_cd = ds[perm]
        wkd = wk[order_cd].contiguous()
        m = int(ds.shape[0])
        count = torch.empty(n, **i32)
        seg = torch.empty((n, 4), **i32)
        self._call("window_edges_count", n, kf_sorted, kf, m, kcd_sorted, kc, wk, wkd, count, seg)
        offsets = torch.zeros(n + 1, **i32)
        torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
        e, n_max = (int(v) for v in torch.stack([offsets[-1], count.max() if n else offsets[-1]]).tolist())   # the one host read
        index0 = torch.empty(e, dtype=torch.int64, device=dev)
        index1 = torch.empty(e, **i32)
        rel = torch.empty((e, 3), **i32)
        flag = torch.zeros(1, **i32)
        order32 = order_f.int()
        self._call("window_edges_fill", n, offsets, seg, order32, order_cd.int(), wk, wkd, xyz.contiguous(), float(c2w), float(qs), int(vmax),
                   index0, index1, rel, flag)
        # the queries window by window: the visiting order of the attention's segmented row passes (queries / keys of one window gather
        # the same rows: pdf_wa_segment_rows_ordered)
        setattr(offsets, _WORDER, (offsets.data_ptr(), offsets._version, order32))
        return index0, index1, offsets, n_max, rel, flag

    def window_logits_supported(self, q, k, table_q):
        return self.wa_atomic_free and q.shape[0] == k.shape[0] and self._wa_ok(q.shape[2], int(table_q.shape[0]), q, k)

    def window_logits(self, q, k, index1, offsets, table_q, table_k, rel_idx):
        """attention_step1_v2(q, k) + dot_prod_with_idx_v3(q, k, table_q, table_k) as ONE pass over the key rows -> (M, h)."""
        n, h, d = q.shape
        m = index1.shape[0]
        out = torch.empty((m, h), dtype=torch.float32, device=q.device)
        self._call("wa_logits_forward", n, m, h, d, int(table_q.shape[0]), q, k, h * d, 1.0, offsets, index1, table_q, table_k, rel_idx, out)
        return out

    def window_logits_backward(self, g, q, k, index1, offsets, table_q, table_k, rel_idx):
        """-> (grad_q, grad_k, grad_table_q, grad_table_k): the sums of the two ops' gradients, each as ONE segmented pass (rows + table term
        together); the edge scalars are brought into key order once for the two key-side kernels."""
        n, h, d = q.shape
        L = int(table_q.shape[0])
        key_off, key_edge, key_q, key_rel = window_csc(index1, offsets, rel_idx, n_keys=n)
        g_key = self._wa_permute(g, key_edge)
        gq, gk = torch.empty_like(q), torch.empty_like(k)
        self._wa_rows(n, h, d, L, offsets, None, index1, rel_idx, g, k, table_q, gq)          # sum g (k[index1] + T_q)
        self._wa_rows(n, h, d, L, key_off, None, key_q, key_rel, g_key, q, table_k, gk)       # sum g (q[query] + T_k)
        gtq = self._wa_table_grad(n, h, d, L, offsets, None, rel_idx, g, q, q)
        gtk = self._wa_table_grad(n, h, d, L, key_off, None, key_rel, g_key, k, q)
        return gq, gk, gtq, gtk

    def attention_step2_with_rel_pos_value_v2_backward(self, grad_out, attn, v, offsets, n_max, index1, table, rel_idx):
        m, h = attn.shape
        n, _, d = v.shape
        L = int(table.shape[0])
        if m == 0 or offsets.shape[0] != n + 1 or not self._wa_ok(d, L, v, grad_out):
            return super().attention_step2_with_rel_pos_value_v2_backward(grad_out, attn, v, offsets, n_max, index1, table, rel_idx)
        _check(grad_out, torch.float32, "grad_output")
        c = h * d
        key_off, key_edge, key_q = window_csc(index1, offsets, n_keys=n)
        ga = torch.empty((m, h), dtype=torch.float32, device=v.device)
        gv = torch.empty_like(v)
        self._call("wa_grad_attn", n, m, h, d, L, grad_out, c, offsets, index1, v, c, table, rel_idx, ga)
        self._wa_rows(n, h, d, 0, key_off, key_edge, key_q, None, attn, grad_out, None, gv)                # grad_v = sum attn grad_out[query]
        gt = self._wa_table_grad(n, h, d, L, offsets, None, rel_idx, attn, grad_out, v)
        return ga, gv, gt

    # The whole attention core of WindowAttention.forward (stratified_transformer_v1m1_origin.py:296-341) on the (N, 3 C) output of the
    # qkv Linear: q / k / v are read as column slices (no permute copy), the query scale rides on the kernels, and the backward writes
    # the three gradients into the slices of one (N, 3 C) buffer.
    def window_attention_core_supported(self, qkv, table_q, table_k, table_v):
        L, h, d, _ = table_q.shape
        return (self.wa_atomic_free and qkv.dim() == 2 and qkv.shape[1] == 3 * h * d and table_k.shape == table_q.shape == table_v.shape
                and qkv.dtype == torch.float32 and qkv.is_contiguous() and self._wa_ok(d, L, qkv) and (h * d) % 4 == 0)

    def window_attention_core(self, qkv, index1, offsets, table_q, table_k, table_v, rel_idx, scale):
        """-> (out (N, C), attn (M, h) after the softmax)."""
        n = qkv.shape[0]
        L, h, d, _ = table_q.shape
        c, m = h * d, index1.shape[0]
        q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
        logits = torch.empty((m, h), dtype=torch.float32, device=qkv.device)
        self._call("wa_logits_forward_ordered", n, m, h, d, L, q, k, 3 * c, float(scale), offsets, index1, table_q, table_k, rel_idx, logits,
                   window_order_of(offsets))
        attn = self.segment_softmax(logits, offsets)
        out = torch.empty((n, c), dtype=torch.float32, device=qkv.device)
        self._wa_rows(n, h, d, L, offsets, None, index1, rel_idx, attn, v, table_v, out, ldx=3 * c, order=window_order_of(offsets))
        return out, attn

    def window_attention_core_backward(self, go, qkv, attn, index1, offsets, table_q, table_k, table_v, rel_idx, scale):
        """-> (grad_qkv (N, 3 C), grad_table_q, grad_table_k, grad_table_v)"""
        n = qkv.shape[0]
        L, h, d, _ = table_q.shape
        c, m = h * d, index1.shape[0]
        q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
        key_off, key_edge, key_q, key_rel = window_csc(index1, offsets, rel_idx, n_keys=n)
        gqkv = torch.empty_like(qkv)
        ga = torch.empty((m, h), dtype=torch.float32, device=qkv.device)
        order = window_order_of(offsets)   # (query side: window by window)
        self._call("wa_grad_attn_ordered", n, m, h, d, L, go, c, offsets, index1, v, 3 * c, table_v, rel_idx, ga, order)
        attn_key = self._wa_permute(attn, key_edge)
        korder = window_key_order(index1)   # (key side: longest rows first, window by window)
        self._wa_rows(n, h, d, 0, key_off, None, key_q, None, attn_key, go, None, gqkv[:, 2 * c:], ldo=3 * c, order=korder)          # grad_v
        gtv = self._wa_table_grad(n, h, d, L, offsets, None, rel_idx, attn, go, qkv)
        g = self.segment_softmax_backward(attn, ga, offsets)
        g_key = self._wa_permute(g, key_edge)
        self._wa_rows(n, h, d, L, offsets, None, index1, rel_idx, g, k, table_q, gqkv[:, :c], ldx=3 * c, ldo=3 * c, oscale=scale, order=order)      # grad_q
        self._wa_rows(n, h, d, L, key_off, None, key_q, key_rel, g_key, q, table_k, gqkv[:, c:2 * c], ldx=3 * c, xscale=scale, ldo=3 * c, order=korder)   # grad_k
        gtq = self._wa_table_grad(n, h, d, L, offsets, None, rel_idx, g, q, qkv, ldx=3 * c, xscale=scale)
        gtk = self._wa_table_grad(n, h, d, L, key_off, None, key_rel, g_key, k, qkv, ldx=3 * c)
        return gqkv, gtq, gtk, gtv

    def _stream(self):
        return c_void_p(raw_stream())

    def openset_metrics(self, logits, pred, score, target, ignore, unknown, k):
        """-> (hist (3, k) int64: intersection | union | target, record (4) float64: aupr, auroc, n_pos, n_neg) on the inputs' device
        (pdf_openset_metrics; csrc/openset_metrics.hip).  Exactly one of ``logits`` (n, c) float32 and ``pred`` (n) int64; ``score`` (n)
        float32 or None; ``unknown``: (k) uint8 on the device or None.  No host read; every byte of the workspace is written before it is
        read, so nothing is zeroed and a captured call holds no memset node."""
        if (logits is None) == (pred is None):
            raise ValueError("openset_metrics: exactly one of logits and pred")
        x = logits if pred is None else pred
        _check(x, torch.float32 if pred is None else torch.int64, "logits" if pred is None else "pred")
        _check(target, torch.int64, "target")
        if score is not None:
            _check(score, torch.float32, "score")
        if unknown is not None:
            _check(unknown, torch.uint8, "unknown")
            if unknown.numel() != k:
                raise ValueError(f"openset_metrics: the unknown-class mask has {unknown.numel()} bytes for {k} classes")
        n, c = x.shape[0], (x.shape[1] if pred is None else 0)
        if target.numel() != n or (score is not None and score.numel() != n):
            raise ValueError("openset_metrics: logits / pred, score and target must have one row count")
        require_current_device(x, score, target, unknown)
        hist = torch.empty((3, k), dtype=torch.int64, device=x.device)
        record = torch.empty((4,), dtype=torch.float64, device=x.device)
        ws = torch.empty((max(int(self.lib.pdf_openset_metrics_workspace_bytes(n, c)), 8),), dtype=torch.uint8, device=x.device)
        self._launch("openset_metrics", n, c, None if logits is None else logits.data_ptr(), None if pred is None else pred.data_ptr(),
                     None if score is None else score.data_ptr(), target.data_ptr(), int(ignore),
                     None if unknown is None else unknown.data_ptr(), int(k), hist.data_ptr(), record.data_ptr(), ws.data_ptr())
        return hist, record

    def rowlin(self, x, w, bias=None, coef=None, relu=False, transpose_w=False, out=None, accumulate=False, stats=False):
        """y = f(x) @ Wt + bias (see include/pdfops.h); x (n,k) with row stride x.stride(0); returns (y, partial|None)."""
        n, k = x.shape
        o = w.shape[1] if transpose_w else w.shape[0]
        y = out if out is not None else torch.empty((n, o), dtype=torch.float32, device=x.device)
        partial = None
        if stats:
            partial = torch.empty((int(self.lib.pdf_rowlin_partial_floats(n, o)),), dtype=torch.float32, device=x.device)
            partial._pdf_rows = int(self.lib.pdf_rowlin_partial_rows(n, k, o))
        self._launch("rowlin_forward", n, k, o, x.data_ptr(), x.stride(0), w.data_ptr(), int(transpose_w),
                     None if bias is None else bias.data_ptr(),
                     None if coef is None else coef.data_ptr(),
                     None if coef is None else coef.data_ptr() + 4 * k, int(relu), y.data_ptr(), y.stride(0),
                     int(accumulate), None if partial is None else partial.data_ptr(), current_mma_input())
        return y, partial

    @staticmethod
    def _ptrs(tensors, n=3):
        return (c_void_p * n)(*[t.data_ptr() if t is not None else None for t in list(tensors) + [None] * (n - len(tensors))])

    def rowlin_multi(self, xs, ws, biases=None, coef=None, relu=False, transpose_w=False, nout=1):
        """nout = 3: [f(xs[0]) @ Wt_i + b_i]; nout = 1: [sum_i xs[i] @ Wt_i (+ b_0)]   (pdf_rowlin_multi)"""
        n, k = xs[0].shape
        o = ws[0].shape[1] if transpose_w else ws[0].shape[0]
        ys = [torch.empty((n, o), dtype=torch.float32, device=xs[0].device) for _ in range(nout)]
        self._launch("rowlin_multi", n, k, o, len(xs), nout, self._ptrs(xs), xs[0].stride(0), self._ptrs(ws), int(transpose_w),
                     None if biases is None else self._ptrs(biases),
                     None if coef is None else coef.data_ptr(), None if coef is None else coef.data_ptr() + 4 * k,
                     int(relu), self._ptrs(ys), o, 0, current_mma_input())
        return ys

    def rowlin_dgrad_bn_backward(self, gs, ws, bx, coef, training=True, relu=True):
        """Input gradient sum_i gs[i] @ ws[i] of Linear layers reading relu(bn(bx)), followed by that BatchNorm's backward with the
        reduction pass folded into the product's epilogue (pdf_rowlin_dgrad_bstats + pdf_bn_act_backward_presummed).
        -> (d bx, d gamma, d beta), or None when the streaming kernels do not cover the shape."""
        n, k = gs[0].shape
        o = ws[0].shape[1]
        require_current_device(bx, *gs)
        dy = self._new(bx, (n, o), torch.float32)
        partial = self._new(bx, (int(self.lib.pdf_rowlin_partial_floats(n, o)),), torch.float32)
        rows = c_int(0)
        sums = self._new(bx, (2 * o,), torch.float32)
        if self._launch("rowlin_dgrad_bstats", n, k, o, len(gs), self._ptrs(gs), gs[0].stride(0), self._ptrs(ws), dy.data_ptr(), o,
                        bx.data_ptr(), bx.stride(0), coef.data_ptr(), int(bool(relu)), partial.data_ptr(),
                        ctypes.byref(rows), current_mma_input(), unsupported_ok=True):
            return None
        self._launch("bn_act_backward_presummed", n, o, dy.data_ptr(), bx.data_ptr(), coef.data_ptr(), int(bool(training)), int(bool(relu)),
                     partial.data_ptr(), rows.value, sums.data_ptr(), dy.data_ptr())
        return dy, sums[o:], sums[:o]

    def wgrad_workspace(self, n, k, o, ng, device):
        """Slab workspace of the weight-gradient entry points (fixed-order reduction instead of float atomics)."""
        return torch.empty((max(int(self.lib.pdf_rowlin_wgrad_ws_floats(int(n), int(k), int(o), int(ng))), 1),), dtype=torch.float32, device=device)

    def rowlin_wgrad_multi(self, gs, x, coef, relu):
        n, o = gs[0].shape
        k = x.shape[1]
        dws = [torch.empty((o, k), dtype=torch.float32, device=x.device) for _ in gs]
        dbs = [torch.empty((o,), dtype=torch.float32, device=x.device) for _ in gs]
        ws = self.wgrad_workspace(n, k, o, len(gs), x.device)
        self._launch("rowlin_wgrad_multi", n, k, o, len(gs), self._ptrs(gs), gs[0].stride(0), x.data_ptr(), x.stride(0),
                     None if coef is None else coef.data_ptr(), None if coef is None else coef.data_ptr() + 4 * k,
                     int(relu), self._ptrs(dws), self._ptrs(dbs), ws.data_ptr(), current_mma_input())
        return dws, dbs

    # -- rigid KPConv of the StratifiedTransformer stem (csrc/kpconv.hip): gather-accumulate and its adjoint
    def kpconv_supported(self, kp, cin):
        return bool(self.lib.pdf_kpconv_supported(int(kp), int(cin)))

    def kpconv_gather(self, query, support, neighbors, x, k_points, extent):
        """-> weighted (N, KP * C_in): per query and kernel point the influence-weighted sum of its neighbours' feature rows."""
        n, m = neighbors.shape
        kp, cin = k_points.shape[0], x.shape[1]
        out = torch.empty((n, kp * cin), dtype=torch.float32, device=x.device)
        self._launch("kpconv_gather", n, m, kp, cin, query.data_ptr(), support.data_ptr(), neighbors.data_ptr(), x.data_ptr(),
                     k_points.data_ptr(), extent, out.data_ptr())
        return out

    def kpconv_scatter(self, query, support, neighbors, grad_weighted, k_points, extent, rows, cin):
        """-> grad_x (rows, C_in): the adjoint of kpconv_gather."""
        n, m = neighbors.shape
        gx = torch.zeros((rows, cin), dtype=torch.float32, device=grad_weighted.device)
        self._launch("kpconv_scatter", n, m, k_points.shape[0], cin, query.data_ptr(), support.data_ptr(), neighbors.data_ptr(),
                     grad_weighted.data_ptr(), k_points.data_ptr(), extent, gx.data_ptr())
        return gx

    def rowlin_wgrad_group(self, gs, xs, coefs, relus, need_bias):
        """Up to five weight gradients of one shape with their own inputs in one launch + one reduction (include/pdfops.h:
        pdf_rowlin_wgrad_group): dW_i = G_i^T f_i(X_i), f_i = relu_i?(x * scale_i + shift_i) for a coef_i = [scale | shift | ...], else the
        identity.  -> (list of dW, list of db | None); None when the shape is outside the streaming kernels."""
        n, o = gs[0].shape
        k = xs[0].shape[1]
        dev = gs[0].device
        dws = [torch.empty((o, k), dtype=torch.float32, device=dev) for _ in gs]
        dbs = [torch.empty((o,), dtype=torch.float32, device=dev) if nb else None for nb in need_bias]
        ws = self.wgrad_workspace(n, k, o, len(gs), dev)
        P = lambda ts: (c_void_p * len(ts))(*[None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])
        sc = [None if cf is None else cf.data_ptr() for cf in coefs]
        sh = [None if cf is None else cf.data_ptr() + 4 * k for cf in coefs]
        if self._launch("rowlin_wgrad_group", n, k, o, len(gs), P(gs), gs[0].stride(0), P(xs), xs[0].stride(0), P(sc), P(sh),
                        (c_int * len(gs))(*[int(bool(r)) for r in relus]), P(dws), P(dbs), ws.data_ptr(), current_mma_input(), unsupported_ok=True):
            return None
        return dws, dbs

    def rowlin_wgrad(self, g, x, coef, relu, need_bias):
        n, o = g.shape
        k = x.shape[1]
        dw = torch.empty((o, k), dtype=torch.float32, device=x.device)
        db = torch.empty((o,), dtype=torch.float32, device=x.device) if need_bias else None
        ws = self.wgrad_workspace(n, k, o, 1, x.device)
        self._launch("rowlin_wgrad", n, k, o, g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0),
                     None if coef is None else coef.data_ptr(),
                     None if coef is None else coef.data_ptr() + 4 * k, int(relu), dw.data_ptr(),
                     None if db is None else db.data_ptr(), ws.data_ptr(), current_mma_input())
        return dw, db

    def bn_coef_from_partial(self, partial, n, c, bn, training):
        """coef (4c) = scale|shift|mean|rstd of BatchNorm ``bn`` from rowlin column partials (training) or running stats."""
        coef = torch.empty((4 * c,), dtype=torch.float32, device=partial.device if partial is not None else bn.weight.device)
        if training:
            rows = partial._pdf_rows
            self._launch("bn_coef_from_partial", partial.data_ptr(), rows, n, c, bn.weight.data_ptr(), bn.bias.data_ptr(),
                         bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.eps, bn.momentum, coef.data_ptr())
        else:
            rstd = torch.rsqrt(bn.running_var + bn.eps)
            sc = bn.weight.detach() * rstd
            coef = torch.cat([sc, bn.bias.detach() - bn.running_mean * sc, bn.running_mean, rstd])
        return coef

    def bn_coef(self, x, bn, training):
        """coef (4c) of BatchNorm ``bn`` over the rows of x: batch statistics (training, updates running stats) or running."""
        n, c = x.shape
        coef = torch.empty((4 * c,), dtype=torch.float32, device=x.device)
        partial = torch.empty((int(self.lib.pdf_bn_partial_floats(n, c)),), dtype=torch.float32, device=x.device) if training else None
        self._launch("bn_coef", n, c, x.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                     bn.running_var.data_ptr(), int(bool(training)), bn.eps, bn.momentum, coef.data_ptr(),
                     None if partial is None else partial.data_ptr())
        return coef

    def bn_apply(self, x, res, coef, relu):
        n, c = x.shape
        y = torch.empty_like(x)
        self._launch("bn_apply", n, c, x.data_ptr(), None if res is None else res.data_ptr(), coef.data_ptr(), int(relu), y.data_ptr())
        return y

    def td_tables(self, p_src, p_new, idx, new_offset, inverse=None):
        """Geometry-only tables of the fused TransitionDown: rel4 (m,16,4), Z (n,32), scene_sums (b,16) (csrc/transition_down.hip).
        ``inverse`` = (inv_off, inv_entry, entry_base) of idx: Z is then summed in destination order (bit-reproducible)."""
        m, n, b = p_new.shape[0], p_src.shape[0], new_offset.shape[0]
        rel4 = torch.empty((m, 16, 4), dtype=torch.float32, device=p_src.device)
        Z = torch.zeros((n, 32), dtype=torch.float32, device=p_src.device)
        sums = torch.zeros((b, 16), dtype=torch.float32, device=p_src.device)
        off, ent, base = inverse if inverse is not None else (None, None, 0)
        self._launch("td_tables", m, b, p_src.data_ptr(), p_new.data_ptr(), idx.data_ptr(), new_offset.data_ptr(), rel4.data_ptr(), Z.data_ptr(),
                     sums.data_ptr(), n, None if off is None else off.data_ptr(), None if ent is None else ent.data_ptr(), int(base))
        return rel4, Z, sums

    # -- whole Bottleneck as one host call per direction (csrc/block.hip); thin methods so that bench.py can time them
    def bottleneck_forward(self, n, k, c, ptrs, training, eps, momentum, storage_bf16=0):
        self._launch("bottleneck_forward", n, k, c, (c_void_p * len(ptrs))(*ptrs), int(training), eps, momentum,
                     self.layer_flags(storage_bf16), current_mma_input())

    def bottleneck_backward(self, n, k, c, ptrs, training, entry_base=0, storage_bf16=0):
        self._launch("bottleneck_backward", n, k, c, (c_void_p * len(ptrs))(*ptrs), int(training), int(entry_base),
                     self.layer_flags(storage_bf16), current_mma_input())

    # -- Bottleneck halves as single host calls (csrc/block.hip) -------------------------------------------
    def _ptable(self, tensors):
        return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])

    def block_call(self, name, n, c, tensors, training, eps=None, momentum=None):
        if eps is None:
            self._launch("block_" + name, n, c, self._ptable(tensors), int(bool(training)), current_mma_input())
        else:
            self._launch("block_" + name, n, c, self._ptable(tensors), int(bool(training)), eps, momentum, current_mma_input())

    # -- BatchNorm + residual + ReLU over (n, c) rows ------------------------------------------------------
    def bn_supported(self, c):
        return bool(self.lib.pdf_bn_supported(int(c)))

    def bn_act_forward(self, x, res, gamma, beta, running_mean, running_var, training, eps, momentum, relu):
        n, c = x.shape
        require_current_device(x, res, gamma)
        coef = self._new(x, (4 * c,), torch.float32)
        partial = self._new(x, (int(self.lib.pdf_bn_partial_floats(n, c)),), torch.float32)
        y = self._new(x, (n, c), torch.float32)
        P = lambda t: None if t is None else self._ptr(t)
        self._launch("bn_act_forward", n, c, P(x), P(res), P(gamma), P(beta), P(running_mean), P(running_var),
                     int(bool(training)), eps, momentum, int(bool(relu)), P(coef), P(partial), P(y))
        return y, coef

    def bn_act_backward(self, gy, x, res, coef, training, relu, need_res):
        n, c = x.shape
        require_current_device(gy, x)
        partial = self._new(x, (int(self.lib.pdf_bn_partial_floats(n, c)),), torch.float32)
        sums = self._new(x, (2 * c,), torch.float32)
        gx = self._new(x, (n, c), torch.float32)
        gres = self._new(x, (n, c), torch.float32) if need_res else None
        P = lambda t: None if t is None else self._ptr(t)
        self._launch("bn_act_backward", n, c, P(gy), P(x), P(res), P(coef), int(bool(training)), int(bool(relu)), P(partial),
                     P(sums), P(gx), P(gres))
        return gx, gres, sums[c:], sums[:c]  # gx, gres, d gamma, d beta

    def radius_neighbors_self(self, nsample, radius, xyz, offset):
        """-> idx (n, nsample) int32, dist2 (n, nsample): the first nsample points of the scene in index order within radius."""
        _check(xyz, torch.float32, "xyz"); _check(offset, torch.int32, "offset")
        n, b = xyz.shape[0], offset.shape[0]
        idx = self._new(xyz, (n, nsample), torch.int32)
        dist2 = self._new(xyz, (n, nsample), torch.float32)
        if b > 64:   # the grid workspace is sized for <= 64 scenes: in-order scan
            order = torch.arange(n, dtype=torch.int32, device=xyz.device)
            return self.ball_query(nsample, radius, 0.0, xyz, xyz, offset, offset, order=order)
        nbytes = int(self.lib.pdf_knn_workspace_bytes(b, n, 0))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        self._call("radius_neighbors_self", n, int(nsample), float(radius), xyz, offset, b, idx, dist2, ws, nbytes)
        return idx, dist2

    ADAPTIVE_DIVISOR, ADAPTIVE_PAD = 16.0, 1e-6   # pointpdf_v1m1_base.py:137-140: ((max - min + 1e-6) / 16).min()

    def radius_neighbors_self_adaptive(self, nsample, xyz, offset):
        """-> idx (n, nsample) int32, dist2 (n, nsample), radii (b,) float32: ``radius_neighbors_self`` with the per-scene radius
        min over the axes of ((max - min) + 1e-6) / 16, derived on the device (no host read: capturable)."""
        _check(xyz, torch.float32, "xyz"); _check(offset, torch.int32, "offset")
        n, b = xyz.shape[0], offset.shape[0]
        if b > 64:   # the grid workspace is sized for <= 64 scenes: one fixed-radius query per scene, the radii read on the host
            if torch.cuda.is_current_stream_capturing():
                raise PdfOpsError("radius_neighbors_self_adaptive: more than 64 scenes need a host read of the radii, "
                                  "which a stream capture cannot hold")
            ends = offset.tolist()
            starts = [0] + ends[:-1]
            extent = lambda c: c.max(0)[0] - c.min(0)[0] if c.shape[0] else c.new_zeros(3)   # (a scene without points: extent 0, as the kernel)
            radii = torch.stack([((extent(xyz[s:e]) + self.ADAPTIVE_PAD) / self.ADAPTIVE_DIVISOR).min() for s, e in zip(starts, ends)])
            idx, dist2 = [], []
            for s, e, r in zip(starts, ends, radii.tolist()):
                if e == s:
                    continue
                i, d = self.radius_neighbors_self(nsample, r, xyz[s:e], torch.tensor([e - s], dtype=torch.int32, device=xyz.device))
                idx.append(torch.where(i >= 0, i + s, i)); dist2.append(d)
            if not idx:
                return self._new(xyz, (0, nsample), torch.int32), self._new(xyz, (0, nsample), torch.float32), radii
            return torch.cat(idx), torch.cat(dist2), radii
        idx = self._new(xyz, (n, nsample), torch.int32)
        dist2 = self._new(xyz, (n, nsample), torch.float32)
        radii = self._new(xyz, (b,), torch.float32)
        nbytes = int(self.lib.pdf_knn_workspace_bytes(b, n, 0))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz.device)
        self._call("radius_neighbors_self_adaptive", n, int(nsample), self.ADAPTIVE_DIVISOR, self.ADAPTIVE_PAD, xyz, offset, b, idx, dist2,
                   radii, ws, nbytes)
        return idx, dist2, radii

    def graph_forest(self, n, eu, ev, nodes, weight=None, active=None, want_chosen=True):
        """One scene's region graph (pseudo-label pass, pointpdf_v1m1_base.py:309-380): directed entries (eu[e], ev[e]) with ``weight[e]``
        (None: all equal) among the ``active`` ones (bool / uint8, None: all); ``nodes``: ids covering every endpoint (repeats allowed).
        -> (chosen (E,) bool or None: the entries of the minimum spanning forest under the order (weight, entry index);
            comp (n,) int32: the root of the component of every listed node, the node's own id elsewhere)."""
        _check(eu, torch.int64, "eu"); _check(ev, torch.int64, "ev"); _check(nodes, torch.int64, "nodes")
        E = int(eu.shape[0])
        if int(ev.shape[0]) != E or (weight is not None and int(weight.shape[0]) != E) or (active is not None and int(active.shape[0]) != E):
            raise ValueError("graph_forest: eu, ev, weight, active disagree on the number of entries")
        if weight is not None:
            _check(weight, torch.float32, "weight")
        if active is not None:
            active = active.view(torch.uint8) if active.dtype == torch.bool else active
            _check(active, torch.uint8, "active")
        comp = torch.arange(int(n), dtype=torch.int32, device=eu.device)
        chosen = torch.empty((E,), dtype=torch.uint8, device=eu.device) if want_chosen else None
        nbytes = int(self.lib.pdf_graph_forest_workspace_bytes(int(n), E, int(nodes.shape[0])))
        ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device=eu.device)
        nul = ctypes.c_void_p(None)
        self._call("graph_forest", int(n), E, eu, ev, nul if weight is None else weight, nul if active is None else active, nodes,
                   int(nodes.shape[0]), comp, nul if chosen is None else chosen, ws, ws.numel() * 8)
        return (chosen.view(torch.bool) if chosen is not None else None), comp

    def gmm2_1d(self, x, iters=100, tol=1e-3, reg=1e-6):
        """Two-component 1-D Gaussian mixture of the float values ``x`` by EM in double, on the device (stands in for
        sklearn.mixture.GaussianMixture(n_components=2).fit, pointpdf_v1m1_base.py:343-345).  -> (8,) float64 on the device: means (2),
        variances (2), weights (2), iterations run, final mean log-likelihood."""
        _check(x, torch.float32, "x")
        xs = torch.sort(x.reshape(-1))[0]
        m = int(xs.shape[0])
        resp = torch.empty((max(2 * m, 1),), dtype=torch.float64, device=x.device)
        out = torch.empty((8,), dtype=torch.float64, device=x.device)
        self._call("gmm2_1d", m, xs, resp, out, int(iters), float(tol), float(reg))
        return out

    def grid_hash(self, coord, offset, grid_size, min_grid, float32_division=False):
        """-> grid (n,3) int64 scene-relative voxel coordinates, key (n) int64 holding the uint64 FNV key bits.
        GridSample front half, pointcept/datasets/transform.py:813-823, 911-925."""
        _check(coord, torch.float32, "coord"); _check(offset, torch.int32, "offset"); _check(min_grid, torch.int64, "min_grid")
        n = coord.shape[0]
        grid = self._new(coord, (n, 3), torch.int64)
        key = self._new(coord, (n,), torch.int64)
        gx, gy, gz = (float(g) for g in grid_size)
        self._call("grid_hash", n, offset.shape[0], coord, offset, gx, gy, gz, 1 if float32_division else 0, min_grid, grid, key)
        return grid, key

    def grid_hash_f64(self, coord, offset, grid_size, min_grid):
        """grid_hash on float64 coordinates (csrc/augment.hip): floor(coord / grid_size) in float64, as the reference divides S3DIS's
        float64 coordinates and RandomRotate's promoted ones."""
        _check(coord, torch.float64, "coord"); _check(offset, torch.int32, "offset"); _check(min_grid, torch.int64, "min_grid")
        n = coord.shape[0]
        if coord.dim() != 2 or coord.shape[1] != 3 or min_grid.shape != (offset.shape[0], 3):
            raise ValueError("grid_hash_f64: coord (n,3), min_grid (b,3)")
        grid = self._new(coord, (n, 3), torch.int64)
        key = self._new(coord, (n,), torch.int64)
        gx, gy, gz = (float(g) for g in grid_size)
        self._call("grid_hash_f64", n, offset.shape[0], coord, offset, gx, gy, gz, min_grid, grid, key)
        return grid, key

    # -- training augmentation (csrc/augment.hip; pointcloudpdf_amd/augment.py drives them) ------------------------------------------
    @staticmethod
    def _i64(v):
        v = int(v) & ((1 << 64) - 1)
        return v - (1 << 64) if v >= 1 << 63 else v

    def philox4x64(self, n, key, ctr0, device):
        """(n, 4) int64 holding the uint64 words of Philox4x64-10 blocks for key (128-bit int) and counters ctr0 .. ctr0 + n - 1."""
        if n < 0:
            raise ValueError("philox4x64: n >= 0")
        out = torch.empty((int(n), 4), dtype=torch.int64, device=device)
        self._call("philox4x64", int(n), self._i64(key), self._i64(int(key) >> 64), self._i64(ctr0), out)
        return out

    def _aug_rows(self, offset, n, *rows):
        _check(offset, torch.int64, "offset")
        if offset.dim() != 1 or offset.shape[0] < 2:
            raise ValueError("offset: (b + 1) int64 scene starts")
        for name, t in rows:
            if t is not None:
                _check(t, torch.float64, name)
                if t.shape != (n, 3):
                    raise ValueError(f"{name}: expected ({n}, 3), got {tuple(t.shape)}")

    def aug_bounds(self, offset, coord, color=None):
        """-> (b, 12) float64 per-scene coord min, coord max, colour min, colour max.  offset (b + 1) int64 scene starts."""
        n = coord.shape[0]
        self._aug_rows(offset, n, ("coord", coord), ("color", color))
        b = offset.shape[0] - 1
        part = self._new(coord, (max(int(self.lib.pdf_aug_bounds_workspace_doubles(b)), 1),), torch.float64)
        bounds = self._new(coord, (b, 12), torch.float64)
        self._call("aug_bounds", b, offset, coord, color if color is not None else ctypes.c_void_p(None), part, bounds)
        return bounds

    def aug_points(self, offset, table, bounds, rec, coord, color=None, normal=None):
        """One segment of the transform list, in place on the fp64 rows.  table (b, 1 + nop, 16) float64 (augment.py: _Program)."""
        n = coord.shape[0]
        self._aug_rows(offset, n, ("coord", coord), ("color", color), ("normal", normal))
        b = offset.shape[0] - 1
        _check(table, torch.float64, "table")
        if table.dim() != 3 or table.shape[0] != b or table.shape[2] != 16 or table.shape[1] < 1:
            raise ValueError("table: (b, 1 + nop, 16) float64")
        if bounds is not None:
            _check(bounds, torch.float64, "bounds")
            if bounds.shape != (b, 12):
                raise ValueError("bounds: (b, 12)")
        if rec is not None:
            _check(rec, torch.float64, "rec")
            if rec.dim() != 3 or rec.shape[1:] != (n, 3):
                raise ValueError("rec: (k, n, 3) float64")
        nul = ctypes.c_void_p(None)
        self._call("aug_points", b, n, offset, table.shape[1] - 1, table, nul if bounds is None else bounds, nul if rec is None else rec,
                   coord, nul if color is None else color, nul if normal is None else normal)

    def aug_keys(self, offset, n, scene_keys, stream_id):
        """-> (n) int64 holding one uint64 Philox key per point (scene key, stream id; counter = index in the scene).
        offset (b + 1) int64 scene starts with offset[-1] == n (the caller's host copy of the sizes gives n)."""
        _check(offset, torch.int64, "offset"); _check(scene_keys, torch.int64, "scene_keys")
        if offset.dim() != 1 or offset.shape[0] < 2 or scene_keys.shape != (offset.shape[0] - 1,) or n < 0:
            raise ValueError("aug_keys: offset (b + 1) int64, scene_keys (b,) int64, n >= 0")
        out = self._new(scene_keys, (int(n),), torch.int64)
        self._call("aug_keys", offset.shape[0] - 1, int(n), offset, scene_keys, self._i64(stream_id), out)
        return out

    def aug_elastic_stage(self, offset, coord, vinfo, total, axes, params, magnitude, scene_keys, stream_id, noise=None, keep_disp=False):
        """One ElasticDistortion stage in place on coord (n,3) f64: noise volume (``noise`` (total,3) float32 recorded, or drawn), two
        rounds of the x / y / z box blur, trilinear sampling.  vinfo (5b + 2) int64: voxel starts, dims (b,3), axis starts; axes f64;
        params (b,2) f64 (fired, float32 flag).  -> (blurred volume (total,3) float32, displacement (n,3) f64 or None)."""
        n = coord.shape[0]
        self._aug_rows(offset, n, ("coord", coord))
        b = offset.shape[0] - 1
        _check(vinfo, torch.int64, "vinfo"); _check(axes, torch.float64, "axes"); _check(params, torch.float64, "params")
        _check(scene_keys, torch.int64, "scene_keys")
        if vinfo.shape != (5 * b + 2,) or params.shape != (b, 2) or scene_keys.shape != (b,) or total < 0:
            raise ValueError("aug_elastic_stage: vinfo (5b + 2), params (b, 2), scene_keys (b,)")
        vh = vinfo.cpu() if vinfo.is_cuda else vinfo
        if int(vh[b]) != total or axes.shape[0] != int(vh[4 * b + 1 + b]) or bool((vh[b + 1:4 * b + 1] < 0).any()):
            raise ValueError("aug_elastic_stage: vinfo disagrees with total / axes")
        a = self._new(coord, (max(total, 1), 3), torch.float32)
        if noise is not None:
            _check(noise, torch.float32, "noise")
            if noise.shape != (total, 3):
                raise ValueError(f"noise: expected ({total}, 3)")
            a[:total].copy_(noise)
        else:
            self._call("aug_elastic_noise", b, int(total), vinfo, scene_keys, self._i64(stream_id), a)
        t = self._new(coord, (max(total, 1), 3), torch.float32)
        for _ in range(2):
            for axis in range(3):
                self._call("aug_elastic_blur", b, int(total), vinfo, a, t, axis)
                a, t = t, a
        disp = self._new(coord, (n, 3), torch.float64, zero=True) if keep_disp else None
        self._call("aug_elastic_apply", b, n, offset, vinfo, axes, a, params, float(magnitude), coord,
                   disp if disp is not None else ctypes.c_void_p(None))
        return a[:total], disp

    def vote_accumulate(self, logits, score, index, pred, score_sum, score_cnt):
        """One test-time fragment into the running vote (engines/test.py:218-229, 243-251); index entries must be distinct."""
        _check(logits, torch.float32, "logits"); _check(index, torch.int64, "index"); _check(pred, torch.float32, "pred")
        if score is not None:
            _check(score, torch.float32, "score"); _check(score_sum, torch.float32, "score_sum"); _check(score_cnt, torch.float32, "score_cnt")
        n, c = logits.shape
        if pred.shape[1] != c:
            raise ValueError("pred and logits disagree on the number of classes")
        nul = ctypes.c_void_p(None)
        self._call("vote_accumulate", n, c, logits, nul if score is None else score, index, pred,
                   nul if score is None else score_sum, nul if score is None else score_cnt)

    # -- criteria (csrc/criteria.hip; segmentor.CrossEntropyLoss and losses.py drive them) ----------------------------------------------
    REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}   # include/pdfops.h: PDF_REDUCE_*

    def _criteria_acc(self, like, c):
        # every float is written before it is read (csrc/criteria.hip): nothing to zero, no memset node in a captured step
        return self._new(like, (int(self.lib.pdf_criteria_workspace_floats(int(c))),), torch.float32)

    @staticmethod
    def _logits_labels(logits, target, what):
        _check(logits, torch.float32, "logits"); _check(target, torch.int64, "target")
        if logits.dim() != 2 or target.shape != (logits.shape[0],) or logits.shape[0] < 1 or logits.shape[1] < 1:
            raise ValueError(f"{what}: logits (n, c) and target (n) expected, got {tuple(logits.shape)}, {tuple(target.shape)}")
        return logits.shape

    @staticmethod
    def _class_vector(v, c, name):
        if v is not None:
            _check(v, torch.float32, name)
            if v.shape != (c,):
                raise ValueError(f"{name}: expected ({c},), got {tuple(v.shape)}")
        return ctypes.c_void_p(None) if v is None else v

    def ce_ex_forward(self, logits, target, weight, label_smoothing, reduction, ignore_index):
        """-> loss (scalar, or (n) for "none"), dlogits (n, c) unscaled, acc.  nn.CrossEntropyLoss in full (include/pdfops.h)."""
        n, c = self._logits_labels(logits, target, "ce_ex_forward")
        w = self._class_vector(weight, c, "weight")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
        require_current_device(logits, target, weight)
        grad = self._new(logits, (n, c), torch.float32)
        acc = self._criteria_acc(logits, c)
        loss = self._new(logits, (n,) if reduction == "none" else (), torch.float32)
        self._call("ce_ex_forward", n, c, logits, target, w, float(label_smoothing), self.REDUCTIONS[reduction], int(ignore_index), grad, acc, loss)
        return loss, grad, acc

    def ce_ex_backward(self, dlogits, acc, gy, reduction):
        _check(dlogits, torch.float32, "dlogits"); _check(acc, torch.float32, "acc"); _check(gy, torch.float32, "grad_output")
        n, c = dlogits.shape
        if gy.numel() != (n if reduction == "none" else 1):
            raise ValueError(f"ce_ex_backward: grad_output of {gy.numel()} elements for reduction {reduction!r} over {n} rows")
        require_current_device(dlogits, acc, gy)
        out = self._new(dlogits, (n, c), torch.float32)   # the saved buffer stays untouched (retain_graph)
        self._call("ce_ex_backward", n, c, dlogits, acc, gy, self.REDUCTIONS[reduction], out)
        return out

    def focal_forward(self, logits, target, alpha, gamma, reduction, ignore_index):
        """-> loss (scalar), dlogits (n, c) unscaled, acc.  ``alpha``: a float or a (c) fp32 tensor on the device."""
        n, c = self._logits_labels(logits, target, "focal_forward")
        if reduction not in ("mean", "sum"):
            raise ValueError("focal_forward: reduction must be 'mean' or 'sum'")
        vec = alpha if isinstance(alpha, torch.Tensor) else None
        a = self._class_vector(vec, c, "alpha")
        require_current_device(logits, target, vec)
        grad = self._new(logits, (n, c), torch.float32)
        acc = self._criteria_acc(logits, c)
        loss = self._new(logits, (), torch.float32)
        self._call("focal_forward", n, c, logits, target, a, 0.0 if vec is not None else float(alpha), float(gamma),
                   self.REDUCTIONS[reduction], int(ignore_index), grad, acc, loss)
        return loss, grad, acc

    def focal_backward(self, dlogits, acc, gy):
        _check(dlogits, torch.float32, "dlogits"); _check(acc, torch.float32, "acc"); _check(gy, torch.float32, "grad_output")
        n, c = dlogits.shape
        require_current_device(dlogits, acc, gy)
        out = self._new(dlogits, (n, c), torch.float32)
        self._call("focal_backward", n, c, dlogits, acc, gy, out)
        return out

    def dice_forward(self, logits, target, smooth, exponent, ignore_index):
        """-> loss (scalar, loss_weight 1), prob (n, c), acc (keeps the class coefficients the backward reads)."""
        n, c = self._logits_labels(logits, target, "dice_forward")
        if not float(exponent) > 0.0:
            raise ValueError(f"dice_forward: exponent must be positive, got {exponent}")
        require_current_device(logits, target)
        prob = self._new(logits, (n, c), torch.float32)
        acc = self._criteria_acc(logits, c)
        loss = self._new(logits, (), torch.float32)
        self._call("dice_forward", n, c, logits, target, float(smooth), float(exponent), int(ignore_index), prob, acc, loss)
        return loss, prob, acc

    def dice_backward(self, prob, target, ignore_index, exponent, acc, gy):
        n, c = self._logits_labels(prob, target, "dice_backward")
        _check(acc, torch.float32, "acc"); _check(gy, torch.float32, "grad_output")
        require_current_device(prob, target, acc, gy)
        out = self._new(prob, (n, c), torch.float32)
        self._call("dice_backward", n, c, prob, target, int(ignore_index), float(exponent), acc, gy, out)
        return out

    def bfocal_forward(self, pred, target, alpha, gamma, logits, reduce):
        """-> loss (scalar, or (n) with reduce=False), dpred (n) unscaled, acc.  pred, target: flat fp32."""
        _check(pred, torch.float32, "pred"); _check(target, torch.float32, "target")
        if pred.dim() != 1 or target.shape != pred.shape or pred.shape[0] < 1:
            raise ValueError(f"bfocal_forward: pred (n) and target (n) expected, got {tuple(pred.shape)}, {tuple(target.shape)}")
        require_current_device(pred, target)
        n = pred.shape[0]
        grad = self._new(pred, (n,), torch.float32)
        acc = self._criteria_acc(pred, 1)
        loss = self._new(pred, () if reduce else (n,), torch.float32)
        self._call("bfocal_forward", n, pred, target, float(alpha), float(gamma), int(bool(logits)), int(bool(reduce)), grad, acc, loss)
        return loss, grad, acc

    def bfocal_backward(self, dpred, acc, gy, reduce):
        _check(dpred, torch.float32, "dpred"); _check(acc, torch.float32, "acc"); _check(gy, torch.float32, "grad_output")
        n = dpred.shape[0]
        if gy.numel() != (1 if reduce else n):
            raise ValueError(f"bfocal_backward: grad_output of {gy.numel()} elements for reduce={reduce} over {n} elements")
        require_current_device(dpred, acc, gy)
        out = self._new(dpred, (n,), torch.float32)
        self._call("bfocal_backward", n, dpred, acc, gy, int(bool(reduce)), out)
        return out

    # -- context-aware classifier head (csrc/cac.hip; pointcloudpdf_amd/cac.py drives them) ----------------------------------------------
    def cac_supported(self, K, c):
        return bool(self.lib.pdf_cac_supported(int(K), int(c)))

    def _cac_ws(self, like, n, K, c, scenes):
        # every float is written before it is read (csrc/cac.hip): nothing to zero, no memset node in a captured step
        return self._new(like, (int(self.lib.pdf_cac_workspace_floats(int(n), int(K), int(c), int(scenes))),), torch.float32)

    def _cac_shapes(self, rows, cols, K, what):
        _check(rows, torch.float32, what)
        n, c = rows.shape
        if n < 1 or cols.shape[0] != n or not self.cac_supported(K, c):
            raise ValueError(f"{what}: ({n}, {c}) rows against {tuple(cols.shape)} with {K} classes is outside the fused class")
        return n, c

    def cac_soft_proto_forward(self, feat, logits, offset, conf_thresh):
        """-> proto (scenes, K, c), mass (scenes, K)."""
        _check(logits, torch.float32, "logits"); _check(offset, torch.int32, "offset")
        K, scenes = logits.shape[1], offset.shape[0]
        n, c = self._cac_shapes(feat, logits, K, "cac_soft_proto_forward")
        require_current_device(feat, logits, offset)
        proto = self._new(feat, (scenes, K, c), torch.float32)
        mass = self._new(feat, (scenes, K), torch.float32)
        ws = self._cac_ws(feat, n, K, c, scenes)
        self._call("cac_soft_proto_forward", n, K, c, scenes, feat, logits, offset, float(conf_thresh), proto, mass, ws)
        return proto, mass

    def cac_soft_proto_backward(self, feat, logits, offset, conf_thresh, proto, mass, gproto, want_logits):
        _check(gproto, torch.float32, "grad_output")
        K, scenes = logits.shape[1], offset.shape[0]
        n, c = self._cac_shapes(feat, logits, K, "cac_soft_proto_backward")
        require_current_device(feat, logits, offset, gproto)
        gfeat = self._new(feat, (n, c), torch.float32)
        glogits = self._new(feat, (n, K), torch.float32) if want_logits else None
        self._call("cac_soft_proto_backward", n, K, c, scenes, feat, logits, offset, float(conf_thresh), proto, mass, gproto, gfeat,
                   ctypes.c_void_p(None) if glogits is None else glogits)
        return gfeat, glogits

    def cac_label_proto_forward(self, feat, target, base):
        """-> proto (K, c), count (K)."""
        _check(target, torch.int64, "target"); _check(base, torch.float32, "base")
        K = base.shape[0]
        n, c = self._cac_shapes(feat, target, K, "cac_label_proto_forward")
        if base.shape != (K, c):
            raise ValueError(f"cac_label_proto_forward: base {tuple(base.shape)} for {c} channels")
        require_current_device(feat, target, base)
        proto = self._new(feat, (K, c), torch.float32)
        count = self._new(feat, (K,), torch.float32)
        self._call("cac_label_proto_forward", n, K, c, feat, target, base, proto, count, self._cac_ws(feat, n, K, c, 1))
        return proto, count

    def cac_label_proto_backward(self, target, count, gproto):
        _check(gproto, torch.float32, "grad_output")
        n, (K, c) = target.shape[0], gproto.shape
        require_current_device(target, count, gproto)
        gfeat = self._new(gproto, (n, c), torch.float32)
        self._call("cac_label_proto_backward", n, K, c, target, count, gproto, gfeat)
        return gfeat

    @staticmethod
    def _cac_proto(proto, offset):
        _check(proto, torch.float32, "proto")
        if offset is not None:
            _check(offset, torch.int32, "offset")
        scenes = 1 if proto.dim() == 2 else proto.shape[0]
        if proto.dim() == 3 and (offset is None or offset.shape[0] != scenes):
            raise ValueError("cosine logits: per-scene prototypes (scenes, K, c) need the scenes' offset")
        return scenes, proto.shape[-2], ctypes.c_void_p(None) if proto.dim() == 2 else offset

    def cac_cosine_forward(self, x, proto, offset, scale):
        scenes, K, off = self._cac_proto(proto, offset)
        n, c = self._cac_shapes(x, x, K, "cac_cosine_forward")
        if proto.shape[-1] != c:
            raise ValueError(f"cac_cosine_forward: prototypes of {proto.shape[-1]} channels for rows of {c}")
        require_current_device(x, proto, offset)
        out = self._new(x, (n, K), torch.float32)
        self._call("cac_cosine_forward", n, K, c, scenes, x, proto, off, float(scale), out)
        return out

    def cac_cosine_backward(self, x, proto, offset, scale, gout):
        _check(gout, torch.float32, "grad_output")
        scenes, K, off = self._cac_proto(proto, offset)
        n, c = self._cac_shapes(x, gout, K, "cac_cosine_backward")
        require_current_device(x, proto, offset, gout)
        gx = self._new(x, (n, c), torch.float32)
        gproto = self._new(x, tuple(proto.shape), torch.float32)
        self._call("cac_cosine_backward", n, K, c, scenes, x, proto, off, float(scale), gout, gx, gproto, self._cac_ws(x, n, K, c, scenes))
        return gx, gproto

    def cac_distill_forward(self, pred, soft, target, smoothness):
        """-> loss (scalar), grad (n, K) unscaled, acc."""
        n, K = self._logits_labels(pred, target, "cac_distill_forward")
        _check(soft, torch.float32, "soft")
        if soft.shape != pred.shape or K > 256:
            raise ValueError(f"cac_distill_forward: pred {tuple(pred.shape)}, soft {tuple(soft.shape)} (at most 256 classes)")
        require_current_device(pred, soft, target)
        grad = self._new(pred, (n, K), torch.float32)
        rowbuf = self._new(pred, (n, 2), torch.float32)
        acc = self._new(pred, (int(self.lib.pdf_cac_distill_workspace_floats(int(K))),), torch.float32)
        loss = self._new(pred, (), torch.float32)
        self._call("cac_distill_forward", n, K, pred, soft, target, float(smoothness), grad, rowbuf, acc, loss)
        return loss, grad, acc

    def cac_distill_backward(self, grad, target, acc, gy):
        _check(gy, torch.float32, "grad_output")
        n, K = grad.shape
        require_current_device(grad, target, acc, gy)
        out = self._new(grad, (n, K), torch.float32)
        self._call("cac_distill_backward", n, K, grad, target, acc, gy, out)
        return out

    # -- sparse convolutions (csrc/sparse_conv.hip; pointcloudpdf_amd/sparse_conv.py drives them) ------------------------------------------
    def spconv_supported(self, k, cin, cout):
        """0: no HIP pass, 1: the matrix-core class, 2: the small-C_in class (the stem)."""
        return int(self.lib.pdf_spconv_supported(int(k), int(cin), int(cout)))

    def spconv_geometry(self, indices, levels, subm_sizes, limits=None):
        """All levels of a stride-2 pyramid over ``indices`` (n, 4) int32 in ONE submission and ONE host read (the counts and the status
        word).  subm_sizes[l]: the kernel sizes whose neighbour tables level l gets; limits[l]: the coarse spatial shape of step l -> l + 1
        or None.  -> (status, [level dict], [step dict]); arrays are views of buffers sized by the fine level."""
        _check(indices, torch.int32, "indices")
        require_current_device(indices)
        n = indices.shape[0]
        dev = indices.device
        new = lambda shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)
        counts = torch.tensor([0, n] + [0] * (levels - 1), dtype=torch.int32, device=dev)   # [status | count of every level]
        ws = new((int(self.lib.pdf_spconv_geometry_workspace_bytes(n)),), torch.uint8)
        padded = int(self.lib.pdf_spconv_bucket_rows(n))
        lv = [dict(indices=indices, skey=new((n,), torch.int64), order=new((n,)), nbr={})]
        self._call("spconv_sort_sites", n, indices, lv[0]["skey"], lv[0]["order"], counts, ws)
        steps = []
        for l in range(levels):
            cur = lv[l]
            for ks in subm_sizes[l]:
                cur["nbr"][ks] = new((n, ks ** 3))
                self._call("spconv_subm_table", n, counts[1 + l:], cur["indices"], cur["skey"],
                           cur["order"] if cur["order"] is not None else ctypes.c_void_p(None), int(ks), cur["nbr"][ks])
            if l == levels - 1:
                break
            st = dict(parent=new((n,)), code=new((n,)), children=new((n, 8)), bucket_perm=new((padded,)), tile_code=new((padded // 128,)),
                      bucket_ptr=new((18,)))
            nxt = dict(indices=new((n, 4)), skey=new((n,), torch.int64), order=None, nbr={})
            lim = None if not limits or limits[l] is None else (ctypes.c_int * 3)(*[int(v) for v in limits[l]])
            self._call("spconv_down", n, counts[1 + l:], cur["indices"], lim, st["parent"], st["code"], nxt["indices"], nxt["skey"],
                       st["children"], st["bucket_perm"], st["tile_code"], st["bucket_ptr"], counts[2 + l:], ws)
            st["truncated"] = lim is not None
            steps.append(st)
            lv.append(nxt)
        host = counts.tolist()   # the one host read of a geometry build
        status, cnt = host[0], host[1:]
        for l, cur in enumerate(lv):
            cur["n"] = cnt[l]
            cur["indices"] = cur["indices"][:cnt[l]]
            cur["nbr"] = {ks: t[:cnt[l]] for ks, t in cur["nbr"].items()}
        for l, st in enumerate(steps):
            st["parent"], st["code"], st["children"] = st["parent"][:cnt[l]], st["code"][:cnt[l]], st["children"][:cnt[l + 1]]
            st["bucket_rows"] = int(self.lib.pdf_spconv_bucket_rows(cnt[l]))
        return status, lv, steps

    def spconv_gather(self, x, tbl, weight, bias, orows, transposed, mirror=False, perm=None, tile_k=None, rows=None, zero=False):
        """pdf_spconv_gather over weight (C_out, K, C_in): transposed = False: x (., C_in) -> (orows, C_out); True: x (., C_out) -> (orows, C_in)."""
        co, K, ci = weight.shape
        cin, cout = (co, ci) if transposed else (ci, co)
        strides = (K * ci, ci, 1) if transposed else (1, ci, K * ci)
        require_current_device(x, tbl, weight)
        out = self._new(x, (orows, cout), torch.float32, zero=zero)
        Kt = 1 if tbl.dim() == 1 else tbl.shape[1]
        null = ctypes.c_void_p(None)
        self._call("spconv_gather", int(orows if rows is None else rows), int(orows), x.shape[0], cin, cout, Kt, x, tbl, int(bool(mirror)),
                   null if perm is None else perm, null if tile_k is None else tile_k, weight, *strides, null if bias is None else bias, out)
        return out

    def spconv_small_forward(self, x, tbl, weight, bias):
        co, K, ci = weight.shape
        require_current_device(x, tbl, weight)
        out = self._new(x, (x.shape[0], co), torch.float32)
        self._call("spconv_small_forward", x.shape[0], ci, co, K, x, tbl, weight, ctypes.c_void_p(None) if bias is None else bias, out)
        return out

    def spconv_small_dgrad(self, g, tbl, weight):
        co, K, ci = weight.shape
        require_current_device(g, tbl, weight)
        out = self._new(g, (g.shape[0], ci), torch.float32)
        self._call("spconv_small_dgrad", g.shape[0], ci, co, K, g, tbl, weight, out)
        return out

    def spconv_wgrad(self, G, D, tbl, shape, swap):
        """dW (C_out, K, C_in) = sum_r G[tbl[r, k]]^T D[r] (swap: G is the output gradient, D the input)."""
        rows, K = tbl.shape
        ca, cb = G.shape[1], D.shape[1]
        require_current_device(G, D, tbl)
        dw = self._new(G, tuple(shape), torch.float32)
        if rows == 0:
            return dw.zero_()
        ws = self._new(G, (int(self.lib.pdf_spconv_wgrad_ws_floats(rows, K, ca, cb)),), torch.float32)
        self._call("spconv_wgrad", rows, G.shape[0], K, ca, cb, G, D, tbl, int(bool(swap)), ws, dw)
        return dw

    def spconv_colsum(self, g):
        rows, c = g.shape
        require_current_device(g)
        out = self._new(g, (c,), torch.float32)
        ws = self._new(g, (int(self.lib.pdf_spconv_colsum_ws_floats(c)),), torch.float32)
        self._call("spconv_colsum", rows, c, g, ws, out)
        return out

    # -- batched test-time fragments (csrc/fragments.hip; pointcloudpdf_amd/testing.py drives them) ------------------------------------
    @staticmethod
    def _fragment_table(table, f0, g, coord=None):
        """-> (n, v) of a ``voxelize.fragment_table`` result after its dtype / shape checks."""
        order, vstart, count = table["order"], table["vstart"], table["count"]
        _check(order, torch.int64, "order"); _check(vstart, torch.int64, "vstart"); _check(count, torch.int64, "count")
        n, v = order.shape[0], count.shape[0]
        if order.dim() != 1 or count.dim() != 1 or vstart.shape != (v,) or v > n:
            raise ValueError("fragment table: order (n), vstart (v), count (v) with v <= n")
        if int(f0) < 0 or int(g) < 1:
            raise ValueError(f"fragment batch: f0 >= 0 and g >= 1 (got f0={f0}, g={g})")
        if coord is not None:
            if coord.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"coord: expected float32 or float64, got {coord.dtype}")
            _check(coord, coord.dtype, "coord")
            if coord.shape != (n, 3):
                raise ValueError(f"coord: expected ({n}, 3), got {tuple(coord.shape)}")
        return n, v

    def fragment_bounds(self, coord, table, f0, g):
        """-> (g, 6) float64 [min xyz | max xyz] of the coordinates test fragments f0 .. f0 + g - 1 select (exact)."""
        n, v = self._fragment_table(table, f0, g, coord)
        ws = self._new(coord, (max(int(self.lib.pdf_fragment_bounds_ws_doubles(int(g))), 1),), torch.float64)
        bounds = self._new(coord, (int(g), 6), torch.float64)
        self._call("fragment_bounds", n, v, int(f0), int(g), 1 if coord.dtype == torch.float64 else 0, coord, table["order"],
                   table["vstart"], table["count"], ws, bounds)
        return bounds

    def fragment_gather(self, coord, table, f0, g, shift, feat_segments, grid_coord=None):
        """The collated batch of test fragments f0 .. f0 + g - 1 in one launch.  shift (g, 3) in coord's dtype; ``feat_segments``: the
        Collect.feat_keys entries in order, each ``None`` (the shifted coordinate) or an (n, w <= 4) float32 tensor; grid_coord (n, 3)
        int64 or None.  -> dict(index (g v) int64, coord (g v, 3) f32, feat (g v, c) f32, offset (g) int32[, grid_coord (g v, 3) int64])."""
        n, v = self._fragment_table(table, f0, g, coord)
        g = int(g)
        _check(shift, coord.dtype, "shift")
        if shift.shape != (g, 3):
            raise ValueError(f"shift: expected ({g}, 3), got {tuple(shift.shape)}")
        if not 1 <= len(feat_segments) <= 4 or g > 256:
            raise ValueError("fragment_gather: 1..4 feat segments, at most 256 fragments per batch")
        widths = []
        for k, t in enumerate(feat_segments):
            if t is None:
                widths.append(3)
                continue
            _check(t, torch.float32, f"feat segment {k}")
            if t.dim() != 2 or t.shape[0] != n or not 1 <= t.shape[1] <= 4:
                raise ValueError(f"feat segment {k}: expected ({n}, w <= 4), got {tuple(t.shape)}")
            self._ptr(t)
            if t.device != coord.device:
                raise PdfOpsError(f"feat segment {k} on {t.device}, coord on {coord.device}")
            widths.append(int(t.shape[1]))
        if grid_coord is not None:
            _check(grid_coord, torch.int64, "grid_coord")
            if grid_coord.shape != (n, 3):
                raise ValueError(f"grid_coord: expected ({n}, 3)")
        rows, c = g * v, sum(widths)
        if rows > 2 ** 31 - 1:
            raise ValueError(f"fragment_gather: {g} fragments of {v} voxels do not fit the int32 offset")
        out = dict(index=self._new(coord, (rows,), torch.int64), coord=self._new(coord, (rows, 3), torch.float32),
                   feat=self._new(coord, (rows, c), torch.float32), offset=self._new(coord, (g,), torch.int32))
        if v == 0:
            out["offset"].zero_()
        if grid_coord is not None:
            out["grid_coord"] = self._new(coord, (rows, 3), torch.int64)
        nul = ctypes.c_void_p(None)
        seg_src = (c_void_p * 4)(*[None if t is None else t.data_ptr() for t in feat_segments])
        seg_w = (c_int * 4)(*widths)
        self._call("fragment_gather", n, v, int(f0), g, 1 if coord.dtype == torch.float64 else 0, coord, table["order"], table["vstart"],
                   table["count"], shift, len(feat_segments), seg_src, seg_w, nul if grid_coord is None else grid_coord, out["index"],
                   out["coord"], out["feat"], out.get("grid_coord", nul), out["offset"])
        return out

    def fragment_vote(self, logits, score, table, f0, g, pred, score_sum, score_cnt):
        """Fold the batch of fragments f0 .. f0 + g - 1 (logits (g v, c), score (g v) or None, rows in gather order) into the running vote
        -- no atomics, a point's fragments in ascending order: bit-identical to g successive ``vote_accumulate`` calls."""
        n, v = self._fragment_table(table, f0, g)
        g = int(g)
        _check(table["voxel_of"], torch.int64, "voxel_of")
        _check(logits, torch.float32, "logits"); _check(pred, torch.float32, "pred")
        if table["voxel_of"].shape != (n,):
            raise ValueError(f"voxel_of: expected ({n},)")
        if logits.dim() != 2 or logits.shape[0] != g * v or pred.dim() != 2 or pred.shape != (n, logits.shape[1]):
            raise ValueError(f"fragment_vote: logits ({g * v}, c) and pred ({n}, c) expected, got {tuple(logits.shape)}, {tuple(pred.shape)}")
        if score is not None:
            _check(score, torch.float32, "score"); _check(score_sum, torch.float32, "score_sum"); _check(score_cnt, torch.float32, "score_cnt")
            if score.shape != (g * v,) or score_sum.shape != (n,) or score_cnt.shape != (n,):
                raise ValueError("fragment_vote: score (g v), score_sum (n), score_cnt (n)")
        nul = ctypes.c_void_p(None)
        self._call("fragment_vote", n, v, int(f0), g, logits.shape[1], logits, nul if score is None else score, table["order"],
                   table["vstart"], table["count"], table["voxel_of"], pred, nul if score is None else score_sum,
                   nul if score is None else score_cnt)

    def group_forward(self, feat, xyz, new_xyz, idx, with_xyz):
        _check(feat, torch.float32, "feat"); _check(idx, torch.int32, "idx")
        m, ns = idx.shape
        c = feat.shape[1]
        out = self._new(feat, (m, ns, c + (3 if with_xyz else 0)), torch.float32)
        if with_xyz:
            _check(xyz, torch.float32, "xyz"); _check(new_xyz, torch.float32, "new_xyz")
            self._call("group_forward_ordered", m, ns, c, 1, feat, xyz, new_xyz, idx, order_of(idx), out)
        else:
            self._call("group_forward_ordered", m, ns, c, 0, feat, feat, feat, idx, order_of(idx), out)
        return out

    def group_backward(self, grad_output, idx, n, c, with_xyz):
        _check(grad_output, torch.float32, "grad_output")
        if not with_xyz and self.use_inverse:
            return self.grouping_backward(grad_output, idx, n)
        m, ns = idx.shape
        if with_xyz and self.use_inverse and grad_output.numel() > 0 and n > 0:
            # rows are [g_rel_xyz (3) | g_feat (c)]: the feature part is summed per source point over the inverse table
            off, ent, base = inverse_table(idx, n)
            gf = self._new(grad_output, (n, c), torch.float32)
            self._call("seg_sum_rows_strided", n, c, grad_output.view(-1)[3:], 3 + c, off, ent, base, 1.0, gf)
            return gf
        gf = self._new(grad_output, (n, c), torch.float32, zero=True)
        self._call("group_backward", m, ns, c, 1 if with_xyz else 0, grad_output, idx, gf)
        return gf

    def interpolation_weights(self, dist2):
        _check(dist2, torch.float32, "dist2")
        n, k = dist2.shape
        w = self._new(dist2, (n, k), torch.float32)
        self._call("interpolation_weights", n, k, dist2, w)
        return w

    # ---- PointTransformer-V2: partition pooling / unpooling (csrc/grid_pool.hip) ----
    def grid_pool_partition(self, coord, offset, grid_size, bounds=None):
        """coord (n, 3) float32, offset (scenes) scene ends -> (cluster (n) int64, sorted (n) int32, idx_ptr (m + 1) int32, m): the
        partition of point_transformer_v2m2_base.py:248-264.  One host read: the cluster count."""
        _check(coord, torch.float32, "coord")
        n = int(coord.shape[0])
        ends = offset.int().contiguous()
        lo, hi = bounds if bounds is not None else self.scene_bounds(coord, ends)
        cluster = torch.empty(n, dtype=torch.int64, device=coord.device)
        srt = torch.empty(n, dtype=torch.int32, device=coord.device)
        idx_ptr = torch.empty(n + 1, dtype=torch.int32, device=coord.device)
        count = torch.empty(1, dtype=torch.int32, device=coord.device)
        ws = torch.empty(int(self.lib.pdf_grid_pool_workspace_bytes(n)), dtype=torch.uint8, device=coord.device)
        self._call("grid_pool_partition", n, coord, ends, int(ends.shape[0]), lo.contiguous(), hi.contiguous(), float(grid_size), cluster, srt,
                   idx_ptr, count, ws)
        m = int(count.item())
        return cluster, srt, idx_ptr[:m + 1], m

    def grid_pool_mean(self, coord, idx_ptr, srt):
        _check(coord, torch.float32, "coord"); _check(idx_ptr, torch.int32, "idx_ptr"); _check(srt, torch.int32, "sorted")
        m = int(idx_ptr.shape[0]) - 1
        out = torch.empty((m, 3), dtype=torch.float32, device=coord.device)
        self._call("grid_pool_reduce", int(coord.shape[0]), m, 0, coord, None, idx_ptr, srt, out, None, None)
        return out

    def grid_pool_max(self, feat, idx_ptr, srt):
        _check(feat, torch.float32, "feat"); _check(idx_ptr, torch.int32, "idx_ptr"); _check(srt, torch.int32, "sorted")
        m, c = int(idx_ptr.shape[0]) - 1, int(feat.shape[1])
        out = torch.empty((m, c), dtype=torch.float32, device=feat.device)
        arg = torch.empty((m, c), dtype=torch.int32, device=feat.device)
        self._call("grid_pool_reduce", int(feat.shape[0]), m, c, None, feat, idx_ptr, srt, None, out, arg)
        return out, arg

    def grid_pool_max_backward(self, grad_out, cluster, arg):
        _check(grad_out, torch.float32, "grad_out"); _check(cluster, torch.int64, "cluster"); _check(arg, torch.int32, "arg")
        n, (m, c) = int(cluster.shape[0]), grad_out.shape
        out = torch.empty((n, c), dtype=torch.float32, device=grad_out.device)
        self._call("grid_pool_max_backward", n, int(m), int(c), grad_out, cluster, arg, out)
        return out

    def grid_unpool_forward(self, x, cluster):
        _check(x, torch.float32, "x"); _check(cluster, torch.int64, "cluster")
        n, (m, c) = int(cluster.shape[0]), x.shape
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        self._call("grid_unpool_forward", n, int(m), int(c), x, cluster, out)
        return out

    def grid_unpool_backward(self, grad_out, idx_ptr, srt):
        """segmented row sums over (idx_ptr, sorted): pdf_seg_sum_rows' table form with entry_base 0"""
        _check(grad_out, torch.float32, "grad_out"); _check(idx_ptr, torch.int32, "idx_ptr"); _check(srt, torch.int32, "sorted")
        m, c = int(idx_ptr.shape[0]) - 1, int(grad_out.shape[1])
        out = torch.empty((m, c), dtype=torch.float32, device=grad_out.device)
        self._call("seg_sum_rows", m, c, grad_out, idx_ptr, srt, 0, 1.0, out)
        return out

    # ---- PointTransformer-V2: grouped vector attention (csrc/gva.hip) ----
    def gva_supported(self, c, groups, s):
        return bool(self.lib.pdf_gva_supported(int(c), int(groups), int(s)))

    def gva_relation_forward(self, query, key, idx, pem, peb):
        n, s = idx.shape
        c = int(query.shape[1])
        rel = torch.empty((n, s, c), dtype=torch.float32, device=query.device)
        self._call("gva_relation_forward", int(n), int(key.shape[0]), int(s), c, query, key, idx, pem, peb, rel)
        return rel

    def gva_relation_backward(self, g_rel, query, key, idx, pem, need_query, need_key, need_pem):
        n, s = idx.shape
        nk, c = int(key.shape[0]), int(query.shape[1])
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=query.device)
        gq = new(n, c) if need_query else None
        gk = new(nk, c) if need_key else None
        gp = new(n, s, c) if need_pem and pem is not None else None
        off, ent, base = inverse_table(idx, nk) if need_key else (None, None, 0)
        if base != 0:
            raise PdfOpsError("gva_relation_backward: inverse table with a non-zero entry base")
        self._call("gva_relation_backward", int(n), nk, int(s), c, g_rel, query, key, idx, pem, off, ent, gq, gk, gp)
        return gq, gk, gp

    def gva_attend_forward(self, logits, value, peb, idx):
        n, s = idx.shape
        c, groups = int(value.shape[1]), int(logits.shape[2])
        out = torch.empty((n, c), dtype=torch.float32, device=value.device)
        p = torch.empty((n, s, groups), dtype=torch.float32, device=value.device)
        self._call("gva_attend_forward", int(n), int(value.shape[0]), int(s), c, groups, logits, value, peb, idx, out, p)
        return out, p

    def gva_attend_backward(self, g_out, p, value, peb, idx, need_value, need_peb):
        n, s = idx.shape
        nv, c, groups = int(value.shape[0]), int(value.shape[1]), int(p.shape[2])
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=value.device)
        gl = new(n, s, groups)
        gv = new(nv, c) if need_value else None
        gp = new(n, s, c) if need_peb and peb is not None else None
        off, ent, base = inverse_table(idx, nv) if need_value else (None, None, 0)
        if base != 0:
            raise PdfOpsError("gva_attend_backward: inverse table with a non-zero entry base")
        self._call("gva_attend_backward", int(n), nv, int(s), c, groups, g_out, p, value, peb, idx, off, ent, gl, gv, gp)
        return gl, gv, gp

    # ---- PointTransformer-V3: serialization, pooling partition, patch attention (csrc/serialization.hip, csrc/serial_attention.hip) ----
    SERIAL_ORDERS = {"z": 0, "z-trans": 1, "hilbert": 2, "hilbert-trans": 3}

    def serial_attn_supported(self, c, h, k):
        return bool(self.lib.pdf_serial_attn_supported(int(c), int(h), int(k)))

    def _serial_ws(self, n, device):
        return torch.empty(int(self.lib.pdf_serial_workspace_bytes(n)), dtype=torch.uint8, device=device)

    def serial_codes(self, grid_coord, batch, depth, orders):
        """grid_coord (n, 3) int32, batch (n) int64 -> code (k, n) int64, one row per curve name in ``orders``."""
        _check(grid_coord, torch.int32, "grid_coord"); _check(batch, torch.int64, "batch")
        n, k = int(grid_coord.shape[0]), len(orders)
        if not 1 <= k <= 8:
            raise ValueError("serial_codes: 1 to 8 orders")
        packed = 0
        for j, o in enumerate(orders):
            packed |= self.SERIAL_ORDERS[o] << (4 * j)
        code = torch.empty((k, n), dtype=torch.int64, device=grid_coord.device)
        self._call("serial_codes", n, k, packed, int(depth), grid_coord, batch, code)
        return code

    def serial_sort(self, code):
        """code (k, n) int64 (non-negative) -> (order, inverse), both (k, n) int64; equal codes keep row order."""
        _check(code, torch.int64, "code")
        k, n = code.shape
        order, inverse = torch.empty_like(code), torch.empty_like(code)
        if n:
            self._call("serial_sort", int(n), int(k), code, order, inverse, self._serial_ws(int(n), code.device))
        return order, inverse

    def serial_pool_partition(self, code0, order0, shift):
        """-> (cluster (n) int64, sorted (n) int32, idx_ptr (m + 1) int32, head (m) int64, m).  One host read: the cluster count."""
        _check(code0, torch.int64, "code"); _check(order0, torch.int64, "order")
        n, dev = int(code0.shape[0]), code0.device
        cluster = torch.empty(n, dtype=torch.int64, device=dev)
        srt = torch.empty(n, dtype=torch.int32, device=dev)
        idx_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        head = torch.empty(n, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        self._call("serial_pool_partition", n, int(shift), code0, order0, cluster, srt, idx_ptr, head, count, self._serial_ws(n, dev))
        m = int(count.item())
        return cluster, srt, idx_ptr[:m + 1], head[:m], m

    def serial_attn_forward(self, qkv, order, qtab, h, scale):
        _check(qkv, torch.float32, "qkv"); _check(order, torch.int64, "order"); _check(qtab, torch.int32, "qtab")
        n, c = int(qkv.shape[0]), int(qkv.shape[1]) // 3
        out = torch.empty((n, c), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((n, h, 2), dtype=torch.float32, device=qkv.device)   # (row maximum, sum of exp(s - maximum))
        self._call("serial_attn_forward", n, c, int(h), float(scale), qkv, order, qtab, int(qtab.shape[0]), out, lse)
        return out, lse

    def serial_attn_backward(self, qkv, out, lse, g_out, order, qtab, ktab, h, scale):
        _check(g_out, torch.float32, "g_out"); _check(ktab, torch.int32, "ktab")
        n, c = int(qkv.shape[0]), int(qkv.shape[1]) // 3
        delta = torch.empty((n, h), dtype=torch.float32, device=qkv.device)
        g_qkv = torch.empty_like(qkv)
        self._call("serial_attn_backward", n, c, int(h), float(scale), qkv, out, lse, g_out, order, qtab, int(qtab.shape[0]), ktab,
                   int(ktab.shape[0]), delta, g_qkv)
        return g_qkv

    # ---- PointGroup: ball table, clustering, proposals, intersection table, bias losses (csrc/point_group.hip) ----
    def pg_ball_table(self, coords, offset, radius):
        """coords (n, 3) fp32, offset (b) int32 scene ends -> (idx (total) int32, start_len (n, 2) int32): ballquery_batch_p as CSR, rows in
        ascending index, cut at 1,000.  One host read (the total)."""
        _check(coords, torch.float32, "coords"); _check(offset, torch.int32, "offset")
        n, b, dev = int(coords.shape[0]), int(offset.shape[0]), coords.device
        start_len = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=dev), start_len
        if not radius > 0:
            raise ValueError("pg_ball_table: radius must be positive")
        nbytes = int(self.lib.pdf_pg_ball_workspace_bytes(n, b))
        if nbytes <= 0:
            raise PdfOpsError(f"pg_ball_table: {b} scenes (1 to 64 supported)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        self._call("pg_ball_count", n, b, float(radius), coords, offset, start_len, total, ws, nbytes)
        t = int(total.item())
        if t >= 2 ** 31:
            raise PdfOpsError(f"pg_ball_table: {t} table entries do not fit the int32 starts of start_len")
        idx = torch.empty(t, dtype=torch.int32, device=dev)
        self._call("pg_ball_fill", n, b, float(radius), coords, offset, start_len, t, idx, ws, nbytes)
        return idx, start_len

    def pg_cluster(self, label, idx, start_len, threshold, with_stats=False):
        """bfs_cluster on the device -> (cluster_idxs (s, 2) int32, cluster_offsets (c + 1) int32); members in ascending index."""
        _check(label, torch.int32, "semantic_label"); _check(idx, torch.int32, "ball_query_idxs"); _check(start_len, torch.int32, "start_len")
        n, dev = int(start_len.shape[0]), label.device
        if label.shape[0] != n:
            raise ValueError("pg_cluster: one label per row of start_len")
        if n == 0:
            out = torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            return out + ({"rounds": 0},) if with_stats else out
        i32 = torch.empty((4, n + 1), dtype=torch.int32, device=dev)
        code = torch.empty((1, n), dtype=torch.int64, device=dev)
        info = torch.empty(3, dtype=torch.int64, device=dev)
        counters = torch.empty(64, dtype=torch.int32, device=dev)
        self._call("pg_cluster_labels", n, label, idx if idx.numel() else None, int(idx.numel()), start_len, int(threshold), i32[0], i32[1], i32[2], i32[3],
                   code, info, counters)
        c, s, rounds = (int(v) for v in info.tolist())
        cluster_idxs = torch.empty((s, 2), dtype=torch.int32, device=dev)
        if s:
            order, _ = self.serial_sort(code)
            self._call("pg_cluster_fill", n, s, code, order, cluster_idxs)
        offsets = i32[3, :c + 1].clone()
        return (cluster_idxs, offsets, {"rounds": rounds, "labels": i32[0, :n]}) if with_stats else (cluster_idxs, offsets)

    def pg_proposals(self, cluster_idxs, cluster_offsets, label, object_idxs, prob, propose_points, want_masks=False):
        """Lines 140-170 of point_group_v1m1_base.py on the compact clusters -> dict(offsets (p + 1) int32, members int32, proposal_of (npts)
        int32, classes (p) int64, scores (p) fp32, masks (p, npts) int32 or None).  One host read (the counts)."""
        _check(cluster_idxs, torch.int32, "cluster_idxs"); _check(cluster_offsets, torch.int32, "cluster_offsets"); _check(label, torch.int32, "label")
        _check(prob, torch.float32, "prob")
        if object_idxs is not None:
            _check(object_idxs, torch.int64, "object_idxs")
        nc, dev = int(cluster_offsets.shape[0]) - 1, prob.device
        npts, k = int(prob.shape[0]), int(prob.shape[1])
        rank = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)
        new_offs = torch.empty(nc + 1, dtype=torch.int32, device=dev)
        info = torch.empty(2, dtype=torch.int64, device=dev)
        self._call("pg_proposals_select", nc, cluster_offsets, int(propose_points), rank, new_offs, info)
        p, s = (int(v) for v in info.tolist())
        members = torch.empty(s, dtype=torch.int32, device=dev)
        prop_of = torch.full((npts,), -1, dtype=torch.int32, device=dev)
        classes = torch.empty(p, dtype=torch.int64, device=dev)
        scores = torch.empty(p, dtype=torch.float32, device=dev)
        masks = torch.zeros((p, npts), dtype=torch.int32, device=dev) if want_masks else None
        if p:
            self._call("pg_proposals_fill", nc, npts, k, int(cluster_idxs.shape[0]), cluster_idxs, cluster_offsets, rank, new_offs, label, int(label.shape[0]), object_idxs, prob,
                       members, prop_of, classes, scores, masks)
        return dict(offsets=new_offs[:p + 1].clone(), members=members, proposal_of=prop_of, classes=classes, scores=scores, masks=masks)

    def pg_intersections(self, prop_of, nprop, slot, nslots, isvoid, index_map=None):
        """-> (table (nprop, nslots), vert_count (nprop), void_intersection (nprop)), int32: the counts of associate_instances."""
        _check(prop_of, torch.int32, "proposal_of"); _check(slot, torch.int32, "slot"); _check(isvoid, torch.bool, "void mask")
        if index_map is not None:
            _check(index_map, torch.int64, "index map")
        dev, m = prop_of.device, int(slot.shape[0])
        table = torch.zeros((nprop, nslots), dtype=torch.int32, device=dev)
        vert = torch.zeros(nprop, dtype=torch.int32, device=dev)
        voidc = torch.zeros(nprop, dtype=torch.int32, device=dev)
        if m and nprop and prop_of.numel():
            self._call("pg_intersections", m, int(prop_of.shape[0]), int(nprop), int(nslots), prop_of, index_map, slot, isvoid,
                       table if nslots else None, vert, voidc)
        return table, vert, voidc

    def pg_bias_loss_forward(self, pred, coord, centroid, instance, ignore):
        _check(pred, torch.float32, "bias_pred"); _check(coord, torch.float32, "coord"); _check(instance, torch.int64, "instance")
        if centroid.dtype not in (torch.float32, torch.float64) or not centroid.is_contiguous():
            raise TypeError("pg_bias_loss: instance_centroid must be a contiguous float32 or float64 tensor")
        n, dev = int(pred.shape[0]), pred.device
        if tuple(pred.shape) != (n, 3) or tuple(coord.shape) != (n, 3) or tuple(centroid.shape) != (n, 3) or tuple(instance.shape) != (n,):
            raise ValueError("pg_bias_loss: bias_pred, coord, instance_centroid (n, 3) and instance (n)")
        f64 = centroid.dtype == torch.float64
        d = torch.empty((2, n, 3), dtype=torch.float32, device=dev)
        acc = torch.empty(int(self.lib.pdf_pg_bias_loss_workspace_doubles()), dtype=torch.float64, device=dev)
        loss = torch.empty(2, dtype=centroid.dtype, device=dev)
        self._call("pg_bias_loss_forward", n, pred if n else None, coord if n else None, centroid if n else None, int(f64), instance if n else None,
                   int(ignore), d[0] if n else None, d[1] if n else None, acc, loss)
        return loss, d, acc

    def pg_bias_loss_backward(self, d, acc, gy):
        n = int(d.shape[1])
        grad = torch.empty((n, 3), dtype=torch.float32, device=d.device)
        if n:
            self._call("pg_bias_loss_backward", n, d[0], d[1], acc, gy.contiguous(), int(gy.dtype == torch.float64), grad)
        return grad

    # -- csrc/scene_contrast.hip (MSC-v1m1) ---------------------------------------------------------------------------------------------
    def msc_nce_supported(self, c):
        return bool(self.lib.pdf_msc_nce_supported(int(c)))

    @staticmethod
    def _msc_nce_check(feat1, feat2, match):
        _check(feat1, torch.float32, "feat1"); _check(feat2, torch.float32, "feat2"); _check(match, torch.int64, "match_index")
        p, c = int(match.shape[0]), int(feat1.shape[1])
        if feat1.dim() != 2 or tuple(feat2.shape[1:]) != (c,) or tuple(match.shape) != (p, 2) or p < 1:
            raise ValueError("msc_nce: feat1 (n1, c), feat2 (n2, c) and match_index (p >= 1, 2)")
        return p, c

    def msc_nce_forward(self, feat1, feat2, match, temperature):
        """-> out (3) = {loss, pos_sim, neg_sim}, saved (what the backward reads: normalised rows, norms, lse)."""
        p, c = self._msc_nce_check(feat1, feat2, match)
        dev = feat1.device
        saved = torch.empty(int(self.lib.pdf_msc_nce_saved_floats(p, c)), dtype=torch.float32, device=dev)
        nbytes = int(self.lib.pdf_msc_nce_workspace_bytes(p, c, 0))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        self._call("msc_nce_forward", p, c, int(feat1.shape[0]), int(feat2.shape[0]), feat1, feat2, match, float(temperature), saved, out, ws, nbytes)
        return out, saved

    def msc_nce_backward(self, feat1, feat2, match, temperature, saved, gy):
        """-> d feat1, d feat2: every row written by the pass (no memset in front)."""
        p, c = self._msc_nce_check(feat1, feat2, match)
        _check(gy, torch.float32, "grad of the loss")
        dev = feat1.device
        g1, g2 = torch.empty_like(feat1), torch.empty_like(feat2)
        nbytes = int(self.lib.pdf_msc_nce_workspace_bytes(p, c, 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._call("msc_nce_backward", p, c, int(feat1.shape[0]), int(feat2.shape[0]), feat1, feat2, match, float(temperature), saved, gy,
                   g1 if g1.numel() else None, g2 if g2.numel() else None, ws, nbytes)
        return g1, g2

    def msc_recon_supported(self, c):
        return bool(self.lib.pdf_msc_recon_supported(int(c)))

    @staticmethod
    def _msc_recon_check(feat1, feat2, mask1, mask2, weight):
        _check(feat1, torch.float32, "view1 feat"); _check(feat2, torch.float32, "view2 feat"); _check(weight, torch.float32, "weight")
        _check(mask1, torch.bool, "view1 mask"); _check(mask2, torch.bool, "view2 mask")
        n1, n2, c = int(feat1.shape[0]), int(feat2.shape[0]), int(weight.shape[1])
        if (tuple(feat1.shape) != (n1, c) or tuple(feat2.shape) != (n2, c) or tuple(weight.shape) != (3, c) or tuple(mask1.shape) != (n1,)
                or tuple(mask2.shape) != (n2,)):
            raise ValueError("msc_recon: feat (n, c), masks (n), weight (3, c)")
        return n1, n2, c

    def msc_recon_forward(self, kind, feat1, feat2, mask1, mask2, weight, bias, target1, target2):
        """kind 0 color / 1 normal -> loss (1), dpred (n1 + n2, 3), acc (the backward's state)."""
        n1, n2, c = self._msc_recon_check(feat1, feat2, mask1, mask2, weight)
        _check(bias, torch.float32, "bias"); _check(target1, torch.float32, "view1 target"); _check(target2, torch.float32, "view2 target")
        if tuple(bias.shape) != (3,) or tuple(target1.shape) != (n1, 3) or tuple(target2.shape) != (n2, 3):
            raise ValueError("msc_recon: bias (3), targets (n, 3)")
        dev = weight.device
        dpred = torch.empty((n1 + n2, 3), dtype=torch.float32, device=dev)
        acc = torch.empty(int(self.lib.pdf_msc_recon_acc_doubles()), dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        self._call("msc_recon_forward", n1, n2, c, int(kind), feat1 if n1 else None, feat2 if n2 else None, mask1 if n1 else None,
                   mask2 if n2 else None, weight, bias, target1 if n1 else None, target2 if n2 else None, dpred if n1 + n2 else None, acc, loss)
        return loss, dpred, acc

    def msc_recon_backward(self, feat1, feat2, mask1, mask2, weight, dpred, acc, gy):
        """-> d feat1, d feat2 (zero rows where unmasked), d weight (3, c), d bias (3)."""
        n1, n2, c = self._msc_recon_check(feat1, feat2, mask1, mask2, weight)
        _check(gy, torch.float32, "grad of the loss")
        dev = weight.device
        g1, g2 = torch.empty_like(feat1), torch.empty_like(feat2)
        gw, gb = torch.empty_like(weight), torch.empty(3, dtype=torch.float32, device=dev)
        slab = torch.empty(int(self.lib.pdf_msc_recon_slab_floats(n1 + n2, c)), dtype=torch.float32, device=dev)
        self._call("msc_recon_backward", n1, n2, c, feat1 if n1 else None, feat2 if n2 else None, mask1 if n1 else None, mask2 if n2 else None,
                   weight, dpred if n1 + n2 else None, acc, gy, g1 if n1 else None, g2 if n2 else None, gw, gb, slab)
        return g1, g2, gw, gb


_lock = threading.Lock()
_hip = None
_override = None  # set only by tests / the CPU-baseline leg (oracle injection)


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise PdfOpsError(
            f"pointcloudpdf_amd: {path} is missing. Build it with `python -m pointcloudpdf_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no fallback implementation."
        )
    return ctypes.CDLL(path)


def hip_backend():
    global _hip
    if _hip is None:
        with _lock:
            if _hip is None:
                _hip = HipBackend(load_library())
    return _hip


# Input precision of the matrix-core products of the streaming Linear kernels (include/pdfops.h: `mma_input`): 0 fp32 operands (the
# parity path), 1 fp16, 2 bfloat16 -- fp32 storage and accumulation in every mode.  The mode is an ARGUMENT of every C entry point that
# runs those products; on the Python side it is state of the CALLING THREAD (a thread-local, so a forward on one thread and an autograd
# backward on another never see each other's mode -- round 3 kept it in a process-wide word inside the library).  ``dense.fp32_path``
# selects 1 / 2 for a forward that runs under torch.autocast(float16 / bfloat16); every autograd node remembers the mode of its forward
# and runs its backward in it.
_MMA = threading.local()
MMA_INPUT_OF_DTYPE = {torch.float16: 1, torch.bfloat16: 2}


def current_mma_input():
    return getattr(_MMA, "mode", 0)


class mma_input:
    """``with mma_input(mode):`` -- product-input mode of the launches this THREAD issues inside the block."""

    def __init__(self, mode):
        self.mode = int(mode)
        if self.mode not in (0, 1, 2):
            raise PdfOpsError(f"mma_input({mode}): expected 0 (fp32), 1 (fp16) or 2 (bfloat16) operands")

    def __enter__(self):
        self.prev = current_mma_input()
        _MMA.mode = self.mode
        return self

    def __exit__(self, *exc):
        _MMA.mode = self.prev
        return False


def backend_for(t):
    """The backend that must serve tensor ``t``.  CPU tensors raise unless a test injected a backend."""
    if _override is not None:
        return _override
    if t.device.type == "cuda":
        return hip_backend()
    raise PdfOpsError(
        f"pointcloudpdf_amd: got a tensor on '{t.device}'. The product path is HIP-only (MI355X); "
        "move inputs to a ROCm device."
    )


def _set_backend_for_testing(backend):
    """TEST / CPU-BASELINE ONLY: route every op through ``backend`` (e.g. the CPU oracle). Returns the previous one."""
    global _override
    prev, _override = _override, backend
    return prev

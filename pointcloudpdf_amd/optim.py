"""Optimizers and the reference's optimizer / scheduler builders (pointcept/utils/optimizer.py, pointcept/utils/scheduler.py).

``FusedOptimizer`` is what ``engine.FusedSGD`` and ``FusedAdam`` / ``FusedAdamW`` share: one HIP launch per parameter group over a
device table of per-tensor records and a ``{tensor, chunk}`` list (csrc/optim.hip), with the host side -- a pinned ring of pointer
tables, cached chunk plans, tables reserved for captured steps, the hand-over of an ``unscale_``'s tables to the ``step()`` of the
same iteration -- written once.  ``build_optimizer`` / ``build_scheduler`` build the fused classes and torch's schedulers from the
reference's config dicts."""
import os

import torch

from .registry import Registry


class FusedOptimizer(torch.optim.Optimizer):
    """Host side of the one-launch optimizers.  A subclass names the width of its record in int64 words (``COLS``), the library entry
    that unscales gradients over that record (``UNSCALE``), fills the state columns of the table (``_state_columns``) and launches in
    ``step()``.  Parameter, gradient and state pointers are read at every step (``model.to()``, ``load_state_dict`` may move them)."""

    RING = 8       # pinned pointer tables in flight (the host may run several steps ahead of the device)
    COLS = 4       # int64 words per record: {param, grad, <state ...>, length, <padding>}
    LENGTH_COL = 3
    UNSCALE = "pdf_grad_unscale"

    def __init__(self, params, defaults, backend=None):
        from . import _native

        self.be = backend if backend is not None else _native.hip_backend()   # (backend: tests of the host logic without a GPU)
        self._rows = 0
        self._ring, self._tabs, self._spare, self._captured, self._plans, self._n = [], [], [], [], {}, 0
        super().__init__(params, defaults)
        every = [p for group in self.param_groups for p in group["params"]]
        assert every and all(p.dtype == torch.float32 and p.is_contiguous() for p in every)
        self.device = every[0].device
        for p in every:
            self._init_state(p)
        self._table_cache, self._table_cache_on = {}, os.environ.get("PDFOPS_SGD_TABLE_CACHE") != "0"
        self.chunk = int(self.be.lib.pdf_sgd_chunk()) if self.be is not None else 4096
        self._size_tables()
        self.reserve_capture_tables(2 * len(self.param_groups))

    def _init_state(self, p):
        raise NotImplementedError

    def _state_columns(self, rows, ps):
        """Write the state pointers of parameters ``ps`` into ``rows`` (normalising state that moved or changed dtype first)."""
        raise NotImplementedError

    def add_param_group(self, param_group):
        """torch.optim.Optimizer.add_param_group + the pointer tables re-sized for the largest group (they are pinned once, not per step)."""
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        group["params"] = [p for p in group["params"] if p.requires_grad]
        if self._rows:   # (during __init__ the tables are sized once, after every group is in)
            self._size_tables()

    def _pin(self):
        return (lambda t: t.pin_memory()) if self.device.type == "cuda" else (lambda t: t)

    def _size_tables(self):
        rows = max(len(g["params"]) for g in self.param_groups)
        if rows <= self._rows:
            return
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.add_param_group: pinning host memory is not allowed during stream capture")
        for _, ev in self._ring:   # tables of steps still in flight stay alive until their launch has run
            if ev is not None:
                ev.synchronize()
        self._rows = rows
        pin, cols = self._pin(), self.COLS
        self._ring = [(pin(torch.zeros((rows, cols), dtype=torch.int64)), torch.cuda.Event() if self.device.type == "cuda" else None)
                      for _ in range(self.RING)]
        self._tabs = [torch.empty((rows, cols), dtype=torch.int64, device=self.device) for _ in range(self.RING)]
        self._spare = [pin(torch.zeros((rows, cols), dtype=torch.int64)) for _ in self._spare]
        self._plans = {}

    def reserve_capture_tables(self, n):
        """Pinned pointer tables for ``n`` more (group, captured step) pairs; must be called outside stream capture."""
        pin = self._pin()
        self._spare += [pin(torch.zeros((self._rows, self.COLS), dtype=torch.int64)) for _ in range(n)]

    @property
    def params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _plan(self, gi, have, params):
        key = (gi, have)
        if key not in self._plans:
            import numpy as np

            pairs = [(row, c) for row, i in enumerate(have) for c in range((params[i].numel() + self.chunk - 1) // self.chunk)]
            lengths = np.array([params[i].numel() for i in have], dtype=np.int64)
            chunks = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2)
            if self.device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
                chunks = chunks.pin_memory().to(self.device, non_blocking=True)   # (the first step of a gradient pattern does not wait either)
            else:
                chunks = chunks.to(self.device)
            self._plans[key] = (chunks.contiguous(), len(pairs), lengths)
        return self._plans[key]

    def _tables(self, gi, group):
        """Device table of records + chunk list of group ``gi`` for the parameters that have a gradient now.
        -> (nchunks, tab, chunks, event | None, gradients kept alive) or None when no parameter of the group has a gradient."""
        from . import _native

        f32 = torch.float32
        params = group["params"]
        all_grads = [p.grad for p in params]   # (one attribute read per parameter and step: 304 of them)
        have = tuple(i for i, g in enumerate(all_grads) if g is not None)
        if not have:
            return None
        _native.require_current_device(self._tabs[0])   # (launches go onto the current device's current stream)
        chunks, nchunks, lengths = self._plan(gi, have, params)
        cols = self.COLS
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:   # a captured step replays this copy + launch: the tables must outlive the graph and never be rewritten
            if not self._spare:
                raise RuntimeError(f"{type(self).__name__}: more captured steps than pinned pointer tables (pinning host memory is not "
                                   "allowed during stream capture); call reserve_capture_tables(n) before capturing")
            host = self._spare.pop()
            tab, ev = torch.empty((len(have), cols), dtype=torch.int64, device=self.device), None
            self._captured.append((host, tab))
        else:
            slot = self._n % self.RING
            host, ev = self._ring[slot]
            tab = self._tabs[slot]
            self._n += 1
            ev.synchronize()   # (the copy AND the launch that last used this slot have run)
        full = len(have) == len(all_grads)
        grads = all_grads if full else [all_grads[i] for i in have]
        fixed = [g if (g.dtype is f32 and g.is_contiguous()) else g.float().contiguous() for g in grads]   # (alive until queued)
        ps = params if full else [params[i] for i in have]
        rows = host.numpy()[:len(have)]
        rows[:, 0] = [q.data_ptr() for q in ps]
        rows[:, 1] = [g.data_ptr() for g in fixed]
        self._state_columns(rows, ps)
        rows[:, self.LENGTH_COL] = lengths
        if not capturing and self._table_cache_on:
            # Replayed steps hand the SAME gradient tensors back every time: the table of the last step is then still right, and the host
            # -> device copy (19 KB through the copy engine, a cross-queue dependency in front of the optimizer launch: ~0.1 ms of idle
            # time on a quiet device, ~0.45 ms beside the pre-pass queues, profiles/r06_z_timeline.txt) is skipped.  The cached table is
            # its own device tensor, written only here.
            last = self._table_cache.get(gi)
            if last is not None and last[0].shape == rows.shape and (last[0] == rows).all():
                return nchunks, last[1], chunks, ev, fixed
            keep = torch.empty((len(have), cols), dtype=torch.int64, device=self.device)
            keep.copy_(host[:len(have)], non_blocking=True)
            self._table_cache[gi] = (rows.copy(), keep)
            return nchunks, keep, chunks, ev, fixed
        tab[:len(have)].copy_(host[:len(have)], non_blocking=True)
        return nchunks, tab, chunks, ev, fixed

    def _grad_key(self):
        return tuple(p.grad.data_ptr() if p.grad is not None else 0 for group in self.param_groups for p in group["params"])

    def _take_prepared(self):
        """The tables an ``unscale_`` of this iteration built, or None.  They are valid only for the gradients they were built from: an
        iteration that aborted between unscale_ and step, or re-assigned gradients, must not reuse stale pointer tables."""
        prepared, self._prepared = getattr(self, "_prepared", None), None
        if prepared is not None:
            key, prepared = prepared
            if key != self._grad_key():
                prepared = None
        return prepared


class FusedAdamW(FusedOptimizer):
    """``torch.optim.AdamW(params, lr, betas, eps, weight_decay)`` -- the optimizer of the reference's ScanNet and StratifiedTransformer
    configs (configs/scannet/openseg-pt-v1-0-*.py: lr 0.005, wd 0.02; openseg-st-v1m1-0-origin-*: lr 0.006 with a ``blocks`` group at
    a tenth of it) -- as TWO HIP launches per parameter group and step over all of the group's tensors (csrc/optim.hip: the per-tensor
    step counts, then the update), against a dozen or more multi-tensor launches of torch's own.  Per element it is the arithmetic of
    torch's single-tensor, non-capturable form (torch/optim/adam.py), all in fp32, the per-call scalars formed in double.

    A ``torch.optim.Optimizer``: the param groups carry every key torch.optim.AdamW's do; ``lr``, ``betas``, ``eps`` and
    ``weight_decay`` are read from the group at every step, so torch's schedulers attach -- OneCycleLR's writes to ``betas`` included,
    and the bias corrections use the betas of the call, as torch's do.  State is torch's: ``state[p] = {"step": 0-dim float32 tensor,
    "exp_avg", "exp_avg_sq"}``, so ``state_dict`` / ``load_state_dict`` move both ways.  The step counts live on the device and are
    advanced there, one per tensor: a parameter without a gradient is skipped and its count does not advance, a step skipped by
    ``found_inf`` leaves parameters, moments and counts untouched, and nothing in ``step()`` reads the device.  State that arrives on
    another device or in another dtype (a CPU-trained torch checkpoint: its ``step`` tensors stay on the CPU) is normalised at the next
    ``step()``; do that step outside stream capture.  ``amsgrad``, ``maximize`` and ``differentiable`` are refused at ``step()``."""

    COLS = 8       # {param, grad, exp_avg, exp_avg_sq, step, length, 0, 0}: 64 bytes
    LENGTH_COL = 5
    UNSCALE = "pdf_adam_grad_unscale"
    DECOUPLED = True
    # torch.optim.AdamW's other keys
    ADAM_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, backend=None, **options):
        unknown = set(options) - set(self.ADAM_DEFAULTS)
        if unknown:
            raise TypeError(f"{type(self).__name__}: unexpected arguments {sorted(unknown)}")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                                      **{**self.ADAM_DEFAULTS, **options}, decoupled_weight_decay=self.DECOUPLED), backend=backend)

    def _init_state(self, p):
        self.state[p].update(step=torch.zeros((), dtype=torch.float32, device=p.device), exp_avg=torch.zeros_like(p),
                             exp_avg_sq=torch.zeros_like(p))

    def _state_columns(self, rows, ps):
        f32 = torch.float32
        state = self.state
        cols = ([], [], [])
        for q in ps:
            st = state[q]
            for key, col in zip(("exp_avg", "exp_avg_sq"), cols):
                buf = st.get(key)
                if buf is None or buf.shape != q.shape or buf.device != q.device or buf.dtype is not f32 or not buf.is_contiguous():
                    buf = st[key] = torch.zeros_like(q) if buf is None else buf.to(q.device, f32).reshape(q.shape).contiguous()
                col.append(buf.data_ptr())
            step = st.get("step")
            if not torch.is_tensor(step) or step.device != q.device or step.dtype is not f32 or step.dim() != 0:
                # (a host value, a CPU tensor of a torch checkpoint, another dtype: host -> device only, nothing is read back)
                step = st["step"] = torch.as_tensor(0.0 if step is None else step).to(q.device, f32).reshape(())
            cols[2].append(step.data_ptr())
        rows[:, 2], rows[:, 3], rows[:, 4] = cols

    @torch.no_grad()
    def step(self, closure=None, found_inf=None):
        """``found_inf``: a device float (``DeviceGradScaler``): non-zero -> parameters, moments and step counts stay untouched."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        prepared = self._take_prepared()
        for gi, group in enumerate(self.param_groups):
            for option in ("amsgrad", "maximize", "differentiable"):
                if group.get(option, False):
                    raise RuntimeError(f"{name}: {option} is not implemented (the reference's configs do not use it)")
            t = prepared[gi] if prepared is not None else self._tables(gi, group)   # (unscale_ of the same iteration built them already)
            if t is None:
                continue
            nchunks, tab, chunks, ev, grads = t
            beta1, beta2 = group["betas"]
            # (one record per gradient: a ring table has the largest group's rows, and only the first len(grads) are written)
            self.be._launch("adam_step", nchunks, len(grads), tab.data_ptr(), chunks.data_ptr(), float(group["lr"]), float(beta1),
                            float(beta2), float(group["eps"]), float(group["weight_decay"]),
                            1 if group.get("decoupled_weight_decay", self.DECOUPLED) else 0,
                            None if found_inf is None else found_inf.data_ptr())
            if ev is not None:
                ev.record()
        return loss


class FusedAdam(FusedAdamW):
    """``torch.optim.Adam``: FusedAdamW with the weight decay in Adam's L2 form (``g += weight_decay * p``), default 0."""

    DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, backend=None, **options):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, backend=backend, **options)


# ---- builders --------------------------------------------------------------------------------------------------------------------

OPTIMIZERS = Registry("optimizers")   # "SGD" is engine.FusedSGD (registered there: it is defined on top of this module)
OPTIMIZERS.register_module(name="Adam", module=FusedAdam)
OPTIMIZERS.register_module(name="AdamW", module=FusedAdamW)


def build_optimizer(cfg, model, param_dicts=None):
    """pointcept/utils/optimizer.py: build_optimizer with the fused classes behind the names ``SGD`` / ``Adam`` / ``AdamW``.
    ``cfg``: ``dict(type=..., lr=..., ...)``.  Without ``param_dicts`` one group holds every trainable parameter.  With it, group
    ``i + 1`` holds the parameters whose name contains ``param_dicts[i]["keyword"]`` (the first entry that matches wins) under that
    entry's own ``lr`` / ``momentum`` / ``weight_decay`` where given, and group 0 the remainder at ``cfg["lr"]``.  Parameters with
    ``requires_grad=False`` (the incremental learner's teacher) are left out."""
    from . import engine  # noqa: F401  (registers "SGD")

    cfg = dict(cfg)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if param_dicts is None:
        cfg["params"] = [p for _, p in named]
    else:
        groups = [dict(params=[], lr=cfg["lr"])]
        for entry in param_dicts:
            groups.append(dict(params=[], **{k: entry[k] for k in ("lr", "momentum", "weight_decay") if k in entry}))
        for n, p in named:
            hit = next((i for i, entry in enumerate(param_dicts) if entry["keyword"] in n), -1)
            groups[hit + 1]["params"].append(p)
        cfg["params"] = groups
    return OPTIMIZERS.build(cfg)


def _fractions(milestones, total_steps):
    return [rate * total_steps for rate in milestones]


def multi_step_lr(optimizer, milestones, total_steps, gamma=0.1, last_epoch=-1):
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=_fractions(milestones, total_steps), gamma=gamma, last_epoch=last_epoch)


def multi_step_with_warmup_lr(optimizer, milestones, total_steps, gamma=0.1, warmup_rate=0.05, warmup_scale=1e-6, last_epoch=-1):
    """MultiStepLR times a linear ramp from ``warmup_scale`` to 1 over the first ``warmup_rate * total_steps`` steps."""
    marks = _fractions(milestones, total_steps)

    def factor(s):
        decay = gamma ** sum(1 for m in marks if s >= m)
        if s <= warmup_rate * total_steps:
            return (1 - (1 - s / warmup_rate / total_steps) * (1 - warmup_scale)) * decay
        return decay

    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=factor, last_epoch=last_epoch)


def poly_lr(optimizer, total_steps, power=0.9, last_epoch=-1):
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda s: (1 - s / (total_steps + 1)) ** power, last_epoch=last_epoch)


def exp_lr(optimizer, total_steps, gamma=0.9, last_epoch=-1):
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda s: gamma ** (s / total_steps), last_epoch=last_epoch)


def cosine_annealing_lr(optimizer, total_steps, eta_min=0, last_epoch=-1):
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=total_steps, eta_min=eta_min, last_epoch=last_epoch)


def one_cycle_lr(optimizer, max_lr, total_steps=None, pct_start=0.3, anneal_strategy="cos", cycle_momentum=True, base_momentum=0.85,
                 max_momentum=0.95, div_factor=25.0, final_div_factor=1e4, three_phase=False, last_epoch=-1):
    return torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=max_lr, total_steps=total_steps, pct_start=pct_start,
                                               anneal_strategy=anneal_strategy, cycle_momentum=cycle_momentum, base_momentum=base_momentum,
                                               max_momentum=max_momentum, div_factor=div_factor, final_div_factor=final_div_factor,
                                               three_phase=three_phase, last_epoch=last_epoch)


# The reference's six schedulers (pointcept/utils/scheduler.py: same names, same constructor defaults) as factories over the installed
# torch's torch.optim.lr_scheduler (no ``verbose`` argument: torch dropped it).
SCHEDULERS = dict(MultiStepLR=multi_step_lr, MultiStepWithWarmupLR=multi_step_with_warmup_lr, PolyLR=poly_lr, ExpLR=exp_lr,
                  CosineAnnealingLR=cosine_annealing_lr, OneCycleLR=one_cycle_lr)


def build_scheduler(cfg, optimizer, total_steps):
    """``cfg``: ``dict(type="OneCycleLR", max_lr=..., ...)`` as in the reference's configs; ``total_steps``: what the reference's trainer
    writes into the config before it builds (iterations per epoch x epochs); milestones are fractions of it.  The scheduler is
    stepped once per iteration (engines/train.py:366)."""
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in SCHEDULERS:
        raise KeyError(f"{kind} is not a scheduler of this package ({', '.join(sorted(SCHEDULERS))})")
    args.pop("total_steps", None)
    return SCHEDULERS[kind](optimizer, total_steps=int(total_steps), **args)

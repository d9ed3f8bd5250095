"""Optimizer construction (optim.py): parameter groups with the reference's
no-decay rule and multi-tensor (foreach) update kernels.

Quirk kept from the reference: build_optimizer is handed the Composer wrapper,
which has no `no_weight_decay`, so the skip set is always empty and 3-D
`logit_scale` is decayed (optim.py:9-14, 53)."""
import torch

from .options import OPTIONS


def set_weight_decay(model, skip_list=()):
    """1-D params and `.bias` -> no decay (optim.py:48-58)."""
    has_decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if len(param.shape) == 1 or name.endswith(".bias") or (name in skip_list):
            no_decay.append(param)
        else:
            has_decay.append(param)
    return [{"params": has_decay}, {"params": no_decay, "weight_decay": 0.0}]


class _HandoverOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the hand-overs of the step's other per-parameter passes
    (``pending_grad_scale``: 1/world, the DDP buckets hold gradient SUMS, ddp.py;
    ``pending_clip``: GradientClipping's norm threshold; ``pending_ema``: the EMA algorithm's
    averaged copies on the batches it updates them), all reset after every step, and graph
    mode's device array of per-step hyper-parameters with its pinned staging ring.

    A subclass sets HYPER_FLOATS and provides _hyper_array() (that many floats, the layout its
    kernel reads), _fused_eligible(), _fused_step() -> done and _foreach_step()."""

    HYPER_FLOATS = 8

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self.pending_clip = None  # global-norm threshold handed over by GradientClipping
        self.pending_grad_scale = 1.0  # gradient multiplier handed over by the trainer (DDP mean)
        self.pending_ema = None  # ([(id(param), ema tensor)], smoothing) from the EMA algorithm
        self.device_hyper = False  # graph mode: hyper-parameters read from a device array at run time
        self._hyper = None
        self._fused = None

    def supports_fused_clip(self):
        return True

    def supports_grad_scale(self):
        return True

    def supports_fused_ema(self, params):
        """The fused step can apply an EMA over exactly these parameters when every one of them
        is in a param group (the trainer asks before handing the EMA over)."""
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        return self._fused_eligible() and mine == {id(p) for p in params}

    def _tensors_fusable(self):
        """Every parameter with a gradient is a contiguous f32 CUDA tensor, in <= 4 groups."""
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.grad.dtype == torch.float32
                        and p.is_contiguous() and p.grad.is_contiguous()):
                    return False
        return len(self.param_groups) <= 4

    def enable_device_hyper(self, device):
        """Graph mode (trainer.capture): the fused update reads its per-step hyper-parameters
        from a device array instead of kernel arguments, so a schedule still applies to
        captured replays."""
        n = self.HYPER_FLOATS
        self._hyper = torch.tensor(self._hyper_array(), dtype=torch.float32, device=device)
        self._hyper_ring = [(torch.empty(n, dtype=torch.float32).pin_memory(), None) for _ in range(4)]
        self._hyper_slot = 0
        self.device_hyper = True
        self.hyper_used = False

    def refresh_hyper(self):
        """Copy the current hyper-parameters of every group into that device array,
        stream-ordered before the next replay (a ring of pinned staging buffers: no host sync
        per step)."""
        if self._hyper is None:
            return
        host, ev = self._hyper_ring[self._hyper_slot]
        if ev is not None:
            ev.synchronize()  # that slot's previous copy (4 steps ago) has been consumed
        host.copy_(torch.tensor(self._hyper_array(), dtype=torch.float32))
        self._hyper.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_ring[self._hyper_slot] = (host, ev)
        self._hyper_slot = (self._hyper_slot + 1) % len(self._hyper_ring)

    def _live_hyper_ptr(self):
        """The device array, inside a capture only (replay() refreshes it); an eager step takes
        the current values as arguments, so a schedule change is never missed."""
        from . import _lib
        if self.device_hyper and self._hyper is not None and torch.cuda.is_current_stream_capturing():
            self.hyper_used = True
            return _lib.ptr(self._hyper)
        return None

    def _workspace(self, nbytes, device):
        if self._fused is None or self._fused.numel() * 4 < nbytes:
            self._fused = torch.empty(nbytes // 4, device=device, dtype=torch.float32)
        return self._fused

    def _apply_pending_grads(self, params):
        """The unfused form of the gradient hand-overs: scale, then clip as GradientClipping would."""
        if self.pending_grad_scale != 1.0 and params:
            torch._foreach_mul_([p.grad for p in params], float(self.pending_grad_scale))
        if self.pending_clip is not None:
            torch.nn.utils.clip_grad_norm_(params, self.pending_clip, foreach=True)

    def _apply_pending_ema(self, params):
        if self.pending_ema is not None:
            emas, a = self.pending_ema
            by_id = dict(emas)
            ps = [p for p in params if id(p) in by_id]
            es = [by_id[id(p)] for p in ps]
            torch._foreach_mul_(es, a)
            torch._foreach_add_(es, ps, alpha=1 - a)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        try:
            if self._fused_eligible() and self._fused_step():
                return loss
            self._foreach_step()
        finally:
            self.pending_clip = None
            self.pending_grad_scale = 1.0
            self.pending_ema = None
        return loss


class DecoupledSGDW(_HandoverOptimizer):
    """SGD + momentum with weight decay decoupled from the gradient and scaled by
    lr / initial_lr (composer.optim.DecoupledSGDW semantics).

    On the GPU one step is libhvk's fused hvk_sgdw_step (include/hvk.h), which also takes the
    hand-overs of the step's other per-parameter passes (_HandoverOptimizer) so none of them
    reads the 141 MB of gradients or weights again.  Elsewhere the same step runs as foreach
    passes."""

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov, initial_lr=lr)
        super().__init__(params, defaults)

    def _fused_eligible(self):
        if not OPTIONS.fused_optim:  # A/B runs: the foreach path
            return False
        gs = self.param_groups
        if not gs or any(g["nesterov"] != gs[0]["nesterov"] or g["momentum"] != gs[0]["momentum"]
                         or g["dampening"] != gs[0]["dampening"] for g in gs):
            return False
        return self._tensors_fusable() and gs[0]["momentum"] != 0

    def _hyper_values(self):
        gs = self.param_groups
        lr = [float(g["lr"]) for g in gs] + [0.0] * (4 - len(gs))
        decay = [1.0 - g["weight_decay"] * g["lr"] / g["initial_lr"] if g["weight_decay"] else 1.0
                 for g in gs] + [1.0] * (4 - len(gs))
        return lr, decay

    def _hyper_array(self):
        lr, decay = self._hyper_values()
        return lr + decay

    def _fused_step(self):
        """Mean + clip + update (+ EMA) of every tensor in a handful of libhvk launches
        (hvk_sgdw_step); False (nothing done) when only some momentum buffers exist yet."""
        import ctypes
        from . import _lib
        ps, grp = [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.grad is not None:
                    ps.append(p)
                    grp.append(gi)
        if not ps:
            return True
        fresh = ["momentum_buffer" not in self.state[p] for p in ps]
        if any(fresh) and not all(fresh):
            return False
        first = all(fresh)
        if first:  # torch SGD semantics: the first step's buffer is the (clipped) gradient
            for p in ps:
                self.state[p]["momentum_buffer"] = torch.empty_like(p)
        n = len(ps)
        P = ctypes.c_void_p * n
        numel = (ctypes.c_longlong * n)(*[p.numel() for p in ps])
        arrs = [P(*[p.data_ptr() for p in ps]), P(*[p.grad.data_ptr() for p in ps]),
                P(*[self.state[p]["momentum_buffer"].data_ptr() for p in ps])]
        ema_arr, ema_a = None, 0.0
        if self.pending_ema is not None:
            emas, ema_a = self.pending_ema
            by_id = dict(emas)
            ema_arr = P(*[by_id[id(p)].data_ptr() for p in ps])
        gs = self.param_groups
        lr_v, decay_v = self._hyper_values()
        lr = (ctypes.c_float * 4)(*lr_v)
        decay = (ctypes.c_float * 4)(*decay_v)
        hyper = self._live_hyper_ptr()
        lib = _lib.load()
        nb = lib.hvk_sgdw_workspace_bytes(n, ctypes.cast(numel, ctypes.c_void_p))
        ws = self._workspace(nb, ps[0].device)
        clip = float(self.pending_clip) if self.pending_clip is not None else 0.0
        g0 = gs[0]
        self._keep = (arrs, ema_arr, numel)  # ctypes tables outlive the call
        _lib.call("hvk_sgdw_step", n, *[ctypes.cast(a, ctypes.c_void_p) for a in arrs],
                  ctypes.cast(ema_arr, ctypes.c_void_p) if ema_arr is not None else None,
                  ctypes.cast(numel, ctypes.c_void_p), ctypes.cast((ctypes.c_int * n)(*grp), ctypes.c_void_p),
                  ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(decay, ctypes.c_void_p), len(gs), hyper,
                  float(self.pending_grad_scale), clip, float(g0["momentum"]), float(g0["dampening"]),
                  int(bool(g0["nesterov"])), int(first), float(ema_a), _lib.ptr(ws), nb,
                  _lib.stream())
        # the kernel wrote the weights through raw pointers: bump their version counters so
        # version-keyed caches (ops._WeightCopies) see the update
        torch.autograd.graph.increment_version(ps)
        return True

    def _foreach_step(self):
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        self._apply_pending_grads(params)  # unfused: scale and clip now
        for g in self.param_groups:
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            grads = [p.grad for p in ps]
            lr, mom, wd = g["lr"], g["momentum"], g["weight_decay"]
            if mom != 0:
                fresh = [p for p in ps if "momentum_buffer" not in self.state[p]]
                seen = set(map(id, fresh))
                old = [p for p in ps if id(p) not in seen]
                for p in fresh:  # first step: buffer = grad (torch.optim.SGD semantics)
                    self.state[p]["momentum_buffer"] = p.grad.detach().clone()
                if old:
                    bl = [self.state[p]["momentum_buffer"] for p in old]
                    torch._foreach_mul_(bl, mom)
                    torch._foreach_add_(bl, [p.grad for p in old], alpha=1 - g["dampening"])
                bl = [self.state[p]["momentum_buffer"] for p in ps]
                grads = torch._foreach_add(grads, bl, alpha=mom) if g["nesterov"] else bl
            if wd != 0:
                torch._foreach_mul_(ps, 1 - wd * lr / g["initial_lr"])
            torch._foreach_add_(ps, grads, alpha=-lr)
        self._apply_pending_ema(params)


class AdamW(_HandoverOptimizer):
    """AdamW with torch.optim.AdamW's state (``step``, ``exp_avg``, ``exp_avg_sq``) and
    arithmetic; weight decay 1 - lr wd per step (torch), or with ``decoupled`` 1 - wd lr /
    initial_lr (composer.optim.DecoupledAdamW).

    On the GPU one step is libhvk's fused hvk_adamw_step (include/hvk.h) with the same
    hand-overs as DecoupledSGDW.  The kernel never sees the step count: the host passes
    step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t), as arguments in an eager step and
    through the device array in a captured one, where refresh_hyper() -- once per replay --
    is what advances t.  Elsewhere (CPU, options.fused_optim off, tensors at different step
    counts) the same step runs as torch's foreach sequence."""

    HYPER_FLOATS = 12  # step_size[4], decay[4], bc2_sqrt, 3 pad

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 decoupled=False, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError("hvamd.optim.AdamW has no amsgrad / maximize form")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or not eps > 0.0:
            raise ValueError(f"betas {betas} must lie in [0, 1) and eps {eps} be positive")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        decoupled=bool(decoupled), initial_lr=lr, amsgrad=False, maximize=False)
        super().__init__(params, defaults)
        self._captured = []  # the parameters of the captured fused call (graph mode)

    def __setstate__(self, state):
        """``step`` is a host number here (torch keeps a CPU tensor per parameter, whose foreach
        increment alone costs the host more than the fused step's launches): a loaded torch state
        is converted, and torch.optim.AdamW converts back when it loads this one."""
        super().__setstate__(state)
        for st in self.state.values():
            if "step" in st:
                st["step"] = float(st["step"])

    def _fused_eligible(self):
        if not OPTIONS.fused_optim:  # A/B runs: the foreach path
            return False
        gs = self.param_groups
        if not gs or any(tuple(g["betas"]) != tuple(gs[0]["betas"]) or g["eps"] != gs[0]["eps"] for g in gs):
            return False
        return self._tensors_fusable()

    @staticmethod
    def _decay(g):
        if not g["weight_decay"]:
            return 1.0
        if g["decoupled"]:
            return 1.0 - g["weight_decay"] * g["lr"] / g["initial_lr"]
        return 1.0 - g["lr"] * g["weight_decay"]

    def _hyper_at(self, t):
        """(step_size per group, decay per group, bc2_sqrt) of step t (>= 1), padded to 4 groups."""
        gs = self.param_groups
        b1, b2 = gs[0]["betas"]
        step_size = [g["lr"] / (1.0 - b1 ** t) for g in gs] + [0.0] * (4 - len(gs))
        decay = [self._decay(g) for g in gs] + [1.0] * (4 - len(gs))
        return step_size, decay, (1.0 - b2 ** t) ** 0.5

    def _hyper_array(self):
        t = self.state[self._captured[0]]["step"] if self._captured else 1.0
        step_size, decay, bc2 = self._hyper_at(max(t, 1.0))
        return step_size + decay + [bc2, 0.0, 0.0, 0.0]

    def refresh_hyper(self):
        """Once per replay of a captured update: this is the step that replay executes, so the
        step count advances here and its step_size / decay / bc2_sqrt go to the device array."""
        if self._hyper is None:
            return
        for p in self._captured:
            self.state[p]["step"] += 1.0
        super().refresh_hyper()

    def _fused_step(self):
        """Mean + clip + update (+ EMA) of every tensor in a handful of libhvk launches
        (hvk_adamw_step); False (nothing done) when the tensors are not at one step count."""
        import ctypes
        from . import _lib
        ps, grp = [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.grad is not None:
                    ps.append(p)
                    grp.append(gi)
        if not ps:
            return True
        counts = {self.state[p].get("step", 0.0) for p in ps}
        if len(counts) != 1:
            return False
        t = counts.pop() + 1.0
        first = t == 1.0
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and (first or not self.device_hyper):
            raise RuntimeError("a captured AdamW update reads its bias corrections from the device array: "
                               "take one eager step and call enable_device_hyper() before the capture")
        if first:  # the kernel writes the moments without reading them
            ms, vs = [torch.empty_like(p) for p in ps], [torch.empty_like(p) for p in ps]
        else:
            ms = [self.state[p]["exp_avg"] for p in ps]
            vs = [self.state[p]["exp_avg_sq"] for p in ps]
        n = len(ps)
        P = ctypes.c_void_p * n
        numel = (ctypes.c_longlong * n)(*[p.numel() for p in ps])
        arrs = [P(*[p.data_ptr() for p in ps]), P(*[p.grad.data_ptr() for p in ps]),
                P(*[m.data_ptr() for m in ms]), P(*[v.data_ptr() for v in vs])]
        ema_arr, ema_a = None, 0.0
        if self.pending_ema is not None:
            emas, ema_a = self.pending_ema
            by_id = dict(emas)
            ema_arr = P(*[by_id[id(p)].data_ptr() for p in ps])
        gs = self.param_groups
        step_v, decay_v, bc2 = self._hyper_at(t)
        step_size = (ctypes.c_float * 4)(*step_v)
        decay = (ctypes.c_float * 4)(*decay_v)
        hyper = self._live_hyper_ptr()
        lib = _lib.load()
        nb = lib.hvk_adamw_workspace_bytes(n, ctypes.cast(numel, ctypes.c_void_p))
        ws = self._workspace(nb, ps[0].device)
        clip = float(self.pending_clip) if self.pending_clip is not None else 0.0
        b1, b2 = gs[0]["betas"]
        self._keep = (arrs, ema_arr, numel)  # ctypes tables outlive the call
        _lib.call("hvk_adamw_step", n, *[ctypes.cast(a, ctypes.c_void_p) for a in arrs],
                  ctypes.cast(ema_arr, ctypes.c_void_p) if ema_arr is not None else None,
                  ctypes.cast(numel, ctypes.c_void_p), ctypes.cast((ctypes.c_int * n)(*grp), ctypes.c_void_p),
                  ctypes.cast(step_size, ctypes.c_void_p), ctypes.cast(decay, ctypes.c_void_p), len(gs),
                  hyper, float(self.pending_grad_scale), clip, float(b1), float(b2), float(gs[0]["eps"]),
                  float(bc2), int(first), float(ema_a), _lib.ptr(ws), nb, _lib.stream())
        if first:
            for p, m, v in zip(ps, ms, vs):
                self.state[p].update(exp_avg=m, exp_avg_sq=v)
        if capturing:  # no kernel ran: each replay's refresh_hyper() counts its own step
            self._captured = ps
        else:
            for p in ps:
                self.state[p]["step"] = t
        # the kernel wrote the weights through raw pointers: bump their version counters so
        # version-keyed caches (ops._WeightCopies) see the update
        torch.autograd.graph.increment_version(ps)
        return True

    def _foreach_step(self):
        """torch's foreach AdamW sequence (one bias correction per tensor: step counts may differ)."""
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if params and params[0].is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("AdamW's fused step is not eligible here and a foreach AdamW would bake its "
                               "bias corrections into the graph: capture needs the fused step "
                               "(options.fused_optim, contiguous f32 CUDA tensors, <= 4 groups)")
        self._apply_pending_grads(params)  # unfused: scale and clip now
        for g in self.param_groups:
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            ts = []
            for p in ps:
                st = self.state[p]
                if "step" not in st:
                    st.update(step=0.0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                st["step"] += 1.0
                ts.append(st["step"])
            grads = [p.grad for p in ps]
            ms = [self.state[p]["exp_avg"] for p in ps]
            vs = [self.state[p]["exp_avg_sq"] for p in ps]
            (b1, b2), lr = g["betas"], g["lr"]
            decay = self._decay(g)
            if decay != 1.0:
                torch._foreach_mul_(ps, decay)
            torch._foreach_lerp_(ms, grads, 1 - b1)
            torch._foreach_mul_(vs, b2)
            torch._foreach_addcmul_(vs, grads, grads, 1 - b2)
            denom = torch._foreach_sqrt(vs)
            torch._foreach_div_(denom, [(1 - b2 ** t) ** 0.5 for t in ts])
            torch._foreach_add_(denom, g["eps"])
            torch._foreach_addcdiv_(ps, ms, denom, [-(lr / (1 - b1 ** t)) for t in ts])
        self._apply_pending_ema(params)


def build_optimizer(config, model):
    skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else {}
    parameters = set_weight_decay(model, skip)
    name = config.optim.name.lower()
    o = config.optim
    if name == "sgd":
        return torch.optim.SGD(parameters, momentum=o.momentum, nesterov=True, lr=o.lr,
                               weight_decay=o.weight_decay, foreach=True)
    if name == "adamw":
        return AdamW(parameters, lr=o.lr, weight_decay=o.weight_decay)
    if name == "decoupledadamw":
        return AdamW(parameters, lr=o.lr, weight_decay=o.weight_decay, decoupled=True)
    if name == "decoupledsgdw":
        return DecoupledSGDW(parameters, lr=o.lr, momentum=o.momentum, weight_decay=o.weight_decay)
    raise ValueError(name)

"""Adam and momentum SGD over one flat parameter buffer: ONE launch per optimizer step (csrc/optim.hip, prifit_adam_flat /
prifit_sgd_flat).

    opt = FlatAdam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    opt = FlatSGD(model.parameters(), lr=1e-3, momentum=0.9)
    ... backward ...; bucket.allreduce(); opt.step()

The reference builds `torch.optim.Adam(classifier.parameters(), lr, betas=(0.9, 0.999), eps=1e-08, weight_decay)`
(train_partseg_shapenet.py:252-259), or `torch.optim.SGD(classifier.parameters(), lr, momentum=0.9)` for any other `--optimizer`
(:260-261), and steps it at :398 / :451.  torch's fused Adam needs three launches for the
MSG network's 144 tensors plus a multi-tensor add for the step counters, and ~0.6-0.9 ms of host time per step
(`_init_group`, grouping by device and dtype); here the parameters are moved ONCE into a flat fp32 buffer (`p.data` becomes a
view of it: the module, its state_dict and checkpoints do not notice), the state lives in flat buffers of the same layout (two
moments for Adam, one momentum buffer for SGD, none for SGD without momentum), and a step is one
launch plus a comparison of the gradients' addresses with the table uploaded earlier (the caching allocator hands a static
step the same blocks every time; a changed address costs one small asynchronous upload).  `_FlatOptimizer` holds what the two
share: the buffer, the address table, the ping-pong step counters, `zero_grad`.

Semantics kept from torch: a parameter whose `.grad` is None is skipped entirely (no weight decay, no state decay, its step
count stays); per-parameter step counts (SGD: only "has stepped", which is what makes its first step `buf = grad`); L2 weight
decay added to the gradient; `param_groups[0]["lr"]` may be changed
between steps (the trainer's schedule, train_partseg_shapenet.py:325-330); `state_dict()` / `load_state_dict()` speak
torch.optim.Adam's / torch.optim.SGD's format, so `optimizer_state_dict` of a checkpoint written by either side loads into the
other; a checkpoint of the other optimizer is refused with a ValueError."""
import ctypes

import torch

from ._lib import call, cur_stream, dll, ptr, query


class _FlatOptimizer:
    """What FlatAdam and FlatSGD share: the flat parameter buffer (and `p.data` re-homed into it), the device table of gradient
    addresses, the ping-pong step counters.  A subclass allocates its state with `_state_buffer()`, sets `param_groups` and
    implements `_launch(src, dst, skip)`."""
    takes_grads = True                                      # step(grads=...) accepts the list ddp.FlatGradBucket.grads() returns
    FORMAT = OTHER_FORMAT = None                            # (torch class name, a param_groups key only that format has)

    def __init__(self, params):
        self.name = type(self).__name__
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("%s: no parameters" % self.name)
        dev = self.params[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in self.params):
            raise RuntimeError("%s needs fp32 parameters on one GPU (HIP backend only, no CPU path)" % self.name)
        align = query("prifit_adam_flat_alignment")
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + align - 1) // align * align
        self.total = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view                               # the module keeps its Parameter objects; their storage is the flat buffer
        n = len(self.params)
        self._off = torch.tensor(self.offsets, dtype=torch.int32, device=dev)
        self._len = torch.tensor([p.numel() for p in self.params], dtype=torch.int32, device=dev)
        self._steps = [torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
        self._cur = 0                                       # _steps[_cur] holds the current counts
        self._gtab = torch.zeros(n, dtype=torch.int64, device=dev)
        self._gtab_host = [torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._gtab_ev = [None, None]
        self._up = 0
        self._cached = None
        self.uploads = 0                                    # how often the address table changed (diagnosis: ~1-3 per run)

    def _state_buffer(self):
        return torch.zeros_like(self.flat)

    def _slice(self, buf, i):
        """Parameter i's part of a flat buffer, in the parameter's shape."""
        p, o = self.params[i], self.offsets[i]
        return buf[o:o + p.numel()].view(p.shape)

    # ------------------------------------------------------------------ step
    def _check_storage(self):
        p0, pl = self.params[0], self.params[-1]
        es = self.flat.element_size()
        if (p0.data_ptr() != self.flat.data_ptr() + self.offsets[0] * es or
                pl.data_ptr() != self.flat.data_ptr() + self.offsets[-1] * es):
            raise RuntimeError("%s: a parameter no longer lives in the flat buffer (module.to() / a re-assigned "
                               "`.data` after the optimizer was built); build the optimizer after moving the model" % self.name)

    def _grad_table(self, grads=None):
        if grads is None:
            grads = [p.grad for p in self.params]           # (~1 us each: FlatGradBucket hands its own list over, see step())
        else:
            # the caller filtered `requires_grad` on its own, at another time: a list of another length would pair gradients
            # with the wrong parameters
            assert len(grads) == len(self.params), (len(grads), len(self.params))
        ptrs = tuple([0 if g is None else g.data_ptr() for g in grads])
        if ptrs != self._cached:
            for p, g in zip(self.params, grads):            # (only when an address changed: the layout the kernel assumes)
                if g is not None and (g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device or g.shape != p.shape):
                    raise RuntimeError("%s: gradients must be contiguous fp32 tensors of their parameter's shape on its device"
                                       % self.name)
            k = self._up
            self._up ^= 1
            if self._gtab_ev[k] is not None:
                self._gtab_ev[k].synchronize()              # the upload that last used this pinned buffer has run
            host = self._gtab_host[k]
            host.copy_(torch.tensor(ptrs, dtype=torch.int64))
            self._gtab.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._gtab_ev[k] = ev
            self._cached = ptrs
            self.uploads += 1

    @torch.no_grad()
    def step(self, skip=None, grads=None):
        """One step over every parameter that has a gradient.  skip: optional int32 device tensor; non-zero makes the launch a
        no-op (a step whose result is being discarded).  grads: the gradients as a list in parameter order (None entries = no
        gradient), when the caller has just read them anyway (ddp.FlatGradBucket.grads())."""
        self._check_storage()
        self._grad_table(grads)
        self._launch(self._steps[self._cur], self._steps[self._cur ^ 1], skip)
        self._cur ^= 1

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @property
    def state(self):
        """torch.optim.Optimizer.state: {parameter: its state_dict() entry} for every parameter that has one (a snapshot: copies,
        the flat buffers are the live state)."""
        return {self.params[i]: st for i, st in self.state_dict()["state"].items()}

    # ------------------------------------------------------------------ checkpoints
    def _checked_ids(self, sd):
        """The parameter ids of a state dict in torch's format -- of THIS optimizer: a checkpoint of the other one is refused here,
        not on a missing key halfway through the load."""
        groups = sd["param_groups"]
        g0 = groups[0]
        mine, other = self.FORMAT, self.OTHER_FORMAT
        if mine[1] not in g0 or other[1] in g0:
            raise ValueError("%s.load_state_dict: expects a state dict in torch.optim.%s's format (param_groups with %r), got %s"
                             % (self.name, mine[0], mine[1], "torch.optim.%s's (param_groups with %r)" % other
                                if other[1] in g0 else "param_groups with the keys %s (neither torch.optim.%s's nor torch.optim.%s's)"
                                % (sorted(k for k in g0 if k != "params"), mine[0], other[0])))
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(self.params):
            raise ValueError("%s.load_state_dict: %d parameters in the checkpoint, %d here" % (self.name, len(ids), len(self.params)))
        return ids


class FlatAdam(_FlatOptimizer):
    FORMAT, OTHER_FORMAT = ("Adam", "betas"), ("SGD", "momentum")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params)
        self.exp_avg = self._state_buffer()
        self.exp_avg_sq = self._state_buffer()
        self.param_groups = [{"params": self.params, "lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}]

    def _launch(self, src, dst, skip):
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        call("prifit_adam_flat", ptr(self.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self._gtab), ptr(self._off),
             ptr(self._len), len(self.params), ctypes.c_longlong(self.total), ptr(src), ptr(dst), ctypes.c_float(g["lr"]),
             ctypes.c_float(b1), ctypes.c_float(b2), ctypes.c_float(g["eps"]), ctypes.c_float(g["weight_decay"]), ptr(skip),
             cur_stream())

    # ------------------------------------------------------------------ checkpoints (torch.optim.Adam's format)
    def state_dict(self):
        steps = self._steps[self._cur].cpu().tolist()
        state = {}
        for i, t in enumerate(steps):
            if t > 0:
                state[i] = {"step": torch.tensor(float(t)), "exp_avg": self._slice(self.exp_avg, i).clone(),
                            "exp_avg_sq": self._slice(self.exp_avg_sq, i).clone()}
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": g["betas"], "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        ids = self._checked_ids(sd)
        g0 = sd["param_groups"][0]
        self.param_groups[0].update(lr=g0["lr"], betas=tuple(g0["betas"]), eps=g0["eps"], weight_decay=g0["weight_decay"])
        steps = [0] * len(self.params)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for pos, pid in enumerate(ids):
            st = sd["state"].get(pid)
            if not st:
                continue
            steps[pos] = int(float(st["step"]))
            self._slice(self.exp_avg, pos).copy_(st["exp_avg"])
            self._slice(self.exp_avg_sq, pos).copy_(st["exp_avg_sq"])
        self._steps[self._cur].copy_(torch.tensor(steps, dtype=torch.int32))


_sgd_group = None


def _torch_sgd_group():
    """`param_groups[0]` of a torch.optim.SGD's state dict as the installed torch writes it (its key set differs between torch
    versions: read, not remembered)."""
    global _sgd_group
    if _sgd_group is None:
        _sgd_group = torch.optim.SGD([torch.zeros(1)], lr=1.0).state_dict()["param_groups"][0]
    return dict(_sgd_group)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov) in one launch.  One state buffer, `momentum_buf`
    (None with momentum == 0: no state at all).  The per-parameter counters only tell the kernel whether a parameter has stepped:
    its first step sets the buffer to the gradient, as torch does when it creates the buffer."""
    FORMAT, OTHER_FORMAT = ("SGD", "momentum"), ("Adam", "betas")

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("FlatSGD: lr, momentum and weight_decay must not be negative (%r, %r, %r)" % (lr, momentum, weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params)
        self.momentum_buf = self._state_buffer() if momentum != 0 else None
        self.param_groups = [{"params": self.params, "lr": lr, "momentum": momentum, "dampening": dampening,
                              "weight_decay": weight_decay, "nesterov": bool(nesterov)}]

    def _launch(self, src, dst, skip):
        g = self.param_groups[0]
        if g["momentum"] != 0 and self.momentum_buf is None:          # momentum switched on between steps: torch creates its
            self.momentum_buf = self._state_buffer()                  # buffers at the next step, so every parameter's is a first one
            src.zero_()
        buf = self.momentum_buf if g["momentum"] != 0 else None
        call("prifit_sgd_flat", ptr(self.flat), ptr(buf), ptr(self._gtab), ptr(self._off), ptr(self._len), len(self.params),
             ctypes.c_longlong(self.total), ptr(src), ptr(dst), ctypes.c_float(g["lr"]), ctypes.c_float(g["momentum"]),
             ctypes.c_float(g["dampening"]), ctypes.c_float(g["weight_decay"]), int(bool(g["nesterov"])), ptr(skip), cur_stream())

    # ------------------------------------------------------------------ checkpoints (torch.optim.SGD's format)
    def state_dict(self):
        """torch writes `state[i] = {"momentum_buffer": tensor}` for a parameter that has stepped with momentum and nothing
        without momentum; so does this.  The counters are not part of the format."""
        g = self.param_groups[0]
        state = {}
        if g["momentum"] != 0 and self.momentum_buf is not None:
            for i, t in enumerate(self._steps[self._cur].cpu().tolist()):
                if t > 0:
                    state[i] = {"momentum_buffer": self._slice(self.momentum_buf, i).clone()}
        group = _torch_sgd_group()
        group.update({k: v for k, v in g.items() if k != "params"})
        group["params"] = list(range(len(self.params)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """A parameter with a `momentum_buffer` tensor continues from it (counter 1); one without (never stepped, or written
        with momentum == 0: None or no entry) takes torch's first-step rule at its next step (counter 0)."""
        ids = self._checked_ids(sd)
        g0 = sd["param_groups"][0]
        self.param_groups[0].update(lr=g0["lr"], momentum=g0["momentum"], dampening=g0["dampening"],
                                    weight_decay=g0["weight_decay"], nesterov=bool(g0["nesterov"]))
        steps = [0] * len(self.params)
        if self.momentum_buf is not None:
            self.momentum_buf.zero_()
        for pos, pid in enumerate(ids):
            st = sd["state"].get(pid)
            buf = st.get("momentum_buffer") if st else None
            if buf is None:
                continue
            if self.momentum_buf is None:
                self.momentum_buf = self._state_buffer()
            steps[pos] = 1
            self._slice(self.momentum_buf, pos).copy_(buf)
        self._steps[self._cur].copy_(torch.tensor(steps, dtype=torch.int32))

"""`HipAdam`: torch.optim.Adam / AdamW whose whole `step()` - `clip_grad_value_` included - is ONE library call
(gdb_adam_step, include/gdb_nerf_hip.h has the definition; csrc/gdb_optim.hip the kernel).

The training recipe gives every parameter a param group of its own (train/optimizer.py), so torch's optimisers run a handful of tiny
launches per tensor; here all tensors of a step go into one call, ceil(tensors / 48) launches.  The arithmetic is torch's
single-tensor Adam, rounding for rounding, so the CPU float32 optimiser is its reference (tests/test_optimizer_referee.py).

* fp32 contiguous CUDA parameters and gradients only; anything else is a ValueError naming the parameter, never another path.
* The kernel writes through raw pointers.  Every cache of packed weights in this package is keyed on (data_ptr, _version), so after
  the call `step()` bumps the version counter of every parameter it updated and of every gradient the clip rewrote
  (torch.autograd.graph.increment_version) - without that the next forward would render with the old weights.
* State is torch Adam's: per parameter `step` (0-dim float32 CPU tensor), `exp_avg`, `exp_avg_sq`; the param groups carry Adam's keys
  (`decoupled_weight_decay` among them).  A `state_dict()` therefore loads into torch.optim.Adam / AdamW and the other way round.
  `clip_value` is an attribute of the optimiser, not of a group: a checkpoint neither carries nor changes it.
* Hyper-parameters are read from the groups on the host at every step: an LR scheduler's writes to group["lr"] take effect."""
import ctypes as C

import torch

from . import _lib


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, decoupled=False,
                 clip_value=None, maximize=False, capturable=False, differentiable=False, foreach=None, fused=None):
        for name, on in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if on:
                raise ValueError(f"HipAdam does not implement {name}=True")
        if isinstance(lr, torch.Tensor):
            raise ValueError("HipAdam reads lr on the host: pass a Python float")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if clip_value is not None and not clip_value > 0:
            raise ValueError(f"Invalid clip_value: {clip_value} (None for no clipping)")
        self.clip_value = None if clip_value is None else float(clip_value)
        self._decoupled_default = bool(decoupled)
        self._vetted = {}   # parameter -> (step, its numpy view, exp_avg, exp_avg_sq) as last checked: see _state_of
        # the keys torch.optim.Adam keeps, so that the param groups of a state_dict serve either class
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for name, value in (("clip_value", None), ("_decoupled_default", False), ("_vetted", {})):   # an unpickled optimiser
            self.__dict__.setdefault(name, value)
        for group in self.param_groups:   # a checkpoint of an older torch Adam has no such key
            group.setdefault("decoupled_weight_decay", getattr(self, "_decoupled_default", False))
            for p in group["params"]:
                st = self.state.get(p, {})
                if len(st) and not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    @staticmethod
    def _check(t, what, index):
        if not (t.is_cuda and t.dtype is torch.float32 and t.is_contiguous()):
            raise ValueError(f"HipAdam: {what} of parameter {index} must be a contiguous float32 CUDA tensor, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")

    def _state_of(self, p, index):
        """The parameter's state, created on first use, and a numpy view of its `step` (a 0-dim CPU tensor: one add through torch
        costs microseconds, 136 of them were most of a step's host time).  The state tensors are checked when they are first seen
        or have been replaced (load_state_dict), not at every step."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        seen = self._vetted.get(p)
        if seen is None or seen[0] is not st["step"] or seen[2] is not st["exp_avg"] or seen[3] is not st["exp_avg_sq"]:
            self._check(st["exp_avg"], "exp_avg", index)
            self._check(st["exp_avg_sq"], "exp_avg_sq", index)
            if st["exp_avg"].shape != p.shape or st["exp_avg_sq"].shape != p.shape:
                raise ValueError(f"HipAdam: the state of parameter {index} does not have the parameter's shape {tuple(p.shape)}")
            step = st["step"]
            if step.device.type != "cpu" or step.dtype != torch.float32 or step.dim() != 0:
                step = st["step"] = step.detach().to("cpu", torch.float32).reshape(())
            seen = self._vetted[p] = (step, step.numpy(), st["exp_avg"], st["exp_avg_sq"])
        return st, seen[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # collect first, refuse before anything is changed
        work, index = {}, -1   # (device, decoupled) -> rows
        for group in self.param_groups:
            for name in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(name):
                    raise ValueError(f"HipAdam does not implement {name}=True (set in a param group)")
            beta1, beta2 = group["betas"]
            hyper = (float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]))
            for p in group["params"]:
                index += 1
                if p.grad is None:
                    continue
                self._check(p, "the data", index)
                self._check(p.grad, "the gradient", index)
                if p.grad.shape != p.shape:
                    raise ValueError(f"HipAdam: the gradient of parameter {index} has shape {tuple(p.grad.shape)}, the parameter {tuple(p.shape)}")
                work.setdefault((p.device, bool(group.get("decoupled_weight_decay", False))), []).append((p, hyper, index))
        lib = _lib.load()
        for (device, decoupled), rows in work.items():
            live = []
            for p, hyper, index in rows:
                st, count = self._state_of(p, index)
                count += 1      # in place, through the view: st["step"] itself
                if p.numel():   # an empty tensor has no storage to point at: its step advances, as torch's does, and nothing else
                    live.append((p, hyper, st, int(count)))
            n = len(live)
            if n == 0:
                continue
            grads = [p.grad for p, _, _, _ in live]
            ptrs = [(C.c_void_p * n)(*[t.data_ptr() for t in col]) for col in
                    ([p for p, _, _, _ in live], grads, [s["exp_avg"] for _, _, s, _ in live], [s["exp_avg_sq"] for _, _, s, _ in live])]
            numel = (C.c_int64 * n)(*[p.numel() for p, _, _, _ in live])
            cols = [(C.c_double * n)(*col) for col in zip(*[h for _, h, _, _ in live])]
            steps = (C.c_int64 * n)(*[t for _, _, _, t in live])
            with torch.cuda.device(device):
                _lib.check(lib.gdb_adam_step(n, *ptrs, numel, *cols, steps, self.clip_value or 0.0, int(decoupled),
                                             torch.cuda.current_stream(device).cuda_stream))
            # written through raw pointers: tell autograd and every (data_ptr, _version) cache
            torch.autograd.graph.increment_version([p for p, _, _, _ in live])
            if self.clip_value:
                torch.autograd.graph.increment_version(grads)
        return loss

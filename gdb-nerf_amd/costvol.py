"""Torch-facing wrappers of the two "next"-row kernels: the plane-sweep cost volume
and the depth regression of the cascade MVS stage, same signatures as the reference functions
(networks/gdb_nerf/depth_net.py:424-514), and `CostReg`, the HIP forward of the cascade's cost-regularisation 3-D U-Nets
(networks/gdb_nerf/cost_reg_net.py), and `MvsStage`, one whole cascade stage as one library call.  CUDA tensors only — there is no CPU fallback here either."""
import ctypes as C
from typing import Tuple

import numpy as np
import torch

from . import _lib


def _c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 CUDA tensor")
    return t.contiguous()


def build_feature_volume(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, inv_depth: bool, pair_layout: bool = True) -> torch.Tensor:
    """pair_layout: let the library re-lay the source maps channel-pair-interleaved first (even C, V <= 4): bit-identical, faster."""
    lib = _lib.load()
    B, V, Cc, Hs, Ws = src_feat.shape
    D, Ht, Wt = depth_values.shape[1:]
    if depth_values.shape[0] != B or tuple(src_exts.shape) != (B, V, 4, 4) or tuple(src_ints.shape) != (B, V, 3, 3) \
            or tuple(tar_exts.shape) != (B, 4, 4) or tuple(tar_ints.shape) != (B, 3, 3):
        raise ValueError("inconsistent cost-volume shapes")
    args = [_c(t, n) for t, n in ((src_feat, "src_feat"), (src_exts, "src_exts"), (src_ints, "src_ints"), (tar_exts, "tar_exts"),
                                  (tar_ints, "tar_ints"), (depth_values, "depth_values"))]
    out = torch.empty((B, Cc, D, Ht, Wt), device=src_feat.device)
    ws = torch.empty((B * V * 12,), device=src_feat.device)
    # scratch for the channel-pair copy of the source maps (the sweep then loads 16 bytes per channel pair).  Allocated per call:
    # torch's caching allocator hands the block back without a device allocation and keeps it stream-safe (a module-level cache keyed
    # by size was shared by every caller on every stream, and the cascade's two stage sizes evicted each other: ADVICE r04)
    n_pair = B * V * Cc * Hs * Ws if (pair_layout and Cc % 2 == 0 and V <= 4) else 0
    pw = torch.empty((n_pair,), device=src_feat.device) if n_pair else None
    _lib.check(lib.gdb_build_feature_volume_ws(*(t.data_ptr() for t in args), B, V, Cc, Hs, Ws, D, Ht, Wt, int(bool(inv_depth)),
                                               ws.data_ptr(), None if pw is None else pw.data_ptr(), out.data_ptr(),
                                               torch.cuda.current_stream(src_feat.device).cuda_stream))
    return out


def feature_volume_backward(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, g_cost, inv_depth: bool,
                            want_src_feat: bool = True, want_depth_values: bool = True, workspace: torch.Tensor = None):
    """gdb_feature_volume_backward: (g_src_feat (B, V, C, Hs, Ws) or None, g_depth_values (B, D, Ht, Wt) or None) from
    the forward's inputs and the upstream g_cost (B, C, D, Ht, Wt), on the current stream.  `workspace`: a contiguous CUDA tensor of
    at least `feature_volume_backward_workspace_bytes` bytes (its contents do not matter); by default allocated per call."""
    lib = _lib.load()
    if not (want_src_feat or want_depth_values):
        raise ValueError("feature_volume_backward: neither output is requested")
    B, V, Cc, Hs, Ws = src_feat.shape
    D, Ht, Wt = depth_values.shape[1:]
    if depth_values.shape[0] != B or tuple(src_exts.shape) != (B, V, 4, 4) or tuple(src_ints.shape) != (B, V, 3, 3) \
            or tuple(tar_exts.shape) != (B, 4, 4) or tuple(tar_ints.shape) != (B, 3, 3) or tuple(g_cost.shape) != (B, Cc, D, Ht, Wt):
        raise ValueError("inconsistent cost-volume shapes")
    args = [_c(t, n) for t, n in ((src_feat, "src_feat"), (src_exts, "src_exts"), (src_ints, "src_ints"), (tar_exts, "tar_exts"),
                                  (tar_ints, "tar_ints"), (depth_values, "depth_values"), (g_cost, "g_cost"))]
    nbytes = feature_volume_backward_workspace_bytes(B, V, Cc, Hs, Ws, D, Ht, Wt)[0]
    dev = src_feat.device
    if workspace is None:   # per call from torch's caching allocator, as CostReg does
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    elif not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"workspace must be a contiguous CUDA tensor of at least {nbytes} bytes")
    g_src = torch.empty((B, V, Cc, Hs, Ws), device=dev) if want_src_feat else None
    g_hyp = torch.empty((B, D, Ht, Wt), device=dev) if want_depth_values else None
    _lib.check(lib.gdb_feature_volume_backward(*(t.data_ptr() for t in args), B, V, Cc, Hs, Ws, D, Ht, Wt, int(bool(inv_depth)),
                                               workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                               None if g_src is None else g_src.data_ptr(), None if g_hyp is None else g_hyp.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream))
    return g_src, g_hyp


def feature_volume_backward_workspace_bytes(B, V, Cc, Hs, Ws, D, Ht, Wt) -> Tuple[int, int]:
    """(workspace bytes, fraction bits F of the fixed-point accumulators) of gdb_feature_volume_backward (host only)."""
    n, f = C.c_size_t(), C.c_int32()
    _lib.check(_lib.load().gdb_feature_volume_backward_workspace_bytes(B, V, Cc, Hs, Ws, D, Ht, Wt, C.byref(n), C.byref(f)))
    return n.value, f.value


class FeatureVolumeFunction(torch.autograd.Function):
    """`build_feature_volume` with a backward: the forward is that call unchanged - the same bits - and the backward is
    gdb_feature_volume_backward, to src_feat and depth_values only (the cameras get None), not differentiable again.
    `FeatureVolumeFunction.apply(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, inv_depth)`."""

    @staticmethod
    def forward(ctx, src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, inv_depth):
        ctx.inv_depth = bool(inv_depth)
        ctx.save_for_backward(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values)
        return build_feature_volume(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, inv_depth)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cost):
        want_src, want_hyp = ctx.needs_input_grad[0], ctx.needs_input_grad[5]
        if not (want_src or want_hyp):
            return (None,) * 7
        g_src, g_hyp = feature_volume_backward(*ctx.saved_tensors, g_cost, ctx.inv_depth, want_src, want_hyp)
        return g_src, None, None, None, None, g_hyp, None


def depth_regression(depth_values, depth_prob, ci_scale: float, inv_depth: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    B, D, H, W = depth_values.shape
    if tuple(depth_prob.shape) != (B, D, H, W):
        raise ValueError("depth_prob shape differs from depth_values")
    dv, pr = _c(depth_values, "depth_values"), _c(depth_prob, "depth_prob")
    depth = torch.empty((B, 1, H, W), device=dv.device)
    ci = torch.empty((B, 2, H, W), device=dv.device)
    _lib.check(lib.gdb_depth_regression(dv.data_ptr(), pr.data_ptr(), B, D, H, W, C.c_float(float(ci_scale)), int(bool(inv_depth)),
                                        depth.data_ptr(), ci.data_ptr(), torch.cuda.current_stream(dv.device).cuda_stream))
    return depth, ci


def cost_reg_keys(depth: int):
    """State-dict keys of a `_UNet3d` in the order gdb_pack_cost_reg_weights takes them (include/gdb_nerf_hip.h); eps follows."""
    keys = []
    for i in range(3 * depth + 1):
        keys += [f"conv{i}.0.weight", f"conv{i}.1.weight", f"conv{i}.1.bias", f"conv{i}.1.running_mean", f"conv{i}.1.running_var"]
    return keys + ["feat_head.weight", "prob_head.weight"]


class CostReg:
    """Eval-mode forward of a `_UNet3d` (cost_reg_net.py:24-54) on the HIP library: `CostReg(module)(cost)` returns
    (volume (B, out, D, H, W), prob (B, D, H, W)) like `module(cost)`, on the current stream.  The module's parameters and
    buffers are packed on the host and uploaded once, and again whenever any of them changes storage or version (running
    statistics included: they are buffers, not parameters); an in-place write through `.data` needs `invalidate()`."""

    def __init__(self, module: torch.nn.Module) -> None:
        self.module = module
        self.depth = int(module._depth)
        self.cin, self.c = int(module.conv0[0].in_channels), int(module.conv0[0].out_channels)
        self.cout = int(module.feat_head.out_channels)
        eps = {float(m.eps) for m in module.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
        if len(eps) != 1:
            raise ValueError(f"the U-Net's batch norms use different eps {sorted(eps)}; the packed form holds one")
        self.eps = eps.pop()
        self._key, self.packed = None, None

    def invalidate(self) -> None:
        self._key = None

    def _versions(self):
        return tuple((t.data_ptr(), t._version) for t in (*self.module.parameters(), *self.module.buffers()))

    def pack(self, device) -> torch.Tensor:
        key = (torch.device(device), self._versions())
        if key == self._key:
            return self.packed
        lib = _lib.load()
        sd = self.module.state_dict()
        keys = cost_reg_keys(self.depth)
        arrs = [np.ascontiguousarray(sd[k].detach().cpu().numpy(), dtype=np.float32) for k in keys]
        arrs.append(np.array([self.eps], dtype=np.float32))
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        n = C.c_size_t()
        _lib.check(lib.gdb_cost_reg_packed_floats(self.depth, self.cin, self.c, self.cout, C.byref(n)))
        host = np.zeros(n.value, dtype=np.float32)
        _lib.check(lib.gdb_pack_cost_reg_weights(self.depth, self.cin, self.c, self.cout, ptrs, host.ctypes.data))
        self.packed, self._key = torch.from_numpy(host).to(device), key
        return self.packed

    def __call__(self, cost: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        lib = _lib.load()
        cost = _c(cost, "cost")
        if cost.dim() != 5 or cost.shape[1] != self.cin:
            raise ValueError(f"cost volume of shape {tuple(cost.shape)}, expected (B, {self.cin}, D, H, W)")
        B, _, D, H, W = cost.shape
        packed = self.pack(cost.device)
        nbytes = C.c_size_t()
        _lib.check(lib.gdb_cost_reg_workspace_bytes(self.depth, self.cin, self.c, self.cout, B, D, H, W, C.byref(nbytes)))
        # allocated per call: torch's caching allocator hands the block back without a device allocation and keeps it stream-safe
        ws = torch.empty(((nbytes.value + 3) // 4,), device=cost.device)
        volume = torch.empty((B, self.cout, D, H, W), device=cost.device)
        prob = torch.empty((B, D, H, W), device=cost.device)
        _lib.check(lib.gdb_cost_reg(self.depth, self.cin, self.c, self.cout, cost.data_ptr(), B, D, H, W, packed.data_ptr(), ws.data_ptr(),
                                    nbytes.value, volume.data_ptr(), prob.data_ptr(), torch.cuda.current_stream(cost.device).cuda_stream))
        return volume, prob


def cost_reg_train_layout(depth: int, cin: int, c: int, cout: int, B: int, D: int, H: int, W: int):
    """gdb_cost_reg_train_layout (host only): ({(buffer, name): (offset, bytes, channels, level)}, saved bytes, workspace bytes);
    buffer 0 is the saved buffer, 1 the backward's workspace.  Raises ValueError for a plan or shape the entries refuse."""
    lib = _lib.load()
    count, saved, ws = C.c_int32(), C.c_size_t(), C.c_size_t()
    _lib.check(lib.gdb_cost_reg_train_layout(depth, cin, c, cout, B, D, H, W, None, 0, C.byref(count), C.byref(saved), C.byref(ws)))
    regs = (_lib.GdbCostRegTrainRegion * count.value)()
    _lib.check(lib.gdb_cost_reg_train_layout(depth, cin, c, cout, B, D, H, W, C.cast(regs, C.c_void_p), count.value, C.byref(count), None, None))
    out = {}
    for r in regs:
        key = (int(r.buffer), r.name.decode())
        if key in out:
            raise _lib.GdbError(f"region {key} is listed twice")
        out[key] = (int(r.offset), int(r.bytes), int(r.channels), int(r.level))
    return out, saved.value, ws.value


class _CostRegTrainFn(torch.autograd.Function):
    """gdb_cost_reg_train / gdb_cost_reg_train_backward.  Inputs: the runner, the cost volume and the parameters in
    `CostRegTrain.params()` order; the backward is not differentiable again.  A cost volume that requires grad gets its gradient from
    gdb_cost_reg_train_backward_cost; one that does not takes gdb_cost_reg_train_backward as before."""

    @staticmethod
    def forward(ctx, runner, cost, *params):
        lib = _lib.load()
        B, _, D, H, W = cost.shape
        dev = cost.device
        regions, saved_bytes, ws_bytes = cost_reg_train_layout(runner.depth, runner.cin, runner.c, runner.cout, B, D, H, W)
        saved = torch.empty((saved_bytes,), dtype=torch.uint8, device=dev)
        volume = torch.empty((B, runner.cout, D, H, W), device=dev)
        prob = torch.empty((B, D, H, W), device=dev)
        stats = torch.empty((2 * sum(runner.channels),), device=dev)
        ptrs = runner.param_pointers(params)
        _lib.check(lib.gdb_cost_reg_train(runner.depth, runner.cin, runner.c, runner.cout, cost.data_ptr(), B, D, H, W, ptrs, runner.eps,
                                          runner.momentum, saved.data_ptr(), saved_bytes, volume.data_ptr(), prob.data_ptr(),
                                          stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        for t in runner.running_buffers():   # written in place by the library: whoever keys on versions (CostReg.pack) sees it
            torch.autograd.graph.increment_version(t)
        ctx.runner, ctx.ws_bytes, ctx.saved_bytes = runner, ws_bytes, saved_bytes
        ctx.save_for_backward(cost, saved, *params)
        if runner.keep:
            runner.last = {"saved": saved, "regions": regions, "batch_stats": stats}
        return volume, prob

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_volume, g_prob):
        lib = _lib.load()
        runner = ctx.runner
        cost, saved, *params = ctx.saved_tensors
        B, _, D, H, W = cost.shape
        g_volume = None if g_volume is None else _c(g_volume, "g_volume")
        g_prob = None if g_prob is None else _c(g_prob, "g_prob")
        ws = torch.empty((ctx.ws_bytes,), dtype=torch.uint8, device=cost.device)
        grads = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in params]
        gptrs = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        args = (runner.depth, runner.cin, runner.c, runner.cout, cost.data_ptr(), B, D, H, W,
                runner.param_pointers(params), None if g_volume is None else g_volume.data_ptr(),
                None if g_prob is None else g_prob.data_ptr(), saved.data_ptr(), ctx.saved_bytes, ws.data_ptr(), ctx.ws_bytes, gptrs)
        stream = torch.cuda.current_stream(cost.device).cuda_stream
        if not ctx.needs_input_grad[1]:
            _lib.check(lib.gdb_cost_reg_train_backward(*args, stream))
            return (None, None, *grads)
        nbytes = C.c_size_t()
        _lib.check(lib.gdb_cost_reg_train_cost_grad_bytes(runner.depth, runner.cin, runner.c, runner.cout, B, D, H, W, C.byref(nbytes)))
        cws = torch.empty((nbytes.value,), dtype=torch.uint8, device=cost.device)
        g_cost = torch.empty_like(cost)
        _lib.check(lib.gdb_cost_reg_train_backward_cost(*args, g_cost.data_ptr(), cws.data_ptr(), nbytes.value, stream))
        return (None, g_cost, *grads)


class CostRegTrain:
    """Training-mode forward and backward of a `_UNet3d` on the HIP library: `CostRegTrain(module)(cost)` returns
    (volume, prob) like `module.train()(cost)`, updates the module's running statistics in place on the device and carries a graph
    to the module's parameters.  With `cost_grad` set a cost volume that requires grad is accepted and gets its gradient
    (gdb_cost_reg_train_backward_cost); without it, as before, one that requires grad is refused.  Nothing falls back: a plan or
    shape the library refuses raises ValueError.  With `keep` set, `last` holds the latest call's saved buffer, its regions and the
    batch statistics (for inspection; off by default: it would pin the buffer until the next call)."""

    def __init__(self, module: torch.nn.Module, cost_grad: bool = False) -> None:
        self.module = module
        self.cost_grad = bool(cost_grad)
        self.depth = int(module._depth)
        self.cin, self.c = int(module.conv0[0].in_channels), int(module.conv0[0].out_channels)
        self.cout = int(module.feat_head.out_channels)
        self.blocks = [getattr(module, f"conv{i}") for i in range(3 * self.depth + 1)]
        bns = [b[1] for b in self.blocks]
        if any(bn.weight is None or bn.momentum is None for bn in bns):
            raise ValueError("the train-mode HIP U-Net needs affine batch norms with a momentum")
        eps, mom = {float(bn.eps) for bn in bns}, {float(bn.momentum) for bn in bns}
        if len(eps) != 1 or len(mom) != 1:
            raise ValueError(f"the U-Net's batch norms use different eps {sorted(eps)} or momentum {sorted(mom)}")
        self.eps, self.momentum = eps.pop(), mom.pop()
        self.channels = [int(b[0].out_channels) for b in self.blocks]
        self.keep, self.last = False, None

    def params(self):
        ps = []
        for b in self.blocks:
            ps += [b[0].weight, b[1].weight, b[1].bias]
        return ps + [self.module.feat_head.weight, self.module.prob_head.weight]

    def running_buffers(self):
        return [t for b in self.blocks for t in (b[1].running_mean, b[1].running_var, b[1].num_batches_tracked) if t is not None]

    def param_pointers(self, params):
        """The d_params array of include/gdb_nerf_hip.h from the parameters in `params()` order and the module's buffers."""
        ptrs = []
        for i, b in enumerate(self.blocks):
            ptrs += [params[3 * i + k].data_ptr() for k in range(3)]
            ptrs += [None if t is None else t.data_ptr() for t in (b[1].running_mean, b[1].running_var, b[1].num_batches_tracked)]
        ptrs += [params[-2].data_ptr(), params[-1].data_ptr()]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def __call__(self, cost: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if cost.requires_grad and not self.cost_grad:
            raise ValueError("CostRegTrain builds the cost volume's gradient only with cost_grad set: pass one that does not require grad")
        cost = _c(cost, "cost")
        if cost.dim() != 5 or cost.shape[1] != self.cin:
            raise ValueError(f"cost volume of shape {tuple(cost.shape)}, expected (B, {self.cin}, D, H, W)")
        params = self.params()
        for p in (*params, *self.running_buffers()):
            if not p.is_cuda or p.device != cost.device or not p.is_contiguous() or (p.dtype != torch.float32 and p.dtype != torch.int64):
                raise ValueError("CostRegTrain needs the module's parameters and buffers contiguous, fp32, on the cost volume's device")
        return _CostRegTrainFn.apply(self, cost, *params)


def _range_dims(search: torch.Tensor):
    if search.dim() == 2:   # (B, 2) near / far: broadcast over the target
        return 1, 1
    if search.dim() != 4 or search.shape[1] != 2:
        raise ValueError(f"search range of shape {tuple(search.shape)}, expected (B, 2) or (B, 2, hr, wr)")
    return int(search.shape[2]), int(search.shape[3])


def mvs_hypotheses(search: torch.Tensor, ratio: float, num_depth: int, Ht: int, Wt: int, inv_depth: bool) -> torch.Tensor:
    """The (B, num_depth, Ht, Wt) hypotheses a stage computes in its kernels from `search` ((B, 2) or (B, 2, 1, 1): broadcast;
    (B, 2, hr, wr): upsampled by `ratio` as F.interpolate(scale_factor=ratio, mode="bilinear", align_corners=False) does), then
    `get_depth_values`.  For tests and diagnosis: MvsStage never materialises them."""
    lib = _lib.load()
    search = _c(search, "search")
    hr, wr = _range_dims(search)
    out = torch.empty((search.shape[0], num_depth, Ht, Wt), device=search.device)
    _lib.check(lib.gdb_mvs_hypotheses(search.data_ptr(), hr, wr, float(ratio), search.shape[0], num_depth, Ht, Wt, int(bool(inv_depth)),
                                      out.data_ptr(), torch.cuda.current_stream(search.device).cuda_stream))
    return out


class MvsStage:
    """One cascade stage of `DepthNet.forward` on the HIP library (gdb_mvs_stage): camera set-up from the unscaled intrinsics, the
    plane sweep with its hypotheses computed in the kernel from `search`, the stage's U-Net, softmax over D and depth regression.
    `MvsStage(reg)` shares the weight pack of the `CostReg` it is given.  Returns (volume (B, out, D, Ht, Wt), depth (B, Ht, Wt),
    ci (B, 2, Ht, Wt), vol_range (B, 2, Ht, Wt)) on the current stream; no tensor op and, once the weights are packed, no host
    synchronisation."""

    def __init__(self, reg: CostReg) -> None:
        self.reg = reg

    def workspace_bytes(self, B, V, Cc, Hs, Ws, D, Ht, Wt) -> int:
        r, n = self.reg, C.c_size_t()
        _lib.check(_lib.load().gdb_mvs_stage_workspace_bytes(B, V, Cc, Hs, Ws, D, Ht, Wt, r.depth, r.cin, r.c, r.cout, C.byref(n)))
        return n.value

    def __call__(self, src_feat, src_exts, src_ints, tar_exts, tar_ints, feat_scale: float, vol_scale: float, search, ratio: float,
                 num_depth: int, Ht: int, Wt: int, inv_depth: bool, ci_scale: float, workspace: torch.Tensor = None):
        lib, r = _lib.load(), self.reg
        if src_feat.dim() != 5:
            raise ValueError(f"src_feat of shape {tuple(src_feat.shape)}, expected (B, V, C, Hs, Ws)")
        B, V, Cc, Hs, Ws = src_feat.shape
        if tuple(src_exts.shape) != (B, V, 4, 4) or tuple(src_ints.shape) != (B, V, 3, 3) or tuple(tar_exts.shape) != (B, 4, 4) \
                or tuple(tar_ints.shape) != (B, 3, 3) or search.shape[0] != B:
            raise ValueError("inconsistent cost-volume shapes")
        args = [_c(t, n) for t, n in ((src_feat, "src_feat"), (src_exts, "src_exts"), (src_ints, "src_ints"), (tar_exts, "tar_exts"),
                                      (tar_ints, "tar_ints"))]
        search = _c(search, "search")
        hr, wr = _range_dims(search)
        dev = src_feat.device
        packed = r.pack(dev)
        nbytes = self.workspace_bytes(B, V, Cc, Hs, Ws, num_depth, Ht, Wt)
        if workspace is None:   # per call from torch's caching allocator, as CostReg does
            workspace = torch.empty(((nbytes + 3) // 4,), device=dev)
        elif not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nbytes:
            raise ValueError(f"workspace must be a contiguous CUDA tensor of at least {nbytes} bytes")
        volume = torch.empty((B, r.cout, num_depth, Ht, Wt), device=dev)
        depth = torch.empty((B, Ht, Wt), device=dev)
        ci = torch.empty((B, 2, Ht, Wt), device=dev)
        vol_range = torch.empty((B, 2, Ht, Wt), device=dev)
        _lib.check(lib.gdb_mvs_stage(*(t.data_ptr() for t in args), C.c_float(float(feat_scale)), C.c_float(float(vol_scale)),
                                     search.data_ptr(), hr, wr, float(ratio), B, V, Cc, Hs, Ws, num_depth, Ht, Wt, int(bool(inv_depth)),
                                     C.c_float(float(ci_scale)), r.depth, r.cin, r.c, r.cout, packed.data_ptr(), workspace.data_ptr(),
                                     workspace.numel() * workspace.element_size(), volume.data_ptr(), depth.data_ptr(), ci.data_ptr(),
                                     vol_range.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return volume, depth, ci, vol_range

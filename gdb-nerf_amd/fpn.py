"""`FeaturePyramid`, the HIP forward of the feature pyramid network (networks/gdb_nerf/feature_net.py) on gdb_fpn
(include/gdb_nerf_hip.h).  CUDA tensors only — there is no CPU fallback here either."""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

BLOCKS = ("conv0.0", "conv0.1", "conv1.0", "conv1.1", "conv2.0", "conv2.1")


def fpn_keys():
    """State-dict keys of a `FeatureNet` in the order gdb_pack_fpn_weights takes them (include/gdb_nerf_hip.h); eps follows."""
    keys = []
    for b in BLOCKS:
        keys += [f"{b}.0.weight", f"{b}.1.weight", f"{b}.1.bias", f"{b}.1.running_mean", f"{b}.1.running_var"]
    return keys + ["out0.weight", "out0.bias", "inner1.weight", "inner1.bias", "inner2.weight", "inner2.bias", "out1.weight", "out2.weight"]


def channels(module: torch.nn.Module):
    """(base_channels, out0, out1, out2) of a `FeatureNet`."""
    return (int(module.conv0[0][0].out_channels), int(module.out0.out_channels), int(module.out1.out_channels),
            int(module.out2.out_channels))


def check_channels(base_channels: int, out_channels: Sequence[int]) -> None:
    """Raise ValueError (the library's message, naming the limit) for a FeatureNet the HIP FPN is not built for."""
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_fpn_packed_floats(int(base_channels), *[int(c) for c in out_channels], C.byref(n)))


class FeaturePyramid:
    """Eval-mode forward of a `FeatureNet` on the HIP library: `FeaturePyramid(module)(x, levels)` returns the list of the three
    pyramid levels like `module(x)`, with None for the levels not asked for, on the current stream.  The module's parameters and
    buffers are packed on the host and uploaded once, and again whenever any of them changes storage or version (running statistics
    included: they are buffers, not parameters); an in-place write through `.data` needs `invalidate()`."""

    def __init__(self, module: torch.nn.Module) -> None:
        self.module = module
        self.channels = channels(module)
        check_channels(self.channels[0], self.channels[1:])
        eps = {float(m.eps) for m in module.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)}
        if len(eps) != 1:
            raise ValueError(f"the FPN's batch norms use different eps {sorted(eps)}; the packed form holds one")
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
        arrs = [np.ascontiguousarray(sd[k].detach().cpu().numpy(), dtype=np.float32) for k in fpn_keys()]
        arrs.append(np.array([self.eps], dtype=np.float32))
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        n = C.c_size_t()
        _lib.check(lib.gdb_fpn_packed_floats(*self.channels, C.byref(n)))
        host = np.zeros(n.value, dtype=np.float32)
        _lib.check(lib.gdb_pack_fpn_weights(*self.channels, ptrs, host.ctypes.data))
        self.packed, self._key = torch.from_numpy(host).to(device), key
        return self.packed

    def __call__(self, x: torch.Tensor, levels: Sequence[int] = (0, 1, 2)) -> List[Optional[torch.Tensor]]:
        lib = _lib.load()
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError("images must be a float32 CUDA tensor")
        x = x.contiguous()
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"images of shape {tuple(x.shape)}, expected (N, 3, H, W)")
        mask = 0
        for l in levels:
            if int(l) not in (0, 1, 2):
                raise ValueError(f"pyramid level {l} (0, 1 or 2)")
            mask |= 1 << int(l)
        N, _, H, W = x.shape
        h, w = (H + 1) // 2, (W + 1) // 2
        shapes = [(N, self.channels[1], (h + 1) // 2, (w + 1) // 2), (N, self.channels[2], h, w), (N, self.channels[3], H, W)]
        packed = self.pack(x.device)
        nbytes = C.c_size_t()
        _lib.check(lib.gdb_fpn_workspace_bytes(*self.channels, N, H, W, mask, C.byref(nbytes)))
        # allocated per call: torch's caching allocator hands the block back without a device allocation and keeps it stream-safe
        ws = torch.empty(((nbytes.value + 3) // 4,), device=x.device)
        outs = [torch.empty(s, device=x.device) if mask >> l & 1 else None for l, s in enumerate(shapes)]
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(lib.gdb_fpn(*self.channels, x.data_ptr(), N, H, W, packed.data_ptr(), mask, ws.data_ptr(), nbytes.value,
                               ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), torch.cuda.current_stream(x.device).cuda_stream))
        return outs

"""The residual-dense decoder in training mode on the HIP library (gdb_decoder_train.hip): the weight pack on the
device, the saved-activation forward and the backward.  fp32, bundle_size 2, whole frames."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from ._lib import GdbConfig, GdbFrame


def decoder_params(module: torch.nn.Module) -> List[torch.Tensor]:
    """The Decoder's parameters in the state-dict order gdb_pack_decoder_weights documents (bundle_size 2: one up stage)."""
    ps = [module.in_conv.weight, module.in_conv.bias]
    for blk in module.blocks:
        ps += [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight, blk.se.fc[0].weight, blk.se.fc[2].weight]
    return ps + [module.up[0].weight, module.up[0].bias, module.out_conv.weight, module.out_conv.bias]


class DecoderTrain:
    """Owns the packed and saved buffers of a Decoder's training-mode forward; both are reused call after call and re-sized on a shape
    change.  `pack()` re-packs on the device, without a host copy or a synchronisation, whenever a parameter's (data_ptr, _version)
    changed since the last pack - an optimiser step bumps `_version`.  `forward(rows, B, H, W)` returns rgb_c (B, 3, 2H, 2W),
    bit-identical to `HotPathEngine.decode` at fp32; `activations()` are named views into the saved buffer."""

    def __init__(self, module: torch.nn.Module, bundle_size: int = 2) -> None:
        self.module = module
        self.num_layers = len(module.blocks)
        self.cfg = GdbConfig(int(bundle_size), 3, 1, 0, 64, 3, 16, 8, 64, 1)
        n = C.c_size_t()
        _lib.check(self.lib.gdb_decoder_train_packed_floats(C.byref(self.cfg), self.num_layers, C.byref(n)))   # refuses what is not built
        self._n_packed = n.value
        self.packed: Optional[torch.Tensor] = None
        self.saved: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._key = None
        self._shape = None
        self.packs = 0      # device packs run so far
        self.forwards = 0   # forwards run so far: the saved buffer holds the last one's activations only

    @property
    def lib(self):
        return _lib.load()

    def params(self) -> List[torch.Tensor]:
        return decoder_params(self.module)

    def pack(self, params: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        params = self.params() if params is None else list(params)
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self.packed is not None and key == self._key:
            return self.packed
        dev = params[0].device
        for p in params:
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("DecoderTrain needs the decoder's parameters contiguous, fp32, on one GPU")
        if self.packed is None or self.packed.device != dev:
            self.packed = torch.empty(self._n_packed, dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        _lib.check(self.lib.gdb_decoder_train_pack(C.byref(self.cfg), self.num_layers, _lib.PREC_F32, ptrs, self.packed.data_ptr(),
                                                   self._n_packed, torch.cuda.current_stream(dev).cuda_stream))
        self._key = key
        self.packs += 1
        return self.packed

    def _frame(self, B: int, H: int, W: int) -> GdbFrame:
        f = GdbFrame()
        f.B, f.H, f.W = int(B), int(H), int(W)
        return f

    def forward(self, rows: torch.Tensor, B: int, H: int, W: int, out: Optional[torch.Tensor] = None,
                params: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        if rows.dim() != 2 or rows.shape[0] != B * H * W or rows.dtype != torch.float32 or not rows.is_cuda or rows.stride(1) != 1:
            raise ValueError(f"bundle rows of shape {tuple(rows.shape)}, expected fp32 CUDA ({B * H * W}, Q) with unit column stride")
        packed = self.pack(params)
        f = self._frame(B, H, W)
        need = C.c_size_t()
        _lib.check(self.lib.gdb_decoder_train_saved_bytes(C.byref(self.cfg), C.byref(f), self.num_layers, C.byref(need)))
        if self.saved is None or self.saved.numel() < need.value or self.saved.device != rows.device:
            self.saved = torch.empty(need.value, dtype=torch.uint8, device=rows.device)
        self._shape = (B, H, W)
        self.forwards += 1
        rgb_c = torch.empty((B, 3, 2 * H, 2 * W), dtype=torch.float32, device=rows.device) if out is None else out
        _lib.check(self.lib.gdb_decoder_train_forward(C.byref(self.cfg), C.byref(f), rows.data_ptr(), int(rows.stride(0)), packed.data_ptr(),
                                                      self.num_layers, _lib.PREC_F32, self.saved.data_ptr(), self.saved.numel(),
                                                      rgb_c.data_ptr(), torch.cuda.current_stream(rows.device).cuda_stream))
        return rgb_c

    def backward(self, rows: torch.Tensor, g_rgb_c: torch.Tensor, want_params: Optional[Sequence[bool]] = None, want_rows: bool = True,
                 g_rows: Optional[torch.Tensor] = None):
        """The gradients of loss = sum(rgb_c * g_rgb_c) for the last `forward` (same rows, same parameters): (g_rows or None, [one
        tensor or None per parameter, in `params()` order, each in that parameter's shape]).  The row gradient is (N_b, rows' width):
        columns 12 .. 38 hold the gradient, 0 .. 11 are zero (rgb_f's path through them is not the decoder's), columns from 39 on are
        whatever `g_rows` held (zero when it is allocated here).  Nothing is accumulated: every requested tensor is overwritten."""
        if self.saved is None or self._shape is None:
            raise ValueError("forward() first")
        B, H, W = self._shape
        params = self.params()
        if tuple((p.data_ptr(), p._version) for p in params) != self._key:
            raise ValueError("a parameter changed between DecoderTrain.forward and backward: the saved activations are another model's")
        if tuple(g_rgb_c.shape) != (B, 3, 2 * H, 2 * W) or g_rgb_c.dtype != torch.float32 or not g_rgb_c.is_cuda:
            raise ValueError(f"g_rgb_c of shape {tuple(g_rgb_c.shape)}, expected fp32 CUDA {(B, 3, 2 * H, 2 * W)}")
        g_rgb_c = g_rgb_c.contiguous()
        want = [True] * len(params) if want_params is None else [bool(w) for w in want_params]
        grads = [torch.empty_like(p) if w else None for p, w in zip(params, want)]
        if want_rows and g_rows is None:
            g_rows = torch.zeros((rows.shape[0], rows.shape[1]), dtype=torch.float32, device=rows.device)
        f, need = self._frame(B, H, W), C.c_size_t()
        _lib.check(self.lib.gdb_decoder_train_backward_bytes(C.byref(self.cfg), C.byref(f), self.num_layers, C.byref(need)))
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != rows.device:
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=rows.device)
        pp = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
        gp = (C.c_void_p * len(params))(*[None if g is None else g.data_ptr() for g in grads])
        _lib.check(self.lib.gdb_decoder_train_backward(
            C.byref(self.cfg), C.byref(f), rows.data_ptr(), int(rows.stride(0)), self.packed.data_ptr(), self.num_layers, _lib.PREC_F32, pp,
            self.saved.data_ptr(), self.saved.numel(), g_rgb_c.data_ptr(), self._ws.data_ptr(), self._ws.numel(), gp,
            g_rows.data_ptr() if want_rows else None, int(g_rows.stride(0)) if want_rows else 0, torch.cuda.current_stream(rows.device).cuda_stream))
        return (g_rows if want_rows else None), grads

    def regions(self, B: int, H: int, W: int):
        """(name, offset, bytes, shape) of every region of the saved buffer (gdb_decoder_train_layout; host only)."""
        f, n = self._frame(B, H, W), C.c_int32()
        _lib.check(self.lib.gdb_decoder_train_layout(C.byref(self.cfg), C.byref(f), self.num_layers, None, 0, C.byref(n)))
        regs = (_lib.GdbDecRegion * n.value)()
        _lib.check(self.lib.gdb_decoder_train_layout(C.byref(self.cfg), C.byref(f), self.num_layers, C.cast(regs, C.c_void_p), n.value, C.byref(n)))
        return [(r.name.decode(), int(r.offset), int(r.bytes), tuple(d for d in r.shape if d)) for r in regs]

    def activations(self) -> Dict[str, torch.Tensor]:
        """Named float32 views into the saved buffer of the last `forward`."""
        if self.saved is None or self._shape is None:
            raise ValueError("forward() first")
        return {name: self.saved[off:off + nbytes].view(torch.float32).view(shape) for name, off, nbytes, shape in self.regions(*self._shape)}


class DecodeTrainFunction(torch.autograd.Function):
    """rgb_c = Decoder(rows[:, 12:39]) on the HIP library with a HIP backward: `apply(dt, rows, B, H, W, *decoder_params(module))`, rows
    the contiguous (N_b, Q) bundle rows.  `backward` returns the (N_b, Q) row gradient (columns 0 .. 11 zero: rgb_f's gradient through
    them is autograd's, and autograd adds it) and the parameter gradients; `needs_input_grad` decides which are computed at all.  The
    saved buffer belongs to `dt` and holds ONE forward: a backward after a later forward of the same `dt` raises."""

    @staticmethod
    def forward(ctx, dt: DecoderTrain, rows: torch.Tensor, B: int, H: int, W: int, *params: torch.Tensor) -> torch.Tensor:
        rows = rows.detach()
        rgb_c = dt.forward(rows, B, H, W, params=[p.detach() for p in params])
        ctx.dt, ctx.ticket = dt, dt.forwards
        ctx.save_for_backward(rows)
        return rgb_c

    @staticmethod
    def backward(ctx, g_rgb_c: torch.Tensor):
        dt = ctx.dt
        if dt.forwards != ctx.ticket:
            raise RuntimeError("DecodeTrainFunction.backward after a later forward of the same DecoderTrain: its saved activations are gone")
        (rows,) = ctx.saved_tensors
        g_rows, grads = dt.backward(rows, g_rgb_c.float(), want_params=ctx.needs_input_grad[5:], want_rows=ctx.needs_input_grad[1])
        return (None, g_rows, None, None, None, *grads)

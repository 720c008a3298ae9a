"""The evaluator's metrics on the HIP library (gdb_eval_image / gdb_eval_depth / gdb_eval_lpips, include/gdb_nerf_hip.h): each call
enqueues its launches on the current stream and writes one record of doubles per batch item into rows of a caller's float64 CUDA
table.  Nothing here copies to the host or waits.  CUDA tensors only — there is no CPU fallback here either (the numpy evaluator is
the CPU path).

LPIPS (VGG-16 backbone) takes its weights from the caller: `lpips_weights_from` turns a mapping or a module into the 33 tensors,
`pack_lpips` into the library's packed buffer.  The `lpips` package is not available to this project; agreement with its published
weights and values is unverified (include/gdb_nerf_hip.h has the definition that is implemented and tested)."""
import ctypes as C
from collections.abc import Mapping
from typing import Dict, Optional, Tuple

import torch

from . import _lib

IMAGE_REC, DEPTH_REC = _lib.GDB_EVAL_IMAGE_REC, _lib.GDB_EVAL_DEPTH_REC
WINDOW = 7


def workspace_bytes(B: int, H: int, W: int) -> int:
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_eval_workspace_bytes(int(B), int(H), int(W), C.byref(n)))
    return n.value


def _f32(t: torch.Tensor, name: str, dims: int) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 CUDA tensor")
    if t.dim() != dims:
        raise ValueError(f"{name} of shape {tuple(t.shape)}, expected {dims} dimensions")
    return t.contiguous()


def _records(records: torch.Tensor, B: int, rec: int, name: str) -> None:
    if not records.is_cuda or records.dtype != torch.float64 or records.dim() != 2 or records.stride(1) != 1:
        raise ValueError("records must be a float64 CUDA table with unit-stride rows")
    if records.shape[0] < B or records.shape[1] < rec:
        raise ValueError(f"records of shape {tuple(records.shape)} for {B} {name} records of {rec} doubles")


def _workspace(B: int, H: int, W: int, device) -> Tuple[torch.Tensor, int]:
    nbytes = workspace_bytes(B, H, W)
    # allocated per call: torch's caching allocator hands the block back without a device allocation and keeps it stream-safe
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=device), nbytes


def eval_image(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, records: torch.Tensor,
               crop: Optional[Tuple[int, int, int, int]] = None) -> None:
    """pred (B,3,H,W), gt (B,H,W,3), mask (B,H,W), fp32 CUDA; crop = (y0, x0, h, w) or None for the whole image.  Row b of `records`
    (a view of B rows of a float64 CUDA table) receives [sum (gt - clamp(pred))^2 over the mask, masked pixels, SSIM-map sum of channel
    0, 1, 2 over the (h - 6) x (w - 6) interior windows].  ValueError when the cropped image holds no 7 x 7 window."""
    pred, gt, mask = _f32(pred, "pred", 4), _f32(gt, "gt", 4), _f32(mask, "mask", 3)
    B, H, W, _ = gt.shape
    if gt.shape[3] != 3 or tuple(pred.shape) != (B, 3, H, W) or tuple(mask.shape) != (B, H, W):
        raise ValueError(f"pred {tuple(pred.shape)}, gt {tuple(gt.shape)}, mask {tuple(mask.shape)}: expected (B,3,H,W), (B,H,W,3), (B,H,W)")
    _records(records, B, IMAGE_REC, "image")
    y0, x0, h, w = (0, 0, H, W) if crop is None else [int(v) for v in crop]
    ws, nbytes = _workspace(B, H, W, gt.device)
    _lib.check(_lib.load().gdb_eval_image(pred.data_ptr(), gt.data_ptr(), mask.data_ptr(), B, H, W, y0, x0, h, w, ws.data_ptr(), nbytes,
                                          records.data_ptr(), records.stride(0), torch.cuda.current_stream(gt.device).cuda_stream))


def eval_depth(depth: torch.Tensor, gt: torch.Tensor, records: torch.Tensor, resize: bool) -> None:
    """depth (B,Hd,Wd) against gt (B,H,W), fp32 CUDA, over gt != 0; `resize` resamples depth to (H, W) as the evaluator's
    `_resize_bilinear` does.  Row b of `records` receives [sum |err|, count(|err| < 2), count(|err| < 10), count(gt != 0)]."""
    depth, gt = _f32(depth, "depth", 3), _f32(gt, "gt depth", 3)
    B, H, W = gt.shape
    if depth.shape[0] != B:
        raise ValueError(f"depth {tuple(depth.shape)} against gt {tuple(gt.shape)}: batch sizes differ")
    _records(records, B, DEPTH_REC, "depth")
    ws, nbytes = _workspace(B, H, W, gt.device)
    _lib.check(_lib.load().gdb_eval_depth(depth.data_ptr(), int(depth.shape[1]), int(depth.shape[2]), gt.data_ptr(), B, H, W, int(bool(resize)),
                                          ws.data_ptr(), nbytes, records.data_ptr(), records.stride(0),
                                          torch.cuda.current_stream(gt.device).cuda_stream))


# ---- LPIPS (VGG-16) -----------------------------------------------------------------------------------------------------------
LPIPS_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                  (512, 512), (512, 512), (512, 512))
LPIPS_TAPS = (1, 3, 6, 9, 12)          # the convolutions whose ReLU output is tapped; a 2 x 2 max-pool follows each but the last
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)
LPIPS_KEEP = _lib.LPIPS_KEEP


def lpips_weight_names():
    """This project's own names of the LPIPS tensors, in the packer's order: conv.0 .. conv.12 `.weight` (cout, cin, 3, 3), then their
    `.bias` (cout), lin.0 .. lin.4 (the taps' 1 x 1 weights, C_l values in any shape), shift and scale (3 values each, optional in a
    mapping: the package's constants by default)."""
    return ([f"conv.{i}.weight" for i in range(13)] + [f"conv.{i}.bias" for i in range(13)] + [f"lin.{l}" for l in range(5)]
            + ["shift", "scale"])


def lpips_weights_from(obj) -> Dict[str, torch.Tensor]:
    """{name: contiguous fp32 CPU tensor} under `lpips_weight_names()` from either
      * a mapping with those names (shift / scale optional), or
      * any nn.Module, taken by STRUCTURE and not by key names: in `modules()` order the thirteen 3 x 3 Conv2d, the five bias-free
        1 x 1 Conv2d with one output channel (a module registered twice is taken once), and buffers named `shift` / `scale` if any.
    An `lpips.LPIPS(net='vgg')` object therefore converts without this project knowing its key strings.  ValueError on anything
    that does not have exactly this structure."""
    out = {}
    if isinstance(obj, Mapping):
        for name in lpips_weight_names()[:31]:
            if name not in obj:
                raise ValueError(f"LPIPS weights: `{name}` is missing (names: conv.0 .. conv.12 .weight / .bias, lin.0 .. lin.4, optional shift, scale)")
            out[name] = obj[name]
        out["shift"] = obj["shift"] if "shift" in obj else torch.tensor(LPIPS_SHIFT)
        out["scale"] = obj["scale"] if "scale" in obj else torch.tensor(LPIPS_SCALE)
    elif isinstance(obj, torch.nn.Module):
        convs, lins = [], []
        for m in obj.modules():      # (modules() yields a module once however often it is registered)
            if isinstance(m, torch.nn.Conv2d):
                if tuple(m.kernel_size) == (3, 3):
                    convs.append(m)
                elif tuple(m.kernel_size) == (1, 1) and m.bias is None and m.out_channels == 1:
                    lins.append(m)
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError(f"LPIPS weights: a module with {len(convs)} 3 x 3 and {len(lins)} bias-free 1 x 1 one-output convolutions (13 and 5 expected)")
        for i, m in enumerate(convs):
            if m.bias is None or tuple(m.stride) != (1, 1) or tuple(m.padding) != (1, 1):
                raise ValueError(f"LPIPS weights: 3 x 3 convolution {i} must have a bias, stride 1 and padding 1")
            out[f"conv.{i}.weight"], out[f"conv.{i}.bias"] = m.weight, m.bias
        for l, m in enumerate(lins):
            out[f"lin.{l}"] = m.weight
        bufs = {k.rsplit(".", 1)[-1]: v for k, v in obj.named_buffers() if k.rsplit(".", 1)[-1] in ("shift", "scale")}
        out["shift"] = bufs.get("shift", torch.tensor(LPIPS_SHIFT))
        out["scale"] = bufs.get("scale", torch.tensor(LPIPS_SCALE))
    else:
        raise ValueError(f"LPIPS weights: a mapping or an nn.Module, not {type(obj).__name__}")
    res = {}
    for name in lpips_weight_names():
        t = out[name]
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"LPIPS weights: `{name}` is not a tensor")
        t = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
        kind, _, rest = name.partition(".")
        if kind == "conv":
            cin, cout = LPIPS_CHANNELS[int(rest.split(".")[0])]
            want = (cout, cin, 3, 3) if rest.endswith("weight") else (cout,)
            if tuple(t.shape) != want:
                raise ValueError(f"LPIPS weights: `{name}` of shape {tuple(t.shape)}, expected {want}")
        else:
            n = LPIPS_CHANNELS[LPIPS_TAPS[int(rest)]][1] if kind == "lin" else 3
            if t.numel() != n:
                raise ValueError(f"LPIPS weights: `{name}` holds {t.numel()} values, expected {n}")
            t = t.reshape(n)
        res[name] = t
    return res


def lpips_packed_floats() -> int:
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_lpips_packed_floats(C.byref(n)))
    return n.value


def pack_lpips(weights, device=None) -> torch.Tensor:
    """The library's packed LPIPS buffer (host-side packing; on `device` when given) from anything `lpips_weights_from` takes."""
    w = lpips_weights_from(weights)
    ts = [w[k] for k in lpips_weight_names()]
    host = torch.empty(lpips_packed_floats(), dtype=torch.float32)
    ptrs = (C.c_void_p * _lib.LPIPS_TENSORS)(*[t.data_ptr() for t in ts])
    _lib.check(_lib.load().gdb_pack_lpips_weights(ptrs, host.data_ptr()))
    return host if device is None else host.to(device)


def lpips_workspace_bytes(B: int, h: int, w: int, flags: int = 0) -> int:
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_lpips_workspace_bytes(int(B), int(h), int(w), int(flags), C.byref(n)))
    return n.value


def lpips_layout(B: int, h: int, w: int, flags: int = 0):
    """{region: (byte offset, bytes, shape)} of a gdb_eval_lpips workspace, in the order the regions are laid out."""
    lib = _lib.load()
    n = C.c_int32()
    _lib.check(lib.gdb_lpips_layout(int(B), int(h), int(w), int(flags), None, 0, C.byref(n)))
    regs = (_lib.GdbDecRegion * n.value)()
    _lib.check(lib.gdb_lpips_layout(int(B), int(h), int(w), int(flags), regs, n.value, C.byref(n)))
    return {r.name.decode(): (int(r.offset), int(r.bytes), tuple(int(v) for v in r.shape if v)) for r in regs}


def eval_lpips(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, packed: torch.Tensor, records: torch.Tensor,
               crop: Optional[Tuple[int, int, int, int]] = None, flags: int = 0, workspace: Optional[torch.Tensor] = None) -> None:
    """pred (B,3,H,W), gt (B,H,W,3), mask (B,H,W), fp32 CUDA, as `eval_image` takes them; `packed` from `pack_lpips` on the same
    device.  Element [b, 0] of `records` (a view of B rows of a float64 CUDA table) receives LPIPS(clamp(pred_b), gt_b) of the cropped
    images, both zeroed except where mask >= 1.  ValueError when the cropped extent is below 16 x 16.  `workspace`: a caller's own CUDA
    buffer of at least `lpips_workspace_bytes(B, h, w, flags)` bytes (the tests read the kept layers from it); else one is taken from
    torch's caching allocator per call."""
    pred, gt, mask = _f32(pred, "pred", 4), _f32(gt, "gt", 4), _f32(mask, "mask", 3)
    B, H, W, _ = gt.shape
    if gt.shape[3] != 3 or tuple(pred.shape) != (B, 3, H, W) or tuple(mask.shape) != (B, H, W):
        raise ValueError(f"pred {tuple(pred.shape)}, gt {tuple(gt.shape)}, mask {tuple(mask.shape)}: expected (B,3,H,W), (B,H,W,3), (B,H,W)")
    if not packed.is_cuda or packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous() or packed.numel() < lpips_packed_floats():
        raise ValueError("packed must be the contiguous float32 CUDA buffer of pack_lpips")
    _records(records, B, 1, "LPIPS")
    y0, x0, h, w = (0, 0, H, W) if crop is None else [int(v) for v in crop]
    if workspace is None:
        nbytes = lpips_workspace_bytes(B, h, w, flags)
        workspace = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=gt.device)
    elif not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous CUDA tensor")
    nbytes = workspace.numel() * workspace.element_size()
    _lib.check(_lib.load().gdb_eval_lpips(pred.data_ptr(), gt.data_ptr(), mask.data_ptr(), B, H, W, y0, x0, h, w, packed.data_ptr(), int(flags),
                                          workspace.data_ptr(), nbytes, records.data_ptr(), records.stride(0),
                                          torch.cuda.current_stream(gt.device).cuda_stream))

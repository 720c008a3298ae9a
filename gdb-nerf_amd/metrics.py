"""The evaluator's metrics on the HIP library (gdb_eval_image / gdb_eval_depth, include/gdb_nerf_hip.h): each call enqueues its
launches on the current stream and writes one record of doubles per batch item into rows of a caller's float64 CUDA table.  Nothing
here copies to the host or waits.  CUDA tensors only — there is no CPU fallback here either (the numpy evaluator is the CPU path)."""
import ctypes as C
from typing import Optional, Tuple

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

"""The training loss of train/losses/gdb_nerf.py: MSE + SSIM on the HIP library (gdb_photometric_loss, include/gdb_nerf_hip.h has
the definition), its plain-torch restatement, the masked smooth-L1 depth monitor, and the VGG-16 perceptual term in plain torch
from caller-supplied weights.

`photometric_terms` is one library call: it enqueues on the current stream and returns three 0-dim CUDA tensors; with a gradient
wanted the same call has already written it, and backward is one multiplication.  Nothing here copies to the host or waits.  CUDA
fp32 tensors only - `photometric_terms_torch` is the CPU path, the path for `train.hip_loss: false`, and the tests' reference.

The perceptual term stays in torch (ten VGG convolutions forward and nine backward per image: MIOpen's are faster than this
project's own LPIPS convolution).  torchvision's weights are not available to this project: `VggPerceptual` takes the ten
convolutions from the caller, and agreement with torchvision's published weights is unverified."""
import ctypes as C
import functools
from collections.abc import Mapping
from typing import Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

WINDOW, SIGMA, C1, C2 = 7, 1.5, 0.01 ** 2, 0.03 ** 2


# ---- plain torch --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ssim_window(dtype, device) -> torch.Tensor:
    with torch.inference_mode(False):   # kept across calls: an inference tensor could not serve a later call under autograd
        x = torch.arange(WINDOW, dtype=torch.float32)
        g = torch.exp(-((x - WINDOW // 2) ** 2) / (2 * SIGMA ** 2))
        g = (g / g.sum()).unsqueeze(1)
        return (g @ g.t()).expand(3, 1, WINDOW, WINDOW).contiguous().to(device=device, dtype=dtype)


def ssim_window(dtype=torch.float32, device=None) -> torch.Tensor:
    """(3, 1, 7, 7): the Gaussian window, formed in fp32 whatever `dtype` is (a float64 evaluation uses the fp32 window's values,
    as a float64 copy of the trained module does).  Formed and uploaded ONCE per (dtype, device) and kept, as the reference keeps
    its window in a module buffer: only the first call for a device copies from the host.  Treat the result as read-only."""
    return _ssim_window(dtype, torch.device("cpu") if device is None else torch.device(device))


def ssim_torch(gt: torch.Tensor, est: torch.Tensor) -> torch.Tensor:
    """Mean of the SSIM map of two (B,3,H,W) batches: five depth-wise convolutions with zero padding 3."""
    w = ssim_window(est.dtype, est.device)
    blur = lambda t: F.conv2d(t, w, padding=WINDOW // 2, groups=3)
    m1, m2 = blur(gt), blur(est)
    m11, m22, m12 = m1.square(), m2.square(), m1 * m2
    s1, s2, s12 = blur(gt.square()) - m11, blur(est.square()) - m22, blur(gt * est) - m12
    return (((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2))).mean()


def photometric_terms_torch(gt: torch.Tensor, est: torch.Tensor, alpha: float, beta: float):
    """(photo, mse, ssim) with photo = alpha mse + beta (1 - ssim), differentiable through `photo`; `mse` and `ssim` are detached,
    as `photometric_terms` returns them."""
    mse = F.mse_loss(gt, est, reduction="mean")
    ssim = ssim_torch(gt, est)
    return alpha * mse + beta * (1 - ssim), mse.detach(), ssim.detach()


def smooth_l1_masked_torch(est: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """Mean of smooth-L1 (beta 1) over mask > 0.5, NaN for an empty mask; a select and two sums, no boolean indexing (which would
    wait for the host to learn the count)."""
    m = mask > 0.5
    per = F.smooth_l1_loss(est, gt, reduction="none")
    return torch.where(m, per, torch.zeros_like(per)).sum() / m.sum()


# ---- HIP ----------------------------------------------------------------------------------------------------------------------
def workspace_bytes(B: int, H: int, W: int) -> int:
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_loss_workspace_bytes(int(B), int(H), int(W), C.byref(n)))
    return n.value


def _f32_cuda(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 CUDA tensor (photometric_terms_torch is the path for anything else)")


def photometric_hip(gt: torch.Tensor, est: torch.Tensor, alpha: float, beta: float, want_grad: bool, workspace=None, grad=None):
    """The library call: (out3 = [mse, ssim, photo] as a (3,) CUDA tensor, G or None).  `gt` (B,3,H,W) is read at its own strides (an
    NCHW tensor or the `permute(0, 3, 1, 2)` view of an NHWC frame, no copy); `est` is made contiguous.  `workspace` / `grad`: the
    caller's own buffers (the tests pre-fill them); else taken from torch's caching allocator per call."""
    _f32_cuda(gt, "gt"), _f32_cuda(est, "est")
    if est.dim() != 4 or est.shape[1] != 3 or gt.shape != est.shape:
        raise ValueError(f"gt {tuple(gt.shape)}, est {tuple(est.shape)}: expected two (B,3,H,W) tensors")
    if gt.device != est.device:
        raise ValueError(f"gt is on {gt.device}, est on {est.device}: one device expected")
    est = est.detach().contiguous()
    gt = gt.detach()
    B, _, H, W = est.shape
    if workspace is None:
        nbytes = workspace_bytes(B, H, W)
        workspace = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=est.device)
    nbytes = workspace.numel() * workspace.element_size()
    if want_grad and grad is None:
        grad = torch.empty_like(est)
    out3 = torch.empty(3, dtype=torch.float32, device=est.device)
    sb, sc, sy, sx = gt.stride()
    with torch.cuda.device(est.device):   # the launch goes to the tensors' device, whichever is current
        _lib.check(_lib.load().gdb_photometric_loss(est.data_ptr(), gt.data_ptr(), sb, sc, sy, sx, B, H, W, float(alpha), float(beta),
                                                    grad.data_ptr() if want_grad else None, workspace.data_ptr(), nbytes, out3.data_ptr(),
                                                    torch.cuda.current_stream(est.device).cuda_stream))
    return out3, (grad if want_grad else None)


class PhotometricFunction(torch.autograd.Function):
    """forward = the one library call, which writes G = d photo / d est as well; backward = grad_photo * G."""

    @staticmethod
    def forward(ctx, est, gt, alpha, beta):
        out3, G = photometric_hip(gt, est, alpha, beta, want_grad=True)
        ctx.save_for_backward(G)
        mse, ssim, photo = out3.unbind(0)
        ctx.mark_non_differentiable(mse, ssim)
        return photo, mse, ssim

    @staticmethod
    @once_differentiable
    def backward(ctx, g_photo, g_mse, g_ssim):
        (G,) = ctx.saved_tensors
        return g_photo * G, None, None, None


def photometric_terms(gt: torch.Tensor, est: torch.Tensor, alpha: float, beta: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(photo, mse, ssim), 0-dim fp32 CUDA tensors, photo = alpha mse + beta (1 - ssim) of gt, est (B,3,H,W).  The gradient is
    written (and kept for backward) when `est.requires_grad` under grad mode; otherwise the library's no-gradient form runs.
    `mse` and `ssim` are NOT differentiable: the loss module uses them for its statistics only (`mse_loss`, `psnr`, `ssim`), and the
    gradient of `photo` is the only one the library forms.  No gradient reaches `gt`."""
    if torch.is_grad_enabled() and est.requires_grad:
        return PhotometricFunction.apply(est, gt, float(alpha), float(beta))
    mse, ssim, photo = photometric_hip(gt, est, alpha, beta, want_grad=False)[0].unbind(0)
    return photo, mse, ssim


def smooth_l1_masked(est: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """0-dim fp32 CUDA tensor: the mean over mask > 0.5 of smooth-L1(est - gt), beta 1; NaN for an empty mask.  Forward only."""
    for t, name in ((est, "est"), (gt, "gt"), (mask, "mask")):
        _f32_cuda(t, name)
    if not (est.device == gt.device == mask.device):
        raise ValueError(f"est on {est.device}, gt on {gt.device}, mask on {mask.device}: one device expected")
    if not (est.shape == gt.shape == mask.shape) or est.numel() < 1:
        raise ValueError(f"est {tuple(est.shape)}, gt {tuple(gt.shape)}, mask {tuple(mask.shape)}: expected three non-empty tensors of one shape")
    est, gt, mask = est.detach().contiguous(), gt.detach().contiguous(), mask.detach().contiguous()
    n = est.numel()
    if n >= 2 ** 31:
        raise ValueError(f"smooth_l1_masked: {n} elements (fewer than 2^31 expected)")
    ws = torch.empty(((workspace_bytes(1, 1, n) + 7) // 8,), dtype=torch.float64, device=est.device)
    out = torch.empty(1, dtype=torch.float32, device=est.device)
    with torch.cuda.device(est.device):
        _lib.check(_lib.load().gdb_smooth_l1_masked(est.data_ptr(), gt.data_ptr(), mask.data_ptr(), n, ws.data_ptr(), ws.numel() * 8,
                                                    out.data_ptr(), torch.cuda.current_stream(est.device).cuda_stream))
    return out[0]


# ---- the perceptual term --------------------------------------------------------------------------------------------------------
VGG_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512))
VGG_BLOCKS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9))    # torchvision vgg16.features[:4], [4:9], [9:16], [16:23]: a 2 x 2 max-pool opens
VGG_MEAN, VGG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # every block but the first


def vgg_weights_from(obj):
    """[(weight (cout,cin,3,3), bias (cout,))] x 10, dtype kept, from either
      * a mapping with this project's LPIPS names `conv.0 .. conv.9` (`.weight` / `.bias`; further entries are ignored, so the file
        exported for `test.lpips_weights` serves), or
      * any nn.Module, by structure: its first ten 3 x 3 Conv2d in `modules()` order (torchvision's `vgg16().features` converts)."""
    if isinstance(obj, Mapping):
        missing = [f"conv.{i}{s}" for i in range(10) for s in (".weight", ".bias") if f"conv.{i}{s}" not in obj]
        if missing:
            raise ValueError(f"VGG weights: {missing[0]} is missing (names: conv.0 .. conv.9 .weight / .bias)")
        pairs = [(obj[f"conv.{i}.weight"], obj[f"conv.{i}.bias"]) for i in range(10)]
    elif isinstance(obj, torch.nn.Module):
        convs = [m for m in obj.modules() if isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3)][:10]
        if len(convs) < 10 or any(m.bias is None or tuple(m.stride) != (1, 1) or tuple(m.padding) != (1, 1) for m in convs):
            raise ValueError("VGG weights: a module whose first ten 3 x 3 convolutions have a bias, stride 1 and padding 1 is expected")
        pairs = [(m.weight, m.bias) for m in convs]
    else:
        raise ValueError(f"VGG weights: a mapping or an nn.Module, not {type(obj).__name__}")
    out = []
    for i, ((cin, cout), (w, b)) in enumerate(zip(VGG_CHANNELS, pairs)):
        if not isinstance(w, torch.Tensor) or not isinstance(b, torch.Tensor) or tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise ValueError(f"VGG weights: conv.{i} must be ({cout},{cin},3,3) with a bias of {cout}")
        out.append((w.detach().clone(), b.detach().clone()))
    return out


class VggPerceptual(torch.nn.Module):
    """The sum over four VGG-16 blocks of the mean L1 distance between the blocks' outputs for the two images, after ImageNet
    normalisation; no resize.  The weights are frozen buffers (they follow `.to()` and stay out of `parameters()`); the gradient
    reaches the images only."""

    def __init__(self, weights):
        super().__init__()
        for i, (w, b) in enumerate(vgg_weights_from(weights)):
            self.register_buffer(f"w{i}", w)
            self.register_buffer(f"b{i}", b)
        self.register_buffer("mean", torch.tensor(VGG_MEAN).view(1, 3, 1, 1))
        self.register_buffer("std", torch.tensor(VGG_STD).view(1, 3, 1, 1))

    def forward(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        if a.shape[1] != 3:
            a, b = a.repeat(1, 3, 1, 1), b.repeat(1, 3, 1, 1)
        x, y = ((t - self.mean.to(t.dtype)) / self.std.to(t.dtype) for t in (a, b))
        loss = 0.0
        for k, block in enumerate(VGG_BLOCKS):
            if k:
                x, y = F.max_pool2d(x, 2, 2), F.max_pool2d(y, 2, 2)
            for i in block:
                w, bias = getattr(self, f"w{i}").to(x.dtype), getattr(self, f"b{i}").to(x.dtype)
                x, y = F.relu(F.conv2d(x, w, bias, padding=1)), F.relu(F.conv2d(y, w, bias, padding=1))
            loss = loss + F.l1_loss(x, y)
        return loss

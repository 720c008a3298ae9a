"""Fixture F9: the reference's own SSIM module (train/losses/ssim_loss.py, loaded by file path: it imports torch alone) and
`F.mse_loss`, as train/losses/photometric_loss.py:16-20 combines them, on seeded inputs.  Per case the inputs, then `mse`, `ssim` and
the gradient of 1.0 * mse + 0.1 * (1 - ssim) with respect to the estimate, recorded from the module in fp32 and from the module
`.double()` on the same inputs.  The reference's VGG term needs torchvision's weights and gets no fixture.

    python tests/golden/make_golden_loss.py REFERENCE_ROOT

The cases are the smallest shapes at which the tiled kernel can go wrong (tests/test_loss_referee.py says what each exercises)."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA, BETA = 1.0, 0.1
CASES = ("one_pixel", "below_window", "noise_33x70", "exact_tiles", "smooth_40x37", "near_equal")
GT_OF = {"near_equal": "noise_33x70"}   # near_equal is the white-noise ground truth again, with an estimate 1e-3 away


def inputs():
    """{case: (gt, est)} as float32 (B,3,H,W) arrays."""
    rng = np.random.default_rng(9)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    out = {}
    gt = rng.random((3, 3, 1, 1))
    out["one_pixel"] = (f(gt), f(gt + 0.1 * rng.standard_normal(gt.shape)))
    gt = rng.random((2, 3, 5, 9))
    out["below_window"] = (f(gt), f(gt + 0.1 * rng.standard_normal(gt.shape)))
    noise = rng.random((1, 3, 33, 70))
    out["noise_33x70"] = (f(noise), f(noise + 0.2 * rng.standard_normal(noise.shape)))
    gt = rng.random((1, 3, 64, 64))
    out["exact_tiles"] = (f(gt), f(gt + 0.05 * rng.standard_normal(gt.shape)))
    y, x = np.meshgrid(np.arange(40.0), np.arange(37.0), indexing="ij")
    gt = np.stack([0.5 + 0.25 * np.sin(0.25 * x + p) * np.cos(0.2 * y - p) for p in (0.0, 0.7, 1.9)])[None]
    out["smooth_40x37"] = (f(gt), f(gt + 0.02 * rng.standard_normal(gt.shape)))
    out["near_equal"] = (f(noise), f(noise + 1e-3 * rng.standard_normal(noise.shape)))
    return out


def main():
    ref_root = sys.argv[1]
    spec = importlib.util.spec_from_file_location("ref_ssim_loss", os.path.join(ref_root, "train", "losses", "ssim_loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (gt, est) in inputs().items():
        out[f"{name}.est"] = est
        if name not in GT_OF:    # (a case listed there reads another case's ground truth: not stored twice)
            out[f"{name}.gt"] = gt
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            module = ref.SSIM(window_size=7, channel=3)
            module = module.double() if dt == torch.float64 else module
            g, e = torch.from_numpy(gt).to(dt), torch.from_numpy(est).to(dt).requires_grad_()
            mse, ssim = F.mse_loss(g, e, reduction="mean"), module(g, e)
            (ALPHA * mse + BETA * (1 - ssim)).backward()
            out[f"{name}.mse{tag}"], out[f"{name}.ssim{tag}"], out[f"{name}.grad{tag}"] = mse.detach().numpy(), ssim.detach().numpy(), e.grad.numpy()
        print(f"{name:14s} {gt.shape}  mse {float(out[name + '.mse64']):.6e}  ssim {float(out[name + '.ssim64']):.8f}")
    path = os.path.join(HERE, "F9_photometric.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()

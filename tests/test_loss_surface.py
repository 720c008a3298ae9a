"""The loss surface without a GPU: the plain-torch restatement against the fixture recorded from the reference's own SSIM module
(tests/golden/make_golden_loss.py), the perceptual term against an nn.Sequential, the NetworkWrapper's contract on the CPU with a
stand-in network, the plugin factory, the build-time properties of gdb_loss.hip and the host-side refusals of its entries."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT, load_golden
from gdb_nerf_amd import _lib, build, losses
from gdb_nerf_amd.configs import make_cfg

CASES = ("one_pixel", "below_window", "noise_33x70", "exact_tiles", "smooth_40x37", "near_equal")
GT_OF = {"near_equal": "noise_33x70"}   # the fixture stores this ground truth once
ALPHA, BETA = 1.0, 0.1
ENTRIES = ("gdb_loss_workspace_bytes", "gdb_photometric_loss", "gdb_smooth_l1_masked")


def restatement(fx, name, dtype):
    gt, est = torch.from_numpy(fx[GT_OF.get(name, name) + ".gt"]).to(dtype), torch.from_numpy(fx[name + ".est"]).to(dtype).requires_grad_()
    photo, mse, ssim = losses.photometric_terms_torch(gt, est, ALPHA, BETA)
    photo.backward()
    return mse.numpy(), ssim.numpy(), est.grad.numpy()


def ulp8(ref):
    return 8.0 * float(np.spacing(np.float32(np.abs(ref).max())))


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_record(name):
    fx = load_golden("F9_photometric")
    for got, key in zip(restatement(fx, name, torch.float32), ("mse32", "ssim32", "grad32")):
        ref = fx[f"{name}.{key}"]
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.abs(got.astype(np.float64) - ref).max() <= ulp8(ref), (name, key)
    for got, key in zip(restatement(fx, name, torch.float64), ("mse64", "ssim64", "grad64")):
        ref = fx[f"{name}.{key}"]
        assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-12, (name, key)


def test_restatement_returns_detached_statistics():
    gt, est = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8, requires_grad=True)
    photo, mse, ssim = losses.photometric_terms_torch(gt, est, 1.0, 0.1)
    assert photo.requires_grad and not mse.requires_grad and not ssim.requires_grad
    assert torch.allclose(photo, 1.0 * mse + 0.1 * (1 - ssim))


def test_the_window_is_formed_once_per_dtype_and_device():
    """The restatement's window is kept, as the reference keeps its module buffer: no per-call host work or upload."""
    w = losses.ssim_window(torch.float32, "cpu")
    assert losses.ssim_window(torch.float32, torch.device("cpu")) is w and losses.ssim_window() is w
    assert losses.ssim_window(torch.float64) is losses.ssim_window(torch.float64)
    assert torch.equal(losses.ssim_window(torch.float64), w.double()) and abs(w[0, 0].sum().item() - 1) < 1e-6
    with torch.inference_mode():
        w16 = losses.ssim_window(torch.float16)
    assert not w16.is_inference()


def test_smooth_l1_masked_torch():
    rng = np.random.default_rng(3)
    est, gt = torch.from_numpy(rng.standard_normal((2, 7, 9)) * 2), torch.from_numpy(rng.standard_normal((2, 7, 9)))
    mask = torch.from_numpy(rng.random((2, 7, 9)))
    keep = mask > 0.5
    want = torch.nn.functional.smooth_l1_loss(est[keep], gt[keep], reduction="mean")
    assert abs(losses.smooth_l1_masked_torch(est, gt, mask).item() - want.item()) <= 1e-14
    assert torch.isnan(losses.smooth_l1_masked_torch(est, gt, torch.zeros_like(mask)))
    est[~keep] = float("nan")   # what the mask leaves out does not reach the mean
    assert abs(losses.smooth_l1_masked_torch(est, gt, mask).item() - want.item()) <= 1e-14


# ---- the perceptual term --------------------------------------------------------------------------------------------------------
def vgg16_features(seed):
    layers, cin = [], 3
    for v in [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512]:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    feats = nn.Sequential(*layers).double()
    g = torch.Generator().manual_seed(seed)
    for m in feats:
        if isinstance(m, nn.Conv2d):
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) * (2.0 / (9 * m.in_channels)) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g, dtype=torch.float64) * 0.1)
    return feats


def test_vgg_perceptual_equals_a_sequential_and_takes_the_lpips_names():
    feats = vgg16_features(4)
    blocks = [feats[:4], feats[4:9], feats[9:16], feats[16:23]]
    g = torch.Generator().manual_seed(5)
    a, b = torch.rand(2, 3, 19, 22, generator=g, dtype=torch.float64), torch.rand(2, 3, 19, 22, generator=g, dtype=torch.float64)
    # (fp32 constants, as the reference registers them: a float64 run sees the fp32 values)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).double(), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).double()
    x, y, want = (a - mean) / std, (b - mean) / std, 0.0
    for blk in blocks:
        x, y = blk(x), blk(y)
        want = want + torch.nn.functional.l1_loss(x, y)
    by_structure = losses.VggPerceptual(feats)
    assert not list(by_structure.parameters())          # frozen: buffers only
    assert abs(by_structure(a, b).item() - want.item()) <= 1e-10
    convs = [m for m in feats if isinstance(m, nn.Conv2d)]
    mapping = {f"conv.{i}.{k}": getattr(m, k).detach() for i, m in enumerate(convs) for k in ("weight", "bias")}
    mapping["lin.0"] = torch.zeros(64)                  # an LPIPS export's further entries are ignored
    by_name = losses.VggPerceptual(mapping)
    assert abs(by_name(a, b).item() - want.item()) <= 1e-10
    b.requires_grad_()
    by_name(a, b).backward()
    assert torch.isfinite(b.grad).all() and b.grad.abs().max() > 0
    del mapping["conv.9.bias"]
    with pytest.raises(ValueError, match="conv.9.bias"):
        losses.VggPerceptual(mapping)
    with pytest.raises(ValueError):
        losses.VggPerceptual(nn.Sequential(*list(feats)[:10]))


# ---- NetworkWrapper on the CPU ----------------------------------------------------------------------------------------------------
class StandIn(nn.Module):
    """Returns a final image, two stage depths and two stage images that depend on one parameter."""

    def __init__(self, imgs, stages, depths):
        super().__init__()
        self.gain = nn.Parameter(torch.tensor(1.0))
        self.imgs, self.stages, self.depths = imgs, stages, depths

    def forward(self, batch):
        return {"rgb": self.imgs * self.gain}, self.depths, [s * self.gain for s in self.stages]


def wrapper_case(opts=()):
    from gdb_nerf_amd.train.trainers import make_wrapper
    cfg = make_cfg("configs/dtu_pretrain.yaml", ["mvs.loss_weight", "[0.05, 0.2]", *opts])
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.rand(*s, generator=g)
    imgs, stages, depths = r(2, 3, 16, 24), [r(2, 3, 4, 6), r(2, 3, 8, 12)], [r(2, 4, 6) * 3, r(2, 8, 12) * 3]
    batch = {"tar_views": {"rgb": r(2, 16, 24, 3)},
             "tar_gt_ms": {"rgb": [r(2, 4, 6, 3), r(2, 8, 12, 3)], "depth": [r(2, 4, 6) * 3, r(2, 8, 12) * 3], "mask": [r(2, 4, 6), r(2, 8, 12)]}}
    net = StandIn(imgs, stages, depths)
    return make_wrapper(cfg, net), net, batch, cfg


def test_network_wrapper_on_the_cpu_with_a_stand_in_network():
    wrapper, net, batch, cfg = wrapper_case(["train.photometric_weights", "[1.0, 0.1, 0.0]"])
    assert type(wrapper).__name__ == "NetworkWrapper" and type(wrapper).__module__.endswith("train.losses.gdb_nerf")
    wrapper.train()
    output, loss, stats, image_stats = wrapper(batch)
    assert set(stats) == {"mse_loss", "psnr", "ssim", "perceptual_loss", "loss", "depth_loss", "depth_loss0", "depth_loss1"}
    assert image_stats == {} and output["rgb"].shape == (2, 3, 16, 24)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    photo = lambda gt, est: losses.photometric_terms_torch(gt, est, 1.0, 0.1)
    colour, mse, ssim = photo(nchw(batch["tar_views"]["rgb"]), net.imgs)
    hand = colour + 0.05 * photo(nchw(batch["tar_gt_ms"]["rgb"][0]), net.stages[0])[0] + 0.2 * photo(nchw(batch["tar_gt_ms"]["rgb"][1]), net.stages[1])[0]
    assert abs(loss.item() - hand.item()) <= 1e-6 and stats["loss"] is loss
    assert abs(stats["depth_loss"].item() - (hand - colour).item()) <= 1e-6
    assert stats["mse_loss"].item() == mse.item() and stats["ssim"].item() == ssim.item() and stats["perceptual_loss"].item() == 0.0
    assert abs(stats["psnr"].item() - (-10.0 * np.log10(mse.item() + 1e-6))) <= 1e-4
    for i in range(2):
        keep = batch["tar_gt_ms"]["mask"][i] > 0.5
        want = torch.nn.functional.smooth_l1_loss(net.depths[i][keep], batch["tar_gt_ms"]["depth"][i][keep])
        assert abs(stats[f"depth_loss{i}"].item() - want.item()) <= 1e-6
    loss.backward()
    assert net.gain.grad is not None and net.gain.grad.abs() > 0
    wrapper.eval()
    with torch.no_grad():
        _, loss_eval, stats_eval, _ = wrapper(batch)
    assert "depth_loss" not in stats_eval and abs(loss_eval.item() - colour.item()) <= 1e-6
    del batch["tar_gt_ms"]["depth"]
    assert set(wrapper(batch)[2]) == {"mse_loss", "psnr", "ssim", "perceptual_loss", "loss"}


def test_network_wrapper_refuses_a_perceptual_weight_without_weights(tmp_path):
    with pytest.raises(ValueError, match=r"(?s)train\.vgg_weights.*photometric_weights"):
        wrapper_case()   # the default weights: [1.0, 0.1, 0.05], no file
    feats = vgg16_features(7).float()
    convs = [m for m in feats if isinstance(m, nn.Conv2d)]
    path = tmp_path / "vgg.pt"
    torch.save({f"conv.{i}.{k}": getattr(m, k).detach() for i, m in enumerate(convs) for k in ("weight", "bias")}, path)
    wrapper, net, batch, _ = wrapper_case(["train.vgg_weights", str(path)])
    wrapper.eval()
    _, loss, stats, _ = wrapper(batch)
    colour = losses.photometric_terms_torch(batch["tar_views"]["rgb"].permute(0, 3, 1, 2), net.imgs, 1.0, 0.1)[0]
    assert stats["perceptual_loss"].item() > 0
    assert abs(loss.item() - (colour + 0.05 * stats["perceptual_loss"]).item()) <= 1e-6


def test_make_wrapper_loads_the_module_at_loss_path(tmp_path):
    from gdb_nerf_amd.train.trainers import make_wrapper
    src = tmp_path / "my_loss.py"
    src.write_text("class NetworkWrapper:\n    def __init__(self, net, cfg):\n        self.net, self.cfg = net, cfg\n")
    cfg = make_cfg("configs/dtu_pretrain.yaml")
    assert cfg.loss_module == "train.losses.gdb_nerf" and cfg.loss_path == "train/losses/gdb_nerf.py"
    assert cfg.train.hip_loss is False and cfg.train.photometric_weights == [1.0, 0.1, 0.05] and cfg.train.vgg_weights == ""
    cfg.loss_module, cfg.loss_path = "my_loss", str(src)
    w = make_wrapper(cfg, "net")
    assert type(w).__module__ == "my_loss" and w.net == "net" and w.cfg is cfg


# ---- the library ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_loss_kernels_use_no_private_memory_and_fit_the_lds(lib):
    path = os.path.join(build.CSRC, "obj", "resource_usage.json")
    if "gdb_loss.hip" not in json.load(open(path)):
        build.build(force=True)
    usage = json.load(open(path))["gdb_loss.hip"]
    names = " ".join(usage)
    for k in ("k_photometricILb1E", "k_photometricILb0E", "k_smooth_l1", "k_loss_finishILb1E", "k_loss_finishILb0E"):
        assert k in names, k
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0 and u["lds_bytes"] <= 64 * 1024, (name, u)


def test_header_declares_the_loss_entries_and_they_refuse_on_the_host(lib):
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(gdb_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.gdb_abi_version() == 7   # additions only
    n = C.c_size_t()
    assert lib.gdb_loss_workspace_bytes(1, 33, 70, C.byref(n)) == _lib.GDB_OK and n.value >= 16 * 3 * 2 * 3
    assert lib.gdb_loss_workspace_bytes(1, 33, 70, None) == _lib.GDB_E_BADARG
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (2 ** 31 - 1, 2 ** 15, 2 ** 15), (6000, 1024, 1024)):   # the last: 2^32 work-items and more
        assert lib.gdb_loss_workspace_bytes(*shape, C.byref(n)) == _lib.GDB_E_SHAPE, shape
    # every refusal comes before the first launch: these pointers are never dereferenced
    p = C.c_void_p(4096)
    call = lambda est=p, gt=p, B=1, ws=p, nbytes=1 << 20, out=p: lib.gdb_photometric_loss(est, gt, 3 * 64, 64, 8, 1, B, 8, 8, 1.0, 0.1, None, ws, nbytes, out, None)
    assert call(est=None) == call(gt=None) == call(ws=None) == call(out=None) == _lib.GDB_E_BADARG
    assert call(B=0) == _lib.GDB_E_SHAPE
    assert call(nbytes=47) == _lib.GDB_E_BADARG and "workspace" in lib.gdb_last_error().decode()
    mon = lambda est=p, n=100, nbytes=1 << 20: lib.gdb_smooth_l1_masked(est, p, p, n, p, nbytes, p, None)
    assert mon(est=None) == _lib.GDB_E_BADARG and mon(n=0) == _lib.GDB_E_SHAPE and mon(nbytes=15) == _lib.GDB_E_BADARG


def test_hip_entries_refuse_cpu_tensors():
    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(ValueError, match="CUDA"):
        losses.photometric_terms(a, a, 1.0, 0.1)
    with pytest.raises(ValueError, match="CUDA"):
        losses.smooth_l1_masked(a, a, a)

"""gdb_photometric_loss / gdb_smooth_l1_masked and the loss plugin on a real MI355X (`pytest -m gpu`), against the float64 CPU
restatement (losses.photometric_terms_torch), which is itself pinned to the record of the reference's own module
(tests/golden/F9_photometric.npz, tests/test_loss_surface.py).

Rule (tests/test_backward_referee.py's), for the gradient elementwise and for each of the three scalars, no element excluded:
|hip - ref64| <= 4 max(E32, 8 fp32 ulp of max |ref64|), E32 = max |float32 CPU restatement - ref64|.  The kernel is not part of the
bound.  The loss is smooth: there is nothing to leave out.

Cases (B, H, W), the smallest shapes at which the 32 x 32-tile kernel can go wrong:
  one_pixel     (3, 1, 1)    a 1 x 1 image
  below_window  (2, 5, 9)    smaller than the window both ways; two different images, so batch indexing shows
  noise_33x70   (1, 33, 70)  white noise; one row and six columns past tile edges, a remainder narrower than the halo
  exact_tiles   (1, 64, 64)  exact tiles
  smooth_40x37  (1, 40, 37)  a smooth sinusoid plus 0.02 noise, SSIM 0.952: the variances are differences of nearly equal moments
  near_equal    (1, 33, 70)  est = gt + 1e-3 noise, SSIM 0.999994: the gradient's two terms cancel
Each runs with the ground truth as an NCHW tensor and as the permuted view of an NHWC one, with the workspace and the gradient
buffer pre-filled with NaN.

Observed |hip - ref64| / bound: profiles/loss/referee_observed.txt (rewritten by a run of this file)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from gdb_nerf_amd import losses, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "loss", "referee_observed.txt")
CASES = ("one_pixel", "below_window", "noise_33x70", "exact_tiles", "smooth_40x37", "near_equal")
GT_OF = {"near_equal": "noise_33x70"}   # the fixture stores this ground truth once
ALPHA, BETA = 1.0, 0.1
_observed = {}


def restate(gt, est, dtype, alpha=ALPHA, beta=BETA):
    """The CPU restatement in `dtype` -> {grad, mse, ssim, photo} as float64 numpy."""
    g = torch.as_tensor(gt).detach().cpu().to(dtype)
    e = torch.as_tensor(est).detach().cpu().to(dtype).requires_grad_()
    photo, mse, ssim = losses.photometric_terms_torch(g, e, alpha, beta)
    photo.backward()
    return {"grad": e.grad.double().numpy(), "mse": mse.double().numpy(), "ssim": ssim.double().numpy(), "photo": photo.detach().double().numpy()}


def check_rule(case, hip, ref64, ref32):
    """Prints each figure, records it, then asserts the rule for every tensor of `hip`."""
    fails = []
    for name, h in hip.items():
        h, r64 = np.asarray(h, np.float64), ref64[name]
        assert h.shape == r64.shape, (case, name, h.shape, r64.shape)
        top = float(np.abs(r64).max())
        e32 = float(np.abs(ref32[name] - r64).max())
        bound = 4.0 * max(e32, 8.0 * float(np.spacing(np.float32(top))))
        err = float(np.abs(h - r64).max()) if np.isfinite(h).all() else float("inf")
        line = f"{case:28s} {name:6s} err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}  max|ref64| {top:.3e}"
        print(line)
        _observed[(case, name)] = line
        if not err <= bound:
            fails.append(line)
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        old = {}
        if os.path.exists(OBSERVED):
            for l in open(OBSERVED):
                if l.strip() and not l.startswith("#"):
                    old[tuple(l.split()[:2])] = l.rstrip("\n")
        old.update(_observed)
        with open(OBSERVED, "w") as f:
            f.write("# |hip - ref64| against the bound 4 * max(E32, 8 ulp of max |ref64|); tests/test_loss_referee.py\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError:
        pass
    assert not fails, "\n".join(fails)


@pytest.fixture(scope="module")
def refs():
    """Per case: the inputs and both CPU restatements, computed once; the float64 one is pinned to the reference's record."""
    fx = load_golden("F9_photometric")
    out = {}
    for name in CASES:
        gt, est = fx[GT_OF.get(name, name) + ".gt"], fx[name + ".est"]
        r64, r32 = restate(gt, est, torch.float64), restate(gt, est, torch.float32)
        for key in ("grad", "mse", "ssim"):
            assert np.abs(r64[key] - fx[f"{name}.{key}64"]).max() <= 1e-12, (name, key)
        out[name] = (gt, est, r64, r32)
    return out


def cu(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")


def npy(t):
    return t.detach().cpu().numpy()


def nan_buffers(est):
    B, _, H, W = est.shape
    ws = torch.full(((losses.workspace_bytes(B, H, W) + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda")
    return ws, torch.full_like(est, float("nan"))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", CASES)
def test_value_and_gradient(refs, name, layout):
    gt_np, est_np, r64, r32 = refs[name]
    est, gt = cu(est_np), cu(gt_np)
    if layout == "nhwc":   # what the loss module passes: the permuted view of a (B,H,W,3) frame, no copy
        gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not gt.is_contiguous() or gt.shape[2] * gt.shape[3] == 1
    ws, grad = nan_buffers(est)
    out3, G = losses.photometric_hip(gt, est, ALPHA, BETA, True, workspace=ws, grad=grad)
    assert G.data_ptr() == grad.data_ptr()
    hip = {"grad": npy(G), "mse": npy(out3[0]), "ssim": npy(out3[1]), "photo": npy(out3[2])}
    check_rule(f"{name}_{layout}", hip, r64, r32)
    # two calls: the same bits, whatever the buffers held
    ws2, grad2 = nan_buffers(est)
    ws2.fill_(3.0), grad2.fill_(-7.0)
    out3b, Gb = losses.photometric_hip(gt, est, ALPHA, BETA, True, workspace=ws2, grad=grad2)
    assert torch.equal(out3b, out3) and torch.equal(Gb, G)
    # no-gradient mode: the same three scalars bit for bit, the gradient buffer untouched
    ws3, grad3 = nan_buffers(est)
    out3c, none = losses.photometric_hip(gt, est, ALPHA, BETA, False, workspace=ws3, grad=grad3)
    assert none is None and torch.equal(out3c, out3) and torch.isnan(grad3).all()


def test_autograd_surface_with_a_non_contiguous_estimate_and_an_upstream_factor(refs):
    gt_np, est_np, r64, r32 = refs["noise_33x70"]
    base = torch.zeros(1, 3, 33, 72, device="cuda")
    base[..., 1:71] = cu(est_np)
    base.requires_grad_()
    est = base[..., 1:71]
    assert not est.is_contiguous()
    photo, mse, ssim = losses.photometric_terms(cu(gt_np), est, ALPHA, BETA)
    assert photo.requires_grad and not mse.requires_grad and not ssim.requires_grad
    (0.37 * photo).backward()
    _, G = losses.photometric_hip(cu(gt_np), est, ALPHA, BETA, True)
    assert torch.equal(base.grad[..., 1:71], torch.tensor(0.37, device="cuda") * G)      # backward is grad_photo * G
    assert not base.grad[..., 0].any() and not base.grad[..., 71].any()
    check_rule("non_contiguous_est", {"grad": npy(G), "mse": npy(mse), "ssim": npy(ssim), "photo": npy(photo)}, r64, r32)
    # without grad mode, or without requires_grad: the no-gradient form, the same scalars
    with torch.no_grad():
        quiet = losses.photometric_terms(cu(gt_np), est, ALPHA, BETA)
    plain = losses.photometric_terms(cu(gt_np), est.detach(), ALPHA, BETA)
    for q in (quiet, plain):
        assert not q[0].requires_grad and torch.equal(torch.stack(q), torch.stack((photo.detach(), mse, ssim)))


def test_the_torch_restatement_does_not_wait_for_the_device(refs):
    """After its first call on a device (which uploads the window once) the restatement, forward and backward, makes no
    synchronising call: torch raises on one under the sync debug mode."""
    gt_np, est_np, _, _ = refs["noise_33x70"]
    gt, est = cu(gt_np), cu(est_np).requires_grad_()
    losses.photometric_terms_torch(gt, est, ALPHA, BETA)[0].backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses.photometric_terms_torch(gt, est, ALPHA, BETA)[0].backward()
        losses.photometric_terms(gt, est, ALPHA, BETA)[0].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_smooth_l1_masked():
    rng = np.random.default_rng(12)
    shape = (2, 37, 61)   # 4,514 elements: three chunks of 2,048, the last one short
    gt = rng.uniform(400.0, 800.0, shape).astype(np.float32)
    err = rng.standard_normal(shape).astype(np.float32) * 1.5        # errors on both sides of 1
    err.flat[:4] = (0.999999, 1.0, 1.000001, -1.0)
    est, mask = (gt + err).astype(np.float32), rng.random(shape).astype(np.float32)
    mask.flat[:4] = 1.0
    d = np.abs(est.astype(np.float64) - gt.astype(np.float64))
    assert (d < 1).sum() > 1000 and (d > 1).sum() > 1000
    per = np.where(d < 1, 0.5 * d * d, d - 0.5)
    keep = mask > 0.5
    ref64 = per[keep].mean()
    ref32 = losses.smooth_l1_masked_torch(torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)).double().numpy()
    got = losses.smooth_l1_masked(cu(est), cu(gt), cu(mask))
    assert got.dim() == 0 and got.dtype == torch.float32
    check_rule("smooth_l1_random_mask", {"value": npy(got)}, {"value": np.asarray(ref64)}, {"value": ref32})
    assert torch.equal(got, losses.smooth_l1_masked(cu(est), cu(gt), cu(mask)))
    assert torch.isnan(losses.smooth_l1_masked(cu(est), cu(gt), torch.zeros(shape, device="cuda")))   # 0 / 0, as torch's empty mean
    one = np.zeros(shape, np.float32)
    one[1, 36, 60] = 1.0      # the last element alone
    assert abs(losses.smooth_l1_masked(cu(est), cu(gt), cu(one)).item() - per[1, 36, 60]) <= 1e-6 * max(per[1, 36, 60], 1.0)


# ---- the plugin -------------------------------------------------------------------------------------------------------------------
def random_vgg(path):
    g = torch.Generator().manual_seed(13)
    w = {}
    for i, (cin, cout) in enumerate(losses.VGG_CHANNELS):
        w[f"conv.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        w[f"conv.{i}.bias"] = torch.randn(cout, generator=g) * 0.1
    torch.save(w, path)


@pytest.mark.parametrize("mode", ["hip", "torch", "hip_vgg"])
def test_network_wrapper_trains_through_the_mirrors(mode, tmp_path):
    """The 32 x 64 frame and the seed of tests/test_backward_referee.py's Network test (its docstring says why that seed).  Parameter
    gradients are not compared across the modes: the PyTorch decoder's backward is not bit-reproducible."""
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    from gdb_nerf_amd.train.trainers import make_wrapper
    fr = synthetic.make_frame(32, 64, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    target = torch.from_numpy(np.random.default_rng(14).random((1, 32, 64, 3)).astype(np.float32)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"]), "rgb": target}, "near_far": t(fr["near_far"])}
    opts = ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "train.hip_loss", str(mode != "torch")]
    gamma = 0.0
    if mode == "hip_vgg":
        random_vgg(tmp_path / "vgg.pt")
        opts += ["train.vgg_weights", str(tmp_path / "vgg.pt")]
        gamma = 0.05
    else:
        opts += ["train.photometric_weights", "[1.0, 0.1, 0.0]"]
    cfg = make_cfg("configs/dtu_eval.yaml", opts)
    torch.manual_seed(109)
    net = make_network(cfg).eval().cuda()
    wrapper = make_wrapper(cfg, net).cuda()
    wrapper.training = True       # the wrapper's own train-mode branch; the network keeps its evaluation-mode statistics
    output, loss, stats, image_stats = wrapper(batch)
    assert set(stats) == {"mse_loss", "psnr", "ssim", "perceptual_loss", "loss", "depth_loss"} and image_stats == {}
    assert stats["depth_loss"] == 0.0     # this DepthNet returns no stage images: an empty sum
    gt = target.permute(0, 3, 1, 2)
    r64, r32 = restate(gt, output["rgb"], torch.float64), restate(gt, output["rgb"], torch.float32)
    perceptual = float(stats["perceptual_loss"].detach())
    assert (perceptual > 0) == (mode == "hip_vgg")
    colour = loss
    if gamma:   # loss = the MSE + SSIM part + gamma * perceptual, to the bit: the library call is deterministic
        colour = losses.photometric_terms(gt, output["rgb"].detach(), cfg.train.photometric_weights[0], cfg.train.photometric_weights[1])[0]
        assert torch.equal(loss.detach(), colour + gamma * stats["perceptual_loss"].detach())
    check_rule(f"wrapper_{mode}", {"mse": npy(stats["mse_loss"]), "ssim": npy(stats["ssim"]), "photo": npy(colour)}, r64, r32)
    assert abs(float(stats["psnr"]) + 10.0 * np.log10(float(stats["mse_loss"]) + 1e-6)) <= 1e-4
    loss.backward()
    for k, p in net.named_parameters():
        if k.startswith(("nerf.", "upsampler.")):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k

"""The depth net's train-time stage render without a GPU: the plain-torch restatement (`_AuxStageNerf.forward`, `composite_stage`,
`build_rays`, `get_img_feat_vectorized`, `DepthNet._render_rays`) in float64 against the record of the reference's own modules
(tests/golden/make_golden_stage.py), the `mvs.stage_render` switch on a tiny frame, and the loss plugin's stage term over the real
network."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gdb_nerf_amd import losses, synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks.gdb_nerf import depth_net as dn

NERF_CASES = ("c32_v3_s8", "c8_v2_s3")
REL = 1e-10


@pytest.fixture(scope="module")
def fx():
    return load_golden("F10_stage_render")


def close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.abs(got - ref).max() <= REL * max(np.abs(ref).max(), 1e-300), (what, np.abs(got - ref).max(), np.abs(ref).max())


def aux_nerf(fx, name, dtype):
    C_f, V, S, n_rays, agg = (int(v) for v in fx[f"nerf.{name}.meta"])
    nerf = dn._AuxStageNerf(64, 8, C_f, bool(agg))
    prefix = f"nerf.{name}.w."
    nerf.load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)}, strict=True)
    return nerf.to(dtype), S, n_rays


@pytest.mark.parametrize("name", NERF_CASES)
def test_aux_nerf_and_composite_equal_the_reference_record(fx, name):
    nerf, S, n_rays = aux_nerf(fx, name, torch.float64)
    vox = torch.from_numpy(fx[f"nerf.{name}.vox"]).double()[None].requires_grad_()
    img = torch.from_numpy(fx[f"nerf.{name}.img"]).double()[None].requires_grad_()
    sigma, rgb = nerf(vox, img)
    assert sigma.shape == (1, n_rays * S) and rgb.shape == (1, n_rays * S, 3)
    rgb_map = dn.composite_stage(sigma.unflatten(1, (n_rays, S)), rgb.unflatten(1, (n_rays, S)))
    (rgb_map * torch.from_numpy(fx[f"nerf.{name}.U"]).double()).sum().backward()
    close(sigma[0].detach(), fx[f"nerf.{name}.sigma64"], "sigma")
    close(rgb[0].detach(), fx[f"nerf.{name}.rgb64"], "rgb")
    close(rgb_map[0].detach(), fx[f"nerf.{name}.rgb_map64"], "rgb_map")
    close(vox.grad[0], fx[f"nerf.{name}.g_vox"], "g_vox")
    close(img.grad[0], fx[f"nerf.{name}.g_img"], "g_img")
    params = dict(nerf.named_parameters())
    assert len(params) == (16 if hasattr(nerf, "view_fc") else 14)
    for k, p in params.items():
        assert np.abs(fx[f"nerf.{name}.g.{k}"]).max() > 0, k      # the fixture's weight law keeps every path alive
        close(p.grad, fx[f"nerf.{name}.g.{k}"], k)


@pytest.mark.parametrize("name", NERF_CASES)
def test_aux_nerf_in_fp32_is_within_8_ulp_of_the_reference_in_fp32(fx, name):
    nerf, S, n_rays = aux_nerf(fx, name, torch.float32)
    with torch.no_grad():
        sigma, rgb = nerf(torch.from_numpy(fx[f"nerf.{name}.vox"])[None], torch.from_numpy(fx[f"nerf.{name}.img"])[None])
        rgb_map = dn.composite_stage(sigma.unflatten(1, (n_rays, S)), rgb.unflatten(1, (n_rays, S)))
    for got, key in ((sigma, "sigma32"), (rgb, "rgb32"), (rgb_map, "rgb_map32")):
        ref = fx[f"nerf.{name}.{key}"]
        assert np.abs(got[0].numpy().astype(np.float64) - ref).max() <= 8 * float(np.spacing(np.float32(np.abs(ref).max()))), key


def stage_net(opts=()):
    torch.manual_seed(0)
    return dn.DepthNet(make_cfg("configs/dtu_pretrain.yaml", list(opts)))


def load_fixture_nerf(nerf, dtype=torch.float32):
    """The fixture's weights: under nn.Linear's default initialisation the color.2 score is almost never positive, the view softmax
    is uniform and the gradient of color.* exactly zero (tests/golden/make_golden_stage.py)."""
    prefix = "nerf.c32_v3_s8.w."
    nerf.load_state_dict({k[len(prefix):]: torch.from_numpy(v).to(dtype) for k, v in load_golden("F10_stage_render").items() if k.startswith(prefix)})


@pytest.mark.parametrize("name", ["depth", "disparity"])
def test_render_rays_equals_the_reference_record(fx, name):
    inv = name == "disparity"
    net = stage_net(["mvs.inv_depth", str([inv, False])]).double()
    prefix = "nerf.c32_v3_s8.w."
    net.nerfs[0].load_state_dict({k[len(prefix):]: torch.from_numpy(v).double() for k, v in fx.items() if k.startswith(prefix)})
    t = lambda k: torch.from_numpy(fx[f"render.{name}.{k}" if f"render.{name}.{k}" in fx else f"render.depth.{k}"])
    volume, feats, ray_range = (t(k).double().requires_grad_() for k in ("volume", "feats", "ray_range"))
    # the reference's pixel grid is fp32 whatever its inputs are: the record was made with fp32 cameras for build_rays
    rays = dn.build_rays(t("tar_ext"), t("tar_int"), ray_range, t("vol_range").double())
    assert rays.dtype == torch.float64 and rays.shape == (1, 20, 12)
    close(rays.detach(), fx[f"render.{name}.rays"], "rays")
    rgb_map = net._render_rays(rays, volume, torch.cat((feats, t("rgb").double()), 2), t("src_exts").double(), t("src_ints").double(), t("tar_ext").double(), 0)
    (rgb_map * t("U").double()).sum().backward()
    close(rgb_map.detach(), fx[f"render.{name}.rgb_map64"], "rgb_map")
    close(volume.grad, fx[f"render.{name}.g_volume"], "g_volume")
    close(feats.grad, fx[f"render.{name}.g_feats"], "g_feats")
    close(ray_range.grad, fx[f"render.{name}.g_ray_range"], "g_ray_range")
    assert np.abs(fx[f"render.{name}.g_ray_range"]).max() > 0
    for k, p in net.nerfs[0].named_parameters():
        if f"render.{name}.g.{k}" in fx:
            close(p.grad, fx[f"render.{name}.g.{k}"], k)


def test_render_rays_ignores_chunk_size(fx):
    """The reference's chunk loop steps over rays and slices samples, so a chunk_size below the ray count leaves samples zero; here
    every sample is evaluated whatever nerf.chunk_size says."""
    t = lambda k: torch.from_numpy(fx[f"render.depth.{k}"])
    outs = []
    for chunk in (1000000, 3):
        net = stage_net(["mvs.inv_depth", "[False, False]", "nerf.chunk_size", str(chunk)])
        prefix = "nerf.c32_v3_s8.w."
        net.nerfs[0].load_state_dict({k[len(prefix):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix)})
        with torch.no_grad():
            rays = dn.build_rays(t("tar_ext"), t("tar_int"), t("ray_range"), t("vol_range"))
            outs.append(net._render_rays(rays, t("volume"), torch.cat((t("feats"), t("rgb")), 2), t("src_exts"), t("src_ints"), t("tar_ext"), 0))
    assert torch.equal(*outs)
    ref = fx["render.depth.rgb_map32"]
    assert np.abs(outs[0].numpy().astype(np.float64) - ref).max() <= 8 * float(np.spacing(np.float32(np.abs(ref).max())))


def test_a_point_behind_a_source_camera_reads_the_border_texel():
    img = torch.arange(2 * 4 * 3 * 5, dtype=torch.float64).view(1, 2, 4, 3, 5)
    eye = torch.eye(4, dtype=torch.float64)
    exts, ints = torch.stack((eye, eye))[None], torch.eye(3, dtype=torch.float64).expand(1, 2, 3, 3)
    xyz = torch.tensor([[[[0.3, 0.2, -1.0], [0.5, 0.5, 1.0]]]], dtype=torch.float64)   # the first: z < 1e-8 -> grid -99 -> texel (0, 0)
    tar = eye.clone()
    tar[:3, 3] = torch.tensor([0.0, 0.0, 5.0])
    out = dn.get_img_feat_vectorized(img, xyz, exts, ints, tar[None])
    assert out.shape == (1, 2, 2, 4 + 4)
    assert torch.equal(out[0, 0, :, :4], img[0, :, :, 0, 0])
    assert torch.allclose(out[0, :, :, 4:7].norm(dim=-1), torch.ones(2, 2, dtype=torch.float64))


# ---- DepthNet on a tiny frame -------------------------------------------------------------------------------------------------------
def tiny_frame(seed=3, B=1):
    """3 views of 64 x 96: stage 0 is 8 x 12 rays of 8 samples, stage 1 is 32 x 48 (the 3-D U-Nets halve a stage's width twice and three
    times: 64 x 80 would make stage 0 ten wide, which they refuse)."""
    fr = synthetic.make_frame(64, 96, V=3, B=B, seed=seed)
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.from_numpy(v) for k, v in fr.items()}
    feats = [(torch.randn(B, 3, 32, 16, 24, generator=g) * 0.5).requires_grad_(), (torch.randn(B, 3, 16, 32, 48, generator=g) * 0.5).requires_grad_(), None]
    return t, feats


def run_depth_net(net, t, feats):
    return net(t["src_images"], feats, t["src_exts"], t["src_ints"], t["tar_ext"], t["tar_int"], t["near_far"])


def test_depth_net_returns_the_stage_images_only_under_the_switch_and_in_training_mode():
    t, feats = tiny_frame(B=2)
    on, off = stage_net(), stage_net(["mvs.stage_render", "False"])
    assert on.stage_render is True and off.stage_render is False
    assert dn.DepthNet(make_cfg("configs/dtu_eval.yaml")).stage_render is False          # absent: off
    off.load_state_dict(on.state_dict())
    on.train(), off.train()
    out_on, out_off = run_depth_net(on, t, feats), run_depth_net(off, t, feats)
    assert len(out_on[4]) == on.num_stages - 1 == 1 and out_on[4][0].shape == (2, 3, 8, 12) and out_on[4][0].requires_grad
    assert torch.isfinite(out_on[4][0]).all() and out_on[4][0].std() > 0
    assert out_off[4] == []
    for a, b in zip(out_on[:4], out_off[:4]):
        assert len(a) == len(b) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    on.eval(), off.eval()
    with torch.no_grad():
        ev_on, ev_off = run_depth_net(on, t, feats), run_depth_net(off, t, feats)
    assert ev_on[4] == [] and ev_off[4] == []
    for a, b in zip(ev_on[:4], ev_off[:4]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_stage_image_reaches_the_nerf_the_cost_regularisation_and_the_feature_maps():
    t, feats = tiny_frame()
    net = stage_net().train()
    load_fixture_nerf(net.nerfs[0])
    image = run_depth_net(net, t, feats)[4][0]
    image.sum().backward()
    for prefix in ("nerfs.0.", "cost_regs.0."):
        grads = {k: p.grad for k, p in net.named_parameters() if k.startswith(prefix)}
        assert grads and all(g is not None and torch.isfinite(g).all() for g in grads.values()), prefix
        assert sum(float(g.abs().sum()) for g in grads.values()) > 0, prefix
    assert all(float(p.grad.abs().max()) > 0 for k, p in net.named_parameters() if k.startswith("nerfs.0.") and k.endswith("weight"))
    assert torch.isfinite(feats[0].grad).all() and feats[0].grad.abs().max() > 0       # the stage's own level
    assert all(p.grad is None for k, p in net.named_parameters() if k.startswith("cost_regs.1."))   # the image is formed before stage 1


def test_stage_render_needs_a_sample_count_per_rendered_stage():
    with pytest.raises(ValueError, match="num_samples"):
        stage_net(["mvs.num_samples", "[]"])
    stage_net(["mvs.num_samples", "[]", "mvs.stage_render", "False"])   # not read without the switch


# ---- the loss plugin over the real network ------------------------------------------------------------------------------------------
class NoHotPath:
    """Stands in for the bundle sampler: `sample` / `encode` are HIP library calls and need a GPU.  Everything else of `Network.forward`
    - the FPN, the depth net with its stage render, the decoder, the merge - is the real module on the CPU."""

    def build_rays(self, *a):
        pass

    def sample(self, *a):
        return (None,) * 7

    def encode(self, *a):
        return None, None


def test_network_wrapper_adds_the_stage_term_over_the_real_network():
    from gdb_nerf_amd.networks.make_network import make_network
    from gdb_nerf_amd.train.trainers import make_wrapper
    cfg = make_cfg("configs/dtu_pretrain.yaml", ["train.photometric_weights", "[1, 0.1, 0]", "nerf.hot_path", "mirrors", "nerf.hip_decoder", "False"])
    torch.manual_seed(0)
    net = make_network(cfg)
    assert type(net).__name__ == "Network" and net.depth_net.stage_render
    load_fixture_nerf(net.depth_net.nerfs[0])
    B, H, W = 1, 32, 48
    g = torch.Generator().manual_seed(8)
    net.sampler = NoHotPath()
    Q = 3 * 4 + net._feat_dim + 3 + net.voxel_dim
    bundle = torch.rand(B * H * W, Q, generator=g)
    net.render_bundles = lambda *a: (bundle, torch.rand(B * H * W, generator=g), torch.rand(B * H * W, generator=g))
    fr = {k: torch.from_numpy(v) for k, v in synthetic.make_frame(64, 96, V=3, seed=4).items()}
    batch = {"src_views": {"rgb": fr["src_images"], "extrinsics": fr["src_exts"], "intrinsics": fr["src_ints"]},
             "tar_views": {"rgb": torch.rand(B, 64, 96, 3, generator=g), "extrinsics": fr["tar_ext"], "intrinsics": fr["tar_int"]},
             "near_far": fr["near_far"], "tar_gt_ms": {"rgb": [torch.rand(B, 8, 12, 3, generator=g)]}}
    wrapper = make_wrapper(cfg, net).train()
    kept = {}
    hook = net.depth_net.register_forward_hook(lambda m, i, o: kept.__setitem__("blend", o[4]))
    output, loss, stats, _ = wrapper(batch)
    hook.remove()
    assert len(kept["blend"]) == 1 and kept["blend"][0].shape == (B, 3, 8, 12)
    want = cfg.mvs.loss_weight[0] * losses.photometric_terms_torch(batch["tar_gt_ms"]["rgb"][0].permute(0, 3, 1, 2), kept["blend"][0], 1.0, 0.1)[0]
    assert stats["depth_loss"].item() == want.item() and want.item() > 0
    colour = losses.photometric_terms_torch(batch["tar_views"]["rgb"].permute(0, 3, 1, 2), output["rgb"], 1.0, 0.1)[0]
    assert abs(loss.item() - (colour + want).item()) <= 1e-6
    loss.backward()
    grad = net.depth_net.nerfs[0].color[0].weight.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0
    assert net.feature_net.parameters().__next__().grad is not None
    wrapper.eval()
    with torch.no_grad():
        assert "depth_loss" not in wrapper(batch)[2]

"""Cascade MVS depth prior: per stage a variance cost volume by homography warping, a 3-D U-Net,
soft-argmax depth and a confidence interval that becomes the next stage's search range and,
after the last stage, the per-bundle depth prior of the hot path (reference
networks/gdb_nerf/depth_net.py:118-198, 399-514).  PyTorch-ROCm.

While training and under `mvs.stage_render` every stage but the last also renders a small colour image from its own feature volume
and feature maps with an auxiliary MVSNeRF-style NeRF over uniform samples inside that stage's confidence interval (reference
:49-116, 182-192, 201-298): the `rgb_predictions` that the loss plugin supervises with `mvs.loss_weight`."""
from types import SimpleNamespace
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .cost_reg_net import CostRegNet, CostRegNet_small


class _AuxStageNerf(nn.Module):
    """The train-only per-stage NeRF of the reference (depth_net.py:201-298).  The reference builds it unconditionally (its ctor runs
    in training mode, depth_net.py:40-47), so its tensors are in every checkpoint; they are kept here under the same keys so that a
    reference `latest.pth` loads with strict=True.  Evaluated only by the stage render (`mvs.stage_render`, training mode)."""

    def __init__(self, hid_dim: int, voxel_dim: int, feat_dim: int, viewdir_agg: bool) -> None:
        super().__init__()
        lin = lambda i, o: nn.Sequential(nn.Linear(i, o), nn.ReLU(inplace=True))
        if viewdir_agg:
            self.view_fc = lin(4, feat_dim + 3)
        self.global_fc = lin(3 * (feat_dim + 3), 32)
        self.agg_w_fc = lin(32, 1)
        self.fc = lin(32, 16)
        self.lr0 = lin(voxel_dim + 16, hid_dim)
        self.sigma = nn.Sequential(nn.Linear(hid_dim, 1), nn.Softplus())
        self.color = nn.Sequential(nn.Linear(hid_dim + voxel_dim + 16 + feat_dim + 3 + 4, hid_dim), nn.ReLU(inplace=True),
                                   nn.Linear(hid_dim, 1), nn.ReLU(inplace=True))

    def forward(self, vox_feat: torch.Tensor, img_feat_rgb_dir: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """vox_feat (B,N,C_v), img_feat_rgb_dir (B,N,V,C_f+3+4) -> sigma (B,N), rgb (B,N,3): the reference's `NeRF.forward` with its
        `agg_viewdir` (:248-298).  Unbiased variance over the views, both view softmaxes over relu(score), colour = the source
        colours `x[..., -7:-4]` blended by the second softmax."""
        V = img_feat_rgb_dir.shape[-2]
        x = img_feat_rgb_dir[..., :-4]
        if hasattr(self, "view_fc"):
            x = x + self.view_fc(img_feat_rgb_dir[..., -4:])
        var, mean = torch.var_mean(x, dim=-2, keepdim=True)
        g = self.global_fc(torch.cat((x, var.expand_as(x), mean.expand_as(x)), dim=-1))
        img_feat = self.fc((g * F.softmax(self.agg_w_fc(g), dim=-2)).sum(dim=-2))
        vox_img = torch.cat((vox_feat, img_feat), dim=-1)
        h = self.lr0(vox_img)
        sigma = self.sigma(h)
        y = torch.cat((torch.stack(V * [torch.cat((h, vox_img), dim=-1)], dim=-2), img_feat_rgb_dir), dim=-1)
        weight = F.softmax(self.color(y), dim=-2)
        return sigma.squeeze(-1), (img_feat_rgb_dir[..., -7:-4] * weight).sum(dim=-2)


def _use_hip(t: torch.Tensor, enabled: bool) -> bool:
    """CUDA tensors take the HIP kernels of the "next" rows N2 / N4 (gdb-nerf_amd/costvol.py; loud failure if the
    library is missing); CPU tensors take the PyTorch formulation below (the CNNs around them are PyTorch too)."""
    return enabled and t.is_cuda and t.dtype == torch.float32


def get_depth_values(near_far: torch.Tensor, num_depth: int, inv_depth: bool) -> torch.Tensor:
    """(B,2,H,W) near/far -> (B,num_depth,H,W) hypotheses, uniform in depth or in disparity (:399-421)."""
    lo, hi = near_far[:, :1], near_far[:, -1:]
    if inv_depth:
        lo, hi = 1.0 / lo, 1.0 / hi
    steps = torch.linspace(0.0, 1.0, num_depth, device=lo.device).view(1, num_depth, 1, 1)
    return lo + (hi - lo) * steps


def build_feature_volume(src_feat, src_exts, src_ints, tar_exts, tar_ints, depth_values, inv_depth) -> torch.Tensor:
    """Variance over source views of the features warped onto the target frustum planes (:424-476).
    src_feat (B,V,C,Hs,Ws); depth_values (B,D,Ht,Wt) -> (B,C,D,Ht,Wt)."""
    B, V, _, Hs, Ws = src_feat.shape
    D, Ht, Wt = depth_values.shape[1:]
    depth = 1.0 / depth_values if inv_depth else depth_values
    # pixel(target) -> pixel(source) homographies through the target projection's inverse
    P_src = src_ints @ src_exts[..., :3, :]
    P_tar = F.pad(tar_ints @ tar_exts[..., :3, :], (0, 0, 0, 1), value=0.0)
    P_tar[..., 3, 3] = 1.0
    Hm = (P_src @ torch.inverse(P_tar).unsqueeze(1)).view(B * V, 3, 4)
    xs, ys = torch.meshgrid(torch.arange(Wt, dtype=src_feat.dtype, device=src_feat.device) + 0.5,
                            torch.arange(Ht, dtype=src_feat.dtype, device=src_feat.device) + 0.5, indexing="xy")
    pix = torch.stack((xs, ys, torch.ones_like(xs)), 0).reshape(1, 3, Ht * Wt)
    d = depth.reshape(B, 1, D, -1).expand(-1, V, -1, -1).reshape(B * V, 1, D, -1)
    p = (Hm[..., :3] @ pix).unsqueeze(2) * d + Hm[..., 3:, None]  # (B*V,3,D,Ht*Wt)
    p = p.permute(0, 2, 3, 1).contiguous()
    g = p[..., :2] / p[..., 2:3].clamp_min(1e-6)
    g[..., 0], g[..., 1] = 2 * g[..., 0] / Ws - 1, 2 * g[..., 1] / Hs - 1
    warped = F.grid_sample(src_feat.flatten(0, 1), g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return torch.var(warped.view(B, V, -1, D, Ht, Wt), dim=1, unbiased=False)


def build_rays(tar_exts, tar_ints, ray_range, vol_range) -> torch.Tensor:
    """One ray per pixel centre of the stage (:301-341): (B,H*W,12) = origin 3, unnormalised direction 3, pixel in [-1,1] 2,
    the ray's interval 2 (`ray_range` (B,2,H,W)) and the volume's first / last hypothesis 2 (`vol_range` (B,2,H,W)).  The pixel grid
    takes the cameras' dtype (the reference's is fp32 always); the concatenation promotes."""
    B, _, H, W = ray_range.shape
    dt, dev = tar_exts.dtype, ray_range.device
    x, y = torch.meshgrid(torch.arange(W, dtype=dt, device=dev) + 0.5, torch.arange(H, dtype=dt, device=dev) + 0.5, indexing="xy")
    x, y = x.flatten(), y.flatten()
    xyz = torch.stack((x, y, torch.ones_like(x)), dim=1)
    c2w = torch.inverse(tar_exts)
    rays_o = c2w[:, None, :3, 3].expand(-1, H * W, -1)
    rays_d = xyz @ (c2w[:, :3, :3] @ torch.inverse(tar_ints)).transpose(-2, -1)
    uv = torch.stack((2 * x / W - 1, 2 * y / H - 1), dim=-1).unsqueeze(0).expand(B, -1, -1)
    return torch.cat((rays_o, rays_d, uv, ray_range.permute(0, 2, 3, 1).flatten(1, 2), vol_range.permute(0, 2, 3, 1).flatten(1, 2)), dim=-1)


def get_img_feat_vectorized(img_feat_rgb, world_xyz, src_exts, src_ints, tar_exts) -> torch.Tensor:
    """Gathers (B,V,C_f+3,H,W) at the projections of world_xyz (B,R,S,3) and appends the 4-vector direction code (:344-396):
    (B,R*S,V,C_f+3+4).  A point at z < 1e-8 of a view reads grid -99 (the border texel); border padding, align_corners=False."""
    B, V, _, H, W = img_feat_rgb.shape
    n = world_xyz.shape[1] * world_xyz.shape[2]
    xyz = world_xyz.reshape(B, -1, 3)
    xyz1 = torch.cat((xyz, torch.ones_like(xyz[..., :1])), dim=-1)
    p = torch.matmul(torch.matmul(xyz1[:, None], src_exts.transpose(-2, -1))[..., :3], src_ints.transpose(-2, -1))   # (B,V,n,3)
    invalid = p[..., 2] < 1e-8
    q = p[..., :2] / p[..., 2:3]
    grid = torch.stack((2 * q[..., 0] / W - 1, 2 * q[..., 1] / H - 1), dim=-1)
    grid = torch.where(invalid[..., None], torch.full_like(grid, -99.0), grid)
    feats = F.grid_sample(img_feat_rgb.flatten(0, 1), grid.view(B * V, -1, 1, 2), mode="bilinear", padding_mode="border", align_corners=False)
    feats = feats.view(B, V, -1, n).permute(0, 3, 1, 2)
    tar_cam = torch.inverse(tar_exts)[:, None, :3, 3]
    src_cam = torch.inverse(src_exts)[..., :3, 3]
    tar_diff = F.normalize(xyz - tar_cam, p=2.0, dim=-1)
    src_diff = F.normalize(xyz[..., None, :] - src_cam[:, None], p=2.0, dim=-1)
    direction = F.normalize(tar_diff[..., None, :] - src_diff, p=2.0, dim=-1)
    dot = torch.sum(tar_diff[..., None, :] * src_diff, dim=-1, keepdim=True)
    return torch.cat((feats, direction, dot), dim=-1)


def composite_stage(sigma: torch.Tensor, rgb: torch.Tensor) -> torch.Tensor:
    """The reference's un-normalised composite (:109-114): sigma (..,S), rgb (..,S,3) -> (..,3) with alpha = 1 - exp(-sigma),
    T_i = prod_{j<i} (1 - alpha_j + 1e-10).  The running product is written out (S <= 16 multiplications) instead of `torch.cumprod`:
    the values are the same product in the same order, but autograd then applies the product rule, where cumprod's backward divides a
    reversed cumulative sum by the factors - in fp32 on the GPU that left the gradients of sigma.0 outside the referee's bound
    (DESIGN.md 4.18)."""
    alpha = 1.0 - torch.exp(-sigma)
    a = 1.0 - alpha + 1e-10
    T = [torch.ones_like(alpha[..., 0])]
    for i in range(sigma.shape[-1] - 1):
        T.append(T[-1] * a[..., i])
    return torch.sum((alpha * torch.stack(T, dim=-1))[..., None] * rgb, dim=-2)


def depth_regression(depth_values, depth_prob, ci_scale: float, inv_depth: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """Soft-argmax depth (B,1,H,W) and the confidence interval (B,2,H,W) = mean ∓ ci_scale·std clipped
    to the hypothesis range (:479-514)."""
    mean = (depth_prob * depth_values).sum(1, keepdim=True)
    std = (depth_prob * (depth_values - mean).square()).sum(1, keepdim=True).clamp_min(1e-12).sqrt()
    half = ci_scale * std
    first, last = depth_values[:, :1], depth_values[:, -1:]
    if inv_depth:  # hypotheses run from large to small disparity
        ci = 1.0 / torch.cat((torch.min(mean + half, first), torch.max(mean - half, last)), 1)
        return 1.0 / mean, ci
    return mean, torch.cat((torch.max(mean - half, first), torch.min(mean + half, last)), 1)


class HipDepthRegression(torch.autograd.Function):
    """`gdb_depth_regression` (costvol.depth_regression) as the forward - the values every other path of the network sees - with the
    derivative of `depth_regression` above as its backward: the soft-argmax, its standard deviation and the clipped interval are
    recomputed from the saved inputs under autograd (a reduction over the hypotheses: not a hot path, no HIP backward is built for
    it).  Taken only under `nerf.position_grad`, where the depth prior has to carry a graph to the 3-D U-Nets."""

    @staticmethod
    def forward(ctx, depth_values, depth_prob, ci_scale, inv_depth):
        from ... import costvol
        ctx.save_for_backward(depth_values, depth_prob)
        ctx.ci_scale, ctx.inv_depth = ci_scale, inv_depth
        return costvol.depth_regression(depth_values, depth_prob, ci_scale, inv_depth)

    @staticmethod
    def backward(ctx, g_depth, g_ci):
        depth_values, depth_prob = ctx.saved_tensors
        with torch.enable_grad():
            hyp, prob = depth_values.detach().requires_grad_(), depth_prob.detach().requires_grad_()
            depth, ci = depth_regression(hyp, prob, ctx.ci_scale, ctx.inv_depth)
            outs, ups = zip(*((o, g) for o, g in ((depth, g_depth), (ci, g_ci)) if g is not None))
            g_hyp, g_prob = torch.autograd.grad(outs, (hyp, prob), ups, allow_unused=True)
        return (g_hyp if ctx.needs_input_grad[0] else None), (g_prob if ctx.needs_input_grad[1] else None), None, None


class DepthNet(nn.Module):
    def __init__(self, config: SimpleNamespace) -> None:
        super().__init__()
        mvs, fpn = config.mvs, config.fpn
        self.vol_levels = list(mvs.vol_levels)
        self.vol_scales = list(mvs.vol_scales)
        self.num_stages = len(self.vol_levels)
        self.feat_scales = [fpn.feat_scales[l] for l in self.vol_levels]
        self.feat_dims = [fpn.feat_dims[l] for l in self.vol_levels]
        self.ci_scales = list(mvs.ci_scales)
        self.num_depth = list(mvs.num_depth)
        self.inv_depth = list(mvs.inv_depth)
        self.hip_cost_volume = bool(getattr(mvs, "hip_cost_volume", True))
        # the 3-D U-Nets on the HIP library (costvol.CostReg): eval mode and fp32 CUDA input only; off by default
        self.hip_cost_reg = bool(getattr(mvs, "hip_cost_reg", False))
        self._hip_regs = {}   # stage -> costvol.CostReg (not a module: no state-dict keys)
        # mvs.hip_cost_reg_train (default false): in training mode fp32 CUDA tensors take the U-Nets' forward with batch statistics
        # and their backward from the HIP library (costvol.CostRegTrain); eval mode, CPU tensors and other dtypes are untouched
        self.hip_cost_reg_train = bool(getattr(mvs, "hip_cost_reg_train", False))
        self._hip_regs_train = {}   # stage -> costvol.CostRegTrain
        # mvs.cost_volume_grad (default false): on fp32 CUDA tensors, while grad mode is on and the feature maps or the
        # hypotheses require grad, the plane sweep runs inside costvol.FeatureVolumeFunction - the same forward call, the same bits -
        # and its HIP backward carries the losses to feature_net and, under nerf.position_grad, to the previous stage's U-Net, as the
        # PyTorch formulation does on the CPU.  Off, the HIP cost volume carries no graph.  mvs.hip_cascade stays eval-only.
        self.cost_volume_grad = bool(getattr(mvs, "cost_volume_grad", False))
        # a whole stage as one library call (costvol.MvsStage): eval mode and fp32 CUDA inputs only; off by default
        self.hip_cascade = bool(getattr(mvs, "hip_cascade", False))
        # nerf.position_grad: the depth prior must carry a graph to the 3-D U-Nets.  Under that switch - and only while
        # grad mode is on and the probabilities require grad - gdb_depth_regression runs inside HipDepthRegression below: the same
        # forward call, the same bits, with the derivative of the PyTorch formulation as its backward
        self.position_grad = bool(getattr(config.nerf, "position_grad", False))
        # the reference indexes feat_dims by the pyramid level again (depth_net.py:32-37); kept for key/shape parity
        nets = [CostRegNet_small(self.feat_dims[self.vol_levels[0]], mvs.voxel_dim, fpn.base_channels)]
        nets += [CostRegNet(self.feat_dims[self.vol_levels[i]], mvs.voxel_dim, fpn.base_channels) for i in range(1, self.num_stages)]
        self.cost_regs = nn.ModuleList(nets)
        self.nerfs = nn.ModuleList(_AuxStageNerf(config.nerf.nerf_hidden_dims, mvs.voxel_dim, self.feat_dims[i], config.nerf.viewdir_agg)
                                   for i in range(self.num_stages - 1))
        # mvs.stage_render (default false): while training, every stage but the last renders its colour image with nerfs[i] (DESIGN.md
        # 4.18), the reference's rgb_predictions.  Off, or in eval mode, forward returns [] for it.
        self.stage_render = bool(getattr(mvs, "stage_render", False))
        self.num_samples = list(getattr(mvs, "num_samples", []))
        if self.stage_render and len(self.num_samples) < self.num_stages - 1:
            raise ValueError(f"mvs.stage_render renders {self.num_stages - 1} stage image(s) and needs as many entries in mvs.num_samples "
                             f"(got {self.num_samples})")
        # mvs.hip_stage_render (default false): fp32 CUDA tensors take the stage NeRF and its composite, forward and backward, from the
        # HIP library (stage_nerf.StageNerf; the two gathers stay F.grid_sample); CPU tensors and other dtypes take the torch code below
        self.hip_stage_render = bool(getattr(mvs, "hip_stage_render", False))
        if self.hip_stage_render and not self.stage_render:
            raise ValueError("mvs.hip_stage_render runs the stage render of mvs.stage_render on the HIP library: it needs mvs.stage_render")
        self._hip_nerfs = {}   # stage -> stage_nerf.StageNerf (not a module: no state-dict keys)

    def _render_rays(self, rays, feat_volume, img_feat_rgb, src_exts, src_ints, tar_exts, idx: int) -> torch.Tensor:
        """rays (B,R,12) of `build_rays` -> rgb_map (B,R,3), the reference's `_render_rays` (:49-116) with its arithmetic as it is: under
        inv_depth it inverts the vol_range columns too, although they already hold disparities.  Every sample is evaluated:
        `nerf.chunk_size` is not read (the reference's chunk loop steps over rays but slices samples)."""
        B, S = rays.shape[0], self.num_samples[idx]
        rays_o, rays_d, uv = rays[..., :3], rays[..., 3:6], rays[..., 6:8]
        ray_near, ray_far, vol_near, vol_far = rays[..., 8:9], rays[..., 9:10], rays[..., 10:11], rays[..., 11:12]
        if self.inv_depth[idx]:
            ray_near, ray_far = 1.0 / ray_far, 1.0 / ray_near
            vol_near, vol_far = 1.0 / vol_far, 1.0 / vol_near
        # (the reference's steps are fp32 whatever the dtype of the rays)
        t_vals = ray_near + (ray_far - ray_near) * torch.linspace(0.0, 1.0, S + 1, device=rays.device, dtype=torch.float32).to(rays.dtype)
        z_vals = 0.5 * (t_vals[..., :-1] + t_vals[..., 1:])
        d = 2 * (z_vals - vol_near) / (vol_far - vol_near) - 1.0
        uvd = torch.cat((uv[..., None, :].expand(-1, -1, S, -1), d[..., None]), dim=-1)
        if self.inv_depth[idx]:
            z_vals = 1.0 / z_vals
        world_xyz = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., None]
        vox_feat = F.grid_sample(feat_volume, uvd.view(B, -1, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=False)
        vox_feat = vox_feat.flatten(2, -1).permute(0, 2, 1)
        img_feat_rgb_dir = get_img_feat_vectorized(img_feat_rgb, world_xyz, src_exts, src_ints, tar_exts)
        if self.hip_stage_render and _use_hip(vox_feat, True) and img_feat_rgb_dir.dtype == torch.float32:
            from ... import stage_nerf
            holder = self._hip_nerfs.get(idx)
            if holder is None or holder.nerf is not self.nerfs[idx]:
                holder = self._hip_nerfs[idx] = stage_nerf.StageNerf(self.nerfs[idx])
            return holder.render(vox_feat.flatten(0, 1), img_feat_rgb_dir.flatten(0, 1), S).view(B, -1, 3)   # the batch folds into the rays
        sigma, rgb = self.nerfs[idx](vox_feat, img_feat_rgb_dir)
        return composite_stage(sigma.unflatten(1, (-1, S)), rgb.unflatten(1, (-1, S)))

    def _stage_image(self, idx, src_images, feats, volume, search, vol_range, src_exts, K_src, tar_exts, K_tar, Hs, Ws) -> torch.Tensor:
        """(B,3,Hs,Ws): the stage's colour image, as the reference forms it in `forward` (:182-192)."""
        B, V = src_images.shape[:2]
        rays = build_rays(tar_exts, K_tar, search, vol_range)
        rgb_lo = F.interpolate(src_images.flatten(0, 1), scale_factor=self.feat_scales[idx], mode="bilinear", align_corners=False)
        img_feat_rgb = torch.cat((feats, rgb_lo.unflatten(0, (B, V))), dim=2)
        ray_rgbs = self._render_rays(rays, volume, img_feat_rgb, src_exts, K_src, tar_exts, idx)
        return ray_rgbs.permute(0, 2, 1).reshape(B, -1, Hs, Ws)

    def use_hip_cost_reg(self, feats) -> bool:
        """The HIP U-Net needs the switch, eval mode (training needs batch statistics and autograd) and fp32 CUDA tensors."""
        return self.hip_cost_reg and not self.training and _use_hip(feats, True)

    def use_hip_cascade(self, *tensors) -> bool:
        """One MvsStage call per stage needs the switch, eval mode and fp32 CUDA tensors throughout."""
        return self.hip_cascade and not self.training and all(_use_hip(t, True) for t in tensors)

    def _hip_reg(self, s: int):
        from ... import costvol
        reg = self._hip_regs.get(s)
        if reg is None or reg.module is not self.cost_regs[s]:
            reg = self._hip_regs[s] = costvol.CostReg(self.cost_regs[s])
        return reg

    def use_hip_cost_reg_train(self, feats) -> bool:
        """The train-mode HIP U-Net (batch statistics + backward) needs its switch, training mode and fp32 CUDA tensors."""
        return self.hip_cost_reg_train and self.training and _use_hip(feats, True)

    def _hip_reg_train(self, s: int):
        from ... import costvol
        reg = self._hip_regs_train.get(s)
        if reg is None or reg.module is not self.cost_regs[s]:
            reg = self._hip_regs_train[s] = costvol.CostRegTrain(self.cost_regs[s], cost_grad=self.cost_volume_grad)
        return reg

    def _cost_reg(self, s: int, cost: torch.Tensor, feats: torch.Tensor):
        if self.use_hip_cost_reg_train(feats):   # a shape the library refuses raises: nothing falls back
            return self._hip_reg_train(s)(cost)
        if not self.use_hip_cost_reg(feats):
            return self.cost_regs[s](cost)
        return self._hip_reg(s)(cost)

    def _forward_hip_cascade(self, H0: int, W0: int, ms_feats, src_exts, src_ints, tar_exts, tar_ints, near_far):
        from ... import costvol
        depths, ranges, vol_ranges, volumes = [], [], [], []
        search, ratio = near_far, 1.0   # (B,2): broadcast by the library
        for s in range(self.num_stages):
            Hs, Ws = int(H0 * self.vol_scales[s]), int(W0 * self.vol_scales[s])
            volume, depth, search, vol_range = costvol.MvsStage(self._hip_reg(s))(
                ms_feats[self.vol_levels[s]], src_exts, src_ints, tar_exts, tar_ints, self.feat_scales[s], self.vol_scales[s], search, ratio,
                self.num_depth[s], Hs, Ws, self.inv_depth[s], self.ci_scales[s])
            depths.append(depth)
            ranges.append(search)
            vol_ranges.append(vol_range)
            volumes.append(volume)
            if s < self.num_stages - 1:   # the next stage upsamples this interval in its kernels
                ratio = self.vol_scales[s + 1] / self.vol_scales[s]
        return depths, ranges, vol_ranges, volumes, []

    def _load_from_state_dict(self, *args, **kwargs):
        for reg in (*self._hip_regs.values(), *self._hip_nerfs.values()):
            reg.invalidate()
        super()._load_from_state_dict(*args, **kwargs)

    def forward(self, src_images, ms_feats: List[torch.Tensor], src_exts, src_ints, tar_exts, tar_ints, near_far):
        """Returns (depths, depth_ranges, vol_ranges, feat_volumes, rgb_predictions) per stage like the
        reference; rgb_predictions (train-time supervision, (B,3,Hi,Wi) for every stage but the last) is filled in training mode under
        `mvs.stage_render` and is [] otherwise."""
        B, V, _, H0, W0 = src_images.shape
        if self.use_hip_cascade(src_images, *(ms_feats[l] for l in self.vol_levels), src_exts, src_ints, tar_exts, tar_ints, near_far):
            return self._forward_hip_cascade(H0, W0, ms_feats, src_exts, src_ints, tar_exts, tar_ints, near_far)
        depths, ranges, vol_ranges, volumes, rgb_predictions = [], [], [], [], []
        search = near_far[..., None, None]  # (B,2,1,1)
        for s in range(self.num_stages):
            feats = ms_feats[self.vol_levels[s]]
            K_src = src_ints.clone()
            K_src[..., :2, :] *= self.feat_scales[s]
            K_tar = tar_ints.clone()
            K_tar[:, :2, :] *= self.vol_scales[s]
            Hs, Ws = int(H0 * self.vol_scales[s]), int(W0 * self.vol_scales[s])
            hyp = get_depth_values(search, self.num_depth[s], self.inv_depth[s]).expand(-1, -1, Hs, Ws)
            if _use_hip(feats, self.hip_cost_volume):
                from ... import costvol
                hyp = hyp.contiguous()
                if self.cost_volume_grad and torch.is_grad_enabled() and (feats.requires_grad or hyp.requires_grad):
                    cost = costvol.FeatureVolumeFunction.apply(feats, src_exts, K_src, tar_exts, K_tar, hyp, self.inv_depth[s])
                else:
                    cost = costvol.build_feature_volume(feats, src_exts, K_src, tar_exts, K_tar, hyp, self.inv_depth[s])
                volume, prob = self._cost_reg(s, cost, feats)
                if self.position_grad and torch.is_grad_enabled() and prob.requires_grad:
                    depth, search = HipDepthRegression.apply(hyp, prob, self.ci_scales[s], self.inv_depth[s])
                else:
                    depth, search = costvol.depth_regression(hyp, prob, self.ci_scales[s], self.inv_depth[s])
            else:
                cost = build_feature_volume(feats, src_exts, K_src, tar_exts, K_tar, hyp, self.inv_depth[s])
                volume, prob = self._cost_reg(s, cost, feats)
                depth, search = depth_regression(hyp, prob, self.ci_scales[s], self.inv_depth[s])
            depths.append(depth.squeeze(1))
            ranges.append(search)
            vol_ranges.append(hyp[:, [0, -1]])
            volumes.append(volume)
            if s < self.num_stages - 1:
                if self.stage_render and self.training:
                    rgb_predictions.append(self._stage_image(s, src_images, feats, volume, search, vol_ranges[-1], src_exts, K_src, tar_exts, K_tar, Hs, Ws))
                search = F.interpolate(search, scale_factor=self.vol_scales[s + 1] / self.vol_scales[s], mode="bilinear", align_corners=False)
        return depths, ranges, vol_ranges, volumes, rgb_predictions

"""Depth-guided bundle sampler with the reference's method signatures
(networks/gdb_nerf/bundle_sampler.py), every method backed by one entry of the C ABI:
build_rays -> gdb_build_rays, sample -> gdb_sample, encode -> gdb_encode.  These materialise the
reference's intermediates; `Network.forward` uses the fused kernel instead.

`encode` is differentiable with respect to the values it gathers (`img_feat`, `feat_volume`) when the sampler's `encode_grad` is set:
the call then goes through `EncodeFunction`, whose backward is `gdb_encode_backward`.

With the sampler's `position_grad` set the sample POSITIONS are differentiable too: `sample` goes through
`SampleFunction` (backward `gdb_sample_backward`: rays_xyz, uvd[:, 2], z_vals, ball_radii -> depth_range, vol_range) and `encode`
returns gradients for rays_xyz, uvd and ball_radii (`gdb_encode_position_backward`; columns 0 and 1 of uvd get zeros: the pixel centre
is not differentiated).  The two switches are independent.  The cameras and the source images get no gradient."""
from typing import Dict, List, Tuple, Union

import torch

from ...engine import HotPathEngine


class EncodeFunction(torch.autograd.Function):
    """`gdb_encode` with `gdb_encode_backward` as its derivative with respect to img_feat and feat_volume, and
    `gdb_encode_position_backward` as its derivative with respect to rays_xyz, uvd and ball_radii; each half runs only when
    `ctx.needs_input_grad` asks for one of its outputs.  Nothing but the inputs is kept: the backward recomputes the coordinates.
    `frame` holds the other tensors of the frame `encode` prepares; when the engine has prepared anything since this forward (another
    frame's forward, for one), the backward prepares this frame again first."""

    @staticmethod
    def forward(ctx, engine, frame, img_feat, feat_volume, rays_xyz, uvd, ball_radii, samples_per_batch, total):
        engine.prepare(dict(frame, img_feat=img_feat, feat_volume=feat_volume))
        rfd, vox = engine.encode(rays_xyz, uvd, ball_radii, samples_per_batch, total)
        ctx.engine, ctx.frame, ctx.prepared = engine, frame, engine.prepare_count
        ctx.save_for_backward(img_feat, feat_volume, rays_xyz, uvd, ball_radii, samples_per_batch, total)
        return rfd, vox

    @staticmethod
    def backward(ctx, g_rfd, g_vox):
        img_feat, feat_volume, rays_xyz, uvd, ball_radii, samples_per_batch, total = ctx.saved_tensors
        eng = ctx.engine
        if eng.prepare_count != ctx.prepared:   # a stale camera block would scatter this frame's samples through another's cameras
            eng.prepare(dict(ctx.frame, img_feat=img_feat, feat_volume=feat_volume))
        n = rays_xyz.shape[0]
        g_rfd = torch.zeros((img_feat.shape[1], n, eng.P), device=img_feat.device) if g_rfd is None else g_rfd.contiguous().float()
        g_vox = torch.zeros((n, feat_volume.shape[1]), device=img_feat.device) if g_vox is None else g_vox.contiguous().float()
        need_img, need_vol = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        g_img = g_vol = g_rays = g_uvd = g_ball = None
        if need_img or need_vol:
            g_img, g_vol = eng.encode_backward(rays_xyz, uvd, ball_radii, samples_per_batch, total, g_rfd, g_vox, need_img, need_vol)
        need_pos = ctx.needs_input_grad[4:7]
        if any(need_pos):
            g_rays, g_uvd, g_ball = eng.encode_position_backward(rays_xyz, uvd, ball_radii, samples_per_batch, total, g_rfd, g_vox, *need_pos)
        return None, None, g_img, g_vol, g_rays, g_uvd, g_ball, None, None


class SampleFunction(torch.autograd.Function):
    """`gdb_sample` with `gdb_sample_backward` as its derivative with respect to depth_range and vol_range.  `frame` holds the target
    camera and near_far.  `encode` always prepares the engine in between (with a depth_range of ones), so the backward prepares this
    frame again whenever the engine's prepare_count has moved.  The counts are data: saved, not differentiated."""

    @staticmethod
    def forward(ctx, engine, frame, im_size, depth_range, vol_range):
        engine.prepare(dict(frame, depth_range=depth_range, vol_range=vol_range), im_size=im_size)
        s = engine.sample()
        n = int(s["total"].item())  # the reference's boolean-mask compaction has the same host-visible size
        ctx.engine, ctx.frame, ctx.im_size, ctx.prepared, ctx.n = engine, frame, im_size, engine.prepare_count, n
        ctx.save_for_backward(depth_range, vol_range, s["samples_per_bundle"], s["total"])
        fixed = (s["indices"][:n], s["samples_per_batch"], s["samples_per_bundle"], s["total"])
        ctx.mark_non_differentiable(*fixed)
        return (s["rays_xyz"][:n], s["uvd"][:n], s["z_vals"][:n], s["ball_radii"][:n]) + fixed

    @staticmethod
    def backward(ctx, g_rays, g_uvd, g_z, g_ball, *_):
        depth_range, vol_range, spb, total = ctx.saved_tensors
        eng = ctx.engine
        need_dr, need_vr = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        ups = [None if g is None else g.contiguous().float() for g in (g_rays, g_uvd, g_z, g_ball)]
        if ctx.n == 0 or all(g is None for g in ups):
            return None, None, None, torch.zeros_like(depth_range) if need_dr else None, torch.zeros_like(vol_range) if need_vr else None
        if eng.prepare_count != ctx.prepared:
            eng.prepare(dict(ctx.frame, depth_range=depth_range, vol_range=vol_range), im_size=ctx.im_size)
        g_dr, g_vr = eng.sample_backward(spb, total, *ups, need_depth=need_dr, need_vol=need_vr)
        return None, None, None, g_dr, g_vr


class BundleSampler:
    def __init__(self, global_num_depth: int, max_mipmap_level: int, encode_grad: bool = False, position_grad: bool = False) -> None:
        self.global_num_depth = global_num_depth
        self.max_mipmap_level = max_mipmap_level
        # nerf.encode_grad: `encode` carries a graph to img_feat / feat_volume (EncodeFunction); off: the calls of before
        self.encode_grad = bool(encode_grad)
        # nerf.position_grad: `sample` carries a graph to depth_range / vol_range (SampleFunction) and `encode` one to the sample
        # positions (EncodeFunction); off: the calls of before
        self.position_grad = bool(position_grad)
        self.H_orig = self.W_orig = None
        self.rays_o = self.rays_d = self.uv = self.tar_pixel_radius = self.z_axis = self.near = self.far = None
        self._tar = None
        self._engines: Dict[tuple, HotPathEngine] = {}
        self._last: HotPathEngine = None

    def _engine(self, device, b: int, S: int, adaptive: bool, inv_depth: bool) -> HotPathEngine:
        key = (str(device), b, S, bool(adaptive), bool(inv_depth))
        if key not in self._engines:
            self._engines[key] = HotPathEngine(bundle_size=b, max_num_samples=S, is_adaptive=adaptive, inv_depth=inv_depth,
                                               global_num_depth=self.global_num_depth, max_mipmap_level=self.max_mipmap_level, device=device)
        return self._engines[key]

    def build_rays(self, tar_exts: torch.Tensor, tar_ints: torch.Tensor, im_size: Union[Tuple[int, int], List[int]],
                   near: torch.Tensor, far: torch.Tensor) -> None:
        self.H_orig, self.W_orig = int(im_size[0]), int(im_size[1])
        self.near, self.far = near, far
        self._tar = {"tar_ext": tar_exts.contiguous().float(), "tar_int": tar_ints.contiguous().float(),
                     "near_far": torch.stack((near, far), -1).contiguous().float()}
        eng = self._engine(tar_exts.device, 1, 1, False, False)
        eng.prepare(self._tar, im_size=(self.H_orig, self.W_orig))
        r = eng.build_rays()
        self.rays_o, self.rays_d, self.uv = r["rays_o"], r["rays_d"], r["uv"]
        self.tar_pixel_radius, self.z_axis = r["tar_pixel_radius"], r["z_axis"]

    def sample(self, depth_range: torch.Tensor, vol_range: torch.Tensor, b_size: int, max_num_samples: int,
               inv_depth: bool = False, is_adaptive: bool = False):
        if self.rays_o is None:
            raise ValueError("Rays have not been built yet. Please call build_rays() first.")
        eng = self._engine(depth_range.device, b_size, max_num_samples, is_adaptive, inv_depth)
        if self.position_grad and torch.is_grad_enabled() and any(t.is_cuda and t.requires_grad for t in (depth_range, vol_range)):
            tar = {k: v.detach() for k, v in self._tar.items()}
            rays_xyz, uvd, z_vals, ball_radii, indices, per_batch, spb, total = SampleFunction.apply(
                eng, tar, (self.H_orig, self.W_orig), depth_range.contiguous().float(), vol_range.contiguous().float())
            self._last, self._total = eng, total
            if is_adaptive:
                spb, per_batch = spb.float(), per_batch.float()
            return (rays_xyz, uvd, z_vals, ball_radii, indices, per_batch, spb)
        frame = dict(self._tar, depth_range=depth_range.contiguous().float(), vol_range=vol_range.contiguous().float())
        eng.prepare(frame, im_size=(self.H_orig, self.W_orig))
        s = eng.sample()
        n = int(s["total"].item())  # the reference's boolean-mask compaction has the same host-visible size
        self._last, self._total = eng, s["total"]
        spb, per_batch = s["samples_per_bundle"], s["samples_per_batch"]
        if is_adaptive:  # dtype wart of the reference: float counts on the adaptive path (:179,:191,:242)
            spb, per_batch = spb.float(), per_batch.float()
        return (s["rays_xyz"][:n], s["uvd"][:n], s["z_vals"][:n], s["ball_radii"][:n], s["indices"][:n], per_batch, spb)

    def encode(self, src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, samples_per_batch):
        B, V, Cfr, H, W = img_feat.shape
        b = src_images.shape[-1] // W
        eng = self._last if (self._last is not None and self._last.b == b) else self._engine(img_feat.device, b, 1, False, False)
        c = lambda t: t.contiguous().float()
        near_far = self._tar["near_far"] if self._tar is not None else torch.ones((B, 2), device=img_feat.device)
        dr = torch.ones((B, 2, H, W), device=img_feat.device)
        grad = torch.is_grad_enabled()
        values = self.encode_grad and grad and any(t.is_cuda and t.requires_grad for t in (img_feat, feat_volume))
        positions = self.position_grad and grad and any(t.is_cuda and t.requires_grad for t in (rays_xyz, uvd, ball_radii))
        if values or positions:
            frame = {"src_images": c(src_images).detach(), "depth_range": dr, "vol_range": dr, "src_exts": c(src_exts).detach(),
                     "src_ints": c(src_ints).detach(), "tar_ext": c(tar_exts).detach(),
                     "tar_int": self._tar["tar_int"] if self._tar else c(src_ints[:, 0]).detach(), "near_far": near_far}
            total = torch.tensor([rays_xyz.shape[0]], dtype=torch.int64, device=img_feat.device)
            val = c if values else (lambda t: c(t).detach())   # a half that is not taken sees no graph: its backward is not run
            pos = c if positions else (lambda t: c(t).detach())
            return EncodeFunction.apply(eng, frame, val(img_feat), val(feat_volume), pos(rays_xyz), pos(uvd), pos(ball_radii),
                                        samples_per_batch.to(torch.int64).contiguous(), total)
        eng.prepare({"src_images": c(src_images), "img_feat": c(img_feat), "feat_volume": c(feat_volume), "depth_range": dr, "vol_range": dr,
                     "src_exts": c(src_exts), "src_ints": c(src_ints), "tar_ext": c(tar_exts), "tar_int": self._tar["tar_int"] if self._tar else c(src_ints[:, 0]),
                     "near_far": near_far})
        n = rays_xyz.shape[0]
        total = torch.tensor([n], dtype=torch.int64, device=img_feat.device)
        return eng.encode(c(rays_xyz), c(uvd), c(ball_radii), samples_per_batch.to(torch.int64).contiguous(), total)

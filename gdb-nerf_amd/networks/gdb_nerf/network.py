"""GDB-NeRF network with the reference's plugin surface (networks/gdb_nerf/network.py): same
constructor config keys, same sub-module names (`feature_net`, `depth_net`, `nerf`, `upsampler` —
the checkpoint prefixes), same `forward(batch) -> (ret, mvs_depths, blend_rgbs)`.

The CNNs run on PyTorch-ROCm.  The hot-path section (reference network.py:145-169) runs on the HIP
library: by default as ONE fused kernel (`gdb_render_bundles_fused`); with `hot_path = "mirrors"`
through the operator mirrors, which materialise the reference's intermediates.

What is differentiable:
  * `hot_path: "mirrors"`: the radiance MLP and the normalised alpha composite have HIP backward kernels, so
    `forward(batch)[0]["rgb"].sum().backward()` fills the gradients of `nerf.*` and of `upsampler.*` (the PyTorch decoder module).
  * `feature_net.*` and `depth_net.*` get none by default: the outputs of `encode` (and `sample`) carry no graph.
  * `nerf.encode_grad: true` (with `hot_path: "mirrors"`; default false): `encode` is differentiable with respect to the VALUES it
    gathers, the feature map and the cost-regularised feature volume (`gdb_encode_backward`), so the colour loss also reaches
    `feature_net.*` and the part of `depth_net.*` that produces the last stage's feature volume.  The sample POSITIONS stay constant.
    With the HIP FPN / cost-regularisation / cascade switches on, those tensors carry no `grad_fn` and the plain calls are made.
  * `nerf.position_grad: true` (with `hot_path: "mirrors"`; default false; independent of `encode_grad`): the sample positions are
    differentiable (`gdb_sample_backward`, `gdb_encode_position_backward`), so the colour loss - and `nerf_depth`,
    through `z_vals` - reaches `depth_net.*` through `depth_range` / `vol_range`: the depth prior moves the samples, as in the
    reference.  The cameras, the source images and `near_far` get no gradient.
  * `nerf.hip_decoder_train: true` (with `hot_path: "mirrors"`, bundle_size 2; default false): in train mode with grad mode on the
    decoder runs on the HIP library with a HIP backward (`decoder_train.DecodeTrainFunction`) instead of the PyTorch
    module under autograd; eval mode and no_grad keep the module.
  * `hot_path: "fused"` is unchanged and non-differentiable: its outputs have no `grad_fn` whatever `requires_grad` says.
  * `mvs.stage_render: true` (training mode; independent of the hot path): `blend_rgbs` holds the depth net's stage images, whose loss
    reaches `depth_net.nerfs.*`, `depth_net.cost_regs[i]` through the stage's feature volume and `feature_net.*` through the gathered
    feature map."""
from types import SimpleNamespace
from typing import Any, Dict, List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...engine import HotPathEngine
from ...parallel import PartialsGather, StripGather, TileGather, decode_window, decoder_halo, gather_strips, row_strip, se_partial_pitch
from . import utils
from .bundle_sampler import BundleSampler
from .decoder_rdn import Decoder
from .depth_net import DepthNet
from .feature_net import FeatureNet
from .nerf import NeRF


class Network(nn.Module):
    def __init__(self, config: SimpleNamespace) -> None:
        super().__init__()
        fpn, mvs, nrf = config.fpn, config.mvs, config.nerf
        # fpn.hip_feature_net: the FPN on the HIP library (fpn.FeaturePyramid) in eval mode on fp32 CUDA images; off by default.  A
        # FeatureNet the library is not built for is refused here, not left to fall back at the first forward.
        hip_fpn = bool(getattr(fpn, "hip_feature_net", False))
        if hip_fpn:
            from ... import fpn as hip_fpn_mod
            hip_fpn_mod.check_channels(fpn.base_channels, fpn.feat_dims)
        self.feature_net = FeatureNet(base_channels=fpn.base_channels, out_channels=fpn.feat_dims, hip=hip_fpn)
        self.voxel_dim = mvs.voxel_dim
        self.depth_net = DepthNet(config)

        self.max_num_samples = nrf.max_num_samples
        self.b_size = nrf.bundle_size
        if self.b_size <= 0 or self.b_size & (self.b_size - 1):
            raise ValueError('`Bundle size` must be a power of 2.')
        self.inv_depth = mvs.inv_depth[-1]
        self.is_adaptive = nrf.is_adaptive
        self.global_num_depth, self.max_mipmap_level = nrf.global_num_depth, nrf.max_mipmap_level
        # nerf.encode_grad: `encode` differentiable with respect to the feature map and the feature volume; needs the
        # operator mirrors, since the fused kernel carries no graph at all and the switch would train nothing, silently
        self.encode_grad = bool(getattr(nrf, "encode_grad", False))
        if self.encode_grad and getattr(nrf, "hot_path", "fused") != "mirrors":
            raise ValueError(f"nerf.encode_grad needs nerf.hot_path 'mirrors' (got {getattr(nrf, 'hot_path', 'fused')!r}): the fused hot path is not differentiable")
        # nerf.position_grad: `sample` and the coordinate arithmetic of `encode` differentiable, so that the colour loss moves the depth
        # prior that places the samples; independent of encode_grad, and refused without the mirrors for the same reason
        self.position_grad = bool(getattr(nrf, "position_grad", False))
        if self.position_grad and getattr(nrf, "hot_path", "fused") != "mirrors":
            raise ValueError(f"nerf.position_grad needs nerf.hot_path 'mirrors' (got {getattr(nrf, 'hot_path', 'fused')!r}): the fused hot path is not differentiable")
        self.sampler = BundleSampler(self.global_num_depth, self.max_mipmap_level, encode_grad=self.encode_grad, position_grad=self.position_grad)
        # nerf.hip_decoder_train: the decoder of the differentiable path on the HIP library with a HIP backward (DESIGN.md 4.23:
        # decoder_train.DecodeTrainFunction) instead of the PyTorch module under autograd.  Needs the operator mirrors (the fused hot
        # path carries no graph), bundle_size 2 and dec_layers 1 .. 16: anything else raises here, with the offending value.
        self.hip_decoder_train = bool(getattr(nrf, "hip_decoder_train", False))
        if self.hip_decoder_train:
            if getattr(nrf, "hot_path", "fused") != "mirrors":
                raise ValueError(f"nerf.hip_decoder_train needs nerf.hot_path 'mirrors' (got {getattr(nrf, 'hot_path', 'fused')!r}): the fused hot path is not differentiable")
            if self.b_size != 2:
                raise ValueError(f"nerf.hip_decoder_train is built for nerf.bundle_size 2 (got {self.b_size})")
            if not 1 <= int(nrf.dec_layers) <= 16:
                raise ValueError(f"nerf.hip_decoder_train is built for nerf.dec_layers 1..16 (got {nrf.dec_layers})")
        self._decoder_train = None

        # pyramid level whose scale is closest to (not below) the bundle map's 1/b   (reference :40-43)
        self.feat_level = next((i for i, s in enumerate(fpn.feat_scales) if s >= 1.0 / self.b_size), len(fpn.feat_scales))
        # the pyramid levels a forward reads: the depth net's volume levels and the image-feature level (a hint to the HIP FPN)
        self.fpn_levels = tuple(sorted(set(mvs.vol_levels) | {self.feat_level}))
        feat_dim = fpn.feat_dims[self.feat_level]
        self.nerf_hidden_dims, self.viewdir_agg = nrf.nerf_hidden_dims, nrf.viewdir_agg
        self.render_scale = 1.0
        self.nerf = NeRF(self.nerf_hidden_dims, feat_dim, self.voxel_dim, self.viewdir_agg)

        self.dec_layers = nrf.dec_layers
        self.upsampler = Decoder(feat_dim + 3 + self.voxel_dim, 3, num_feats=64, num_layers=self.dec_layers, upscale_factor=self.b_size)
        self.reweighting = nrf.reweighting
        self.hot_path = getattr(nrf, "hot_path", "fused")  # "fused" | "mirrors"
        # arithmetic of the NeRF MLP in the fused kernel: "f32" (fp32 MFMA, the reference's precision; default) | "f16" (f16 operands) |
        # "f32x" (split-f16 operand pairs: fp32-grade at close to the f16 rate)
        self.precision = {"f32": 1, "f16": 0, "f32x": 2}[str(getattr(nrf, "precision", "f32"))]
        # N1: the decoder on the HIP library (fp32 MFMA implicit-GEMM convolutions, channel-last, reading bundle_feat in place);
        # False keeps the PyTorch-ROCm module.  The HIP decoder takes any number of dense blocks up to 16 (every reference config has 3) and
        # bundle_size 2 (one up stage, folded with out_conv) or 4 (two: decoder_rdn.py:59-62 - the first as four sub-pixel convolutions,
        # the second folded; round 6); b = 1 (no up stage) keeps the PyTorch module.
        self.hip_decoder = bool(getattr(nrf, "hip_decoder", True)) and self.b_size in (2, 4) and 1 <= int(self.dec_layers) <= 16
        # Multi-GPU: "rows" = when torch.distributed is initialised, every rank renders one contiguous strip of
        # bundle-map rows of the frame and ONE all-gather of the packed rows (RCCL over xGMI) leaves the whole bundle map on every
        # rank; decoder and merge then run replicated (the decoder's squeeze-excitation takes a global mean over the image,
        # decoder_rdn.py:10,20, so it does not shard by rows).  "none" (default): every rank renders whole frames.
        # "tiles": each rank renders its strip plus the decoder's halo (parallel.decode_window), decodes its strip by row windows
        # with one all-gather of the squeeze-excitation sums per dense block (the mean's only non-local input), merges its strip,
        # and ONE all-gather of the image tiles with the bundle-resolution depth and opacity (3 b^2 + 2 floats per bundle) leaves
        # the frame on every rank.  Needs the HIP decoder and the fused hot path.  The FPN and the depth net stay replicated.
        self.shard = str(getattr(nrf, "shard", "none"))
        if self.shard not in ("none", "rows", "tiles"):
            raise ValueError(f"nerf.shard must be 'none', 'rows' or 'tiles', got {self.shard!r}")
        if self.shard == "tiles" and not self.hip_decoder:
            raise ValueError("nerf.shard 'tiles' shards the HIP decoder by rows: it needs nerf.hip_decoder with bundle_size 2 or 4 and "
                             f"dec_layers 1..16 (got hip_decoder {bool(getattr(nrf, 'hip_decoder', True))}, bundle_size {self.b_size}, "
                             f"dec_layers {self.dec_layers})")
        if self.shard == "tiles" and self.hot_path != "fused":
            raise ValueError(f"nerf.shard 'tiles' needs nerf.hot_path 'fused' (got {self.hot_path!r}): the operator mirrors render whole frames")
        # The decoder's arithmetic: "auto" (default, also when absent: fp32 MFMA, or the split-f16 convolutions when `precision` is "f16" /
        # "f32x" - both fp32-grade) | "f16" (plain f16 MFMA, half-precision activations, the contract of DESIGN.md section 4.10:
        # HotPathEngine.decode_f16).  "f16" needs bundle_size 2 and the HIP decoder, and does not run by row windows (`shard: tiles`).
        self.decoder_precision = str(getattr(nrf, "decoder_precision", "auto"))
        if self.decoder_precision not in ("auto", "f16"):
            raise ValueError(f"nerf.decoder_precision must be 'auto' or 'f16', got {self.decoder_precision!r}")
        if self.decoder_precision == "f16":
            if self.b_size != 2:
                raise ValueError(f"nerf.decoder_precision 'f16' is built for bundle_size 2 (got {self.b_size})")
            if not self.hip_decoder:
                raise ValueError("nerf.decoder_precision 'f16' is a form of the HIP decoder: it needs nerf.hip_decoder and dec_layers 1..16 "
                                 f"(got hip_decoder {bool(getattr(nrf, 'hip_decoder', True))}, dec_layers {self.dec_layers})")
            if self.shard == "tiles":
                raise ValueError("nerf.decoder_precision 'f16' does not run by row windows: nerf.shard 'tiles' keeps the fp32 / split-f16 decoder")
        # The intermediates of a frame (packed render, decoder image) always live in per-engine buffers reused frame after frame.
        # The tensors in the returned dict are fresh by default, as the reference's are (a caller may keep them across frames);
        # `nerf.reuse_outputs: true` makes them per-engine buffers too, overwritten by the next forward: no allocation at all in
        # the per-frame path, for loops that consume a frame's outputs before the next one (bench.py, tools/bench_network.py).
        self.reuse_outputs = bool(getattr(nrf, "reuse_outputs", False))
        self._feat_dim = feat_dim
        self._engine = None
        self._gather = None
        self._tiles_state = None

    # ---- hot path ------------------------------------------------------------------------
    def _get_engine(self, device) -> HotPathEngine:
        if self._engine is None or self._engine.device != torch.device(device):
            self._engine = HotPathEngine(bundle_size=self.b_size, max_num_samples=self.max_num_samples, is_adaptive=self.is_adaptive,
                                         inv_depth=self.inv_depth, global_num_depth=self.global_num_depth,
                                         max_mipmap_level=self.max_mipmap_level, feat_dim=self._feat_dim, voxel_dim=self.voxel_dim,
                                         hid_dim=self.nerf_hidden_dims, viewdir_agg=self.viewdir_agg, device=device)
        self._engine.precision = self.precision
        self._engine.reuse_outputs = self.reuse_outputs
        self._engine.reuse_internal = True
        self.nerf.sync_engine(self._engine)
        if self.hip_decoder:
            # (storage, version) per tensor, as NeRF.param_versions: `p.data = ...` and load_state_dict(assign=True) change the
            # storage without touching the version counter.  (`p.data.copy_()` changes neither: call invalidate_packed_weights().)
            v = tuple((p.data_ptr(), p._version) for p in self.upsampler.parameters())
            if getattr(self._engine, "_dec_versions", None) != v:
                self._engine.load_decoder_weights({k: t.detach() for k, t in self.upsampler.state_dict().items()}, self.dec_layers)
                self._engine._dec_versions = v
        return self._engine

    def invalidate_packed_weights(self) -> None:
        """Force a re-pack of the NeRF and decoder weights on the next forward (needed only after an in-place write through
        `.data`, which PyTorch does not version)."""
        if self._engine is not None:
            self._engine._dec_versions = None
            self._engine._nerf_versions = None

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_packed_weights()
        return super()._load_from_state_dict(*args, **kwargs)

    def _dist(self):
        """torch.distributed when this forward is to be row-sharded, else None."""
        if self.shard not in ("rows", "tiles"):
            return None
        import torch.distributed as dist
        return dist if dist.is_available() and dist.is_initialized() else None

    def _render_packed(self, eng, B: int, H: int, W: int) -> torch.Tensor:
        """The hot path of the prepared frame into packed rows [bundle_feat | depth | opacity] (n_bundles, Q + 2); row-sharded over
        the ranks of the default process group when `nerf.shard: rows` (reference call site network.py:145-169; the eval loop
        run.py:54-66 calls this once per frame on every rank)."""
        if not eng.fused_supported:
            # bundle_size 1 / 4 (configs/dtu_pretrain.yaml:33 "4 for 4*4"; network.py:31-34 accepts any power of two): the fused kernel
            # is built for b = 2, so the frame goes through the HIP operator mirrors (gdb_sample -> gdb_encode -> gdb_mlp ->
            # gdb_composite), whole on every rank (the mirrors take no row strip).
            return eng.render_unfused_packed()
        dist = self._dist()
        if dist is None:
            return eng.render_packed()
        world, rank = dist.get_world_size(), dist.get_rank()
        C = eng.Q + 2
        # RCCL ("nccl") moves device tensors; a gloo group (CPU tests, the one-GPU rehearsal) exchanges host copies
        stage = dist.get_backend() == "gloo"
        if B == 1:  # one contiguous strip per rank: in-place all-gather, buffers cached per shape
            g = self._gather
            if g is None or (g.H, g.W, g.C, g.world, g.rank) != (H, W, C, world, rank) or g.full.device != torch.device(eng.device):
                g = self._gather = StripGather(H, W, C, world, rank, eng.device, dist, stage_cpu=stage)
            r0, r1 = g.strip
            eng.render_packed(r0, r1, None, g.full)
            return g.gather()
        from ...parallel import row_strip
        r0, r1 = row_strip(H, rank, world)
        full = eng.render_packed(r0, r1)  # fresh, zero-filled outside the strip
        if stage and full.is_cuda:
            return gather_strips(full.cpu(), H, world, dist, B=B).to(full.device)
        return gather_strips(full, H, world, dist, B=B)

    def _forward_tiles(self, eng, B: int, H: int, W: int, dist):
        """`nerf.shard: tiles` on the prepared frame: this rank's window render, its strip's decode in num_layers + 1 phases with one
        all-gather of the squeeze-excitation sums between each, its strip's merge, then ONE all-gather of the tiles.  Returns the
        frame's (img, nerf_depth, opacity) on every rank, bit-identical to `shard: none`."""
        world, rank = dist.get_world_size(), dist.get_rank()
        b, L, Q = self.b_size, int(self.dec_layers), eng.Q
        r0, r1 = row_strip(H, rank, world)
        w0, w1 = decode_window(H, rank, world, decoder_halo(b, L))
        stage = dist.get_backend() == "gloo"   # gloo exchanges host copies, as `rows` does
        key = (B, H, W, world, rank, str(eng.device), id(eng))
        st = self._tiles_state
        if st is None or st["key"] != key:
            dec = eng.decoder_rows(r0, r1) if r1 > r0 else None
            if dec is not None and dec.window != (w0, w1):
                raise RuntimeError(f"decoder window {dec.window} != parallel.decode_window {(w0, w1)}")
            part = dec.part if dec is not None else torch.zeros((B, H, se_partial_pitch(W)), device=eng.device)
            st = self._tiles_state = {"key": key, "dec": dec, "packed": torch.zeros((B * H * W, Q + 2), device=eng.device),
                                      "partials": PartialsGather(part, world, rank, dist, stage_cpu=stage),
                                      "tiles": TileGather(B, H, W, b, world, rank, eng.device, dist, stage_cpu=stage)}
        dec, packed, pg, tg = st["dec"], st["packed"], st["partials"], st["tiles"]
        if dec is not None:
            if eng.fused_supported:
                eng.render_packed(w0, w1, None, packed)   # the halo rows are re-rendered here: bundles are independent
            else:
                packed = eng.render_unfused_packed()      # (the operator mirrors take no row range: the whole frame)
        rgb_c = None
        for p in range(L + 1):
            if p:
                pg.gather()
            if dec is not None:
                rgb_c = dec.run_phase(packed, p)
        if dec is not None:
            eng.merge_packed_rows(packed, rgb_c, self.reweighting, r0, r1, tg.tile)
            tg.maps[:, : r1 - r0].copy_(packed.view(B, H, W, Q + 2)[:, r0:r1, :, Q:Q + 2])
        img, maps = tg.gather()
        nerf_depth, opacity = eng.upsample_maps(maps)
        return img, nerf_depth, opacity

    def render_bundles(self, rgbs_feat_rgb_dir, vox_feat, z_vals, indices, samples_per_bundle):
        """MLP + normalised alpha composite on materialised samples (reference network.py:54-91)."""
        sigma, feat = self.nerf(vox_feat, rgbs_feat_rgb_dir)
        n_bundles = samples_per_bundle.shape[0]
        weights, inverse = utils.render_weight_from_density(sigma, indices, n_bundles)
        if self.inv_depth:
            z_vals = 1.0 / z_vals
        feat, depth, opacity = utils.accumulate_value_along_rays(feat, z_vals, weights, indices, n_bundles, inverse)
        if self.inv_depth:
            depth = 1.0 / depth
        return feat, depth, opacity

    def _decoder_train_applies(self, bundle_feat: torch.Tensor) -> bool:
        """nerf.hip_decoder_train takes the decoder of this forward: the switch is on, the module trains, grad mode is on, the rows or a
        decoder parameter require grad, and everything is fp32 on a GPU.  Otherwise the PyTorch module runs as it always did."""
        if not (self.hip_decoder_train and self.training and torch.is_grad_enabled()):
            return False
        ps = list(self.upsampler.parameters())
        if not (bundle_feat.requires_grad or any(p.requires_grad for p in ps)):
            return False
        return all(t.is_cuda and t.dtype == torch.float32 for t in (bundle_feat, *ps))

    def forward(self, batch: Dict[str, Any]) -> Tuple[Dict[str, torch.Tensor], List[torch.Tensor], List[torch.Tensor]]:
        src, tar = batch["src_views"], batch["tar_views"]
        near_far = batch["near_far"]
        src_images = src["rgb"]
        B, V, _, Ho, Wo = src_images.shape
        src_exts, tar_exts = src["extrinsics"], tar["extrinsics"]
        src_ints, tar_ints = src["intrinsics"].clone(), tar["intrinsics"].clone()

        if "render_scale" in batch:
            self.render_scale = batch["render_scale"][0].item()
        if self.render_scale != 1.0:
            src_images = F.interpolate(src_images.flatten(0, 1), scale_factor=self.render_scale, mode="bilinear",
                                       align_corners=False).unflatten(0, (B, V))
            Ho, Wo = src_images.shape[-2:]
            src_ints[..., :2, :] *= self.render_scale
            tar_ints[:, :2, :] *= self.render_scale

        ms_feats = [None if f is None else f.unflatten(0, (B, V)) for f in self.feature_net(src_images.flatten(0, 1), self.fpn_levels)]
        mvs_depths, ranges, vol_ranges, volumes, blend_rgbs = self.depth_net(src_images, ms_feats, src_exts, src_ints, tar_exts, tar_ints, near_far)
        depth_range, vol_range, feat_volume, mvs_depth = ranges[-1], vol_ranges[-1], volumes[-1], mvs_depths[-1]

        b = self.b_size
        H, W = Ho // b, Wo // b
        if depth_range.shape[2:] != (H, W):
            depth_range = F.interpolate(depth_range, size=(H, W), mode="bilinear", align_corners=False)
            vol_range = F.interpolate(vol_range, size=(H, W), mode="bilinear", align_corners=False)
            mvs_depth = F.interpolate(mvs_depth.unsqueeze(1), size=(H, W), mode="nearest").squeeze(1)
        img_feat = ms_feats[self.feat_level]
        if img_feat.shape[-2:] != (H, W):
            img_feat = F.interpolate(img_feat.flatten(0, 1), size=(H, W), mode="bilinear", align_corners=False).unflatten(0, (B, V))
        eng = None
        if self.hot_path == "fused":
            c = lambda t: t.contiguous().float()
            eng = self._get_engine(src_images.device)
            # a rank of a row-sharded forward plans its own strip of bundle-map rows only, and - for frames large enough for the bound's
            # launch to pay - builds only the strip's reach of the pyramids (gdb_prepare_rows; any bundle size)
            dist = self._dist()
            rows = None
            if dist is not None and self.shard == "tiles":   # the strip plus the decoder's halo (an empty strip plans the frame)
                rows = decode_window(H, dist.get_rank(), dist.get_world_size(), decoder_halo(b, int(self.dec_layers)))
                rows = rows if rows[1] > rows[0] else None
            elif dist is not None:
                rows = row_strip(H, dist.get_rank(), dist.get_world_size())
            # N3: the kernel resamples the colour channels itself (no torch.cat / F.interpolate of the source images)
            eng.prepare({"src_images": c(src_images), "fpn_feat": c(img_feat), "feat_volume": c(feat_volume),
                         "depth_range": c(depth_range), "vol_range": c(vol_range), "src_exts": c(src_exts), "src_ints": c(src_ints),
                         "tar_ext": c(tar_exts), "tar_int": c(tar_ints), "near_far": c(near_far)}, rows=rows)
            if dist is not None and self.shard == "tiles":
                img, nerf_depth, opacity = self._forward_tiles(eng, B, H, W, dist)
                return {"rgb": img, "nerf_depth": nerf_depth, "mvs_depth": mvs_depth, "opacity": opacity}, mvs_depths, blend_rgbs
            packed = self._render_packed(eng, B, H, W)
            if self.hip_decoder:
                # reads channels 3 b^2 .. Q-1 of the packed rows in place
                rgb_c = eng.decode_f16(packed) if self.decoder_precision == "f16" else eng.decode(packed)
            else:
                rgb_c = self.upsampler(packed[:, 3 * b * b:eng.Q].view(B, H, W, -1).permute(0, 3, 1, 2)).contiguous().float()
            # N1: pixel-shuffle + add (+ re-weighting) + the two x b upsamplings in one HIP kernel, on the packed rows in place
            img, nerf_depth, opacity = eng.merge_packed(packed, rgb_c, self.reweighting)
            return {"rgb": img, "nerf_depth": nerf_depth, "mvs_depth": mvs_depth, "opacity": opacity}, mvs_depths, blend_rgbs
        else:
            rgb_lo = F.interpolate(src_images.flatten(0, 1), size=(H, W), mode="bilinear", align_corners=False).unflatten(0, (B, V))
            img_feat_rgb = torch.cat((img_feat, rgb_lo), dim=2)
            self.sampler.build_rays(tar_exts, tar_ints, (Ho, Wo), near_far[:, 0], near_far[:, 1])
            rays_xyz, uvd, z_vals, ball_radii, indices, per_batch, per_bundle = self.sampler.sample(
                depth_range, vol_range, b, self.max_num_samples, self.inv_depth, self.is_adaptive)
            rfd, vox = self.sampler.encode(src_images, img_feat_rgb, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch)
            bundle_feat, bundle_depth, bundle_opacity = self.render_bundles(rfd, vox, z_vals, indices, per_bundle)

        nerf_feat = bundle_feat.view(B, H, W, -1).permute(0, 3, 1, 2)
        n_rgb = 3 * b * b
        if self._decoder_train_applies(bundle_feat):
            from ...decoder_train import DecodeTrainFunction, DecoderTrain, decoder_params
            if self._decoder_train is None:
                self._decoder_train = DecoderTrain(self.upsampler, self.b_size)
            rgb_c = DecodeTrainFunction.apply(self._decoder_train, bundle_feat.contiguous(), B, H, W, *decoder_params(self.upsampler))
        else:
            rgb_c = self.upsampler(nerf_feat[:, n_rgb:])
        rgb_f = F.pixel_shuffle(nerf_feat[:, :n_rgb], b)
        up = lambda t: F.interpolate(t.view(B, 1, H, W), scale_factor=b, mode="bilinear", align_corners=False).squeeze(1)
        img = rgb_c + rgb_f
        if self.reweighting:
            img = 0.5 * (img + rgb_f)
        ret = {"rgb": img, "nerf_depth": up(bundle_depth), "mvs_depth": mvs_depth, "opacity": up(bundle_opacity)}
        return ret, mvs_depths, blend_rgbs

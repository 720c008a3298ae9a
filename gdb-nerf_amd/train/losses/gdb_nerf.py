"""The loss plugin, same contract as the reference's train/losses/gdb_nerf.py:7-55: `NetworkWrapper(net, cfg)` whose
`forward(batch) -> (output, loss, scalar_stats, image_stats)`.

loss = photometric(final image) + sum_i mvs.loss_weight[i] * photometric(blend_rgbs[i]) while training, with
photometric = a * MSE + b * (1 - SSIM) + c * VGG perceptual and (a, b, c) = `train.photometric_weights` (the reference's
[1.0, 0.1, 0.05]).  `scalar_stats`: mse_loss, psnr = -10 log10(mse + 1e-6), ssim, perceptual_loss, loss; depth_loss while training;
depth_loss{i} (masked smooth-L1 of the stage depths, monitoring only) when the batch carries ground-truth depths.

`train.hip_loss: True` (default off) takes the MSE + SSIM part and the monitor from the HIP library (losses.photometric_terms /
smooth_l1_masked: one call each, the gradient written by the forward call) whenever the tensors are fp32 CUDA; otherwise, and with
the switch off, the plain-torch restatement of losses.py runs.  Either way `forward` holds no `.item()`, no boolean indexing and no
host copy, so nothing in it waits for the device; the one exception is the restatement's first call on a device, which forms the
SSIM window and uploads it once (losses.ssim_window keeps it, as the reference keeps its window in a module buffer).

The perceptual term needs VGG-16 weights, which this project cannot download: `train.vgg_weights` names a file with them
(INTEGRATION.md has the export recipe; the file exported for `test.lpips_weights` holds the same ten tensors).  A non-zero third
weight without that file is an error, never a silently dropped term."""
import torch
import torch.nn as nn

from ... import losses


class NetworkWrapper(nn.Module):
    def __init__(self, net, cfg):
        super().__init__()
        self.device = torch.device("cuda:{}".format(getattr(cfg, "local_rank", 0)))
        self.net = net
        train = getattr(cfg, "train", None)
        self.alpha, self.beta, self.gamma = (float(v) for v in getattr(train, "photometric_weights", [1.0, 0.1, 0.05]))
        self.hip_loss = bool(getattr(train, "hip_loss", False))
        self.loss_weight = list(cfg.mvs.loss_weight)
        self.num_stages = len(cfg.mvs.vol_scales)
        self.perceptual = None
        if self.gamma != 0.0:
            path = getattr(train, "vgg_weights", "")
            if not path:
                raise ValueError(f"train.photometric_weights gives the VGG perceptual term the weight {self.gamma} but train.vgg_weights "
                                 "names no weights file: set train.vgg_weights to a file with the ten VGG-16 convolutions (conv.0 .. "
                                 "conv.9, INTEGRATION.md), or set the third entry of train.photometric_weights to 0")
            self.perceptual = losses.VggPerceptual(torch.load(path, map_location="cpu", weights_only=True))

    def _on_hip(self, *tensors) -> bool:
        return self.hip_loss and all(t.is_cuda and t.dtype == torch.float32 for t in tensors)

    def photometric_loss(self, gt, est):
        """(total, mse, ssim, perceptual) of gt, est (B,3,H,W); `gt` may be the permuted view of an NHWC frame."""
        terms = losses.photometric_terms if self._on_hip(gt, est) else losses.photometric_terms_torch
        photo, mse, ssim = terms(gt, est, self.alpha, self.beta)
        if self.perceptual is None:
            return photo, mse, ssim, torch.zeros_like(mse)
        perceptual = self.perceptual(gt, est)
        return photo + self.gamma * perceptual, mse, ssim, perceptual

    def forward(self, batch):
        output, depth_prediction, blend_rgbs = self.net(batch)
        scalar_stats = {}

        rgb_gt = batch["tar_views"]["rgb"].permute(0, 3, 1, 2)
        color_loss, mse_loss, ssim, perceptual_loss = self.photometric_loss(rgb_gt, output["rgb"])
        with torch.no_grad():
            psnr = -10.0 * torch.log10(mse_loss + 1e-6)
        scalar_stats.update({"mse_loss": mse_loss, "psnr": psnr, "ssim": ssim, "perceptual_loss": perceptual_loss})

        depth_loss = 0.0
        if self.training:   # the stage images: as many as the network returns
            stage_gt = [rgb.permute(0, 3, 1, 2) for rgb in batch["tar_gt_ms"]["rgb"]] if len(blend_rgbs) else []
            for i in range(len(blend_rgbs)):
                depth_loss = depth_loss + self.loss_weight[i] * self.photometric_loss(stage_gt[i], blend_rgbs[i])[0]
            scalar_stats["depth_loss"] = depth_loss

        with torch.no_grad():   # monitoring only
            if "depth" in batch.get("tar_gt_ms", {}):
                gts, masks = batch["tar_gt_ms"]["depth"], batch["tar_gt_ms"]["mask"]
                for i in range(self.num_stages):
                    est, gt, mask = depth_prediction[i], gts[i], masks[i].to(gts[i].dtype)
                    monitor = losses.smooth_l1_masked if self._on_hip(est, gt, mask) else losses.smooth_l1_masked_torch
                    scalar_stats[f"depth_loss{i}"] = monitor(est, gt, mask)

        loss = color_loss + depth_loss
        scalar_stats["loss"] = loss
        return output, loss, scalar_stats, {}

"""`SyntheticFrames`: a sized iterable of training batches in the layout the reference's data loaders produce, for TESTS AND SMOKE
RUNS ONLY.  The cameras are `synthetic.make_frame`'s; the source images and the target image are independent smoothed noise, so the
frames are NOT multi-view consistent: a network trained on them learns nothing about geometry, it only gives the loop, the optimiser
and the checkpoints something of the right shape to run on.  The DTU / LLFF readers of the reference need cv2 and data sets that are
not part of this package.

A batch (CPU float32 tensors; the trainer moves them):
  src_views: rgb (B,V,3,H,W), extrinsics (B,V,4,4), intrinsics (B,V,3,3)
  tar_views: rgb (B,H,W,3), extrinsics (B,4,4), intrinsics (B,3,3)
  near_far (B,2)
  tar_gt_ms: rgb = [the target image area-averaged to (B, H s, W s, 3) for s in cfg.mvs.vol_scales]"""
import numpy as np
import torch

from .. import synthetic


class SyntheticFrames(object):
    def __init__(self, cfg, length, H, W, V=3, seed=0, B=1, scene="dtu"):
        self.scales = [float(s) for s in cfg.mvs.vol_scales]
        for s in self.scales:
            k = round(1.0 / s)
            if k < 1 or abs(k * s - 1.0) > 1e-9 or H % k or W % k:
                raise ValueError(f"SyntheticFrames: {H} x {W} does not divide by mvs.vol_scales entry {s}")
        self.length, self.H, self.W, self.V, self.B, self.seed, self.scene = int(length), int(H), int(W), int(V), int(B), int(seed), scene
        self.epoch = 0

    def __len__(self):
        return self.length

    def batch(self, i):
        B, H, W = self.B, self.H, self.W
        fr = synthetic.make_frame(H, W, V=self.V, B=B, scene=self.scene, seed=self.seed + i)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        rng = np.random.default_rng([self.seed + i, 1])
        tar = synthetic._box(rng.random((B, 3, H, W), dtype=np.float32), 5)
        ms = []
        for s in self.scales:
            k = round(1.0 / s)
            ms.append(t(tar.reshape(B, 3, H // k, k, W // k, k).mean(axis=(3, 5), dtype=np.float32).transpose(0, 2, 3, 1)))
        return {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
                "tar_views": {"rgb": t(tar.transpose(0, 2, 3, 1)), "extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])},
                "near_far": t(fr["near_far"]), "tar_gt_ms": {"rgb": ms}}

    def __iter__(self):
        return (self.batch(i) for i in range(self.length))

"""Evaluator with the reference's surface (evaluators/gdb_nerf.py:12-151): `evaluate(output, batch)`
accumulates masked PSNR, SSIM and optional depth errors; `summarize()` prints per-scene rows and
returns {'psnr', 'ssim'[, 'lpips']}.

skimage, lpips and cv2 are not in the MI355X image, so the two skimage metrics are restated in numpy:
  * peak_signal_noise_ratio(gt[mask], pred[mask], data_range=1)           (reference :82)
  * structural_similarity(gt, pred, channel_axis=-1) with skimage's defaults for float images:
    7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, data_range 2 (dtype range of
    float images), mean over the interior and the channels                  (reference :86)
LPIPS (VGG-16 backbone): with `test.lpips_weights` naming a weights file (torch.save of the mapping `metrics.lpips_weights_from`
documents; INTEGRATION.md has the export recipe) the definition of include/gdb_nerf_hip.h is restated below in plain torch
(`lpips_torch`: F.conv2d, from the same weights) and the `lpips` package is never imported.  The package is not available to this
project: the restatement follows its written definition (release 0.1.4, net='vgg', eval mode, spatial=False), and agreement with the
package's published weights and values is unverified.  With the key empty `eval_lpips: True` needs the package, and is an error
without it.

`test.hip_metrics: True` (default off) keeps the frame on the device: with fp32 CUDA prediction and ground truth, `evaluate` only
enqueues the metric kernels of the HIP library (metrics.py, gdb_eval_image / gdb_eval_depth) and returns; each frame leaves a
row of float64 sums in a device table that `summarize` copies to the host once.  With the switch off, CPU tensors or non-fp32
images the numpy path below runs unchanged.  With LPIPS weights the device path enqueues gdb_eval_lpips into column 13 of the same row."""
import math
import os
import struct
import zlib
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage import uniform_filter


def psnr(gt: np.ndarray, pred: np.ndarray, data_range: float = 1.0) -> float:
    mse = float(np.mean((np.asarray(gt, np.float64) - np.asarray(pred, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * math.log10(data_range ** 2 / mse)


def ssim(gt: np.ndarray, pred: np.ndarray, win: int = 7, data_range: float = 2.0) -> float:
    """(H,W,C) float images."""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    norm = win * win / (win * win - 1.0)
    pad = (win - 1) // 2
    vals = []
    for ch in range(gt.shape[-1]):
        x, y = gt[..., ch].astype(np.float64), pred[..., ch].astype(np.float64)
        ux, uy = uniform_filter(x, win), uniform_filter(y, win)
        vx = norm * (uniform_filter(x * x, win) - ux * ux)
        vy = norm * (uniform_filter(y * y, win) - uy * uy)
        vxy = norm * (uniform_filter(x * y, win) - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        vals.append(s[pad:-pad, pad:-pad].mean())
    return float(np.mean(vals))


# ---- LPIPS (VGG-16) restated in plain torch: the numpy path's arithmetic and the tests' fp32 / float64 reference -------------------
LPIPS_TAPS = (1, 3, 6, 9, 12)   # the convolutions whose ReLU output is tapped; a 2 x 2 max-pool (floor) follows each but the last


def lpips_scale(img: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The input map and the scaling layer: img (N,3,h,w) in [0, 1] -> ((2 img - 1) - shift_c) / scale_c."""
    return ((img * 2.0 - 1.0) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)


def lpips_conv(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """One 3 x 3 convolution with zero padding 1, bias and ReLU."""
    return F.relu(F.conv2d(x, weight, bias, stride=1, padding=1))


def lpips_pool(x: torch.Tensor) -> torch.Tensor:
    """The 2 x 2 stride-2 max-pool between the groups; floor: an odd last row or column is dropped."""
    return F.max_pool2d(x, kernel_size=2, stride=2, ceil_mode=False)


def lpips_tap(fa: torch.Tensor, fb: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """One tap: unit-normalise over the channels (eps 1e-10 outside the root), squared difference, the tap's 1 x 1 weights (no bias),
    mean over the pixels.  fa, fb (N,C,h,w), lin (C,) -> (N,)."""
    na = torch.sqrt(torch.sum(fa ** 2, dim=1, keepdim=True)) + 1e-10
    nb = torch.sqrt(torch.sum(fb ** 2, dim=1, keepdim=True)) + 1e-10
    d = F.conv2d((fa / na - fb / nb) ** 2, lin.view(1, -1, 1, 1))
    return d.mean(dim=(2, 3))[:, 0]


def lpips_torch(a: torch.Tensor, b: torch.Tensor, weights) -> torch.Tensor:
    """LPIPS of the image batches a, b (N,3,h,w), values in [0, 1], from `weights` (metrics.lpips_weights_from's mapping, in the
    images' dtype and on their device): (N,) values.  The same chain, term by term, as the HIP library's gdb_eval_lpips."""
    with torch.no_grad():
        x = lpips_scale(torch.cat([a, b]), weights["shift"], weights["scale"])
        total, tap = 0.0, 0
        for i in range(13):
            x = lpips_conv(x, weights[f"conv.{i}.weight"], weights[f"conv.{i}.bias"])
            if i == LPIPS_TAPS[tap]:
                total = total + lpips_tap(x[:len(a)], x[len(a):], weights[f"lin.{tap}"])
                tap += 1
                if tap < len(LPIPS_TAPS):
                    x = lpips_pool(x)
        return total


def _resize_bilinear(img: np.ndarray, size_hw) -> np.ndarray:
    """cv2.resize(..., INTER_LINEAR) for a single-channel map (half-pixel centres, edge clamp)."""
    H, W = img.shape
    h, w = size_hw
    ys = np.clip((np.arange(h) + 0.5) * H / h - 0.5, 0, H - 1)
    xs = np.clip((np.arange(w) + 0.5) * W / w - 0.5, 0, W - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def write_png(path: str, rgb_u8: np.ndarray) -> None:
    """Minimal 8-bit RGB PNG writer (cv2.imwrite stand-in)."""
    h, w, _ = rgb_u8.shape
    raw = b"".join(b"\x00" + rgb_u8[y].tobytes() for y in range(h))
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


class Evaluator:
    # columns of a frame's row in the device table: the image record, then the depth records of the NeRF and the MVS depth
    _COLS = 16   # 5 + 4 + 4 + 1, padded to whole 128-byte rows
    _NERF_DEPTH, _MVS_DEPTH, _LPIPS = 5, 9, 13

    def __init__(self, cfg):
        self.cfg = cfg
        self._reset()
        self.hip_metrics = bool(getattr(cfg.test, "hip_metrics", False))
        self._table, self._rows = None, []   # device rows (capacity, _COLS) and per row on the host (scene, SSIM windows, has depth)
        self.loss_fn_vgg = None
        self.lpips_weights, self._lpips_on = None, {}   # the 33 CPU tensors; per device: (the weights there, the packed buffer)
        path = getattr(cfg.test, "lpips_weights", "")
        if getattr(cfg, "eval_lpips", False) and path:  # caller-supplied weights: the `lpips` package is never imported
            from .. import metrics
            self.lpips_weights = metrics.lpips_weights_from(torch.load(path, map_location="cpu", weights_only=True))
        elif getattr(cfg, "eval_lpips", False):
            try:
                import lpips  # noqa: F401
            except ImportError as e:
                raise RuntimeError("eval_lpips is set but the `lpips` package (and its VGG weights) is not available") from e
            self.loss_fn_vgg = lpips.LPIPS(net="vgg").cuda()
        if cfg.test.eval_depth:  # MVSNeRF protocol, reference :23-31
            self.eval_depth_scenes = ["scan1", "scan8", "scan21", "scan103", "scan110"]
            self.depth = defaultdict(list)
        if getattr(cfg, "save_result", False):
            os.makedirs(cfg.result_dir, exist_ok=True)

    def _reset(self):
        self.psnrs, self.ssims, self.lpips = [], [], []
        self.scene = defaultdict(lambda: defaultdict(list))

    def _lpips_weights_on(self, device, packed=False):
        """The LPIPS weights on `device` (cached), or their packed buffer for gdb_eval_lpips (packed once per device, on the host)."""
        device = torch.device(device)
        ent = self._lpips_on.setdefault(device, [None, None])
        if packed:
            if ent[1] is None:
                from .. import metrics
                ent[1] = metrics.pack_lpips(self.lpips_weights, device)
            return ent[1]
        if ent[0] is None:
            ent[0] = {k: v.to(device) for k, v in self.lpips_weights.items()}
        return ent[0]

    def use_hip_metrics(self, output, batch) -> bool:
        """The switch is on, and prediction, ground truth (fp32) and mask are CUDA tensors."""
        pred, gt, mask = output["rgb"], batch["tar_views"]["rgb"], batch["tar_views"]["mask"]
        return self.hip_metrics and all(getattr(t, "is_cuda", False) for t in (pred, gt, mask)) and \
            pred.dtype == gt.dtype == torch.float32

    def _next_rows(self, n, device):
        """A view of the next n free rows of the device table, which grows by doubling (the copy is enqueued on the stream)."""
        used = len(self._rows)
        if self._table is None or self._table.device != device or used + n > self._table.shape[0]:
            cap = max(64, 2 * (used + n))
            table = torch.empty((cap, self._COLS), dtype=torch.float64, device=device)
            if used:
                table[:used].copy_(self._table[:used])
            self._table = table
        return self._table[used:used + n]

    def _evaluate_hip(self, output, batch):
        """The device path of `evaluate`: enqueue and return.  No host copy, no `.item()`, no synchronising call — except for
        `save_result`, whose PNG is written from a host copy (that copy waits for the stream), and `eval_lpips` through the `lpips`
        package, whose `.item()` does (with `test.lpips_weights` LPIPS is enqueued like the rest: column 13 of the frame's row).
        An image too small for one 7 x 7 window raises ValueError (skimage raises there too; the numpy path returns NaN with a
        warning)."""
        from .. import metrics
        B, _, _, H, W = batch["src_views"]["rgb"].shape
        pred, gt, mask = output["rgb"].detach(), batch["tar_views"]["rgb"].detach(), batch["tar_views"]["mask"]
        if mask.dtype != torch.float32:
            mask = mask.float()   # on the device
        h, w = gt.shape[1:3]
        crop = (0, 0, h, w)
        if self.cfg.test.eval_center:  # the numpy path's [ch:-ch, cw:-cw], with ch, cw from the source views' size as there
            ch, cw = int(H * 0.1), int(W * 0.1)
            crop = (ch, cw, max(h - 2 * ch, 0) if ch else 0, max(w - 2 * cw, 0) if cw else 0)
        rows = self._next_rows(B, gt.device)
        metrics.eval_image(pred, gt, mask, rows, crop)
        if self.lpips_weights is not None:
            metrics.eval_lpips(pred, gt, mask, self._lpips_weights_on(gt.device, packed=True), rows[:, self._LPIPS:], crop)
        if getattr(self.cfg, "save_result", False) or self.loss_fn_vgg is not None:
            pc = pred.permute(0, 2, 3, 1).clamp(0.0, 1.0)[:, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
            keep = (mask >= 1)[:, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3], None]
        for b in range(B):
            scene = batch["meta"]["scene"][b]
            if getattr(self.cfg, "save_result", False):  # a host copy: waits for the stream
                name = "{}_{}_{}.png".format(scene, batch["meta"]["tar_view"][b].item(), batch["meta"]["frame_id"][b].item())
                write_png(os.path.join(self.cfg.result_dir, name), (pc[b].cpu().numpy() * 255).clip(0, 255).astype(np.uint8))
            if self.loss_fn_vgg is not None:
                t = lambda a: ((a * keep[b])[None].permute(0, 3, 1, 2) - 0.5) * 2.0
                gc = gt[b, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
                v = self.loss_fn_vgg(t(gc), t(pc[b])).item()
                self.lpips.append(v)
                self.scene[scene]["lpips"].append(v)
            depth = bool(self.cfg.test.eval_depth and scene in self.eval_depth_scenes)
            if depth:
                row = rows[b:b + 1]
                metrics.eval_depth(output["nerf_depth"][b:b + 1].detach().float(), batch["tar_views"]["depth"][b:b + 1].float(),
                                   row[:, self._NERF_DEPTH:], resize=True)
                metrics.eval_depth(output["mvs_depth"][b:b + 1].detach().float(), batch["tar_gt_ms"]["depth"][-1][b:b + 1].float(),
                                   row[:, self._MVS_DEPTH:], resize=False)
            self._rows.append((scene, (crop[2] - 6) * (crop[3] - 6), depth, self.lpips_weights is not None))

    @property
    def capacity(self) -> int:
        """Frames the device table holds before it grows again (0 before the first device frame)."""
        return 0 if self._table is None else int(self._table.shape[0])

    def collect(self):
        """The frames the device path has enqueued since the last call, onto the host lists: ONE device-to-host copy of their rows,
        then per frame what the numpy path appends in `evaluate`.  `summarize` calls it."""
        if not self._rows:
            return
        table = self._table[:len(self._rows)].cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            for (scene, windows, depth, has_lpips), r in zip(self._rows, table):
                mse = float(r[0] / (3.0 * r[1]))
                row = {"psnr": float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse),
                       "ssim": float(np.mean(r[2:5] / windows))}
                for k, v in row.items():
                    getattr(self, k + "s").append(v)
                    self.scene[scene][k].append(v)
                if has_lpips:
                    self.lpips.append(float(r[self._LPIPS]))
                    self.scene[scene]["lpips"].append(float(r[self._LPIPS]))
                if depth:
                    for tag, o in (("", self._NERF_DEPTH), ("mvs_", self._MVS_DEPTH)):
                        for k, i in (("abs", 0), ("acc_2", 1), ("acc_10", 2)):
                            self.depth[tag + k].append(r[o + i] / r[o + 3])
        self._rows = []

    def evaluate(self, output, batch):
        if self.use_hip_metrics(output, batch):
            return self._evaluate_hip(output, batch)
        B, _, _, H, W = batch["src_views"]["rgb"].shape
        gt = batch["tar_views"]["rgb"].detach().cpu().numpy()
        masks = batch["tar_views"]["mask"].cpu().numpy() >= 1
        pred = output["rgb"].permute(0, 2, 3, 1).detach().clamp(0.0, 1.0).cpu().numpy()
        if self.cfg.test.eval_center:  # LLFF protocol: drop a 10 % border   (reference :41-45)
            ch, cw = int(H * 0.1), int(W * 0.1)
            gt, pred, masks = gt[:, ch:-ch, cw:-cw], pred[:, ch:-ch, cw:-cw], masks[:, ch:-ch, cw:-cw]
        for b in range(B):
            scene = batch["meta"]["scene"][b]
            if getattr(self.cfg, "save_result", False):
                name = "{}_{}_{}.png".format(scene, batch["meta"]["tar_view"][b].item(), batch["meta"]["frame_id"][b].item())
                write_png(os.path.join(self.cfg.result_dir, name), (pred[b] * 255).clip(0, 255).astype(np.uint8))
            m = masks[b]
            g, p = gt[b].copy(), pred[b].copy()
            g[~m], p[~m] = 0.0, 0.0
            row = {"psnr": psnr(g[m], p[m], 1.0), "ssim": ssim(g, p)}
            if self.lpips_weights is not None:   # the plain-torch restatement, on the device the frame came on
                dev = output["rgb"].device
                t = lambda a: torch.from_numpy(a)[None].permute(0, 3, 1, 2).contiguous().float().to(dev)   # fp32 like the weights, whatever the frame was
                row["lpips"] = lpips_torch(t(p), t(g), self._lpips_weights_on(dev))[0].item()
            elif self.loss_fn_vgg is not None:
                t = lambda a: (torch.from_numpy(a)[None].permute(0, 3, 1, 2) - 0.5) * 2.0
                row["lpips"] = self.loss_fn_vgg(t(g).cuda(), t(p).cuda()).item()
            for k, v in row.items():
                getattr(self, k + "s" if k != "lpips" else "lpips").append(v)
                self.scene[scene][k].append(v)
            if self.cfg.test.eval_depth and scene in self.eval_depth_scenes:
                nd, ngt = output["nerf_depth"].cpu().numpy()[b], batch["tar_views"]["depth"].cpu().numpy()[b]
                md, mgt = output["mvs_depth"].cpu().numpy()[b], batch["tar_gt_ms"]["depth"][-1][b].cpu().numpy()
                nd = _resize_bilinear(nd, ngt.shape)
                for tag, d, g_ in (("", nd, ngt), ("mvs_", md, mgt)):
                    valid = g_ != 0.0
                    err = np.abs(d[valid] - g_[valid])
                    self.depth[tag + "abs"].append(err.mean())
                    self.depth[tag + "acc_2"].append((err < 2).mean())
                    self.depth[tag + "acc_10"].append((err < 10).mean())

    def summarize(self):
        self.collect()
        ret = {"psnr": np.mean(self.psnrs), "ssim": np.mean(self.ssims)}
        if self.loss_fn_vgg is not None or self.lpips_weights is not None:
            ret["lpips"] = np.mean(self.lpips)
        print("=" * 30)
        for scene, rows in self.scene.items():
            line = scene.ljust(16) + " psnr: {:.2f} ssim: {:.3f} ".format(np.mean(rows["psnr"]), np.mean(rows["ssim"]))
            if "lpips" in rows:
                line += "lpips:{:.3f}".format(np.mean(rows["lpips"]))
            print(line)
        print("=" * 30)
        print(ret)
        if self.cfg.test.eval_depth:
            for prefix in ("", "mvs_"):
                print({prefix + k: np.mean(self.depth[prefix + k]) for k in ("abs", "acc_2", "acc_10")})
            self.depth = defaultdict(list)
        self._reset()
        if getattr(self.cfg, "save_result", False):
            print("Save visualization results to: {}".format(self.cfg.result_dir))
        return ret

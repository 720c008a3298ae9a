"""LPIPS-VGG per frame from caller-supplied (here: random, seeded) weights, B = 1, a CUDA-resident frame, at 512 x 640 and at
378 x 504 with eval_center (a 304 x 404 crop):
  (a) the HIP path (metrics.eval_lpips -> gdb_eval_lpips): us per frame with a synchronise behind every call, the host time until the
      call returns, and the fraction of the fp32 matrix peak (157.3 TFLOP/s) the thirteen convolutions' FLOPs of the pair make of (a);
  (b) the same frame through the plain-torch restatement (evaluators/gdb_nerf.py lpips_torch: F.conv2d through MIOpen) on the card,
      with its `.item()`;
  (c) frames per second of a --frames loop Network.forward + evaluate + one summarize with every HIP switch on and `eval_lpips`
      with weights, `test.hip_metrics` off (PSNR / SSIM in numpy, LPIPS by (b)) and on (all three enqueued);
  (d) GPU time of every launch of one call at 512 x 640 from a kernel trace: run `rocprofv3 --kernel-trace --output-format csv -d DIR
      -- python tools/bench_lpips.py --trace`, then `--fold "DIR/**/*kernel_trace.csv" --into FILE.json`.
Medians over --iters calls after --warmup.  Prints a JSON object (and writes it to --out).

    python tools/bench_lpips.py [--iters 10] [--warmup 2] [--frames 20] [--out FILE]"""
import argparse, json, os, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_evaluator as be
from gdb_nerf_amd import metrics
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.evaluators import make_evaluator
from gdb_nerf_amd.evaluators.gdb_nerf import lpips_torch

PEAK_F32_MATRIX = 157.3e12
WORKLOADS = {"512 x 640": (512, 640, False), "378 x 504, eval_center": (378, 504, True)}


def weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    w = {}
    for i, (ci, co) in enumerate(metrics.LPIPS_CHANNELS):
        w[f"conv.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        w[f"conv.{i}.bias"] = torch.randn(co, generator=g) * 0.05
    for l, t in enumerate(metrics.LPIPS_TAPS):
        w[f"lin.{l}"] = torch.rand(metrics.LPIPS_CHANNELS[t][1], generator=g)
    return w


def conv_flops(h, w):
    """FLOPs of the thirteen convolutions for the pair of images."""
    total, g = 0, 0
    for i, (ci, co) in enumerate(metrics.LPIPS_CHANNELS):
        if i in (2, 4, 7, 10):
            g += 1
        total += 2 * 9 * ci * co * (h >> g) * (w >> g)
    return 2 * total


LAUNCHES = ["conv.0", "conv.1", "tap.0", "pool.0", "conv.2", "conv.3", "tap.1", "pool.1", "conv.4", "conv.5", "conv.6", "tap.2", "pool.2",
            "conv.7", "conv.8", "conv.9", "tap.3", "pool.3", "conv.10", "conv.11", "conv.12", "tap.4", "finish"]   # gdb_eval_lpips, flags 0


def fold(trace_csv, into):
    """Per launch of one gdb_eval_lpips call at 512 x 640: the median GPU time over the traced calls (after the first two), and per
    convolution the fraction of the fp32 matrix peak; written into the record `into` as "(d) ..."."""
    import csv, glob
    rows = [r for p in glob.glob(trace_csv, recursive=True) for r in csv.DictReader(open(p)) if "k_lpips_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = len(LAUNCHES)
    assert rows and len(rows) % n == 0, (len(rows), n)
    calls = [rows[i:i + n] for i in range(0, len(rows), n)][2:]
    res = json.load(open(into))
    split, g = {}, 0
    for k, name in enumerate(LAUNCHES):
        us = float(np.median([(int(c[k]["End_Timestamp"]) - int(c[k]["Start_Timestamp"])) / 1e3 for c in calls]))
        kern = calls[0][k]["Kernel_Name"].split("(")[0]
        assert ("conv" in kern) == name.startswith("conv") and ("tap" in kern) == name.startswith("tap"), (name, kern)
        split[name] = {"kernel": kern, "median_us": round(us, 1)}
        if name.startswith("conv"):
            i = int(name.split(".")[1])
            g += i in (2, 4, 7, 10)
            ci, co = metrics.LPIPS_CHANNELS[i]
            fl = 2 * 2 * 9 * ci * co * (512 >> g) * (640 >> g)
            split[name].update({"gflop": round(fl / 1e9, 2), "fraction_of_fp32_matrix_peak": round(fl / (us * 1e-6) / PEAK_F32_MATRIX, 3)})
    split["sum_us"] = round(sum(v["median_us"] for v in split.values()), 1)
    res["(d) gpu time per launch of one call at 512 x 640, rocprofv3 --kernel-trace, median of %d calls" % len(calls)] = split
    json.dump(res, open(into, "w"), indent=1)
    print(json.dumps(split, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true", help="only run eval_lpips at 512 x 640 (under rocprofv3 --kernel-trace)")
    ap.add_argument("--fold", help="a rocprofv3 kernel_trace.csv (glob) of a --trace run to add to --into as the per-layer split")
    ap.add_argument("--into")
    args = ap.parse_args()
    if args.fold:
        return fold(args.fold, args.into)
    w = weights()
    path = os.path.join(tempfile.mkdtemp(), "lpips_vgg.pth")
    torch.save(w, path)
    packed = metrics.pack_lpips(w, "cuda")
    if args.trace:
        out, batch = be.frame(512, 640)
        rec = torch.zeros(1, 16, dtype=torch.float64, device="cuda")
        for _ in range(args.warmup + args.iters):
            metrics.eval_lpips(out["rgb"], batch["tar_views"]["rgb"], batch["tar_views"]["mask"], packed, rec[:, 13:], None)
        torch.cuda.synchronize()
        return
    wd = {k: v.cuda() for k, v in metrics.lpips_weights_from(w).items()}
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "frames": args.frames,
           "weights": "random, seeded (no published LPIPS weights are available offline)", "fp32_matrix_peak_tflops": PEAK_F32_MATRIX / 1e12}
    for name, (H, W, center) in WORKLOADS.items():
        out, batch = be.frame(H, W)
        pred, gt, mask = out["rgb"], batch["tar_views"]["rgb"], batch["tar_views"]["mask"]
        ch, cw = (int(H * 0.1), int(W * 0.1)) if center else (0, 0)
        crop = (ch, cw, H - 2 * ch, W - 2 * cw)
        rec = torch.zeros(1, 16, dtype=torch.float64, device="cuda")
        hip = lambda: metrics.eval_lpips(pred, gt, mask, packed, rec[:, 13:], crop)
        keep = (mask >= 1)[:, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]][:, None]
        a = (pred.clamp(0, 1)[:, :, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]] * keep).contiguous()
        b = (gt.permute(0, 3, 1, 2)[:, :, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]] * keep).contiguous()
        vals = []
        r = {"crop (y0, x0, h, w)": crop,
             "(a) hip, eval_lpips + synchronise": be.wall(hip, args.iters, args.warmup, True),
             "(a) hip, eval_lpips until it returns": be.wall(hip, args.iters, args.warmup, False),
             "(b) torch restatement on the card, with .item()": be.wall(lambda: vals.append(lpips_torch(a, b, wd)[0].item()), args.iters, args.warmup, False)}
        torch.cuda.synchronize()
        flops = conv_flops(crop[2], crop[3])
        t = r["(a) hip, eval_lpips + synchronise"]["median_ms"] * 1e-3
        r["conv GFLOP of the pair"] = round(flops / 1e9, 2)
        r["(a) us per frame"] = round(t * 1e6, 1)
        r["(a) fraction of the fp32 matrix peak"] = round(flops / t / PEAK_F32_MATRIX, 4)
        r["values (hip, torch)"] = [float(rec[0, 13].item()), vals[-1]]
        r["workspace MB"] = round(metrics.lpips_workspace_bytes(1, crop[2], crop[3]) / 2 ** 20, 1)
        res[name] = r
    loops = {}
    make_ev = lambda hipm: make_evaluator(make_cfg("configs/dtu_eval.yaml", [
        "test.hip_metrics", str(bool(hipm)), "eval_lpips", "True", "test.lpips_weights", path]))
    for label, hipm in (("hip_metrics off: LPIPS by the torch restatement, .item() per frame", False), ("hip_metrics on: LPIPS enqueued", True)):
        loops[label] = be.loop_fps(hipm, args.frames, make_ev)
    res["(c) loop of Network.forward + evaluate with LPIPS, 512 x 640, every HIP switch on"] = loops
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

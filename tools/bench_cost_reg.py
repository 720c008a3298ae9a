"""The cascade's two cost-regularisation U-Nets (networks/gdb_nerf/cost_reg_net.py) at the stage shapes of a frame: the HIP forward
(costvol.CostReg, gdb_cost_reg) against the PyTorch-ROCm module (MIOpen), random weights with non-trivial BN statistics, B = 1.
configs/dtu_eval.yaml stages: vol_scales [0.125, 0.5], num_depth [64, 8], fpn.feat_dims at the volume levels 32 / 16, base 8.
Per shape: mean wall time per forward over --iters back-to-back calls after --warmup (synchronised, CUDA events), the max
abs difference of the two outputs.  Prints a JSON object.

    python tools/bench_cost_reg.py [--iters 50] [--warmup 10] [--workloads c2,c4]"""
import argparse, json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import costvol
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d

FRAMES = {"c2": (512, 640), "c4": (800, 800)}
STAGES = [("stage0 CostRegNet_small", 2, 32, 64, 0.125), ("stage1 CostRegNet", 3, 16, 8, 0.5)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workloads", default="c2,c4")
    args = ap.parse_args()
    res = {}
    for wl in args.workloads.split(","):
        H0, W0 = FRAMES[wl]
        total = {"hip_ms": 0.0, "torch_ms": 0.0}
        for name, depth, cin, D, scale in STAGES:
            H, W = int(H0 * scale), int(W0 * scale)
            torch.manual_seed(0)
            m = _UNet3d(cin, 8, 8, depth).eval().cuda()
            with torch.no_grad():
                for mod in m.modules():
                    if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                        mod.running_mean.uniform_(-0.1, 0.1)
                        mod.running_var.uniform_(0.8, 1.2)
            cost = torch.rand(1, cin, D, H, W, device="cuda")
            reg = costvol.CostReg(m)
            with torch.no_grad():
                v, p = reg(cost)
                vr, pr = m(cost)
                hip = timed(lambda: reg(cost), args.iters, args.warmup)
                ref = timed(lambda: m(cost), args.iters, args.warmup)
            res[f"{wl} {name} (1, {cin}, {D}, {H}, {W})"] = {
                "hip_ms": round(hip, 4), "torch_ms": round(ref, 4), "speedup": round(ref / hip, 2),
                "max_abs_diff_volume": float((v - vr).abs().max()), "max_abs_diff_prob": float((p - pr).abs().max())}
            total["hip_ms"] += hip; total["torch_ms"] += ref
        res[f"{wl} both U-Nets"] = {k: round(v, 4) for k, v in total.items()}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

"""Times the cost-regularisation U-Nets in training mode: costvol.CostRegTrain (gdb_cost_reg_train +
gdb_cost_reg_train_backward) against the PyTorch module in `.train()` under autograd on the same card, forward + backward, at the two
c2 stage shapes - (1, 32, 64, 64, 80) at depth 2 and (1, 16, 8, 256, 320) at depth 3 - with the largest relative difference of every
gradient between the two sides; and one NetworkWrapper forward + backward at 512 x 640 with `mvs.stage_render` on (the step of DESIGN.md
4.18), for `mvs.hip_cost_reg_train` off and on.  Writes profiles/cost_reg_train/bench.json.

    python tools/bench_cost_reg_train.py [--out FILE] [--kernel-stats DIR [--share-only]] [--no-wrapper]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<what>_<n> -o trace -- python tools/bench_cost_reg_train.py --kernels-only <what> <n>

Call times: device events around a window of at least 0.5 s of back-to-back calls, after a warm-up, the sides alternated in one
process, median of the windows (tools/bench_loss.py).
The U-Nets' share of the step, switch off: kernel time from `rocprofv3 --kernel-trace --stats` runs of their own (tracing slows the
host, so only kernel durations are read from them).  `--kernels-only step N` runs N wrapper steps with the switch off, `--kernels-only
step_hip N` with it on.  Each is traced at two N, after one untraced run that lets the convolution library finish its tuning; the
difference of the summed kernel time over the difference in N is the per-step kernel time without start-up.  Everything but the
U-Nets is the same work on both sides, so the PyTorch U-Nets' kernel time inside the step is (off - on) + the k_crt_* kernels of the
on side.  `--kernel-stats DIR` merges every *kernel_stats.csv below DIR/<what>_<n>/."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_loss import alternate  # noqa: E402
from gdb_nerf_amd import costvol, synthetic  # noqa: E402
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d  # noqa: E402

SHAPES = {"c2_stage0_d2": (2, 32, 8, 8, (1, 32, 64, 64, 80)), "c2_stage1_d3": (3, 16, 8, 8, (1, 16, 8, 256, 320))}


def draw(depth, cin, c, cout, shape, seed=0):
    torch.manual_seed(seed)
    m = _UNet3d(cin, cout, c, depth)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.normal_(0.0, 0.3)
    B, _, D, H, W = shape
    return m.cuda().train(), torch.randn(shape).abs().cuda(), torch.randn(B, cout, D, H, W).cuda(), torch.randn(B, D, H, W).cuda()


def unet_sides(name):
    depth, cin, c, cout, shape = SHAPES[name]
    m, x, gv, gp = draw(depth, cin, c, cout, shape)
    reg = costvol.CostRegTrain(m)

    def torch_fwd_bwd():
        m.zero_grad(set_to_none=True)
        vol, prob = m(x)
        ((vol * gv).sum() + (prob * gp).sum()).backward()

    def hip_fwd_bwd():
        m.zero_grad(set_to_none=True)
        vol, prob = reg(x)
        ((vol * gv).sum() + (prob * gp).sum()).backward()

    def hip_fwd():
        with torch.no_grad():
            reg(x)

    def torch_fwd():
        with torch.no_grad():
            m(x)

    # the two sides' gradients once, before anything is timed
    torch_fwd_bwd()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    hip_fwd_bwd()
    diff = {n: float((p.grad - ref[n]).abs().max() / ref[n].abs().max()) for n, p in m.named_parameters()}
    return {"hip_forward_backward": hip_fwd_bwd, "torch_forward_backward": torch_fwd_bwd, "hip_forward": hip_fwd, "torch_forward": torch_fwd}, diff


def wrapper_sides(switches=(False, True), Ho=512, Wo=640):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    from gdb_nerf_amd.train.trainers import make_wrapper
    fr = synthetic.make_frame(Ho, Wo, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"]), "rgb": torch.rand(1, Ho, Wo, 3, device="cuda")},
             "near_far": t(fr["near_far"]), "tar_gt_ms": {"rgb": [torch.rand(1, Ho // 8, Wo // 8, 3, device="cuda")]}}
    sides = {}
    for on in switches:
        cfg = make_cfg("configs/dtu_pretrain.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "mvs.hip_stage_render", "True",
                                                     "mvs.hip_cost_reg_train", str(on), "train.photometric_weights", "[1.0, 0.1, 0.0]"])
        torch.manual_seed(109)
        net = make_network(cfg).eval().cuda()
        net.depth_net.train()        # the stage images, and the U-Nets' batch statistics, belong to training mode
        wrapper = make_wrapper(cfg, net)
        wrapper.training = True

        def step(wrapper=wrapper):
            wrapper.zero_grad(set_to_none=True)
            wrapper(batch)[1].backward()
        sides["wrapper_hip_cost_reg_train" if on else "wrapper_torch_cost_reg"] = step
    return sides


def kernels_only(what, n):
    fn = list(wrapper_sides((what == "step_hip",)).values())[0]
    for _ in range(n):
        fn()
    torch.cuda.synchronize()


def kernel_totals(root):
    """{"step_3": [all kernels' ns, the k_crt_* kernels' ns], ...} from the traced runs below `root`."""
    out = {}
    for d in sorted(glob.glob(os.path.join(root, "step*_*"))):
        total = crt = 0.0
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                ns = float(row.get("TotalDurationNs") or float(row["Calls"]) * float(row["AverageNs"]))
                total += ns
                if "k_crt_" in (row.get("Name") or row.get("KernelName") or ""):
                    crt += ns
        if total:
            out[os.path.basename(d)] = [total, crt]
    return out


def share(totals):
    """Per step, from the two trace lengths of each side: everything but the U-Nets is the same work with the switch off and on, so
    the PyTorch U-Nets' kernel time is (off - on) + the k_crt_* kernels' time of the on side."""
    per = {}
    for what in ("step", "step_hip"):
        ns = sorted(int(k.rsplit("_", 1)[1]) for k in totals if k.rsplit("_", 1)[0] == what)
        if len(ns) < 2:
            return None
        lo, hi = f"{what}_{ns[0]}", f"{what}_{ns[-1]}"
        per[what] = [(totals[hi][i] - totals[lo][i]) / (ns[-1] - ns[0]) / 1e6 for i in (0, 1)]
    off, on, crt = per["step"][0], per["step_hip"][0], per["step_hip"][1]
    return {"step_kernel_ms_switch_off": off, "step_kernel_ms_switch_on": on, "hip_unets_kernel_ms_in_step": crt,
            "torch_unets_kernel_ms_in_step": off - on + crt, "torch_unets_share_of_step_kernel_time": (off - on + crt) / off,
            "traced_totals_ns": totals}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_reg_train", "bench.json"))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--kernels-only", nargs=2, default=None, metavar=("WHAT", "N"), help="step | step_hip, and the steps, for a profiler run")
    ap.add_argument("--no-wrapper", action="store_true")
    ap.add_argument("--share-only", action="store_true", help="add the traced share (--kernel-stats) to an existing --out file; no GPU work")
    args = ap.parse_args()
    if args.share_only:
        res = json.load(open(args.out))
        res["unets_share_switch_off"] = share(kernel_totals(args.kernel_stats))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["unets_share_switch_off"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_cost_reg_train.py measures on the GPU; none is available")
    if args.kernels_only:
        kernels_only(args.kernels_only[0], int(args.kernels_only[1]))
        return
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in SHAPES:
        sides, diff = unet_sides(name)
        r = alternate(sides)
        r["ratio_torch_over_hip_forward_backward"] = r["torch_forward_backward"]["ms"] / r["hip_forward_backward"]["ms"]
        r["ratio_torch_over_hip_forward"] = r["torch_forward"]["ms"] / r["hip_forward"]["ms"]
        r["gradient_max_relative_difference"] = diff
        r["gradient_max_relative_difference_worst"] = max(diff.values())
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
    if not args.no_wrapper:
        res["network_wrapper_512x640_forward_backward"] = alternate(wrapper_sides(), rounds=3)
        print(json.dumps(res["network_wrapper_512x640_forward_backward"]), flush=True)
    if args.kernel_stats:
        res["unets_share_switch_off"] = share(kernel_totals(args.kernel_stats))
        print(json.dumps(res["unets_share_switch_off"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

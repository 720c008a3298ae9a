"""Times the decoder in training mode: decoder_train.DecodeTrainFunction (gdb_decoder_train_forward +
gdb_decoder_train_backward) against the PyTorch module under autograd on the same card, at the c2 bundle map (B = 1, 256 x 320, three
blocks) and at the F7 shape (1, 32, 48): forward + backward, the forward alone, the device pack alone, with the largest relative
difference of every gradient between the two sides and the number of ReLU mask elements on which the two forwards differ; and one NetworkWrapper forward + backward at 512 x 640 with
`nerf.hip_decoder_train` off (the path before this switch existed) and on, in two configurations (WRAPPER_CONFIGS).  Writes profiles/decoder_train/bench.json.

    python tools/bench_decoder_train.py [--out FILE] [--kernel-stats DIR [--stats-only]] [--no-wrapper | --wrapper-only]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bench_decoder_train.py --kernels-only N

Call times: device events around a window of at least 0.5 s of back-to-back calls, after a warm-up, the sides alternated in one
process, median of the windows (tools/bench_loss.py).  Kernel time per kernel: a `rocprofv3 --kernel-trace --stats` run of its own of
N forward + backward calls of the Function at the c2 shape (`--kernels-only N`; tracing slows the host, so only kernel durations are
read from it); `--kernel-stats DIR` merges every *kernel_stats.csv below DIR into the result, per call."""
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
from gdb_nerf_amd import synthetic  # noqa: E402
from gdb_nerf_amd.decoder_train import DecodeTrainFunction, DecoderTrain, decoder_params  # noqa: E402
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder  # noqa: E402

SHAPES = {"c2_1x256x320_L3": (1, 256, 320, 3), "f7_1x32x48_L3": (1, 32, 48, 3)}
Q = 39
FORWARD_GFLOP = lambda B, H, W, L: 2e-9 * B * H * W * 9 * (27 * 64 + L * (64 * 32 + 96 * 32 + 128 * 64) + 64 * 12)


def decoder_sides(name):
    B, H, W, L = SHAPES[name]
    torch.manual_seed(0)
    m = Decoder(27, 3, 64, L, 2).cuda().train()
    rows = torch.randn(B * H * W, Q, device="cuda").requires_grad_()
    g = torch.randn(B, 3, 2 * H, 2 * W, device="cuda")
    dt = DecoderTrain(m)
    params = decoder_params(m)

    def zero():
        m.zero_grad(set_to_none=True)
        rows.grad = None

    def torch_fwd_bwd():
        zero()
        (m(rows[:, 12:].view(B, H, W, 27).permute(0, 3, 1, 2)) * g).sum().backward()

    def hip_fwd_bwd():
        zero()
        (DecodeTrainFunction.apply(dt, rows, B, H, W, *params) * g).sum().backward()

    def hip_backward_call():   # the library call alone, on the saved buffer of the last forward
        dt.backward(rows.detach(), g)

    def hip_fwd():
        with torch.no_grad():
            dt.forward(rows.detach(), B, H, W)

    def torch_fwd():
        with torch.no_grad():
            m(rows[:, 12:].view(B, H, W, 27).permute(0, 3, 1, 2))

    def hip_pack():
        dt._key = None
        dt.pack()

    # the module's ReLU masks on this input, for the comparison with the masks the HIP forward saved: a pre-activation that the two
    # forwards round to different sides of zero flips one mask element, and every gradient upstream of it differs by that element's term
    masks, hooks = {}, []
    for i, blk in enumerate(m.blocks):
        for j, conv in enumerate((blk.conv1, blk.conv2)):
            hooks.append(conv.register_forward_hook(lambda mod, inp, out, key=(i, j): masks.__setitem__(key, (out > 0).permute(0, 2, 3, 1))))
    torch_fwd_bwd()
    for h in hooks:
        h.remove()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    ref["rows"] = rows.grad.clone()
    hip_fwd_bwd()
    got = {n: p.grad for n, p in m.named_parameters()}
    got["rows"] = rows.grad
    diff = {n: float((got[n] - ref[n]).abs().max() / ref[n].abs().max()) for n in ref}
    acts = dt.activations()
    flips = {f"blocks.{i}.conv{j + 1}": int((masks[(i, j)] != (acts[f"ab.{i}"][..., 32 * j:32 * j + 32] > 0)).sum()) for (i, j) in masks}
    sides = {"hip_forward_backward": hip_fwd_bwd, "torch_forward_backward": torch_fwd_bwd, "hip_forward": hip_fwd, "torch_forward": torch_fwd,
             "hip_backward_call": hip_backward_call, "hip_device_pack": hip_pack}
    return sides, diff, flips


# the two steps timed: "plain" = `hot_path: mirrors` and nothing else on the HIP library in training mode (every other module under
# autograd); "hip_training" = the step of DESIGN.md 4.19 - the stage render and the cost-regularisation U-Nets' train mode on the HIP
# library too
WRAPPER_CONFIGS = {"plain": [], "hip_training": ["mvs.hip_stage_render", "True", "mvs.hip_cost_reg_train", "True"]}


def wrapper_sides(config="plain", switches=(False, True), Ho=512, Wo=640):
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
        cfg = make_cfg("configs/dtu_pretrain.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "nerf.hip_decoder_train", str(on),
                                                     "train.photometric_weights", "[1.0, 0.1, 0.0]", *WRAPPER_CONFIGS[config]])
        torch.manual_seed(109)
        net = make_network(cfg).train().cuda()
        wrapper = make_wrapper(cfg, net)
        wrapper.training = True

        def step(wrapper=wrapper):
            wrapper.zero_grad(set_to_none=True)
            wrapper(batch)[1].backward()
        sides["wrapper_hip_decoder_train" if on else "wrapper_torch_decoder"] = step
    return sides


def kernels_only(n):
    sides, _, _ = decoder_sides("c2_1x256x320_L3")
    for _ in range(n):
        sides["hip_forward_backward"]()
    torch.cuda.synchronize()


def kernel_stats(root, calls):
    """{kernel: ms per forward + backward call} of the library's kernels, from the traced run below `root`."""
    out = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or float(row["Calls"]) * float(row["AverageNs"]))
            if "k_dect_" in name or "k_conv16" in name or "k_se_gate" in name:
                key = name.split("(")[0]
                e = out.setdefault(key, {"ms_per_call": 0.0, "launches_per_call": 0.0})
                e["ms_per_call"] += ns / 1e6 / calls
                e["launches_per_call"] += float(row["Calls"]) / calls
    return out


def wrappers(res):
    for config in WRAPPER_CONFIGS:
        key = "network_wrapper_512x640_forward_backward" + ("" if config == "plain" else "_" + config)
        res[key] = alternate(wrapper_sides(config), rounds=3)
        res[key]["config"] = WRAPPER_CONFIGS[config]
        print(config, json.dumps(res[key]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_train", "bench.json"))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--kernel-stats-calls", type=int, default=0, help="the N of the traced --kernels-only run")
    ap.add_argument("--kernels-only", type=int, default=0, metavar="N", help="N forward + backward calls at the c2 shape, for a profiler run")
    ap.add_argument("--no-wrapper", action="store_true")
    ap.add_argument("--wrapper-only", action="store_true", help="time the NetworkWrapper steps alone and add them to an existing --out file")
    ap.add_argument("--stats-only", action="store_true", help="add the traced kernel times (--kernel-stats) to an existing --out file; no GPU work")
    args = ap.parse_args()
    if args.stats_only:
        res = json.load(open(args.out))
        res["kernel_ms_per_forward_backward_c2"] = kernel_stats(args.kernel_stats, args.kernel_stats_calls)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["kernel_ms_per_forward_backward_c2"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder_train.py measures on the GPU; none is available")
    if args.kernels_only:
        kernels_only(args.kernels_only)
        return
    if args.wrapper_only:
        res = json.load(open(args.out))
        wrappers(res)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in SHAPES:
        sides, diff, flips = decoder_sides(name)
        r = alternate(sides)
        r["ratio_torch_over_hip_forward_backward"] = r["torch_forward_backward"]["ms"] / r["hip_forward_backward"]["ms"]
        r["ratio_torch_over_hip_forward"] = r["torch_forward"]["ms"] / r["hip_forward"]["ms"]
        r["forward_gflop"] = FORWARD_GFLOP(*SHAPES[name])
        r["gradient_max_relative_difference"] = diff
        r["gradient_max_relative_difference_worst"] = max(diff.values())
        r["relu_mask_elements_that_differ_from_the_modules"] = flips
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
    if not args.no_wrapper:
        wrappers(res)
    if args.kernel_stats:
        res["kernel_ms_per_forward_backward_c2"] = kernel_stats(args.kernel_stats, args.kernel_stats_calls)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Times the optimiser step of the training loop on the dtu_pretrain network's trainable tensors with random gradients:

  (a) reference_recipe   clip_grad_value_ + torch.optim.Adam, ONE PARAM GROUP PER PARAMETER - what the reference's make_optimizer builds
  (b) one_group_foreach  the same tensors in one group (torch's multi-tensor path)
  (c) one_group_fused    one group with fused=True, if this torch build accepts it on the card (else recorded as unavailable)
  (d) hip_adam           optim.HipAdam, one group per parameter, clip inside the one library call (gdb_adam_step)

    python tools/bench_optimizer.py [--out FILE] [--no-wrapper] [--launches "DIR/**/*kernel_trace.csv"]
    rocprofv3 --kernel-trace --output-format csv -d DIR/<arm> -- python tools/bench_optimizer.py --kernels-only <arm>

Per arm: GPU time of a step (device events around a window of at least 0.5 s of back-to-back steps, after a warm-up, the arms
alternated in one process, median / min / max of the windows) and the host time of a step (host clock around the same loop before
its synchronise: the enqueue).  The yardstick is (a).  Launches per step come from a kernel trace in a run of its own per arm
(`--kernels-only`: a few steps, a marker launch, STEPS steps, a marker launch; `--launches` counts the kernels between the markers
and merges the counts into the output file).  The last part is the NetworkWrapper step of tools/bench_costvol_backward.py at
512 x 640 (forward + backward, `mvs.cost_volume_grad` off) followed by (a) and by (d): steps per second."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gdb_nerf_amd.configs import make_cfg  # noqa: E402
from gdb_nerf_amd.optim import HipAdam  # noqa: E402

CLIP = 40.0
ARMS = ("reference_recipe", "one_group_foreach", "one_group_fused", "hip_adam")
STEPS = 20          # steps between the two markers of a --kernels-only run
MARKER = "k_smooth_l1"


def tensors(seed=3):
    """Trainable tensors of the dtu_pretrain network as fresh CUDA leaves per arm (same values), each with a random gradient."""
    from gdb_nerf_amd.networks import make_network
    cfg = make_cfg("configs/dtu_pretrain.yaml")
    torch.manual_seed(seed)
    net = make_network(cfg)
    return [p.detach().clone() for p in net.parameters() if p.requires_grad]


def make_arm(name, base, cfg):
    g = torch.Generator(device="cuda").manual_seed(17)
    params = [torch.nn.Parameter(t.cuda().clone()) for t in base]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 20          # a few percent beyond the clip
    kw = dict(lr=cfg.train.lr, weight_decay=cfg.train.weight_decay, eps=cfg.train.eps)
    per_param = [{"params": [p], **kw} for p in params]
    if name == "reference_recipe":
        opt = torch.optim.Adam(per_param, cfg.train.lr, weight_decay=cfg.train.weight_decay, eps=cfg.train.eps)
    elif name == "one_group_foreach":
        opt = torch.optim.Adam(params, foreach=True, **kw)
    elif name == "one_group_fused":
        opt = torch.optim.Adam(params, fused=True, **kw)
    else:
        opt = HipAdam(per_param, cfg.train.lr, weight_decay=cfg.train.weight_decay, eps=cfg.train.eps, clip_value=CLIP)
    if name == "hip_adam":
        return opt.step, params
    clip = torch.nn.utils.clip_grad_value_

    def step():
        clip(params, CLIP)
        opt.step()
    return step, params


def window(fn, iters):
    """(GPU ms per call, host ms per call) of `iters` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e3 / iters
    b.synchronize()
    return a.elapsed_time(b) / iters, host


def alternate(sides, min_window_s=0.5, rounds=5):
    iters = {}
    for name, fn in sides.items():
        window(fn, 10)
        iters[name] = max(10, int(min_window_s * 1e3 / max(window(fn, 20)[0], 1e-4)) + 1)
    got = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            got[name].append(window(fn, iters[name]))
    out = {}
    for name, v in got.items():
        gpu, host = [x[0] for x in v], [x[1] for x in v]
        out[name] = {"gpu_ms": statistics.median(gpu), "gpu_min_ms": min(gpu), "gpu_max_ms": max(gpu), "host_ms": statistics.median(host),
                     "host_min_ms": min(host), "host_max_ms": max(host), "calls_per_window": iters[name]}
    return out


def build_arms(cfg):
    base = tensors()
    arms, unavailable = {}, {}
    for name in ARMS:
        try:
            step, params = make_arm(name, base, cfg)
            step()                      # creates the state; a torch build without the fused kernel on this card refuses here or above
            torch.cuda.synchronize()
            arms[name] = step
        except (RuntimeError, ValueError, TypeError) as e:
            if name != "one_group_fused":
                raise
            unavailable[name] = str(e).splitlines()[0][:200]
    return arms, unavailable, base


def kernels_only(name, cfg):
    """For a kernel trace: warm-up steps, a marker launch, STEPS steps, a marker launch."""
    from gdb_nerf_amd import losses
    step, _ = make_arm(name, tensors(), cfg)
    z = torch.zeros(64, device="cuda")
    for _ in range(3):
        step()
    losses.smooth_l1_masked(z, z, z + 1)
    for _ in range(STEPS):
        step()
    losses.smooth_l1_masked(z, z, z + 1)
    torch.cuda.synchronize()


def count_launches(pattern):
    """{arm: {launches_per_step, kernels: {name: per step}}} from the kernel_trace.csv files matching `pattern` (the arm is the name of a
    directory on the file's path)."""
    out = {}
    for path in glob.glob(pattern, recursive=True):
        arm = next((a for a in ARMS if a in path.split(os.sep)), None)
        if arm is None:
            continue
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
        if len(marks) < 2:
            continue
        inside = [r["Kernel_Name"].split("(")[0] for r in rows[marks[-2] + 1:marks[-1]] if MARKER not in r["Kernel_Name"] and "k_loss_finish" not in r["Kernel_Name"]]
        names = {}
        for k in inside:
            names[k] = names.get(k, 0) + 1
        out[arm] = {"launches_per_step": len(inside) / STEPS, "kernels_per_step": {k[:120]: v / STEPS for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:8]}}
    return out


def wrapper_steps(cfg):
    """The NetworkWrapper forward + backward at 512 x 640 followed by arm (a) / arm (d) on the network's own parameters."""
    from bench_costvol_backward import wrapper_sides
    from gdb_nerf_amd.train.optimizer import make_optimizer
    fwd_bwd = wrapper_sides()["wrapper_cost_volume_grad_off"]
    wrapper = fwd_bwd.__defaults__[0]
    sides = {"forward_backward_only": fwd_bwd}
    for name, hip in (("then_reference_recipe", False), ("then_hip_adam", True)):
        c = make_cfg("configs/dtu_pretrain.yaml", ["train.hip_optimizer", str(hip)])
        opt = make_optimizer(c, wrapper.net)
        params = list(wrapper.parameters())

        def step(opt=opt, hip=hip, params=params):
            fwd_bwd()
            if not hip:
                torch.nn.utils.clip_grad_value_(params, CLIP)
            opt.step()
        sides[name] = step
    r = alternate(sides, rounds=3)
    for v in r.values():
        v["steps_per_second"] = 1e3 / v["gpu_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer", "bench.json"))
    ap.add_argument("--no-wrapper", action="store_true")
    ap.add_argument("--kernels-only", default="", choices=("",) + ARMS)
    ap.add_argument("--launches", default="", help="glob of kernel_trace.csv files of --kernels-only runs: count and merge into --out")
    args = ap.parse_args()
    if args.launches:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["launches"] = count_launches(args.launches)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(res["launches"], indent=1))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py measures on the GPU; none is available")
    cfg = make_cfg("configs/dtu_pretrain.yaml")
    if args.kernels_only:
        kernels_only(args.kernels_only, cfg)
        return
    arms, unavailable, base = build_arms(cfg)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "tensors": len(base), "elements": sum(t.numel() for t in base),
           "median_numel": int(statistics.median(t.numel() for t in base)), "clip_value": CLIP, "arms": alternate(arms), "unavailable": unavailable}
    a, d = res["arms"]["reference_recipe"], res["arms"]["hip_adam"]
    res["acceptance"] = {"gpu_time_hip_max_below_reference_min": d["gpu_max_ms"] < a["gpu_min_ms"],
                         "host_time_hip_max_below_reference_min": d["host_max_ms"] < a["host_min_ms"],
                         "gpu_ratio_reference_over_hip": a["gpu_ms"] / d["gpu_ms"], "host_ratio_reference_over_hip": a["host_ms"] / d["host_ms"]}
    print(json.dumps(res, indent=1), flush=True)
    if not args.no_wrapper:
        res["network_wrapper_512x640_step"] = wrapper_steps(cfg)
        print(json.dumps(res["network_wrapper_512x640_step"], indent=1), flush=True)
    if os.path.exists(args.out):   # keep the launch counts of an earlier --launches
        old = json.load(open(args.out))
        if "launches" in old:
            res["launches"] = old["launches"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

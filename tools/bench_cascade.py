"""The depth net as one library call per stage (mvs.hip_cascade) against the same net with the switch off, every other HIP switch on
(mvs.hip_cost_reg, fpn.hip_feature_net), at DTU eval 512 x 640 with 3 source views and random-init weights.

    python tools/bench_cascade.py [--rounds R] [--iters N]    # timing: JSON on stdout
    python tools/bench_cascade.py --one-forward on|off         # one warmed DepthNet.forward between two markers, for a kernel trace

Timing: the two configurations ALTERNATE in one process, R rounds of N forwards each after a warm-up of both; a round's figure
is the host clock around N forwards ending in a device synchronise, divided by N.  Reported per configuration: the median over
the rounds and the spread (min, max) of the round means, for Network.forward and for DepthNet.forward alone (its inputs, the
feature pyramid, computed once).  With the switch off the code that runs is what ran before the switch existed."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--one-forward", choices=("on", "off"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_cascade.py measures on the GPU; none is visible")

fr = synthetic.make_frame(512, 640, V=3, seed=0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
         "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}
COMMON = ["mvs.hip_cost_reg", "True", "fpn.hip_feature_net", "True", "nerf.reuse_outputs", "True"]


def make(cascade):
    torch.manual_seed(0)
    return make_network(make_cfg("configs/dtu_eval.yaml", COMMON + ["mvs.hip_cascade", str(cascade)])).eval().cuda()


nets = {"off": make(False), "on": make(True)}
src = batch["src_views"]["rgb"]
with torch.no_grad():
    ms = [f.unflatten(0, src.shape[:2]) for f in nets["off"].feature_net(src.flatten(0, 1))]
dn_args = (src, ms, batch["src_views"]["extrinsics"], batch["src_views"]["intrinsics"], batch["tar_views"]["extrinsics"],
           batch["tar_views"]["intrinsics"], batch["near_far"])
runs = {"network": lambda n: n(batch), "depth_net": lambda n: n.depth_net(*dn_args)}

if args.one_forward:
    n = nets[args.one_forward]
    with torch.no_grad():
        for _ in range(3):
            runs["depth_net"](n)
        torch.cuda.synchronize()
        # the traced forward sits between two launches of a kernel that appears nowhere else in it (a 7-element fill)
        mark = torch.empty(7, device="cuda")
        mark.fill_(1.0); runs["depth_net"](n); mark.fill_(2.0)
        torch.cuda.synchronize()
    sys.exit(0)

res = {}
with torch.no_grad():
    for what, run in runs.items():
        for n in nets.values():
            for _ in range(8):
                run(n)
        torch.cuda.synchronize()
        rounds = {"off": [], "on": []}
        for _ in range(args.rounds):
            for key, n in nets.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.iters):
                    run(n)
                torch.cuda.synchronize(); rounds[key].append(1e3 * (time.perf_counter() - t0) / args.iters)
        res[what] = {key: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                           "rounds_ms": [round(x, 4) for x in v]} for key, v in rounds.items()}
        res[what]["on_minus_off_ms_median"] = round(res[what]["on"]["ms_median"] - res[what]["off"]["ms_median"], 4)
    # same seeded weights on both sides: the depth the two paths hand to the hot path, at the size timed
    a, b = nets["off"].depth_net(*dn_args), nets["on"].depth_net(*dn_args)
    res["max_abs_final_depth_on_vs_off"] = float((a[0][-1] - b[0][-1]).abs().max())
    res["max_abs_final_range_on_vs_off"] = float((a[1][-1] - b[1][-1]).abs().max())
res["protocol"] = {"rounds": args.rounds, "iters_per_round": args.iters, "frame": "512x640, 3 views", "alternating": True}
print(json.dumps(res, indent=1))

"""The evaluator per frame (evaluators/gdb_nerf.py) at c2 (512 x 640) and c5 (1200 x 1600), B = 1, a CUDA-resident frame:
  (a) wall time of evaluate() on the numpy path (test.hip_metrics off: the code path before the switch existed), synchronised;
  (b) wall time of evaluate() with test.hip_metrics on: the host time until the call returns (the enqueue), and with a synchronise
      behind every call (enqueue + the kernels);
  (c) GPU time of the launches of (b) from a kernel trace: run `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
      python tools/bench_evaluator.py --trace c2|c5`, then `--fold DIR/.../*kernel_stats.csv --into FILE.json --label c2|c5`;
  (d) frames per second of a --frames loop Network.forward + evaluate + one summarize with every HIP switch on (512 x 640, 3 source
      views, random weights), with the switch off and on.
Medians over --iters calls after --warmup.  numpy's thread pool is whatever the environment gives it (OMP_NUM_THREADS is left alone).
Prints a JSON object (and writes it to --out).

    python tools/bench_evaluator.py [--iters 20] [--warmup 3] [--frames 50] [--out FILE] [--baseline-commit HASH] [--commit HASH]"""
import argparse, csv, glob, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.evaluators import make_evaluator
from gdb_nerf_amd.networks import make_network

WORKLOADS = {"c2": (512, 640), "c5": (1200, 1600)}
HIP_NETWORK = ["mvs.hip_cost_reg", "True", "fpn.hip_feature_net", "True", "nerf.reuse_outputs", "True"]


def frame(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(1, H, W, 3, generator=g)
    pred = (gt + 0.1 * torch.randn(1, H, W, 3, generator=g)).permute(0, 3, 1, 2).contiguous()
    mask = (torch.rand(1, H, W, generator=g) >= 0.3).float()
    batch = {"src_views": {"rgb": torch.zeros(1, 3, 3, H, W)}, "tar_views": {"rgb": gt.cuda(), "mask": mask.cuda()},
             "meta": {"scene": ["scan1"], "tar_view": torch.zeros(1, dtype=torch.long), "frame_id": torch.zeros(1, dtype=torch.long)}}
    return {"rgb": pred.cuda()}, batch


def evaluator(hip):
    return make_evaluator(make_cfg("configs/dtu_eval.yaml", ["test.hip_metrics", str(bool(hip))]))


def wall(fn, iters, warmup, sync):
    """Median and spread (ms) of the host time of fn(); with `sync` the device is drained inside the timed window."""
    ts = []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = np.array(ts[warmup:])
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}


def loop_fps(hip, frames, make_ev=None):
    """Network.forward + evaluate per frame, one summarize at the end: wall clock from the first forward to summarize's return.
    `make_ev(hip)`: another evaluator factory than `evaluator` (tools/bench_lpips.py: LPIPS on)."""
    fr = synthetic.make_frame(512, 640, V=3, seed=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.manual_seed(0)
    net = make_network(make_cfg("configs/dtu_eval.yaml", HIP_NETWORK)).eval().cuda()
    g = torch.Generator().manual_seed(1)
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"]), "rgb": torch.rand(1, 512, 640, 3, generator=g).cuda(),
                           "mask": torch.ones(1, 512, 640).cuda()},
             "near_far": t(fr["near_far"]),
             "meta": {"scene": ["scan1"], "tar_view": torch.zeros(1, dtype=torch.long), "frame_id": torch.zeros(1, dtype=torch.long)}}
    ev = (make_ev or evaluator)(hip)
    out = []
    with torch.no_grad():
        for rep in range(3):   # the first repetition warms MIOpen, the library and the allocator; the median of the rest is reported
            n = frames if rep else 5
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ret, _, _ = net(batch)
                ev.evaluate(ret, batch)
            sys.stdout, keep = open(os.devnull, "w"), sys.stdout
            try:
                ev.summarize()
            finally:
                sys.stdout.close(); sys.stdout = keep
            torch.cuda.synchronize()
            if rep:
                out.append(n / (time.perf_counter() - t0))
        net_ms = wall(lambda: net(batch), 10, 2, True)["median_ms"]
    return {"fps": round(float(np.median(out)), 2), "fps_runs": [round(x, 2) for x in out], "network_forward_ms": net_ms}


def fold(stats_csv, into, label):
    res = json.load(open(into))
    rows = [r for p in glob.glob(stats_csv) for r in csv.DictReader(open(p)) if "k_eval_" in r["Name"]]
    res.setdefault("(c) gpu time of the launches, rocprofv3 --kernel-trace --stats", {})[label] = {
        r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                                  "max_us": round(float(r["MaxNs"]) / 1e3, 2)} for r in rows}
    json.dump(res, open(into, "w"), indent=1)
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--baseline-commit", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--trace", nargs="?", const="c2", help="only run evaluate() with the switch on at this workload (under rocprofv3)")
    ap.add_argument("--fold", help="a rocprofv3 kernel_stats.csv (glob) to add to --into as (c)")
    ap.add_argument("--into")
    ap.add_argument("--label", default="c2", help="the workload the folded trace ran")
    args = ap.parse_args()
    if args.fold:
        return fold(args.fold, args.into, args.label)
    if args.trace:
        out, batch = frame(*WORKLOADS[args.trace])
        ev = evaluator(True)
        for _ in range(args.warmup + args.iters):
            ev.evaluate(out, batch)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "frames": args.frames,
           "baseline_commit": args.baseline_commit, "build_commit": args.commit,
           "host_threads": {"OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"), "torch": torch.get_num_threads()}}
    for wl, (H, W) in WORKLOADS.items():
        out, batch = frame(H, W)
        off, on = evaluator(False), evaluator(True)
        assert on.use_hip_metrics(out, batch) and not off.use_hip_metrics(out, batch)
        r = {"(a) numpy path, evaluate() wall": wall(lambda: off.evaluate(out, batch), args.iters, args.warmup, True),
             "(b) hip_metrics, evaluate() until it returns": wall(lambda: on.evaluate(out, batch), args.iters, args.warmup, False),
             "(b) hip_metrics, evaluate() + synchronise": wall(lambda: on.evaluate(out, batch), args.iters, args.warmup, True)}
        sys.stdout, keep = open(os.devnull, "w"), sys.stdout
        try:
            a, b = off.summarize(), on.summarize()
        finally:
            sys.stdout.close(); sys.stdout = keep
        r["summaries (numpy, hip)"] = {k: [float(a[k]), float(b[k])] for k in a}
        res[f"{wl} ({H} x {W})"] = r
    res["(d) loop of Network.forward + evaluate, c2, every HIP switch on"] = {"numpy path": loop_fps(False, args.frames),
                                                                             "hip_metrics": loop_fps(True, args.frames)}
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

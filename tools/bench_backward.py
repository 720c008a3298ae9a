"""Time of the backward entries at V = 3, on the samples of the c2 frame (512 x 640, S_max 3 adaptive, seeded synthetic: every sample
engine.sample -> encode yields) and on its first 65,537 samples:
  gdb_mlp_backward, gdb_render_weights_backward, gdb_accumulate_backward; beside them the forward gdb_mlp; and torch autograd
  (forward + backward, and the backward alone) of a plain-torch restatement of the same MLP on the same card.
Medians over --iters calls after --warmup, a synchronise behind every call (hipEvent times).  No time is fixed in advance: the record
holds all figures and the ratio backward / torch autograd backward.

    python tools/bench_backward.py [--iters 20] [--warmup 3] [--out profiles/backward/bench_backward.json]"""
import argparse, json, os, sys
import numpy as np, torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import HotPathEngine

FRAME_KEYS = ("src_images", "img_feat", "feat_volume", "depth_range", "vol_range", "src_exts", "src_ints", "tar_ext", "tar_int", "near_far")


def torch_mlp(w, vox, x):
    """nerf.py:58-115 in plain torch ops (feat_dim 16, viewdir_agg)."""
    lin = lambda n, t: F.linear(t, w[n + ".weight"], w[n + ".bias"])
    f = x[..., -23:]
    g = f[..., :19] + F.relu(lin("view_fc.0", f[..., 19:]))
    var, mean = torch.var_mean(g, dim=0, keepdim=True)
    G = F.relu(lin("global_fc.0", torch.cat((g, var.expand_as(g), mean.expand_as(g)), -1)))
    a = torch.softmax(F.relu(lin("agg_w_fc.0", G)), 0)
    h = torch.cat((vox, F.relu(lin("fc.0", (G * a).sum(0)))), -1)
    xh = F.relu(lin("lr0.0", h))
    sigma = F.softplus(lin("sigma.0", xh))[:, 0]
    V = x.shape[0]
    wi = torch.cat((xh[None].expand(V, -1, -1), h[None].expand(V, -1, -1), f), -1)
    wv = torch.softmax(F.relu(lin("weight.2", F.relu(lin("weight.0", wi)))), 0)
    return sigma, torch.cat(((x[..., :-4] * wv).sum(0), F.relu(lin("feat_head.0", xh))), -1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backward", "bench_backward.json"))
    args = ap.parse_args()
    frame = synthetic.make_frame(512, 640, V=3, scene="dtu", seed=11)
    w = synthetic.make_nerf_weights(seed=3)
    eng = HotPathEngine(); eng.load_weights(w)
    eng.prepare({k: torch.from_numpy(np.ascontiguousarray(frame[k])).cuda() for k in FRAME_KEYS})
    s = eng.sample()
    rfd_all, vox_all = eng.encode(s["rays_xyz"], s["uvd"], s["ball_radii"], s["samples_per_batch"], s["total"])
    total = int(s["total"].item())
    wt = {k: torch.from_numpy(np.asarray(v)).cuda().requires_grad_() for k, v in w.items()}
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json"))).get("gdb_backward.hip", {})
    rec = {"device": torch.cuda.get_device_name(0), "V": 3, "iters": args.iters, "unit": "us", "workloads": {},
           "resource_usage": {k: v for k, v in usage.items()}, "mlp_backward_layout(V=3, n=c2)": eng.mlp_backward_layout(3, total)}
    for name, n in (("c2 (%d samples)" % total, total), ("65537 samples", min(65537, total))):
        rfd, vox = rfd_all[:, :n].contiguous(), vox_all[:n].contiguous()
        idx, z, nb = s["indices"][:n].contiguous(), s["z_vals"][:n].contiguous(), eng.n_bundles
        g = torch.Generator(device="cuda").manual_seed(1)
        gs, gf = torch.randn(n, device="cuda", generator=g), torch.randn(n, eng.Q, device="cuda", generator=g)
        gF, gZ, gO = torch.randn(nb, eng.Q, device="cuda", generator=g), torch.randn(nb, device="cuda", generator=g), torch.randn(nb, device="cuda", generator=g)
        sigma, feat = eng.mlp(vox, rfd)
        wgt = eng.render_weights(sigma, idx, nb)
        r = {"gdb_mlp (forward)": timed(lambda: eng.mlp(vox, rfd), args.iters, args.warmup),
             "gdb_mlp_backward": timed(lambda: eng.mlp_backward(vox, rfd, gs, gf), args.iters, args.warmup),
             "gdb_render_weights_backward": timed(lambda: eng.render_weights_backward(sigma, idx, nb, gs), args.iters, args.warmup),
             "gdb_accumulate_backward": timed(lambda: eng.accumulate_backward(wgt, feat, z, idx, nb, gF, gZ, gO), args.iters, args.warmup)}
        vt, xt = vox.clone().requires_grad_(), rfd.clone().requires_grad_()
        leaves = [vt, xt, *wt.values()]

        def fwd_bwd():
            so, fo = torch_mlp(wt, vt, xt)
            torch.autograd.grad([so, fo], leaves, [gs, gf])
        r["torch restatement, forward"] = timed(lambda: torch_mlp(wt, vt, xt), args.iters, args.warmup)
        r["torch restatement, forward + autograd backward"] = timed(fwd_bwd, args.iters, args.warmup)
        r["torch restatement, autograd backward (difference)"] = r["torch restatement, forward + autograd backward"] - r["torch restatement, forward"]
        r["ratio gdb_mlp_backward / torch autograd backward"] = r["gdb_mlp_backward"] / max(r["torch restatement, autograd backward (difference)"], 1e-9)
        r["ratio gdb_mlp_backward / torch forward + backward"] = r["gdb_mlp_backward"] / r["torch restatement, forward + autograd backward"]
        rec["workloads"][name] = r
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

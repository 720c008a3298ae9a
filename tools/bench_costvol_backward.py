"""Times the cost volume's backward: costvol.feature_volume_backward (gdb_feature_volume_backward) against torch
autograd's backward of `depth_net.build_feature_volume` on the same card, at the two 512 x 640 stage shapes of configs/dtu_pretrain.yaml
with V = 3, with both outputs and with g_src_feat alone; and one NetworkWrapper forward + backward at 512 x 640 (the step of DESIGN.md
4.19: `mvs.stage_render`, `mvs.hip_stage_render` and `mvs.hip_cost_reg_train` on) with `mvs.cost_volume_grad` off and on.  Writes
profiles/costvol_backward/bench.json.

    python tools/bench_costvol_backward.py [--out FILE] [--no-wrapper]

Call times: device events around a window of at least 0.5 s of back-to-back calls, after a warm-up, the sides alternated in one
process, median of the windows (tools/bench_loss.py).  The torch side times the backward alone: its forward graph is built once
outside the window and kept (`retain_graph`).
Atomic rate: an upper count of the scatter's atomic bytes - every voxel, view, channel and all four taps, 8 bytes each - over the time
of the whole g_src_feat-only entry (maxima, zeroing, scatter, fold), beside the 1.11 .. 1.44 TB/s DESIGN.md 4.15 measured for int64
atomics; taps that fall outside a source map add no atomic, so the true byte count is lower.
The recorded difference to torch's float32 gradients is taken with the upstream zeroed where the referee excludes a voxel
(`referee_exclusions`); the share of such voxels is recorded with it."""
import argparse
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
from gdb_nerf_amd.configs import make_cfg  # noqa: E402
from gdb_nerf_amd.networks.gdb_nerf import depth_net  # noqa: E402


def stage_inputs(s, V=3, Ho=512, Wo=640, seed=21):
    """Stage s as DepthNet.forward builds it from configs/dtu_pretrain.yaml: scaled intrinsics, C, D, inv_depth from the config."""
    cfg = make_cfg("configs/dtu_pretrain.yaml")
    lvl = cfg.mvs.vol_levels[s]
    ss, ts = cfg.fpn.feat_scales[lvl], cfg.mvs.vol_scales[s]
    Cc, D, inv = cfg.fpn.feat_dims[lvl], cfg.mvs.num_depth[s], bool(cfg.mvs.inv_depth[s])
    fr = synthetic.make_frame(Ho, Wo, V=V, B=1, seed=seed, scene="dtu")
    Ks, Kt = fr["src_ints"].copy(), fr["tar_int"].copy()
    Ks[..., :2, :] *= np.float32(ss); Kt[:, :2, :] *= np.float32(ts)
    Hs, Ws, Ht, Wt = int(Ho * ss), int(Wo * ss), int(Ho * ts), int(Wo * ts)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator().manual_seed(seed)
    nf = t(fr["near_far"]).view(1, 2, 1, 1).expand(1, 2, Ht, Wt)
    hyp = depth_net.get_depth_values(nf, D, inv).contiguous()
    feat = torch.randn((1, V, Cc, Hs, Ws), generator=g).cuda()
    up = torch.randn((1, Cc, D, Ht, Wt), generator=g).cuda()
    return dict(args=(feat, t(fr["src_exts"]), t(Ks), t(fr["tar_ext"]), t(Kt), hyp), inv=inv, up=up,
                shape=dict(V=V, C=Cc, Hs=Hs, Ws=Ws, D=D, Ht=Ht, Wt=Wt, inv_depth=inv))


def referee_exclusions(c, kink=1e-4):
    """(1, D, Ht, Wt) bool on the card: the exclusions of tests/test_costvol_backward_referee.py, decided in float64 - some view's z
    below 1e-3 of the plane depth, or some view's ix / iy within `kink` of an integer inside the tap range, where d val / d ix jumps."""
    feat, se, si, te, ti, hyp = (a.double().cpu().numpy() for a in c["args"])
    Hs, Ws = feat.shape[3:]
    Ht, Wt = hyp.shape[2:]
    depth = 1.0 / hyp if c["inv"] else hyp
    P_tar = np.zeros((1, 4, 4)); P_tar[:, :3] = ti @ te[:, :3]; P_tar[:, 3, 3] = 1
    Hm = (si @ se[..., :3, :]) @ np.linalg.inv(P_tar)[:, None]                                        # (1,V,3,4)
    xs, ys = np.meshgrid(np.arange(Wt) + 0.5, np.arange(Ht) + 0.5, indexing="xy")
    q = Hm[..., :3, 0, None, None] * xs + Hm[..., :3, 1, None, None] * ys + Hm[..., :3, 2, None, None]   # (1,V,3,Ht,Wt)
    p = q[:, :, :, None] * depth[:, None, None] + Hm[..., :3, 3, None, None, None]                      # (1,V,3,D,Ht,Wt)
    bad = (p[:, :, 2] < 1e-3 * depth[:, None]).any(1)
    z = np.maximum(p[:, :, 2], 1e-6)
    ix, iy = p[:, :, 0] / z - 0.5, p[:, :, 1] / z - 0.5
    inside = (ix >= -1 - kink) & (ix <= Ws + kink) & (iy >= -1 - kink) & (iy <= Hs + kink)
    near = (np.abs(ix - np.round(ix)) < kink) | (np.abs(iy - np.round(iy)) < kink)
    return torch.from_numpy(bad | (inside & near).any(1)).cuda()


def costvol_sides(c):
    feat, se, si, te, ti, hyp = c["args"]
    # the upstream is zero where the referee excludes a voxel, so that the difference to torch below compares like with like; the
    # kernels' work does not depend on the upstream's values
    excl = referee_exclusions(c)
    c["up"] = c["up"] * ~excl[:, None]
    graphs = {}
    for both in (True, False):
        f, h = feat.clone().requires_grad_(), hyp.clone().requires_grad_(both)
        graphs[both] = (depth_net.build_feature_volume(f, se, si, te, ti, h, c["inv"]), (f, h) if both else (f,))

    def torch_bwd(both):
        vol, leaves = graphs[both]
        return torch.autograd.grad(vol, leaves, c["up"], retain_graph=True)

    hip = lambda both: costvol.feature_volume_backward(*c["args"], c["up"], c["inv"], True, both)
    ref, got = torch_bwd(True), hip(True)
    diff = {n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(("g_src_feat", "g_depth_values"), got, ref)}
    diff["excluded_share_of_voxels"] = float(excl.float().mean())
    sides = {"hip_both": lambda: hip(True), "torch_both": lambda: torch_bwd(True), "hip_g_src_feat": lambda: hip(False),
             "torch_g_src_feat": lambda: torch_bwd(False)}
    return sides, diff


def wrapper_sides(Ho=512, Wo=640):
    from gdb_nerf_amd.networks import make_network
    from gdb_nerf_amd.train.trainers import make_wrapper
    fr = synthetic.make_frame(Ho, Wo, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"]), "rgb": torch.rand(1, Ho, Wo, 3, device="cuda")},
             "near_far": t(fr["near_far"]), "tar_gt_ms": {"rgb": [torch.rand(1, Ho // 8, Wo // 8, 3, device="cuda")]}}
    sides = {}
    for on in (False, True):
        cfg = make_cfg("configs/dtu_pretrain.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "mvs.hip_stage_render", "True",
                                                     "mvs.hip_cost_reg_train", "True", "mvs.cost_volume_grad", str(on),
                                                     "train.photometric_weights", "[1.0, 0.1, 0.0]"])
        torch.manual_seed(109)
        net = make_network(cfg).eval().cuda()
        net.depth_net.train()
        wrapper = make_wrapper(cfg, net)
        wrapper.training = True

        def step(wrapper=wrapper):
            wrapper.zero_grad(set_to_none=True)
            wrapper(batch)[1].backward()
        sides["wrapper_cost_volume_grad_on" if on else "wrapper_cost_volume_grad_off"] = step
    return sides


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "costvol_backward", "bench.json"))
    ap.add_argument("--no-wrapper", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_costvol_backward.py measures on the GPU; none is available")
    res = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for s in (0, 1):
        c = stage_inputs(s)
        sides, diff = costvol_sides(c)
        r = alternate(sides)
        sh = c["shape"]
        r["shape"] = sh
        r["ratio_torch_over_hip_both"] = r["torch_both"]["ms"] / r["hip_both"]["ms"]
        r["ratio_torch_over_hip_g_src_feat"] = r["torch_g_src_feat"]["ms"] / r["hip_g_src_feat"]["ms"]
        r["max_relative_difference_hip_vs_torch"] = diff
        atomic_bytes = 8.0 * sh["D"] * sh["Ht"] * sh["Wt"] * sh["V"] * sh["C"] * 4
        r["atomic_bytes_upper_count"] = atomic_bytes
        r["atomic_TBps_over_g_src_feat_entry_time"] = atomic_bytes / (r["hip_g_src_feat"]["ms"] * 1e-3) / 1e12
        r["int64_atomic_TBps_measured_in_4_15"] = [1.11, 1.44]
        res["shapes"][f"c2_stage{s}"] = r
        print(f"c2_stage{s}", json.dumps(r), flush=True)
    if not args.no_wrapper:
        res["network_wrapper_512x640_forward_backward"] = alternate(wrapper_sides(), rounds=3)
        print(json.dumps(res["network_wrapper_512x640_forward_backward"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Times the depth net's train-time stage render: the HIP entries (gdb_stage_nerf, gdb_stage_nerf_backward) against the
plain-torch restatement on the same card - which is what training runs with `mvs.hip_stage_render` off - forward alone and forward +
backward, at the pretrain shape (5,120 rays x 8 samples, V = 3, feat_dim 32) and at four times that; the two `F.grid_sample` gathers of
`_render_rays` with their backward, separately; and one NetworkWrapper forward + backward at 512 x 640 with `mvs.stage_render` on, for
`mvs.hip_stage_render` off and on.  Writes profiles/stage_render/bench_stage_render.json.

    python tools/bench_stage_render.py [--out FILE] [--kernel-stats DIR] [--no-wrapper]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/5120 -o trace -- python tools/bench_stage_render.py --kernels-only 5120

Call times: device events around a window of at least 0.5 s of back-to-back calls, after a warm-up, the sides alternated in one
process, median of the windows (tools/bench_loss.py).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
`--kernels-only` (tracing slows the host, so nothing else is read from it): `--kernel-stats DIR` merges every *kernel_stats.csv below
DIR/<rays>/."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_loss import alternate  # noqa: E402
from gdb_nerf_amd import stage_nerf, synthetic  # noqa: E402
from gdb_nerf_amd.networks.gdb_nerf import depth_net as dn  # noqa: E402

RAYS = (5120, 20480)
V, S, C_F = 3, 8, 32


def draw(n_rays, seed=0):
    torch.manual_seed(seed)
    nerf = dn._AuxStageNerf(64, 8, C_F, True)
    with torch.no_grad():   # the referee's law: every path of the network alive
        for m in nerf.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn_like(m.weight) * 1.5 / m.in_features ** 0.5)
                m.bias.copy_(torch.randn_like(m.bias) * 0.3)
    N = n_rays * S
    vox = torch.randn(N, 8) * 0.5
    img = torch.randn(N, V, C_F + 7) * 0.5
    img[..., -4:-1] = F.normalize(torch.randn(N, V, 3), dim=-1)
    return nerf.cuda(), vox.cuda(), img.cuda(), torch.randn(n_rays, 3).cuda()


def nerf_sides(n_rays):
    nerf, vox, img, U = draw(n_rays)
    holder = stage_nerf.StageNerf(nerf)
    packed = holder.sync(vox.device)
    ws = torch.empty((holder.layout(V, S, n_rays)[0] // 4,), device="cuda")
    gp = torch.empty((holder.floats,), device="cuda")
    vl, il = vox.clone().requires_grad_(), img.clone().requires_grad_()

    def torch_fwd():
        with torch.no_grad():
            sigma, rgb = nerf(vox[None], img[None])
            return dn.composite_stage(sigma.unflatten(1, (n_rays, S)), rgb.unflatten(1, (n_rays, S)))

    def torch_fwd_bwd():
        vl.grad = il.grad = None
        nerf.zero_grad(set_to_none=True)
        sigma, rgb = nerf(vl[None], il[None])
        (dn.composite_stage(sigma.unflatten(1, (n_rays, S)), rgb.unflatten(1, (n_rays, S)))[0] * U).sum().backward()

    def hip_fwd_bwd():
        holder.forward(packed, vox, img, S)
        holder.backward(packed, vox, img, S, U, workspace=ws, g_packed=gp)

    return {"hip_forward": lambda: holder.forward(packed, vox, img, S), "torch_forward": torch_fwd,
            "hip_forward_backward": hip_fwd_bwd, "torch_forward_backward": torch_fwd_bwd}


def gather_sides(n_rays):
    """The two gathers of _render_rays at the recipe's stage 0 (64 hypotheses, 64 x 80 volume, 128 x 160 feature maps), with backward
    into the volume, the maps and the sample positions."""
    torch.manual_seed(1)
    N = n_rays * S
    volume = torch.randn(1, 8, 64, 64, 80, device="cuda", requires_grad=True)
    maps = torch.randn(V, C_F + 3, 128, 160, device="cuda", requires_grad=True)
    uvd = (torch.rand(1, N, 1, 1, 3, device="cuda") * 2 - 1).requires_grad_()
    grid = (torch.rand(V, N, 1, 2, device="cuda") * 2 - 1).requires_grad_()

    def vol():
        volume.grad = uvd.grad = None
        F.grid_sample(volume, uvd, mode="bilinear", padding_mode="border", align_corners=False).sum().backward()

    def img():
        maps.grad = grid.grad = None
        F.grid_sample(maps, grid, mode="bilinear", padding_mode="border", align_corners=False).sum().backward()

    return {"volume_gather_forward_backward": vol, "map_gather_forward_backward": img}


def wrapper_sides(Ho=512, Wo=640):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    from gdb_nerf_amd.train.trainers import make_wrapper
    fr = synthetic.make_frame(Ho, Wo, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"]), "rgb": torch.rand(1, Ho, Wo, 3, device="cuda")},
             "near_far": t(fr["near_far"]), "tar_gt_ms": {"rgb": [torch.rand(1, Ho // 8, Wo // 8, 3, device="cuda")]}}
    sides = {}
    for name, on in (("wrapper_hip_stage_render", True), ("wrapper_torch_stage_render", False)):
        cfg = make_cfg("configs/dtu_pretrain.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False", "mvs.hip_stage_render", str(on),
                                                     "train.photometric_weights", "[1.0, 0.1, 0.0]"])
        torch.manual_seed(109)
        net = make_network(cfg).eval().cuda()
        net.depth_net.train()        # the stage images are rendered in training mode only
        wrapper = make_wrapper(cfg, net)
        wrapper.training = True

        def step(wrapper=wrapper):
            wrapper.zero_grad(set_to_none=True)
            wrapper(batch)[1].backward()
        sides[name] = step
    return sides


def kernel_stats(root):
    out = {}
    for n_rays in RAYS:
        for path in glob.glob(os.path.join(root, str(n_rays), "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = (row.get("Name") or row.get("KernelName") or "").replace("void ", "")
                if name.startswith("k_stage_"):
                    out.setdefault(str(n_rays), {})[name] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_render", "bench_stage_render.json"))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--kernels-only", default="", help="RAYS: 50 forward and backward calls of the HIP entries, for a profiler run")
    ap.add_argument("--no-wrapper", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage_render.py measures on the GPU; none is available")
    if args.kernels_only:
        sides = nerf_sides(int(args.kernels_only))
        for _ in range(50):
            sides["hip_forward_backward"]()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "V": V, "S": S, "feat_dim": C_F, "rays": {}}
    kst = kernel_stats(args.kernel_stats) if args.kernel_stats else {}
    for n_rays in RAYS:
        r = alternate(nerf_sides(n_rays))
        r["ratio_torch_over_hip_forward"] = r["torch_forward"]["ms"] / r["hip_forward"]["ms"]
        r["ratio_torch_over_hip_forward_backward"] = r["torch_forward_backward"]["ms"] / r["hip_forward_backward"]["ms"]
        r.update(alternate(gather_sides(n_rays)))
        if str(n_rays) in kst:
            r["kernels"] = kst[str(n_rays)]
        res["rays"][str(n_rays)] = r
        print(n_rays, json.dumps(r), flush=True)
    if not args.no_wrapper:
        res["network_wrapper_512x640_forward_backward"] = alternate(wrapper_sides(), rounds=3)
        print(json.dumps(res["network_wrapper_512x640_forward_backward"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

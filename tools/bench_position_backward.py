"""Time of gdb_encode_position_backward and gdb_sample_backward at V = 3, on the samples of the c2 frame (512 x 640, S_max 3 adaptive,
seeded synthetic: every sample engine.sample yields) and on its first 65,537 samples:
  gdb_encode and gdb_encode_backward (for scale); gdb_encode_position_backward with all three outputs and with each alone;
  gdb_sample_backward (the whole bundle map; upstreams for the workload's samples); and torch autograd's backward of a plain-torch
  restatement of encode (F.grid_sample on the source images, the volume and each mip level, the camera and level arithmetic) with
  rays_xyz, uvd and ball_radii as leaves, on the same card - the only other way to this gradient.
Medians over --iters calls after --warmup, hipEvent times around each call.  No time is fixed in advance: the record holds all figures,
the ratio of the two new entries together to the torch backward, and their ratio to gdb_mlp_backward at the same size
(profiles/backward/bench_backward.json).

    python tools/bench_position_backward.py [--iters 20] [--warmup 3] [--workloads c2,65537] [--out profiles/position_backward/bench_position_backward.json]"""
import argparse, json, math, os, sys
import numpy as np, torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import HotPathEngine

FRAME_KEYS = ("src_images", "img_feat", "feat_volume", "depth_range", "vol_range", "src_exts", "src_ints", "tar_ext", "tar_int", "near_far")


def torch_encode(fr, pyr, rays_xyz, uvd, ball, b):
    """bundle_sampler.py:267-371 for batch item 0 in plain torch ops, differentiable in the three sample arrays."""
    V, _, Ho, Wo = fr["src_images"][0].shape
    H, W = pyr[0].shape[-2:]
    L = len(pyr) - 1
    n, _, bb = rays_xyz.shape
    vox = F.grid_sample(fr["feat_volume"], uvd.view(1, 1, 1, n, 3), mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0, 0].t()
    pts = rays_xyz.permute(0, 2, 1).reshape(-1, 3)
    ph = torch.cat((pts, torch.ones_like(pts[:, :1])), 1)
    cam = (ph @ fr["src_exts"][0].transpose(1, 2))[..., :3]
    im = cam @ fr["src_ints"][0].transpose(1, 2)
    zc = im[..., 2:].clamp(min=1e-6)
    g = torch.cat((2.0 * (im[..., :1] / zc) / Wo - 1.0, 2.0 * (im[..., 1:2] / zc) / Ho - 1.0), -1)
    rgb = F.grid_sample(fr["src_images"][0], g[:, :, None, :], mode="bilinear", padding_mode="border", align_corners=False)[..., 0]
    rgbs = rgb.reshape(V, 3, n, bb).permute(0, 2, 1, 3).reshape(V, n, 3 * bb)
    ccam = cam.reshape(V, n, bb, 3).mean(2)
    dist = ccam.norm(dim=-1)
    sec2 = (dist / ccam[..., 2]) ** 2
    Ks = fr["src_ints"][0].clone()
    Ks[:, :2] /= b
    pixr = 1.0 / torch.sqrt(Ks[:, 0, 0] * Ks[:, 1, 1] * math.pi)
    a = torch.sqrt(torch.clamp((dist / ball[None]) ** 2 - 1.0, min=1e-12))
    c = torch.sqrt(torch.clamp(sec2 - 1.0, min=1e-12))
    level = torch.log2(sec2 / (a + c) / pixr[:, None])
    cim = ccam @ Ks.transpose(1, 2)
    z = cim[..., 2].clamp(min=1e-6)
    uv = torch.stack((cim[..., 0] / z / W, cim[..., 1] / z / H), -1)
    lv = torch.nan_to_num(level, nan=0.0).clamp(0.0, float(L))
    l0 = lv.floor()
    l1 = (l0 + 1).clamp(max=float(L))
    frc = (lv - l0)[..., None]
    gg = (2.0 * uv - 1.0)[:, :, None, :]
    feat = 0
    for l, tex in enumerate(pyr):
        s = F.grid_sample(tex, gg, mode="bilinear", padding_mode="border", align_corners=False)[:, :, :, 0].permute(0, 2, 1)
        feat = feat + s * ((l0 == l)[..., None] * (1.0 - frc) + ((l1 == l) & (frc[..., 0] > 0))[..., None] * frc)
    ctr = rays_xyz.mean(-1)
    tar_c, src_c = torch.inverse(fr["tar_ext"])[0, :3, 3], torch.inverse(fr["src_exts"][0])[:, :3, 3]
    td = F.normalize(ctr - tar_c[None], dim=-1)
    sd = F.normalize(ctr[None] - src_c[:, None], dim=-1)
    return torch.cat((rgbs, feat, F.normalize(td[None] - sd, dim=-1), (td[None] * sd).sum(-1, keepdim=True)), -1), vox


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_backward", "bench_position_backward.json"))
    ap.add_argument("--workloads", default="c2,65537", help="which sizes to run (a kernel trace of one size alone: --workloads c2)")
    args = ap.parse_args()
    frame = synthetic.make_frame(512, 640, V=3, scene="dtu", seed=11)
    fr = {k: torch.from_numpy(np.ascontiguousarray(frame[k])).cuda() for k in FRAME_KEYS}
    eng = HotPathEngine()
    L = eng.prepare(fr)
    s = eng.sample()
    total = int(s["total"].item())
    B, V, _, H, W = fr["img_feat"].shape
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json"))).get("gdb_position_backward.hip", {})
    mlp = json.load(open(os.path.join(ROOT, "profiles", "backward", "bench_backward.json")))["workloads"]
    mlp = {("c2" if k.startswith("c2") else "65537"): v["gdb_mlp_backward"] for k, v in mlp.items()}
    rec = {"device": torch.cuda.get_device_name(0), "V": 3, "iters": args.iters, "unit": "us", "mip_levels": L, "workloads": {},
           "resource_usage": usage}
    with torch.no_grad():
        pyr = [fr["img_feat"][0]]
        for _ in range(L):
            pyr.append(F.avg_pool2d(pyr[-1], 2))
    for name, tag, n in (("c2 (%d samples)" % total, "c2", total), ("65537 samples", "65537", min(65537, total))):
        if tag not in args.workloads.split(","):
            continue
        smp = [s[k][:n].contiguous() for k in ("rays_xyz", "uvd", "ball_radii")]
        spb, tot = torch.tensor([n], dtype=torch.int64, device="cuda"), torch.tensor([n], dtype=torch.int64, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        g_rfd, g_vox = torch.randn(V, n, eng.P, device="cuda", generator=g), torch.randn(n, 8, device="cuda", generator=g)
        g_z = torch.randn(n, device="cuda", generator=g)
        pos = lambda **kw: eng.encode_position_backward(*smp, spb, tot, g_rfd, g_vox, **kw)
        only = lambda k: pos(**{f: f == k for f in ("need_rays", "need_uvd", "need_ball")})
        g_rays, g_uvd, g_ball = pos()
        cnt = s["samples_per_bundle"]
        smp_bwd = lambda: eng.sample_backward(cnt, tot, g_rays, g_uvd, g_z, g_ball)
        r = {"gdb_encode (forward)": timed(lambda: eng.encode(*smp, spb, tot), args.iters, args.warmup),
             "gdb_encode_backward (both)": timed(lambda: eng.encode_backward(*smp, spb, tot, g_rfd, g_vox), args.iters, args.warmup),
             "gdb_encode_position_backward (all three)": timed(pos, args.iters, args.warmup),
             "gdb_encode_position_backward (rays_xyz alone)": timed(lambda: only("need_rays"), args.iters, args.warmup),
             "gdb_encode_position_backward (uvd alone)": timed(lambda: only("need_uvd"), args.iters, args.warmup),
             "gdb_encode_position_backward (ball_radii alone)": timed(lambda: only("need_ball"), args.iters, args.warmup),
             "gdb_sample_backward": timed(smp_bwd, args.iters, args.warmup)}
        # torch autograd of the plain-torch restatement, the positions as leaves
        leaves = [t.clone().requires_grad_() for t in smp]

        def fwd_bwd():
            out, vox = torch_encode(fr, pyr, *leaves, eng.b)
            return torch.autograd.grad([out, vox], leaves, [g_rfd, g_vox])
        r["torch restatement, forward"] = timed(lambda: torch_encode(fr, pyr, *leaves, eng.b), args.iters, args.warmup)
        r["torch restatement, forward + autograd backward"] = timed(fwd_bwd, args.iters, args.warmup)
        r["torch restatement, autograd backward (difference)"] = r["torch restatement, forward + autograd backward"] - r["torch restatement, forward"]
        new = r["gdb_encode_position_backward (all three)"] + r["gdb_sample_backward"]
        r["new entries together"] = new
        r["ratio new entries together / torch autograd backward"] = new / max(r["torch restatement, autograd backward (difference)"], 1e-9)
        r["gdb_mlp_backward at this size (profiles/backward/bench_backward.json)"] = mlp[tag]
        r["ratio new entries together / gdb_mlp_backward"] = new / mlp[tag]
        # same inputs, close to torch's answer away from the kinks (a sanity figure, not the referee: tests/test_position_backward_referee.py
        # is): the median absolute difference per tensor against the median magnitude
        t_rays, t_uvd, t_ball = fwd_bwd()
        r["median |hip - torch autograd| / median |torch|: rays_xyz, uvd[:, 2], ball_radii"] = [
            float((a - b).abs().median() / b.abs().median().clamp(min=1e-30)) for a, b in ((g_rays, t_rays), (g_uvd[:, 2], t_uvd[:, 2]), (g_ball, t_ball))]
        rec["workloads"][name] = r
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

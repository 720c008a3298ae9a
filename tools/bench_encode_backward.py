"""Time of gdb_encode_backward at V = 3, on the samples of the c2 frame (512 x 640, S_max 3 adaptive, seeded synthetic: every sample
engine.sample yields) and on its first 65,537 samples:
  gdb_encode (forward, for scale); gdb_encode_backward with both outputs and with each alone; and torch autograd's backward of a
  plain-torch restatement of the gather (F.grid_sample on the volume and on each mip level, an avg_pool2d chain) on the same card,
  the coordinates and levels computed beforehand, outside the timed region.
Medians over --iters calls after --warmup, hipEvent times around each call.  No time is fixed in advance: the record holds all figures,
the ratio to the torch backward, the ratio to gdb_mlp_backward at the same size (profiles/backward/bench_backward.json) and the 64-bit
integer atomic bytes added per second - over the WHOLE call each alone (memset of the accumulators, the scale reduction and the fold
included), so a lower bound of the scatter kernel's own rate.

    python tools/bench_encode_backward.py [--iters 20] [--warmup 3] [--workloads c2,65537] [--out profiles/encode_backward/bench_encode_backward.json]"""
import argparse, json, math, os, sys
import numpy as np, torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import HotPathEngine

FRAME_KEYS = ("src_images", "img_feat", "feat_volume", "depth_range", "vol_range", "src_exts", "src_ints", "tar_ext", "tar_int", "near_far")


def coordinates(fr, rays_xyz, ball, b, W, H):
    """bundle_sampler.py:327-353 for batch item 0: texture coordinate (V, n, 2) and mip level (V, n) of every (view, sample)."""
    n, _, bb = rays_xyz.shape
    pts = rays_xyz.permute(0, 2, 1).reshape(-1, 3)
    ph = torch.cat((pts, torch.ones_like(pts[:, :1])), 1)
    cam = (ph @ fr["src_exts"][0].transpose(1, 2))[..., :3]
    ccam = cam.reshape(-1, n, bb, 3).mean(2)
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
    return torch.stack((cim[..., 0] / z / W, cim[..., 1] / z / H), -1), level


def torch_gather(img, vol, uvd, uv, level, L):
    """The two differentiable fetches of encode in plain torch ops: img (V,C,H,W), vol (1,C_v,D,H,W)."""
    vox = F.grid_sample(vol, uvd.view(1, 1, 1, -1, 3), mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0, 0].t()
    pyr = [img]
    for _ in range(L):
        pyr.append(F.avg_pool2d(pyr[-1], 2))
    lv = torch.nan_to_num(level, nan=0.0).clamp(0.0, float(L))
    l0 = lv.floor()
    l1 = (l0 + 1).clamp(max=float(L))
    fr = (lv - l0)[..., None]
    g = (2.0 * uv - 1.0)[:, :, None, :]
    out = 0
    for l, tex in enumerate(pyr):
        s = F.grid_sample(tex, g, mode="bilinear", padding_mode="border", align_corners=False)[:, :, :, 0].permute(0, 2, 1)
        out = out + s * ((l0 == l)[..., None] * (1.0 - fr) + ((l1 == l) & (fr[..., 0] > 0))[..., None] * fr)
    return out, vox


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_backward", "bench_encode_backward.json"))
    ap.add_argument("--workloads", default="c2,65537", help="which sizes to run (a kernel trace of one size alone: --workloads c2)")
    args = ap.parse_args()
    frame = synthetic.make_frame(512, 640, V=3, scene="dtu", seed=11)
    fr = {k: torch.from_numpy(np.ascontiguousarray(frame[k])).cuda() for k in FRAME_KEYS}
    eng = HotPathEngine()
    L = eng.prepare(fr)
    s = eng.sample()
    total = int(s["total"].item())
    B, V, _, H, W = fr["img_feat"].shape
    D = fr["feat_volume"].shape[2]
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json"))).get("gdb_encode_backward.hip", {})
    mlp = json.load(open(os.path.join(ROOT, "profiles", "backward", "bench_backward.json")))["workloads"]
    mlp = {("c2" if k.startswith("c2") else "65537"): v["gdb_mlp_backward"] for k, v in mlp.items()}
    rec = {"device": torch.cuda.get_device_name(0), "V": 3, "iters": args.iters, "unit": "us", "mip_levels": L, "workloads": {},
           "atomics": "64-bit integer, no-return global atomic add, agent scope, one per (tap, channel) contribution",
           "guide_f32_atomic_rate_TB_per_s": 1.3, "resource_usage": usage}
    for name, tag, n in (("c2 (%d samples)" % total, "c2", total), ("65537 samples", "65537", min(65537, total))):
        if tag not in args.workloads.split(","):
            continue
        smp = [s[k][:n].contiguous() for k in ("rays_xyz", "uvd", "ball_radii")]
        spb, tot = torch.tensor([n], dtype=torch.int64, device="cuda"), torch.tensor([n], dtype=torch.int64, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        g_rfd, g_vox = torch.randn(V, n, eng.P, device="cuda", generator=g), torch.randn(n, 8, device="cuda", generator=g)
        ws_bytes, Fbits, _, _ = eng.encode_backward_layout(n)
        bwd = lambda **kw: eng.encode_backward(*smp, spb, tot, g_rfd, g_vox, **kw)
        r = {"gdb_encode (forward)": timed(lambda: eng.encode(*smp, spb, tot), args.iters, args.warmup),
             "gdb_encode_backward (both)": timed(bwd, args.iters, args.warmup),
             "gdb_encode_backward (img_feat alone)": timed(lambda: bwd(need_vol=False), args.iters, args.warmup),
             "gdb_encode_backward (feat_volume alone)": timed(lambda: bwd(need_img=False), args.iters, args.warmup),
             "workspace_bytes": ws_bytes, "fraction_bits_F": Fbits}
        # the adds the scatters make (counted from the coordinates, not timed)
        with torch.no_grad():
            uv, level = coordinates(fr, smp[0], smp[2], eng.b, W, H)
            lv = torch.nan_to_num(level, nan=0.0).clamp(0.0, float(L))
            tex_adds = int((4 * 19 * (1 + ((lv - lv.floor()) > 0).long())).sum().item())
            xyz = [((smp[1][:, i] + 1) * size - 1) / 2 for i, size in enumerate((W, H, D))]
            taps = 1
            for x, size in zip(xyz, (W, H, D)):
                taps = taps * (1 + (x.clamp(0, size - 1).floor() + 1 <= size - 1).long())
            vol_adds = int((8 * taps).sum().item())
        r["atomic adds, pyramid"], r["atomic adds, volume"] = tex_adds, vol_adds
        r["atomic TB/s over the whole call, pyramid alone"] = 8 * tex_adds / r["gdb_encode_backward (img_feat alone)"] * 1e-6
        r["atomic TB/s over the whole call, volume alone"] = 8 * vol_adds / r["gdb_encode_backward (feat_volume alone)"] * 1e-6
        # torch autograd of the plain-torch gather
        img_t, vol_t = fr["img_feat"][0].clone().requires_grad_(), fr["feat_volume"].clone().requires_grad_()
        g_feat = g_rfd[..., 3 * eng.b ** 2:3 * eng.b ** 2 + 19].contiguous()

        def fwd_bwd():
            out, vox = torch_gather(img_t, vol_t, smp[1], uv, level, L)
            torch.autograd.grad([out, vox], [img_t, vol_t], [g_feat, g_vox])
        r["torch restatement, forward"] = timed(lambda: torch_gather(img_t, vol_t, smp[1], uv, level, L), args.iters, args.warmup)
        r["torch restatement, forward + autograd backward"] = timed(fwd_bwd, args.iters, args.warmup)
        r["torch restatement, autograd backward (difference)"] = r["torch restatement, forward + autograd backward"] - r["torch restatement, forward"]
        r["ratio gdb_encode_backward / torch autograd backward"] = r["gdb_encode_backward (both)"] / max(r["torch restatement, autograd backward (difference)"], 1e-9)
        r["gdb_mlp_backward at this size (profiles/backward/bench_backward.json)"] = mlp[tag]
        r["ratio gdb_encode_backward / gdb_mlp_backward"] = r["gdb_encode_backward (both)"] / mlp[tag]
        # same inputs, same answer as torch's (a sanity figure, not the referee: tests/test_encode_backward_referee.py is)
        gi, gv = bwd()
        out, vox = torch_gather(img_t, vol_t, smp[1], uv, level, L)
        ti, tv = torch.autograd.grad([out, vox], [img_t, vol_t], [g_feat, g_vox])
        r["max |hip - torch autograd|, img_feat / feat_volume"] = [float((gi[0] - ti).abs().max()), float((gv - tv).abs().max())]
        rec["workloads"][name] = r
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""The HIP backward of `encode` (gdb_encode_backward) against float64 autograd of the CPU restatement (`gdb_oracle_torch.encode`) with
`img_feat` and `feat_volume` as leaves.  Runs on a real MI355X: `pytest -m gpu`.

Rule (that of test_backward_referee.py, restated here), per gradient tensor, elementwise, no element excluded:
|hip - ref64| <= 4 max(E32, 8 fp32 ulp of max |ref64|), E32 = max |float32 CPU autograd of the same restatement - ref64|.  The kernel is
not involved in the bound.  Both sides get the same float32 sample arrays; the loss is sum(g_rfd * rfd) + sum(g_vox * vox) for random
normal upstreams.  There are no ReLU kinks and so no exclusions: bilinear and mip blends are continuous across tap and level changes.

Samples come from `engine.sample()` on synthetic frames with ZOOMED source cameras (`src_focal_scale`): the default frames only ever
touch mip levels 0 and 1.  Observed |hip - ref64| / bound per case and tensor: profiles/encode_backward/referee_observed.txt
(rewritten by a run of this file)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gdb_oracle_torch as oracle_t
from conftest import FRAME_KEYS, load_golden
from gdb_nerf_amd import _lib, synthetic
from gdb_nerf_amd.engine import HotPathEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "encode_backward", "referee_observed.txt")
SAMPLE_KEYS = ("rays_xyz", "uvd", "ball_radii")

# name: (Ho, Wo, V, B, bundle_size, seed, src_focal_scale, mip levels built)
CASES = {
    "levels_0_1_3_clamped": (32, 64, 3, 1, 2, 11, (1.0, 3.0, 12.0), 3),
    "levels_0_1_2": (32, 64, 3, 1, 2, 11, (1.0, 2.5, 6.0), 3),
    "odd_extent_chain_stops_at_2": (32, 40, 3, 1, 2, 11, (1.0, 3.0, 12.0), 2),
    "two_batch_items_bundle_4": (32, 64, 2, 2, 4, 5, (1.0, 6.0), 3),
    "five_views_bundle_1": (16, 24, 5, 1, 1, 7, (1.0, 2.5, 6.0, 12.0, 1.5), 3),
}


# ---- referee ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)   # the restatement allocates its tables with the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def encode_ref(fr, smp, spb, g_rfd, g_vox, b, dtype, max_mip=3):
    """Autograd of the restatement on the CPU in `dtype` -> {"img_feat", "feat_volume"}: gradients as float64 numpy."""
    with default_dtype(dtype):
        c = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        img, vol = c(fr["img_feat"]).requires_grad_(), c(fr["feat_volume"]).requires_grad_()
        s = {k: c(smp[k]) for k in SAMPLE_KEYS}
        s["samples_per_batch"] = torch.as_tensor(np.asarray(spb), dtype=torch.int64)
        Ho, Wo = fr["src_images"].shape[-2:]
        rfd, vox = oracle_t.encode(c(fr["src_images"]), img, vol, s, c(fr["src_exts"]), c(fr["src_ints"]), c(fr["tar_ext"]), b, Ho, Wo, max_mip)
        ((rfd * c(g_rfd)).sum() + (vox * c(g_vox)).sum()).backward()
    return {"img_feat": img.grad.double().numpy(), "feat_volume": vol.grad.double().numpy()}


_observed = {}


def check_rule(case, hip, ref64, ref32):
    """hip, ref64, ref32: {name: array}.  Prints each figure, records it, then asserts the rule for every tensor."""
    fails = []
    for name, r64 in ref64.items():
        h = np.asarray(hip[name], np.float64)
        assert h.shape == r64.shape, (case, name, h.shape, r64.shape)
        top = float(np.abs(r64).max())
        e32 = float(np.abs(ref32[name] - r64).max())
        bound = 4.0 * max(e32, 8.0 * float(np.spacing(np.float32(top))))
        err = float(np.abs(h - r64).max()) if np.isfinite(h).all() else float("inf")
        line = (f"{case:32s} {name:12s} err {err:.3e}  bound {bound:.3e}  err/bound {err / bound if bound else 0.0:.3f}  E32 {e32:.3e}  "
                f"max|ref64| {top:.3e}")
        print(line)
        _observed[(case, name)] = line
        if not err <= bound:
            fails.append(line)
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        old = {}
        if os.path.exists(OBSERVED):
            for l in open(OBSERVED):
                if l.strip() and not l.startswith("#"):
                    old[tuple(l.split()[:2])] = l.rstrip("\n")
        old.update(_observed)
        with open(OBSERVED, "w") as f:
            f.write("# |hip - ref64| per gradient tensor against the bound 4 * max(E32, 8 ulp of max |ref64|); tests/test_encode_backward_referee.py\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError:
        pass
    assert not fails, "\n".join(fails)


# ---- HIP side ----------------------------------------------------------------------------------------------------------------
def cu(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


def cuda_frame(fr):
    return {k: cu(fr[k]) for k in FRAME_KEYS}


def hip_grads(eng, smp, spb, g_rfd, g_vox, total=None, **need):
    n = smp["rays_xyz"].shape[0]
    total = torch.tensor([n if total is None else total], dtype=torch.int64, device="cuda")
    g_img, g_vol = eng.encode_backward(cu(smp["rays_xyz"]), cu(smp["uvd"]), cu(smp["ball_radii"]), cu(spb, torch.int64), total,
                                       cu(g_rfd), cu(g_vox), **need)
    return {"img_feat": npy(g_img), "feat_volume": npy(g_vol)}


def upstreams(V, n, P, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, n, P)).astype(np.float32), rng.standard_normal((n, 8)).astype(np.float32)


_cases = {}


def case(name):
    """Frame, engine (prepared), the valid samples of engine.sample(), upstreams and both referee runs: built once, shared, read-only."""
    if name not in _cases:
        Ho, Wo, V, B, b, seed, fs, levels = CASES[name]
        fr = synthetic.make_frame(Ho, Wo, V=V, B=B, bundle_size=b, scene="dtu", seed=seed, src_focal_scale=fs)
        eng = HotPathEngine(bundle_size=b)
        assert eng.prepare(cuda_frame(fr)) == levels
        s = eng.sample()
        n = int(s["total"].item())
        smp = {k: npy(s[k])[:n] for k in SAMPLE_KEYS}
        spb = npy(s["samples_per_batch"])
        assert spb.sum() == n and (B == 1 or (spb > 0).all())
        g_rfd, g_vox = upstreams(V, n, eng.P, 100 + seed)
        ref64, ref32 = (encode_ref(fr, smp, spb, g_rfd, g_vox, b, dt) for dt in (torch.float64, torch.float32))
        _cases[name] = dict(fr=fr, eng=eng, smp=smp, spb=spb, n=n, b=b, g_rfd=g_rfd, g_vox=g_vox, ref64=ref64, ref32=ref32)
    c = _cases[name]
    c["eng"].prepare(cuda_frame(c["fr"]))   # (another test may have prepared the engine for something else)
    return c


@pytest.mark.parametrize("name", list(CASES))
def test_encode_backward_on_zoomed_frames(name):
    c = case(name)
    hip = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    check_rule(name, hip, c["ref64"], c["ref32"])
    if name == "levels_0_1_3_clamped":
        # what the case is for: the coarse levels and the border are reached (gradient arrives at edge texels of every view)
        g = hip["img_feat"][0]
        assert all(np.abs(g[v, :, :, 0]).max() > 0 and np.abs(g[v, :, 0, :]).max() > 0 for v in range(3))


def test_encode_backward_on_the_committed_mip_fixture_through_the_abi():
    """F4_encode_mips (V = 4, its own rays_xyz / uvd / ball_radii), every call made on the C ABI directly."""
    fx = load_golden("F4_encode_mips")
    lib = _lib.load()
    cfg = _lib.GdbConfig(2, int(fx["S_max"]), int(bool(fx["adaptive"])), int(bool(fx["inv_depth"])), 64, 3, 16, 8, 64, 1)
    fr = {k: fx[k] for k in FRAME_KEYS}
    B, V, _, Ho, Wo = fr["src_images"].shape
    H, W, D = Ho // 2, Wo // 2, fr["feat_volume"].shape[2]
    dev = cuda_frame(fr)
    f = _lib.GdbFrame(B, V, Ho, Wo, H, W, D, *(dev[k].data_ptr() for k in FRAME_KEYS))
    need = C.c_size_t()
    _lib.check(lib.gdb_workspace_bytes(C.byref(cfg), C.byref(f), C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gdb_prepare(C.byref(cfg), C.byref(f), ws.data_ptr(), ws.numel(), st))
    smp = {k: np.ascontiguousarray(fx[k], np.float32) for k in SAMPLE_KEYS}
    n = smp["uvd"].shape[0]
    spb = np.asarray(fx["samples_per_batch"]).astype(np.int64)
    g_rfd, g_vox = upstreams(V, n, 35, 4)
    lay = (C.c_size_t * 4)()
    _lib.check(lib.gdb_encode_backward_layout(C.byref(cfg), C.byref(f), n, lay))
    bws = torch.empty(lay[0], dtype=torch.uint8, device="cuda")
    t = {k: cu(smp[k]) for k in SAMPLE_KEYS}
    spb_d, total, gr, gv = cu(spb, torch.int64), cu([n], torch.int64), cu(g_rfd), cu(g_vox)
    g_img, g_vol = torch.empty((B, V, 19, H, W), device="cuda"), torch.empty((B, 8, D, H, W), device="cuda")
    args = (C.byref(cfg), C.byref(f), ws.data_ptr(), t["rays_xyz"].data_ptr(), t["uvd"].data_ptr(), t["ball_radii"].data_ptr(),
            spb_d.data_ptr(), total.data_ptr(), n, gr.data_ptr(), gv.data_ptr())
    assert lib.gdb_encode_backward(*args, None, None, bws.data_ptr(), bws.numel(), st) == _lib.GDB_E_BADARG
    assert lib.gdb_encode_backward(*args, g_img.data_ptr(), g_vol.data_ptr(), bws.data_ptr(), lay[0] - 1, st) == _lib.GDB_E_WORKSPACE
    _lib.check(lib.gdb_encode_backward(*args, g_img.data_ptr(), g_vol.data_ptr(), bws.data_ptr(), bws.numel(), st))
    torch.cuda.synchronize()
    ref64, ref32 = (encode_ref(fr, smp, spb, g_rfd, g_vox, 2, dt) for dt in (torch.float64, torch.float32))
    check_rule("F4_encode_mips_abi", {"img_feat": npy(g_img), "feat_volume": npy(g_vol)}, ref64, ref32)


def test_encode_backward_one_sample():
    c = case("levels_0_1_3_clamped")
    smp = {k: c["smp"][k][:1] for k in SAMPLE_KEYS}
    spb, g_rfd, g_vox = np.array([1]), np.ascontiguousarray(c["g_rfd"][:, :1]), c["g_vox"][:1]
    hip = hip_grads(c["eng"], smp, spb, g_rfd, g_vox)
    check_rule("one_sample", hip, *(encode_ref(c["fr"], smp, spb, g_rfd, g_vox, 2, dt) for dt in (torch.float64, torch.float32)))


def test_rows_past_total_change_nothing():
    """*d_total = n - 37, NaN in the tail rows of every array, positions and upstreams alike: the referee on the first n - 37 rows."""
    c = case("levels_0_1_3_clamped")
    n = c["n"] - 37
    smp = {k: c["smp"][k].copy() for k in SAMPLE_KEYS}
    g_rfd, g_vox = c["g_rfd"].copy(), c["g_vox"].copy()
    head = ({k: smp[k][:n].copy() for k in SAMPLE_KEYS}, np.array([n]), np.ascontiguousarray(g_rfd[:, :n]), g_vox[:n].copy())
    for a in smp.values():
        a[n:] = np.nan
    g_rfd[:, n:], g_vox[n:] = np.nan, np.nan
    hip = hip_grads(c["eng"], smp, np.array([n]), g_rfd, g_vox, total=n)
    check_rule("total_below_n_alloc", hip, *(encode_ref(c["fr"], *head, 2, dt) for dt in (torch.float64, torch.float32)))
    clean = hip_grads(c["eng"], head[0], head[1], head[2], head[3])
    assert np.array_equal(hip["img_feat"], clean["img_feat"]) and np.array_equal(hip["feat_volume"], clean["feat_volume"])


def test_one_output_alone_is_bit_identical_to_the_pair():
    c = case("levels_0_1_3_clamped")
    both = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    vol_only = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"], need_img=False)
    img_only = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"], need_vol=False)
    assert vol_only["img_feat"] is None and np.array_equal(vol_only["feat_volume"], both["feat_volume"])
    assert img_only["feat_volume"] is None and np.array_equal(img_only["img_feat"], both["img_feat"])
    with pytest.raises(ValueError):
        hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"], need_img=False, need_vol=False)


def test_encode_backward_is_deterministic_and_survives_another_frame_in_between():
    from gdb_nerf_amd.networks.gdb_nerf.bundle_sampler import BundleSampler
    other, c = case("odd_extent_chain_stops_at_2"), case("levels_0_1_3_clamped")
    a = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    b = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    assert np.array_equal(a["img_feat"], b["img_feat"]) and np.array_equal(a["feat_volume"], b["feat_volume"])

    # the same through BundleSampler.encode + .backward(), with ONE engine preparing the other case's frame between forward and backward
    sampler = BundleSampler(64, 3, encode_grad=True)

    def forward(cs):
        fr = cuda_frame(cs["fr"])
        Ho, Wo = fr["src_images"].shape[-2:]
        sampler.build_rays(fr["tar_ext"], fr["tar_int"], (Ho, Wo), fr["near_far"][:, 0], fr["near_far"][:, 1])
        rays_xyz, uvd, _, ball, _, per_batch, _ = sampler.sample(fr["depth_range"], fr["vol_range"], 2, 3, False, True)
        for got, key in ((rays_xyz, "rays_xyz"), (uvd, "uvd"), (ball, "ball_radii")):
            assert np.array_equal(npy(got), cs["smp"][key])
        img, vol = fr["img_feat"].requires_grad_(), fr["feat_volume"].requires_grad_()
        rfd, vox = sampler.encode(fr["src_images"], img, vol, rays_xyz, uvd, ball, fr["src_exts"], fr["src_ints"], fr["tar_ext"], per_batch)
        assert rfd.grad_fn is not None and vox.grad_fn is not None
        return sampler._last, img, vol, rfd, vox

    eng1, img, vol, rfd, vox = forward(c)
    eng2 = forward(other)[0]
    assert eng1 is eng2
    ((rfd * cu(c["g_rfd"])).sum() + (vox * cu(c["g_vox"])).sum()).backward()
    assert np.array_equal(npy(img.grad), a["img_feat"]) and np.array_equal(npy(vol.grad), a["feat_volume"])


def test_zero_and_non_finite_upstreams():
    c = case("levels_0_1_3_clamped")
    z = hip_grads(c["eng"], c["smp"], c["spb"], np.zeros_like(c["g_rfd"]), np.zeros_like(c["g_vox"]))
    assert not z["img_feat"].any() and not z["feat_volume"].any()
    g_vox = c["g_vox"].copy()
    g_vox[c["n"] // 2, 3] = np.inf
    bad = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], g_vox)
    assert np.isnan(bad["img_feat"]).all() and np.isnan(bad["feat_volume"]).all()
    # the workspace is zeroed by every call: nothing of the refused upstream is left behind
    again = hip_grads(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    check_rule("after_a_non_finite_call", again, c["ref64"], c["ref32"])


# ---- Network ----------------------------------------------------------------------------------------------------------------
def test_network_encode_grad_trains_the_feature_net_and_the_depth_net():
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    fr = synthetic.make_frame(32, 64, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}
    torch.manual_seed(109)
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False",
                                                          "nerf.encode_grad", "True"])).eval().cuda()
    seen = {"up": {}, "grad": {}}
    inner = net.sampler.encode

    def encode(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch):
        rfd, vox = inner(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch)
        if torch.is_grad_enabled():
            assert img_feat.requires_grad and feat_volume.requires_grad and rfd.grad_fn is not None and vox.grad_fn is not None
            seen.update(fr={"src_images": npy(src_images), "img_feat": npy(img_feat), "feat_volume": npy(feat_volume), "src_exts": npy(src_exts),
                            "src_ints": npy(src_ints), "tar_ext": npy(tar_exts)},
                        smp={"rays_xyz": npy(rays_xyz), "uvd": npy(uvd), "ball_radii": npy(ball_radii)}, spb=npy(per_batch).astype(np.int64))
            img_feat.register_hook(lambda g: seen["grad"].__setitem__("img_feat", npy(g)))
            feat_volume.register_hook(lambda g: seen["grad"].__setitem__("feat_volume", npy(g)))
            rfd.register_hook(lambda g: seen["up"].__setitem__("rfd", npy(g)))
            vox.register_hook(lambda g: seen["up"].__setitem__("vox", npy(g)))
        return rfd, vox

    net.sampler.encode = encode
    ret = net(batch)[0]
    before = ret["rgb"].detach().clone()
    ret["rgb"].square().mean().backward()
    assert set(seen["grad"]) == {"img_feat", "feat_volume"} and set(seen["up"]) == {"rfd", "vox"}
    args = (seen["fr"], seen["smp"], seen["spb"], seen["up"]["rfd"], seen["up"]["vox"], net.b_size)
    check_rule("network_encode_grad_32x64", seen["grad"], encode_ref(*args, torch.float64), encode_ref(*args, torch.float32))
    trained = {"feature_net": 0, "depth_net": 0}
    for k, p in net.named_parameters():
        if k.startswith(("nerf.", "upsampler.")):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
        elif p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
            trained[k.split(".")[0]] += int(p.grad.abs().max() > 0)
    assert trained["feature_net"] > 0 and trained["depth_net"] > 0, trained
    # a step on those two networks ALONE changes the next forward
    torch.optim.SGD(list(net.feature_net.parameters()) + list(net.depth_net.parameters()), lr=1e-2).step()
    with torch.no_grad():
        after = net(batch)[0]["rgb"]
    assert not torch.equal(before, after)

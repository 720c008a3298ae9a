"""The HIP backward of `encode` with respect to the sample positions (gdb_encode_position_backward) and of `sample`
(gdb_sample_backward) against float64 autograd of the CPU restatements.  Runs on a real MI355X: `pytest -m gpu`.

Rule (the project's own, restated), per gradient tensor, elementwise: |hip - ref64| <= 4 max(E32, 8 fp32 ulp of max |ref64|),
E32 = max |float32 CPU autograd of the same restatement - ref64|.  The kernel is not involved in the bound.

`encode`: leaves rays_xyz, uvd, ball_radii of `gdb_oracle_torch.encode` on the float32 sample arrays of `engine.sample()`; uvd is compared
in column 2 only (columns 0 and 1 of the HIP result must be exact zeros: u, v sit on voxel centres and are not differentiated); loss
sum(g_rfd * rfd) + sum(g_vox * vox) with seeded normal upstreams.

Kinks.  Unlike the gradients of DESIGN.md 4.15 these are only piecewise continuous, so samples near a derivative discontinuity leave
BOTH sides: their upstream rows are zeroed before both backwards.  The margin m_i is computed in float64 from the float32 arrays as the
minimum of |c - round(c)| over the volume depth coordinate ((d + 1) D - 1) / 2, every view's and sub-ray's source-pixel coordinates
im_x / z - 1/2, im_y / z - 1/2, every view's unclamped mip level, and every view's texel coordinates u W_l - 1/2, v H_l - 1/2 at both
blended levels (texture, image and level clamps all sit on integers).  m_i < 1e-4 is excluded; at most 5 % of a case's samples may
be, asserted.  No clamp_min floor may be near either: projected depths > 1e-3, both radicands of the mip level > 1e-9, asserted.

`sample` is refereed at its own boundary by `oracle_t.sample_bundles_counted`, the restatement of `sample_bundles` that takes the counts as
data (ceil can differ between dtypes; the counts are the HIP forward's); at float32 it is bit-equal to `oracle_t.sample_bundles`, asserted.  Random
upstreams on all four outputs, same rule, nothing excluded.  One end-to-end case chains both entries against autograd of the chained
restatements.

Observed |hip - ref64| / bound per case and tensor: profiles/position_backward/referee_observed.txt (rewritten by a run of this file)."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch

import gdb_oracle_torch as oracle_t
from conftest import FRAME_KEYS
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import HotPathEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "position_backward", "referee_observed.txt")
SAMPLE_KEYS = ("rays_xyz", "uvd", "ball_radii")
POS_NAMES = ("rays_xyz", "uvd_d", "ball_radii")
KINK_MARGIN, KINK_CAP = 1e-4, 0.05

# name: (Ho, Wo, V, B, bundle_size, seed, src_focal_scale, inv_depth, mip levels built)
CASES = {
    "levels_0_1_3_clamped": (32, 64, 3, 1, 2, 11, (1.0, 3.0, 12.0), False, 3),
    "levels_0_1_2": (32, 64, 3, 1, 2, 11, (1.0, 2.5, 6.0), False, 3),
    "odd_extent_chain_stops_at_2": (32, 40, 3, 1, 2, 11, (1.0, 3.0, 12.0), False, 2),
    "two_batch_items_bundle_4": (32, 64, 2, 2, 4, 5, (1.0, 6.0), False, 3),
    "five_views_bundle_1": (16, 24, 5, 1, 1, 7, (1.0, 2.5, 6.0, 12.0, 1.5), False, 3),
    "default_cameras": (32, 64, 3, 1, 2, 11, None, False, 3),
    "levels_0_1_2_inv_depth": (32, 64, 3, 1, 2, 11, (1.0, 2.5, 6.0), True, 3),
}
S_MAX, NUM_DEPTH = 3, 64   # HotPathEngine's defaults


# ---- referee ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)   # the restatement allocates its tables with the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _enc(fr, s, b, c, max_mip=3):
    Ho, Wo = fr["src_images"].shape[-2:]
    return oracle_t.encode(c(fr["src_images"]), c(fr["img_feat"]), c(fr["feat_volume"]), s, c(fr["src_exts"]), c(fr["src_ints"]), c(fr["tar_ext"]),
                           b, Ho, Wo, max_mip)


def encode_pos_ref(fr, smp, spb, g_rfd, g_vox, b, dtype):
    """Autograd of the restatement on the CPU in `dtype`, the positions as leaves -> gradients as float64 numpy."""
    with default_dtype(dtype):
        c = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        s = {k: c(smp[k]).requires_grad_() for k in SAMPLE_KEYS}
        s["samples_per_batch"] = torch.as_tensor(np.asarray(spb), dtype=torch.int64)
        rfd, vox = _enc(fr, s, b, c)
        ((rfd * c(g_rfd)).sum() + (vox * c(g_vox)).sum()).backward()
    return {"rays_xyz": s["rays_xyz"].grad.double().numpy(), "uvd_d": s["uvd"].grad[:, 2].double().numpy(),
            "ball_radii": s["ball_radii"].grad.double().numpy()}


def kink_margins(fr, smp, spb, b, levels):
    """Per sample the distance of its nearest coordinate to a derivative discontinuity (module docstring), in float64 from the float32
    arrays -> (margin (n,), smallest projected depth, smallest radicand of the mip level)."""
    d = torch.float64
    c = lambda a: torch.tensor(np.asarray(a), dtype=d)
    frac = lambda x: (x - torch.round(x)).abs()
    xyz, uvd, ball = c(smp["rays_xyz"]), c(smp["uvd"]), c(smp["ball_radii"])
    src_exts, src_ints = c(fr["src_exts"]), c(fr["src_ints"])
    B, V, _, Ho, Wo = fr["src_images"].shape
    H, W, D, bb = Ho // b, Wo // b, fr["feat_volume"].shape[2], b * b
    Ks = src_ints.clone()
    Ks[..., :2, :] = Ks[..., :2, :] / b
    pixr = 1.0 / torch.sqrt(Ks[..., 0, 0] * Ks[..., 1, 1] * math.pi)
    m = frac(((uvd[:, 2] + 1.0) * D - 1.0) / 2.0)
    min_depth, min_rad, start = math.inf, math.inf, 0
    for bi in range(B):
        n = int(spb[bi])
        sl = slice(start, start + n)
        pts = xyz[sl].permute(0, 2, 1).reshape(-1, 3)
        cam = (torch.cat((pts, torch.ones(pts.shape[0], 1, dtype=d)), 1) @ src_exts[bi].transpose(1, 2))[..., :3]   # (V, n bb, 3)
        im = cam @ src_ints[bi].transpose(1, 2)
        z = im[..., 2]
        pix = torch.minimum(frac(im[..., 0] / z - 0.5), frac(im[..., 1] / z - 0.5)).reshape(V, n, bb)
        mm = pix.amin(dim=(0, 2))
        ccam = cam.reshape(V, n, bb, 3).mean(dim=2)
        dist = ccam.norm(dim=-1)
        sec2 = (dist / ccam[..., 2]) ** 2
        ra, rc = (dist / ball[sl][None]) ** 2 - 1.0, sec2 - 1.0
        level = torch.log2(sec2 / (torch.sqrt(ra) + torch.sqrt(rc)) / pixr[bi][:, None])   # (V, n)
        cim = ccam @ Ks[bi].transpose(1, 2)
        z2 = cim[..., 2]
        u, v = cim[..., 0] / z2 / W, cim[..., 1] / z2 / H
        lv = level.clamp(0.0, float(levels))
        l0 = torch.floor(lv)
        l1 = torch.clamp(l0 + 1.0, max=float(levels))
        mm = torch.minimum(mm, frac(level).amin(dim=0))
        for l in (l0, l1):
            sc = torch.pow(2.0, -l)
            mm = torch.minimum(mm, torch.minimum(frac(u * (W * sc) - 0.5), frac(v * (H * sc) - 0.5)).amin(dim=0))
        m[sl] = torch.minimum(m[sl], mm)
        min_depth = min(min_depth, float(z.min()), float(z2.min()))
        min_rad = min(min_rad, float(ra.min()), float(rc.min()))
        start += n
    return m.numpy(), min_depth, min_rad


sample_restated = oracle_t.sample_bundles_counted   # the one counts-as-data restatement (its float32 bit-equality is asserted below)


def rays_of(fr, dtype):
    """The float32 ray tables of the restatement (constants of the differentiation), cast to `dtype`."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    Ho, Wo = fr["src_images"].shape[-2:]
    return {k: v.to(dtype) for k, v in oracle_t.build_rays(t(fr["tar_ext"]), t(fr["tar_int"]), Ho, Wo).items()}


def sample_ref(fr, cnt, b, inv_depth, ups, dtype):
    """Autograd of `sample_restated` with depth_range / vol_range as leaves; ups = upstreams of (rays_xyz, uvd, z_vals, ball_radii)."""
    with default_dtype(dtype):
        c = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        dr, vr = c(fr["depth_range"]).requires_grad_(), c(fr["vol_range"]).requires_grad_()
        s = sample_restated(rays_of(fr, dtype), dr, vr, b, inv_depth, torch.as_tensor(np.asarray(cnt), dtype=torch.int64))
        sum((s[k] * c(g)).sum() for k, g in zip(("rays_xyz", "uvd", "z_vals", "ball_radii"), ups)).backward()
    return {"depth_range": dr.grad.double().numpy(), "vol_range": vr.grad.double().numpy()}


def chain_ref(fr, cnt, b, inv_depth, g_rfd, g_vox, dtype):
    """Autograd of sample_restated -> gdb_oracle_torch.encode, depth_range / vol_range as leaves."""
    with default_dtype(dtype):
        c = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        dr, vr = c(fr["depth_range"]).requires_grad_(), c(fr["vol_range"]).requires_grad_()
        s = sample_restated(rays_of(fr, dtype), dr, vr, b, inv_depth, torch.as_tensor(np.asarray(cnt), dtype=torch.int64))
        rfd, vox = _enc(fr, s, b, c)
        ((rfd * c(g_rfd)).sum() + (vox * c(g_vox)).sum()).backward()
    return {"depth_range": dr.grad.double().numpy(), "vol_range": vr.grad.double().numpy()}


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
        line = (f"{case:36s} {name:12s} err {err:.3e}  bound {bound:.3e}  err/bound {err / bound if bound else 0.0:.3f}  E32 {e32:.3e}  "
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
            f.write("# |hip - ref64| per gradient tensor against the bound 4 * max(E32, 8 ulp of max |ref64|); tests/test_position_backward_referee.py\n")
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


def hip_pos(eng, smp, spb, g_rfd, g_vox, total=None, **need):
    n = smp["rays_xyz"].shape[0]
    total = torch.tensor([n if total is None else total], dtype=torch.int64, device="cuda")
    g_rays, g_uvd, g_ball = eng.encode_position_backward(cu(smp["rays_xyz"]), cu(smp["uvd"]), cu(smp["ball_radii"]), cu(spb, torch.int64), total,
                                                         cu(g_rfd), cu(g_vox), **need)
    if g_uvd is not None:
        assert not npy(g_uvd)[:, :2].any()   # u, v are not differentiated: exact zeros
    return {"rays_xyz": npy(g_rays), "uvd_d": None if g_uvd is None else npy(g_uvd)[:, 2], "ball_radii": npy(g_ball), "uvd": npy(g_uvd)}


def hip_sample(eng, cnt, ups, total=None, **need):
    n = next(g for g in ups if g is not None).shape[0]
    total = torch.tensor([n if total is None else total], dtype=torch.int64, device="cuda")
    g_dr, g_vr = eng.sample_backward(cu(cnt, torch.int32), total, *(None if g is None else cu(g) for g in ups), **need)
    return {"depth_range": npy(g_dr), "vol_range": npy(g_vr)}


def same(a, b, names):
    return all(np.array_equal(a[k], b[k]) for k in names)


_cases = {}


def case(name):
    """Frame, engine (prepared), the valid samples of engine.sample(), the kink mask, upstreams (kink rows zeroed) and both referee runs
    of `encode`: built once, shared, read-only."""
    if name not in _cases:
        Ho, Wo, V, B, b, seed, fs, inv, levels = CASES[name]
        fr = synthetic.make_frame(Ho, Wo, V=V, B=B, bundle_size=b, scene="dtu", seed=seed, src_focal_scale=fs)
        eng = HotPathEngine(bundle_size=b, inv_depth=inv)
        assert eng.prepare(cuda_frame(fr)) == levels
        s = eng.sample()
        n = int(s["total"].item())
        assert 600 <= n <= 1300, n
        smp = {k: npy(s[k])[:n] for k in SAMPLE_KEYS}
        spb, cnt = npy(s["samples_per_batch"]), npy(s["samples_per_bundle"]).astype(np.int64)
        assert spb.sum() == n == cnt.sum() and (B == 1 or (spb > 0).all())
        margin, min_depth, min_rad = kink_margins(fr, smp, spb, b, levels)
        kink = margin < KINK_MARGIN
        print(f"{name}: n {n}, excluded near a kink {int(kink.sum())} ({kink.mean():.2%}), min projected depth {min_depth:.3g}, "
              f"min radicand {min_rad:.3g}")
        assert kink.mean() <= KINK_CAP, (name, kink.mean())
        assert min_depth > 1e-3 and min_rad > 1e-9, (name, min_depth, min_rad)   # no clamp_min floor is near
        rng = np.random.default_rng(100 + seed)
        g_rfd, g_vox = rng.standard_normal((V, n, eng.P)).astype(np.float32), rng.standard_normal((n, 8)).astype(np.float32)
        g_rfd[:, kink], g_vox[kink] = 0.0, 0.0   # samples near a discontinuity leave both sides
        ref64, ref32 = (encode_pos_ref(fr, smp, spb, g_rfd, g_vox, b, dt) for dt in (torch.float64, torch.float32))
        _cases[name] = dict(fr=fr, eng=eng, smp=smp, spb=spb, cnt=cnt, n=n, b=b, inv=inv, kink=kink, g_rfd=g_rfd, g_vox=g_vox, ref64=ref64,
                            ref32=ref32, z_vals=npy(s["z_vals"])[:n])
    c = _cases[name]
    c["eng"].prepare(cuda_frame(c["fr"]))   # (another test may have prepared the engine for something else)
    return c


def sample_upstreams(c, seed):
    rng = np.random.default_rng(seed)
    n, bb = c["n"], c["b"] ** 2
    return tuple(rng.standard_normal(shp).astype(np.float32) for shp in ((n, 3, bb), (n, 3), (n,), (n,)))


# ---- encode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_encode_position_backward(name):
    c = case(name)
    hip = hip_pos(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    check_rule(name, hip, c["ref64"], c["ref32"])
    for k in POS_NAMES:   # the case differentiates something: no tensor is all zeros, every excluded row is
        assert np.abs(hip[k]).max() > 0 and not hip[k][c["kink"]].any(), k


# ---- sample ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sample_backward(name):
    c = case(name)
    Ho, Wo, V, B, b, seed, fs, inv, levels = CASES[name]
    fr = c["fr"]
    # the restatement with the counts given IS the oracle's sample_bundles at float32 (a CPU statement)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    rays = rays_of(fr, torch.float32)
    o = oracle_t.sample_bundles(rays, t(fr["depth_range"]), t(fr["vol_range"]), t(fr["near_far"][:, 0]), t(fr["near_far"][:, 1]), b, S_MAX,
                                NUM_DEPTH, inv, True)
    r = sample_restated(rays, t(fr["depth_range"]), t(fr["vol_range"]), b, inv, o["samples_per_bundle"].to(torch.int64))
    for k in ("rays_xyz", "uvd", "z_vals", "ball_radii", "indices", "samples_per_batch"):
        assert torch.equal(r[k], o[k]), (name, k)
    ups = sample_upstreams(c, 300 + seed)
    hip = hip_sample(c["eng"], c["cnt"], ups)
    check_rule(name, hip, *(sample_ref(fr, c["cnt"], b, inv, ups, dt) for dt in (torch.float64, torch.float32)))
    assert all(np.abs(hip[k]).max() > 0 for k in hip)


def test_both_entries_chained_against_the_chained_restatements():
    name = "levels_0_1_2"
    c = case(name)
    p = hip_pos(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    hip = hip_sample(c["eng"], c["cnt"], (p["rays_xyz"], p["uvd"], None, p["ball_radii"]))
    check_rule(name + "_chained", hip, *(chain_ref(c["fr"], c["cnt"], c["b"], c["inv"], c["g_rfd"], c["g_vox"], dt) for dt in (torch.float64, torch.float32)))


def test_fixed_counts():
    """is_adaptive = False, S_max = 4: every bundle holds four samples."""
    Ho, Wo, V, B, b, seed, fs, inv, levels = CASES["odd_extent_chain_stops_at_2"]
    fr = synthetic.make_frame(Ho, Wo, V=V, B=B, bundle_size=b, scene="dtu", seed=seed, src_focal_scale=fs)
    eng = HotPathEngine(bundle_size=b, max_num_samples=4, is_adaptive=False)
    assert eng.prepare(cuda_frame(fr)) == levels
    s = eng.sample()
    n = int(s["total"].item())
    cnt = npy(s["samples_per_bundle"]).astype(np.int64)
    assert n == 4 * (Ho // b) * (Wo // b) <= 1300 and (cnt == 4).all()
    smp, spb = {k: npy(s[k])[:n] for k in SAMPLE_KEYS}, npy(s["samples_per_batch"])
    margin, min_depth, min_rad = kink_margins(fr, smp, spb, b, levels)
    kink = margin < KINK_MARGIN
    assert kink.mean() <= KINK_CAP and min_depth > 1e-3 and min_rad > 1e-9
    rng = np.random.default_rng(17)
    g_rfd, g_vox = rng.standard_normal((V, n, eng.P)).astype(np.float32), rng.standard_normal((n, 8)).astype(np.float32)
    g_rfd[:, kink], g_vox[kink] = 0.0, 0.0
    hip = hip_pos(eng, smp, spb, g_rfd, g_vox)
    check_rule("fixed_counts_S4", hip, *(encode_pos_ref(fr, smp, spb, g_rfd, g_vox, b, dt) for dt in (torch.float64, torch.float32)))
    ups = tuple(rng.standard_normal(shp).astype(np.float32) for shp in ((n, 3, b * b), (n, 3), (n,), (n,)))
    check_rule("fixed_counts_S4", hip_sample(eng, cnt, ups), *(sample_ref(fr, cnt, b, False, ups, dt) for dt in (torch.float64, torch.float32)))


# ---- further properties ----------------------------------------------------------------------------------------------------------
def test_each_output_alone_is_bit_identical_to_the_full_call():
    c = case("levels_0_1_3_clamped")
    args = (c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    full = hip_pos(*args)
    for k, flag in zip(POS_NAMES, ("need_rays", "need_uvd", "need_ball")):
        alone = hip_pos(*args, **{f: f == flag for f in ("need_rays", "need_uvd", "need_ball")})
        assert np.array_equal(alone[k], full[k]) and all(alone[o] is None for o in POS_NAMES if o != k), k
    with pytest.raises(ValueError):
        hip_pos(*args, need_rays=False, need_uvd=False, need_ball=False)
    ups = sample_upstreams(c, 5)
    both = hip_sample(c["eng"], c["cnt"], ups)
    dr = hip_sample(c["eng"], c["cnt"], ups, need_vol=False)
    vr = hip_sample(c["eng"], c["cnt"], ups, need_depth=False)
    assert dr["vol_range"] is None and np.array_equal(dr["depth_range"], both["depth_range"])
    assert vr["depth_range"] is None and np.array_equal(vr["vol_range"], both["vol_range"])
    # an upstream left out is an upstream of zeros
    zeros = hip_sample(c["eng"], c["cnt"], (ups[0], np.zeros_like(ups[1]), np.zeros_like(ups[2]), ups[3]))
    assert same(hip_sample(c["eng"], c["cnt"], (ups[0], None, None, ups[3])), zeros, ("depth_range", "vol_range"))
    with pytest.raises(ValueError):
        hip_sample(c["eng"], c["cnt"], ups, need_depth=False, need_vol=False)


def test_two_calls_are_bit_identical():
    c = case("two_batch_items_bundle_4")
    a, b = (hip_pos(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"]) for _ in range(2))
    assert same(a, b, POS_NAMES)
    ups = sample_upstreams(c, 6)
    assert same(hip_sample(c["eng"], c["cnt"], ups), hip_sample(c["eng"], c["cnt"], ups), ("depth_range", "vol_range"))


def test_rows_past_total_are_zero_and_never_read():
    """*d_total = n - 37, NaN in the tail rows of every array, positions and upstreams alike."""
    c = case("levels_0_1_3_clamped")
    n = c["n"] - 37
    smp = {k: c["smp"][k].copy() for k in SAMPLE_KEYS}
    g_rfd, g_vox = c["g_rfd"].copy(), c["g_vox"].copy()
    head = ({k: smp[k][:n].copy() for k in SAMPLE_KEYS}, np.array([n]), np.ascontiguousarray(g_rfd[:, :n]), g_vox[:n].copy())
    for a in smp.values():
        a[n:] = np.nan
    g_rfd[:, n:], g_vox[n:] = np.nan, np.nan
    hip = hip_pos(c["eng"], smp, np.array([n]), g_rfd, g_vox, total=n)
    clean = hip_pos(c["eng"], *head)
    for k in POS_NAMES + ("uvd",):
        assert np.array_equal(hip[k][:n], clean[k]) and not hip[k][n:].any(), k
    check_rule("total_below_n_alloc", {k: hip[k][:n] for k in POS_NAMES}, *(encode_pos_ref(c["fr"], *head, 2, dt) for dt in (torch.float64, torch.float32)))
    # sample: the rows past the total are not read - the same as zeros there
    ups = sample_upstreams(c, 7)
    nan_tail, zero_tail = [u.copy() for u in ups], [u.copy() for u in ups]
    for a, z in zip(nan_tail, zero_tail):
        a[n:], z[n:] = np.nan, 0.0
    assert same(hip_sample(c["eng"], c["cnt"], nan_tail, total=n), hip_sample(c["eng"], c["cnt"], zero_tail), ("depth_range", "vol_range"))


def test_one_sample():
    c = case("levels_0_1_3_clamped")
    i = int(np.flatnonzero(~c["kink"])[0])
    assert i == 0 or not c["kink"][0]   # (row 0 is what one allocated row holds)
    smp = {k: c["smp"][k][:1] for k in SAMPLE_KEYS}
    spb, g_rfd, g_vox = np.array([1]), np.ascontiguousarray(c["g_rfd"][:, :1]), c["g_vox"][:1]
    check_rule("one_sample", hip_pos(c["eng"], smp, spb, g_rfd, g_vox), *(encode_pos_ref(c["fr"], smp, spb, g_rfd, g_vox, 2, dt) for dt in (torch.float64, torch.float32)))
    ups = sample_upstreams(c, 8)
    only_first = [np.zeros_like(u) for u in ups]
    for z, u in zip(only_first, ups):
        z[0] = u[0]
    one = hip_sample(c["eng"], c["cnt"], [np.ascontiguousarray(u[:1]) for u in ups], total=1)
    assert same(one, hip_sample(c["eng"], c["cnt"], only_first), ("depth_range", "vol_range"))
    assert np.abs(one["depth_range"]).max() > 0 and np.count_nonzero(one["depth_range"]) <= 2


def test_zero_upstreams_give_exact_zeros():
    c = case("levels_0_1_3_clamped")
    z = hip_pos(c["eng"], c["smp"], c["spb"], np.zeros_like(c["g_rfd"]), np.zeros_like(c["g_vox"]))
    assert not any(z[k].any() for k in POS_NAMES)
    z = hip_sample(c["eng"], c["cnt"], [np.zeros_like(u) for u in sample_upstreams(c, 9)])
    assert not z["depth_range"].any() and not z["vol_range"].any()


def test_sampler_backward_is_deterministic_and_survives_another_frame_in_between():
    """sampler.sample -> sampler.encode -> .backward() with ONE engine preparing another case's frame between forward and backward."""
    from gdb_nerf_amd.networks.gdb_nerf.bundle_sampler import BundleSampler
    other, c = case("default_cameras"), case("levels_0_1_3_clamped")
    p = hip_pos(c["eng"], c["smp"], c["spb"], c["g_rfd"], c["g_vox"])
    direct = hip_sample(c["eng"], c["cnt"], (p["rays_xyz"], p["uvd"], None, p["ball_radii"]))
    sampler = BundleSampler(64, 3, position_grad=True)

    def forward(cs):
        fr = cuda_frame(cs["fr"])
        Ho, Wo = fr["src_images"].shape[-2:]
        sampler.build_rays(fr["tar_ext"], fr["tar_int"], (Ho, Wo), fr["near_far"][:, 0], fr["near_far"][:, 1])
        dr, vr = fr["depth_range"].requires_grad_(), fr["vol_range"].requires_grad_()
        rays_xyz, uvd, z_vals, ball, _, per_batch, _ = sampler.sample(dr, vr, 2, 3, False, True)
        assert all(t.grad_fn is not None for t in (rays_xyz, uvd, z_vals, ball))
        for got, key in ((rays_xyz, "rays_xyz"), (uvd, "uvd"), (ball, "ball_radii")):
            assert np.array_equal(npy(got), cs["smp"][key])
        rfd, vox = sampler.encode(fr["src_images"], fr["img_feat"], fr["feat_volume"], rays_xyz, uvd, ball, fr["src_exts"], fr["src_ints"],
                                  fr["tar_ext"], per_batch)
        assert rfd.grad_fn is not None and vox.grad_fn is not None
        return sampler._last, dr, vr, rfd, vox

    eng1, dr, vr, rfd, vox = forward(c)
    eng2 = forward(other)[0]
    assert eng1 is eng2
    ((rfd * cu(c["g_rfd"])).sum() + (vox * cu(c["g_vox"])).sum()).backward()
    assert np.array_equal(npy(dr.grad), direct["depth_range"]) and np.array_equal(npy(vr.grad), direct["vol_range"])
    # with the switch off the same calls carry no graph
    plain = BundleSampler(64, 3)
    fr = cuda_frame(c["fr"])
    plain.build_rays(fr["tar_ext"], fr["tar_int"], fr["src_images"].shape[-2:], fr["near_far"][:, 0], fr["near_far"][:, 1])
    out = plain.sample(fr["depth_range"].requires_grad_(), fr["vol_range"].requires_grad_(), 2, 3, False, True)
    assert all(t.grad_fn is None for t in out[:4])


# ---- Network -------------------------------------------------------------------------------------------------------------------
def _network(overrides):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    torch.manual_seed(109)
    return make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False"] + overrides)).eval().cuda()


def _batch():
    fr = synthetic.make_frame(32, 64, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
            "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}


def test_network_position_grad_trains_the_depth_net_through_the_depth_prior():
    """Plumbing only: no tolerance on sums fed by the decoder (repeatability)."""
    batch = _batch()
    net = _network(["nerf.position_grad", "True"])
    assert net.position_grad and not net.encode_grad
    seen = {"grad": {}, "up": {}}
    inner_sample, inner_encode = net.sampler.sample, net.sampler.encode
    hook = lambda where, key: (lambda g: seen[where].__setitem__(key, g.detach().clone()))

    def sample(depth_range, vol_range, *a):
        out = inner_sample(depth_range, vol_range, *a)
        if torch.is_grad_enabled():
            assert depth_range.requires_grad and vol_range.requires_grad and all(t.grad_fn is not None for t in out[:4])
            seen.update(dr=depth_range.detach(), vr=vol_range.detach(), eng=net.sampler._last, total=net.sampler._total,
                        tar=dict(net.sampler._tar), im_size=(net.sampler.H_orig, net.sampler.W_orig))
            depth_range.register_hook(hook("grad", "depth_range"))
            vol_range.register_hook(hook("grad", "vol_range"))
            for t, k in zip(out[:4], ("rays_xyz", "uvd", "z_vals", "ball_radii")):
                t.register_hook(hook("up", k))
            seen["cnt"] = out[6].to(torch.int32).contiguous()
        return out

    def encode(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch):
        rfd, vox = inner_encode(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch)
        if torch.is_grad_enabled():
            assert rfd.grad_fn is not None and vox.grad_fn is not None
            c = lambda t: t.detach().contiguous().float()
            B, _, _, H, W = img_feat.shape
            ones = torch.ones((B, 2, H, W), device="cuda")
            seen.update(enc_frame={"src_images": c(src_images), "img_feat": c(img_feat), "feat_volume": c(feat_volume), "depth_range": ones,
                                   "vol_range": ones, "src_exts": c(src_exts), "src_ints": c(src_ints), "tar_ext": c(tar_exts),
                                   "tar_int": net.sampler._tar["tar_int"], "near_far": net.sampler._tar["near_far"]},
                        smp=(c(rays_xyz), c(uvd), c(ball_radii)), spb=per_batch.to(torch.int64).contiguous())
            rfd.register_hook(hook("up", "rfd"))
            vox.register_hook(hook("up", "vox"))
        return rfd, vox

    net.sampler.sample, net.sampler.encode = sample, encode
    ret = net(batch)[0]
    before = ret["rgb"].detach().clone()
    (ret["rgb"].square().mean() + ret["nerf_depth"].mean()).backward()   # nerf_depth: the path through z_vals (AccumulateFunction)
    assert set(seen["grad"]) == {"depth_range", "vol_range"} and {"rays_xyz", "uvd", "z_vals", "ball_radii", "rfd", "vox"} <= set(seen["up"])
    assert seen["up"]["z_vals"].abs().max() > 0
    for k, g in seen["grad"].items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
    # the two engine calls made directly on the captured upstreams give the same bits
    eng, up = seen["eng"], seen["up"]
    n = seen["smp"][0].shape[0]
    total = torch.tensor([n], dtype=torch.int64, device="cuda")
    eng.prepare(seen["enc_frame"])
    g_rays, g_uvd, g_ball = eng.encode_position_backward(*seen["smp"], seen["spb"], total, up["rfd"].contiguous(), up["vox"].contiguous())
    assert torch.equal(g_rays, up["rays_xyz"]) and torch.equal(g_uvd, up["uvd"]) and torch.equal(g_ball, up["ball_radii"])
    eng.prepare(dict(seen["tar"], depth_range=seen["dr"].contiguous().float(), vol_range=seen["vr"].contiguous().float()), im_size=seen["im_size"])
    g_dr, g_vr = eng.sample_backward(seen["cnt"], total, g_rays, g_uvd, up["z_vals"].contiguous(), g_ball)
    assert torch.equal(g_dr, seen["grad"]["depth_range"]) and torch.equal(g_vr, seen["grad"]["vol_range"])
    trained = {"feature_net": 0, "depth_net": 0}
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
            if k.split(".")[0] in trained:
                trained[k.split(".")[0]] += int(p.grad.abs().max() > 0)
    assert trained["depth_net"] > 0 and trained["feature_net"] == 0, trained
    # a step on the depth net ALONE changes the next forward
    torch.optim.SGD(net.depth_net.parameters(), lr=1e-2).step()
    with torch.no_grad():
        after = net(batch)[0]["rgb"]
    assert not torch.equal(before, after)


def test_network_with_both_switches_keeps_the_value_gradients_of_encode_grad_alone():
    """The upstream gradients of two forwards are not bit-reproducible (they come out of the PyTorch decoder's backward: DESIGN.md
    4.14, repeatability), so the two networks are compared on what does not depend on them: the forward is bit-identical, and under
    either setting the gradients that reach img_feat / feat_volume are, bit for bit, what `encode_grad` alone runs - `encode_backward`
    on the frame `encode` prepared - gives for the upstreams that network saw."""
    batch, seen = _batch(), {}
    for key, extra in (("alone", []), ("both", ["nerf.position_grad", "True"])):
        net = _network(["nerf.encode_grad", "True"] + extra)
        got = seen[key] = {}
        inner = net.sampler.encode
        hook = lambda got, k: (lambda g: got.__setitem__(k, g.detach().clone()))

        def encode(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch, inner=inner, got=got, net=net):
            rfd, vox = inner(src_images, img_feat, feat_volume, rays_xyz, uvd, ball_radii, src_exts, src_ints, tar_exts, per_batch)
            if torch.is_grad_enabled():
                c = lambda t: t.detach().contiguous().float()
                B, _, _, H, W = img_feat.shape
                ones = torch.ones((B, 2, H, W), device="cuda")
                got.update(rfd=rfd.detach().clone(), eng=net.sampler._last, smp=(c(rays_xyz), c(uvd), c(ball_radii)), spb=per_batch.to(torch.int64).contiguous(),
                           frame={"src_images": c(src_images), "img_feat": c(img_feat), "feat_volume": c(feat_volume), "depth_range": ones,
                                  "vol_range": ones, "src_exts": c(src_exts), "src_ints": c(src_ints), "tar_ext": c(tar_exts),
                                  "tar_int": net.sampler._tar["tar_int"], "near_far": net.sampler._tar["near_far"]})
                assert (rays_xyz.grad_fn is not None) == (key == "both")
                img_feat.register_hook(hook(got, "img_feat"))
                feat_volume.register_hook(hook(got, "feat_volume"))
                rfd.register_hook(hook(got, "g_rfd"))
                vox.register_hook(hook(got, "g_vox"))
            return rfd, vox

        net.sampler.encode = encode
        net(batch)[0]["rgb"].square().mean().backward()
        assert {"img_feat", "feat_volume", "g_rfd", "g_vox"} <= set(got)
        eng = got["eng"]
        eng.prepare(got["frame"])
        total = torch.tensor([got["smp"][0].shape[0]], dtype=torch.int64, device="cuda")
        g_img, g_vol = eng.encode_backward(*got["smp"], got["spb"], total, got["g_rfd"].contiguous(), got["g_vox"].contiguous())
        assert torch.equal(g_img, got["img_feat"]) and torch.equal(g_vol, got["feat_volume"]), key
    assert torch.equal(seen["alone"]["rfd"], seen["both"]["rfd"])   # the switch does not change the forward
    assert all(torch.equal(a, b) for a, b in zip(seen["alone"]["smp"], seen["both"]["smp"]))

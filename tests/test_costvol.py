""""Next" rows N2 / N4: cost-volume build and depth regression.  CPU: the oracle against
fixture F8 (the reference's own functions, tests/golden/make_golden_costvol.py — fully pinned, no third-party
op involved).  GPU: the HIP kernels through the C ABI against F8 and the oracle; further down every kernel
instantiation against a float64 referee, each GPU case with a CPU half that proves its inputs and referee."""
import numpy as np
import pytest
import torch

import gdb_oracle as oracle
from conftest import load_golden, max_abs


@pytest.fixture(scope="module")
def f8():
    return load_golden("F8_costvol")


def _case(fx, tag):
    return {k[len(tag) + 1:]: v for k, v in fx.items() if k.startswith(tag + "_")}


@pytest.mark.parametrize("tag", ["coarse", "fine"])
def test_oracle_cost_volume_matches_reference(f8, tag):
    c = _case(f8, tag)
    vol = oracle.build_feature_volume(c["src_feat"], c["src_exts"], c["src_ints"], c["tar_ext"], c["tar_int"], c["depth_values"], bool(c["inv_depth"]))
    assert vol.shape == c["volume"].shape
    assert max_abs(vol, c["volume"]) <= 1e-4  # values up to ~6
    d, ci = oracle.depth_regression(c["depth_values"], c["prob"], 1.0, bool(c["inv_depth"]))
    assert max_abs(d, c["depth"]) <= 1e-5 * float(np.abs(c["depth"]).max())
    assert max_abs(ci, c["ci"]) <= 1e-5 * float(np.abs(c["ci"]).max())


def test_oracle_depth_values():
    nf = np.array([[425.0, 905.0]], np.float32)[..., None, None]
    lin = oracle.get_depth_values(nf, 8, False)[0, :, 0, 0]
    assert np.allclose(lin, np.linspace(425, 905, 8), rtol=1e-6)
    inv = oracle.get_depth_values(nf, 8, True)[0, :, 0, 0]
    assert np.allclose(inv, np.linspace(1 / 425, 1 / 905, 8), rtol=1e-6)


def test_bilinear_zeros_padding():
    img = np.arange(12, dtype=np.float32).reshape(1, 3, 4)
    g = lambda px, size: 2 * (px + 0.5) / size - 1  # pixel centre -> normalised
    out = oracle.bilinear_zeros(img, np.array([g(1, 4), g(-1, 4), g(3.5, 4), g(1e9, 4)], np.float32),
                                np.array([g(1, 3), g(1, 3), g(2, 3), g(1, 3)], np.float32))
    assert out[0, 0] == 5 and out[0, 1] == 0 and abs(out[0, 2] - 5.5) < 1e-6 and out[0, 3] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["coarse", "fine"])
def test_hip_cost_volume_matches_reference(f8, tag):
    from gdb_nerf_amd import costvol
    c = _case(f8, tag)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda()
    vol = costvol.build_feature_volume(t("src_feat"), t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("depth_values"), bool(c["inv_depth"]))
    e = max_abs(vol.cpu().numpy(), c["volume"])
    print(f"cost volume {tag}: max abs err {e:.3e}")
    assert e <= 1e-4
    # the default takes the channel-pair re-layout of the source maps (gdb_build_feature_volume_ws); the planar form: bit-identical
    planar = costvol.build_feature_volume(t("src_feat"), t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("depth_values"), bool(c["inv_depth"]),
                                          pair_layout=False)
    assert torch.equal(vol, planar)
    d, ci = costvol.depth_regression(t("depth_values"), t("prob"), 1.0, bool(c["inv_depth"]))
    assert max_abs(d.cpu().numpy(), c["depth"]) <= 1e-5 * float(np.abs(c["depth"]).max())
    assert max_abs(ci.cpu().numpy(), c["ci"]) <= 1e-5 * float(np.abs(c["ci"]).max())


@pytest.mark.gpu
def test_hip_cost_volume_edges_vs_oracle():
    """Views that look away / far-off planes: most taps fall outside the source image (zeros padding), points
    behind a camera hit the z clamp; ragged width; 5 views."""
    from gdb_nerf_amd import costvol, synthetic
    rng = np.random.default_rng(3)
    fr = synthetic.make_frame(48, 72, V=5, B=1, seed=8, src_focal_scale=(1.0, 4.0, 0.3, 9.0, 1.0))
    fr["src_exts"][0, 4, :3, 3] += np.array([400.0, -250.0, 900.0], np.float32)  # a camera far off to the side / behind
    feat = rng.standard_normal((1, 5, 8, 24, 36)).astype(np.float32)
    Ks, Kt = fr["src_ints"].copy(), fr["tar_int"].copy()
    Ks[..., :2, :] *= 0.5; Kt[:, :2, :] *= 0.25
    dv = oracle.get_depth_values(np.broadcast_to(np.array([30.0, 2000.0], np.float32)[None, :, None, None], (1, 2, 12, 18)), 6, True)
    want = oracle.build_feature_volume(feat, fr["src_exts"], Ks, fr["tar_ext"], Kt, dv, True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = costvol.build_feature_volume(t(feat), t(fr["src_exts"]), t(Ks), t(fr["tar_ext"]), t(Kt), t(dv), True)
    assert (want == 0).mean() < 0.9 and np.isfinite(want).all()
    assert max_abs(got.cpu().numpy(), want) <= 1e-4
    with pytest.raises(ValueError):
        costvol.build_feature_volume(t(feat), t(fr["src_exts"]), t(Ks), t(fr["tar_ext"])[:, :3], t(Kt), t(dv), True)


# ================================================================================================================
# Every instantiation against a float64 referee.
#
# Referee: the repo's own PyTorch formulation (networks/gdb_nerf/depth_net.py, the CPU branch of the module that calls the
# kernels), pinned to fixture F8 at float32 first, then evaluated on float64 copies of the float32 inputs (`ref64`).
# E_ref = max |oracle fp32 - ref64|: what the reference ARITHMETIC loses on this input; the kernel is not involved.
# Rule: max |hip - ref64| <= max(K_RULE * E_ref, 8 ulp(fp32) of max |ref64|) over the compared voxels.  K_RULE = 4: kernel and
# oracle are two realisations (another projection inverse, another order of the tap products) of one fp32 computation; the
# maximum of such an error over 1e4 .. 1e6 voxels moves by a small factor between realisations, while a wrong tap weight,
# a dropped border column or a wrong view count errs by the feature differences themselves (thousands of E_ref).
# Excluded voxels: only where, in float64, some view's depth z is below 1e-3 of the plane depth (the perspective divide
# next to the 1e-6 clamp amplifies rounding without bound); at most 1 % of a case, asserted in the CPU half.
# ================================================================================================================
import ctypes as C
import functools

from gdb_nerf_amd import _lib, costvol, synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks.gdb_nerf import depth_net

K_RULE = 4.0
EXCLUDED_CAP = 0.01
F32 = np.float32


def _ulp32(x):
    return float(np.spacing(F32(abs(x)))) if x else 0.0


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


VOL_KEYS = ("feat", "src_exts", "src_ints", "tar_ext", "tar_int", "dv")


def _torch_volume(c, dtype):
    a = [torch.from_numpy(np.ascontiguousarray(c[k])).to(dtype) for k in VOL_KEYS]
    return depth_net.build_feature_volume(*a, bool(c["inv"])).numpy()


def _excluded(c):
    """The exclusion rule on float64 alone: some view's z below 1e-3 of the plane depth (degenerate cases: or a plane at
    infinite / undefined depth, which the rule cannot rank)."""
    f = lambda k: np.asarray(c[k], np.float64)
    B, V = c["feat"].shape[:2]
    D, Ht, Wt = c["dv"].shape[1:]
    with np.errstate(all="ignore"):
        depth = 1.0 / f("dv") if c["inv"] else f("dv")
        P_tar = np.zeros((B, 4, 4)); P_tar[:, :3] = f("tar_int") @ f("tar_ext")[:, :3]; P_tar[:, 3, 3] = 1
        Hm = (f("src_ints") @ f("src_exts")[..., :3, :]) @ np.linalg.inv(P_tar)[:, None]      # (B,V,3,4)
        xs, ys = np.meshgrid(np.arange(Wt) + 0.5, np.arange(Ht) + 0.5, indexing="xy")
        rz = Hm[..., 2, 0, None, None] * xs + Hm[..., 2, 1, None, None] * ys + Hm[..., 2, 2, None, None]   # (B,V,Ht,Wt)
        z = rz[:, :, None] * depth[:, None] + Hm[..., 2, 3, None, None, None]                 # (B,V,D,Ht,Wt)
        bad = (z < 1e-3 * depth[:, None]).any(1) | ~np.isfinite(z).all(1) | ~np.isfinite(depth)
    return np.broadcast_to(bad[:, None], (B, c["feat"].shape[2], D, Ht, Wt))


def _strip(c, rows):
    """The same case restricted to target rows y0:y1 (the full-size V = 5 stage: the referee is evaluated on row strips)."""
    y0, y1 = rows
    s = dict(c)
    s["dv"] = np.ascontiguousarray(c["dv"][:, :, y0:y1])
    s["tar_int"] = c["tar_int"].copy()
    s["tar_int"][:, 1, 2] -= F32(y0)
    return s


def _referee_of(c):
    with np.errstate(all="ignore"):
        parts = [_strip(c, r) for r in c["strips"]] if c.get("strips") else [c]
        ref64 = np.concatenate([_torch_volume(p, torch.float64) for p in parts], axis=3)
        orc = np.concatenate([oracle.build_feature_volume(*(p[k] for k in VOL_KEYS), bool(p["inv"])) for p in parts], axis=3)
        excl = np.concatenate([_excluded(p) for p in parts], axis=3)
    keep = ~excl
    e_ref = float(np.abs(orc.astype(np.float64) - ref64)[keep].max()) if keep.any() else 0.0
    top = float(np.abs(ref64[keep]).max()) if keep.any() else 0.0
    return dict(ref64=ref64, oracle=orc, excl=excl, keep=keep, e_ref=e_ref, floor=8 * _ulp32(top), top=top)


def _rows_of(c, vol):
    """The rows of a full (B,C,D,Ht,Wt) result that the referee covers."""
    return np.concatenate([vol[:, :, :, y0:y1] for y0, y1 in c["strips"]], axis=3) if c.get("strips") else vol


def _rule(got, r, floor_only=False):
    """(error over the compared voxels, bound)."""
    err = float(np.abs(np.asarray(got, np.float64) - r["ref64"])[r["keep"]].max()) if r["keep"].any() else 0.0
    return err, (r["floor"] if floor_only else max(K_RULE * r["e_ref"], r["floor"]))


def _report(name, r, err, bound):
    ratio = err / r["e_ref"] if r["e_ref"] else float("nan")
    print(f"[costvol] {name}: E_ref {r['e_ref']:.3e}  hip err {err:.3e}  ratio {ratio:.2f}  bound {bound:.3e}  "
          f"max|ref64| {r['top']:.3e}  excluded {r['excl'].mean():.4f}")


# ---- case builders (shared by the CPU and the GPU half of every case) -------------------------------------------
def _hyp(rng, B, D, Ht, Wt, inv, perpix, near=425.0, far=905.0):
    if perpix:   # per-pixel windows of +-20 as in F8
        mid = (near + 20 + (far - near - 40) * rng.random((B, 1, Ht, Wt))).astype(F32)
        nf = np.concatenate((mid - F32(20), mid + F32(20)), 1)
    else:
        nf = np.broadcast_to(np.array([near, far], F32)[None, :, None, None], (B, 2, Ht, Wt))
    return np.ascontiguousarray(oracle.get_depth_values(nf, D, inv))


GEOM = {  # frame (Ho, Wo), source scale and size, target scale and size
    "q8": ((64, 96), 0.25, (16, 24), 0.125, (8, 12)),
    "h2": ((64, 96), 0.5, (32, 48), 0.5, (32, 48)),
    "odd": ((62, 90), 0.5, (31, 45), 0.25, (15, 23)),
}


def _frame_case(V, B, Cc, inv, perpix, geom, D, seed, smooth=0, offset=0.0, frame=None, ss=None, src=None, ts=None, tar=None, strips=None):
    """synthetic.make_frame cameras, intrinsics scaled per stage as DepthNet.forward does, features drawn per case."""
    if geom is not None:
        frame, ss, src, ts, tar = GEOM[geom]
    rng = np.random.default_rng(1000 + seed)
    fr = synthetic.make_frame(frame[0], frame[1], V=V, B=B, seed=seed, feat_dim=1, voxel_dim=1, num_depth=1)
    Ks, Kt = fr["src_ints"].copy(), fr["tar_int"].copy()
    Ks[..., :2, :] *= F32(ss); Kt[:, :2, :] *= F32(ts)
    feat = rng.standard_normal((B, V, Cc, src[0], src[1]), dtype=F32)
    if smooth:
        feat = synthetic._box(feat, smooth) * F32(smooth)
    feat = (feat + F32(offset)).astype(F32)
    return dict(feat=feat, src_exts=fr["src_exts"], src_ints=Ks, tar_ext=fr["tar_ext"], tar_int=Kt,
                dv=_hyp(rng, B, D, tar[0], tar[1], inv, perpix), inv=inv, strips=strips)


def _stage_case(s, V, Ho, Wo, seed, strips=None):
    """A cascade stage as DepthNet.forward builds it from configs/dtu_eval.yaml (C, D, scales, inv_depth from the config)."""
    cfg = make_cfg("configs/dtu_eval.yaml")
    lvl = cfg.mvs.vol_levels[s]
    ss, ts = cfg.fpn.feat_scales[lvl], cfg.mvs.vol_scales[s]
    return _frame_case(V, 1, cfg.fpn.feat_dims[lvl], bool(cfg.mvs.inv_depth[s]), s > 0, None, cfg.mvs.num_depth[s], seed, frame=(Ho, Wo),
                       ss=ss, src=(int(Ho * ss), int(Wo * ss)), ts=ts, tar=(int(Ho * ts), int(Wo * ts)), strips=strips)


def _shift_case(Cc, src, tar, shifts, seed, dyadic=True, depths=(256.0, 512.0, 1024.0), inv=False):
    """The warp as a pure pixel shift: identity extrinsics, one power-of-two focal length, source principal point = target
    principal point + (dx_v, dy_v).  Then p / z = (px + dx_v, py + dy_v) on every plane and the sampled coordinate is
    (x + dx_v, y + dy_v); with power-of-two sizes, dyadic shifts / features and power-of-two depths nothing rounds before the
    final products.  One view per entry of `shifts`.  The target is larger than the source, so its columns / rows sweep across
    both source borders whatever the shift: x0 = -1 (fx 0 and 0.5), x0 = Ws - 1, x0 = Ws, integer coordinates, y0 = -1, y0 = Hs - 1
    and every e0 / e1 hand-over are reached by construction."""
    rng = np.random.default_rng(2000 + seed)
    Hs, Ws = src
    Ht, Wt = tar
    V = len(shifts)
    f = F32(64.0)
    Kt = np.array([[f, 0, Wt / 2], [0, f, Ht / 2], [0, 0, 1]], F32)[None]
    Ks = np.stack([np.array([[f, 0, Wt / 2 + dx], [0, f, Ht / 2 + dy], [0, 0, 1]], F32) for dx, dy in shifts])[None]
    eye = np.eye(4, dtype=F32)
    feat = rng.standard_normal((1, V, Cc, Hs, Ws)).astype(F32)
    if dyadic:
        feat = (np.clip(np.round(feat * 8), -32, 32) / 8).astype(F32)
    dv = np.broadcast_to(np.array(depths, F32)[None, :, None, None], (1, len(depths), Ht, Wt)).copy()
    if inv:
        dv = (F32(1) / dv).astype(F32)
    return dict(feat=feat, src_exts=np.broadcast_to(eye, (1, V, 4, 4)).copy(), src_ints=Ks, tar_ext=eye[None].copy(), tar_int=Kt,
                dv=dv, inv=inv, shifts=list(shifts), exact=dyadic)


def _closed_form(c):
    """Expected volume of a shift case by hand, float64: per view the map shifted by (dx, dy), zero outside, the two
    neighbours blended with the fractions; biased variance over the views; the same on every plane."""
    feat = c["feat"][0].astype(np.float64)
    V, Cc, Hs, Ws = feat.shape
    D, Ht, Wt = c["dv"].shape[1:]
    pad = 4 + max(Ht, Wt)
    Z = np.zeros((V, Cc, Hs + 2 * pad, Ws + 2 * pad))
    Z[:, :, pad:pad + Hs, pad:pad + Ws] = feat
    warped = np.zeros((V, Cc, Ht, Wt))
    for v, (dx, dy) in enumerate(c["shifts"]):
        sx, sy = int(np.floor(dx)), int(np.floor(dy))
        fx, fy = dx - sx, dy - sy
        for j, wy in ((0, 1 - fy), (1, fy)):
            for i, wx in ((0, 1 - fx), (1, fx)):
                warped[v] += wy * wx * Z[v, :, pad + sy + j:pad + sy + j + Ht, pad + sx + i:pad + sx + i + Wt]
    var = ((warped - warped.mean(0)) ** 2).mean(0)
    return np.broadcast_to(var[None, :, None], (1, Cc, D, Ht, Wt))


def _behind_case():
    """View 1's camera is turned round: it lies in front of every plane looking away, z < 0 for every voxel of that view."""
    c = _frame_case(3, 1, 8, False, True, "h2", 6, seed=31)
    twin = dict(c, feat=c["feat"].copy(), src_exts=c["src_exts"].copy())
    twin["feat"][0, 1] = 0    # the twin: view 1 where it was, with an all-zero map - it contributes 0 as well, inside the rule's domain
    flip = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(F32)    # half a turn about the camera's y axis
    c["src_exts"][0, 1] = flip @ c["src_exts"][0, 1]
    c["degenerate"], c["twin"] = True, twin
    return c


def _infinite_case():
    """inv_depth with a hypothesis of 0: plane 2 lies at infinite depth (and a handful of single pixels on the other planes)."""
    c = _frame_case(4, 1, 8, True, False, "q8", 6, seed=32)
    c["dv"][:, 2] = 0
    c["dv"][0, 0, 3, 5] = 0; c["dv"][0, 5, 7, 11] = 0; c["dv"][0, 4, 0, 0] = 0
    c["degenerate"] = True
    return c


VOL_CASES = {
    # section 3: V = 1 .. 8, pair and planar
    "V1-planar-B1-C1-D1": lambda: _frame_case(1, 1, 1, False, False, "q8", 1, 1),
    "V1-pair-B2-C8-D6-inv": lambda: _frame_case(1, 2, 8, True, True, "h2", 6, 2),
    "V2-planar-B3-C7-D12-inv": lambda: _frame_case(2, 3, 7, True, False, "odd", 12, 3),
    "V2-pair-B1-C16-D6": lambda: _frame_case(2, 1, 16, False, True, "q8", 6, 4),
    "V3-planar-B2-C1-D12": lambda: _frame_case(3, 2, 1, False, True, "h2", 12, 5),
    "V3-pair-B1-C32-D6-inv": lambda: _frame_case(3, 1, 32, True, False, "odd", 6, 6),
    "V4-planar-B1-C7-D12-inv": lambda: _frame_case(4, 1, 7, True, True, "q8", 12, 7),
    "V4-pair-B3-C8-D6": lambda: _frame_case(4, 3, 8, False, False, "h2", 6, 8),
    "V4-pair-B1-C16-D1": lambda: _frame_case(4, 1, 16, False, True, "odd", 1, 9),
    "V5-planar-B2-C16-D6-inv": lambda: _frame_case(5, 2, 16, True, False, "odd", 6, 10),
    "V6-planar-B1-C7-D12": lambda: _frame_case(6, 1, 7, False, True, "q8", 12, 11),
    "V7-planar-B3-C8-D1-inv": lambda: _frame_case(7, 3, 8, True, True, "h2", 1, 12),
    "V8-planar-B1-C32-D6": lambda: _frame_case(8, 1, 32, False, False, "odd", 6, 13),
    # smooth features: E_ref drops with the smoothing, the rule turns sensitive to weights and variance arithmetic
    "V3-pair-smooth": lambda: _frame_case(3, 1, 8, False, True, "h2", 6, 14, smooth=5),
    "V4-pair-smooth": lambda: _frame_case(4, 2, 8, True, False, "h2", 6, 15, smooth=5),
    # large-magnitude features: the two-pass variance stays within the rule, a one-pass E[x^2] - E[x]^2 would not
    "V3-pair-plus30": lambda: _frame_case(3, 1, 8, False, True, "h2", 6, 16, offset=30.0),
    "V4-planar-plus100": lambda: _frame_case(4, 1, 7, True, False, "h2", 6, 17, offset=100.0),
    # section 4: constructed borders (pure pixel shifts)
    # 8 x 16 source (Hs - 1 = 7, Ws - 1 = 15), 12 x 20 target: expected values exact up to the final products
    "shift-8x16-V2-pair": lambda: _shift_case(4, (8, 16), (12, 20), [(-2, 0), (-1.5, -0.5)], 1),
    "shift-8x16-V4-pair": lambda: _shift_case(4, (8, 16), (12, 20), [(-1, -1), (-0.5, 0.25), (-0.25, 7), (0, 7.5)], 2),
    "shift-8x16-V4-pair-b": lambda: _shift_case(2, (8, 16), (12, 20), [(0.25, 8), (0.5, -2), (1, 0.5), (15, -0.25)], 3, inv=True),
    "shift-8x16-V4-planar": lambda: _shift_case(3, (8, 16), (12, 20), [(1, 0.5), (15, -0.25), (15.5, 1), (16, -1.5)], 4),
    "shift-8x16-V2-planar": lambda: _shift_case(3, (8, 16), (12, 20), [(15.5, 1), (-0.25, -1)], 5),
    "shift-8x16-V5-planar": lambda: _shift_case(4, (8, 16), (12, 20), [(-2, 0), (-1.5, -0.5), (-1, -1), (-0.5, 0.25), (-0.25, 7)], 6),
    "shift-8x16-V5-planar-b": lambda: _shift_case(3, (8, 16), (12, 20), [(0, 7.5), (0.25, 8), (0.5, -2), (1, 0.5), (16, -0.25)], 7),
    # Ws = 2, Hs = 1: the smallest source the launcher accepts
    "shift-1x2-V4-pair": lambda: _shift_case(2, (1, 2), (4, 6), [(-1.5, -0.5), (-1, 0), (-0.5, 0.25), (0, -1)], 8),
    "shift-1x2-V5-planar": lambda: _shift_case(3, (1, 2), (4, 6), [(0.25, 0), (0.5, 0.5), (1, -0.25), (1.5, -1.5), (2, 0)], 9),
    "shift-1x2-V2-pair": lambda: _shift_case(2, (1, 2), (4, 6), [(-0.25, -0.5), (1, 0.5)], 10),
    # 7 x 13 source, depths that are no powers of two: the normalise / un-normalise pair rounds, the general rule applies
    "shift-7x13-V4-pair": lambda: _shift_case(4, (7, 13), (11, 17), [(-2, 0), (-1.5, -0.5), (-1, 6), (-0.5, 6.5)], 11, dyadic=False,
                                              depths=(430.0, 611.3, 902.7)),
    "shift-7x13-V2-planar": lambda: _shift_case(3, (7, 13), (11, 17), [(12.5, 1), (-0.25, -1)], 12, dyadic=False, depths=(430.0, 611.3, 902.7)),
    "shift-7x13-V5-planar": lambda: _shift_case(4, (7, 13), (11, 17), [(0, 7), (0.25, -2), (0.5, 0.5), (1, -0.25), (12, 0)], 13, dyadic=False,
                                                depths=(430.0, 611.3, 902.7), inv=True),
    "behind-V3": _behind_case,
    "infinite-V4": _infinite_case,
    # section 7: launch geometry
    "grid-1-block": lambda: _frame_case(3, 1, 8, False, True, None, 1, 18, frame=(64, 64), ss=0.25, src=(16, 16), ts=0.25, tar=(16, 16)),
    "grid-3-blocks": lambda: _frame_case(3, 1, 7, True, False, None, 3, 19, frame=(64, 64), ss=0.25, src=(16, 16), ts=0.25, tar=(16, 16)),
    "grid-10-blocks-ragged": lambda: _frame_case(2, 1, 8, False, True, "odd", 5, 20),
    "dtu-stage0-512x640": lambda: _stage_case(0, 3, 512, 640, 21),
    "dtu-stage1-512x640": lambda: _stage_case(1, 3, 512, 640, 22),
    # V = 5 at the 1200 x 1600 stage-1 size: the kernel runs the whole stage, the float64 referee three 8-row strips of it (top,
    # middle, bottom: 3.1e5 x 8 planes x 16 channels voxels compared; the whole volume in float64 would take 2.5 GB per view set)
    "dtu-stage1-1200x1600-V5-strips": lambda: _stage_case(1, 5, 1200, 1600, 23, strips=((0, 8), (296, 304), (592, 600))),
}
VOL_IDS = list(VOL_CASES)


@functools.lru_cache(maxsize=None)
def _vol_case(name):
    c = VOL_CASES[name]()
    return c, _referee_of(c)


def _is_pair(c):
    return c["feat"].shape[2] % 2 == 0 and c["feat"].shape[1] <= 4


def test_torch_formulation_matches_reference_f8(f8):
    """The referee before it is one: depth_net.build_feature_volume / depth_regression at float32 on the CPU against F8,
    under the bounds of test_oracle_cost_volume_matches_reference."""
    for tag in ("coarse", "fine"):
        c = _case(f8, tag)
        t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k]))
        vol = depth_net.build_feature_volume(t("src_feat"), t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("depth_values"), bool(c["inv_depth"]))
        assert tuple(vol.shape) == c["volume"].shape and vol.dtype == torch.float32
        assert max_abs(vol.numpy(), c["volume"]) <= 1e-4
        d, ci = depth_net.depth_regression(t("depth_values"), t("prob"), 1.0, bool(c["inv_depth"]))
        assert max_abs(d.numpy(), c["depth"]) <= 1e-5 * float(np.abs(c["depth"]).max())
        assert max_abs(ci.numpy(), c["ci"]) <= 1e-5 * float(np.abs(c["ci"]).max())
        # and the float64 run is a refinement of the same thing, not something else
        a64 = [t(k).double() for k in ("src_feat", "src_exts", "src_ints", "tar_ext", "tar_int", "depth_values")]
        v64 = depth_net.build_feature_volume(*a64, bool(c["inv_depth"]))
        assert v64.dtype == torch.float64 and max_abs(v64.numpy(), c["volume"]) <= 1e-4


def test_case_table_covers_what_it_claims():
    """V = 1 .. 8; pair and planar for every V <= 4; B, C, D, both inv_depth settings, per-pixel and broadcast ranges."""
    sec3 = [VOL_CASES[n]() for n in VOL_IDS if n[0] == "V" and "smooth" not in n and "plus" not in n]
    assert {c["feat"].shape[1] for c in sec3} == set(range(1, 9))
    for V in (1, 2, 3, 4):
        assert {_is_pair(c) for c in sec3 if c["feat"].shape[1] == V} == {True, False}
    assert {c["feat"].shape[0] for c in sec3} == {1, 2, 3} and {c["feat"].shape[2] for c in sec3} == {1, 7, 8, 16, 32}
    assert {c["dv"].shape[1] for c in sec3} == {1, 6, 12} and {c["inv"] for c in sec3} == {True, False}
    assert {(c["feat"].shape[3:], c["dv"].shape[2:]) for c in sec3} == {((16, 24), (8, 12)), ((32, 48), (32, 48)), ((31, 45), (15, 23))}
    assert {bool(np.ptp(c["dv"][:, 0]) > 0) for c in sec3} == {True, False}
    for n, pair in (("V", None), ("shift-8x16-V2-pair", True), ("shift-8x16-V5-planar", False), ("shift-1x2-V4-pair", True)):
        if pair is not None:
            assert _is_pair(VOL_CASES[n]()) == pair and (("pair" in n) == pair)
    for n in VOL_IDS:
        if "-pair" in n or "-planar" in n:
            assert _is_pair(VOL_CASES[n]()) == ("-pair" in n), n
    c0, c1, c5 = (VOL_CASES[n]() for n in ("dtu-stage0-512x640", "dtu-stage1-512x640", "dtu-stage1-1200x1600-V5-strips"))
    assert c0["feat"].shape == (1, 3, 32, 128, 160) and c0["dv"].shape == (1, 64, 64, 80) and c0["inv"] is True
    assert c1["feat"].shape == (1, 3, 16, 256, 320) and c1["dv"].shape == (1, 8, 256, 320) and c1["inv"] is False
    assert c5["feat"].shape == (1, 5, 16, 600, 800) and c5["dv"].shape == (1, 8, 600, 800)
    blocks = lambda c: c["dv"].shape[0] * c["dv"].shape[1] * ((c["dv"].shape[2] * c["dv"].shape[3] + 255) // 256)
    assert [blocks(VOL_CASES[n]()) for n in ("grid-1-block", "grid-3-blocks", "grid-10-blocks-ragged")] == [1, 3, 10]
    assert (15 * 23) % 256 != 0


@pytest.mark.parametrize("name", VOL_IDS)
def test_cost_volume_case_referee(name):
    """CPU half of every cost-volume case: the inputs, ref64, the fp32 oracle, E_ref, the exclusion cap, and the closed form of
    the constructed shifts - proven sane before a GPU is involved."""
    c, r = _vol_case(name)
    V = c["feat"].shape[1]
    print(f"[costvol cpu] {name}: E_ref {r['e_ref']:.3e}  floor {r['floor']:.3e}  max|ref64| {r['top']:.3e}  excluded {r['excl'].mean():.4f}")
    assert r["ref64"].dtype == np.float64 and r["oracle"].dtype == np.float32 and r["ref64"].shape == r["oracle"].shape
    if c.get("degenerate"):
        # built to leave the rule's domain: the oracle stays finite everywhere and sees the other views
        assert np.isfinite(r["oracle"]).all() and (r["oracle"] != 0).any() and r["excl"].any()
        if "twin" in c:   # a view behind the planes contributes exactly 0: the volume is that of the twin, which the rule covers
            rt = _referee_of(c["twin"])
            assert r["excl"].all() and not rt["excl"].any() and rt["e_ref"] > 0
            assert np.array_equal(r["oracle"], rt["oracle"])
    else:
        assert r["excl"].mean() <= EXCLUDED_CAP
        assert np.isfinite(r["ref64"]).all() and np.isfinite(r["oracle"]).all()
    if "shifts" in c:
        want = _closed_form(c)
        assert (want != 0).mean() > 0.1                      # the views overlap the target: the variance is not trivially 0
        assert np.abs(r["ref64"] - want).max() <= 1e-10 * max(1.0, r["top"])
        if c["exact"]:   # nothing rounds before the final products: fp32 arithmetic reaches the floor
            assert r["e_ref"] <= r["floor"]
    elif V == 1:
        assert r["e_ref"] == 0 and not r["ref64"].any()      # the variance of one view
    elif not c.get("degenerate"):
        assert r["e_ref"] > 0 and r["top"] > 0.1


def _raw_volume(c, entry, pair_ws=None, poison=True, feat=None):
    """The C entries through ctypes, with the output and both scratch buffers holding NaN beforehand."""
    lib = _lib.load()
    B, V, Cc, Hs, Ws = c["feat"].shape
    D, Ht, Wt = c["dv"].shape[1:]
    fill = float("nan") if poison else 0.0
    args = [_cuda(c[k]) if (k != "feat" or feat is None) else feat for k in VOL_KEYS]
    out = torch.full((B, Cc, D, Ht, Wt), fill, device="cuda")
    ws = torch.full((B * V * 12,), fill, device="cuda")
    tail = [ws.data_ptr()]
    if entry == "ws":
        pw = torch.full((B * V * Cc * Hs * Ws,), fill, device="cuda") if pair_ws else None
        tail.append(None if pw is None else pw.data_ptr())
    fn = lib.gdb_build_feature_volume_ws if entry == "ws" else lib.gdb_build_feature_volume
    _lib.check(fn(*(t.data_ptr() for t in args), B, V, Cc, Hs, Ws, D, Ht, Wt, int(c["inv"]), *tail, out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", VOL_IDS)
def test_hip_cost_volume_vs_float64(name):
    """Every k_costvol<V, PAIR> instantiation, both C entries and both layouts against the float64 referee under the rule above.
    Degenerate cases (a camera behind the planes, a plane at infinite depth): outside the rule's domain the kernel's output is
    finite and has the fp32 oracle's zero / non-zero pattern (a view that contributes nothing contributes nothing in both).  The
    float64 PyTorch formulation agrees there as well as far as it is defined: behind the camera it divides by the 1e-6 clamp
    like everyone else and samples far outside (0); at infinite depth p is inf or NaN, grid_sample is handed NaN coordinates
    and what it returns for them is not specified - those voxels are in the excluded set and never compared."""
    c, r = _vol_case(name)
    B, V, Cc, Hs, Ws = c["feat"].shape
    dev = {k: _cuda(c[k]) for k in VOL_KEYS}
    full = costvol.build_feature_volume(*(dev[k] for k in VOL_KEYS), c["inv"])
    got = _rows_of(c, full.cpu().numpy())
    err, bound = _rule(got, r, floor_only=c.get("exact", False))
    _report(name, r, err, bound)
    assert got.shape == r["ref64"].shape
    assert err <= bound
    if c.get("degenerate"):
        assert np.isfinite(got).all()
        assert np.array_equal(got[r["excl"]] == 0, r["oracle"][r["excl"]] == 0)
    if "twin" in c:   # the values of the all-excluded case: bit for bit those of its twin, and the twin is held to the rule
        rt = _referee_of(c["twin"])
        twin = costvol.build_feature_volume(*(_cuda(c["twin"][k]) for k in VOL_KEYS), c["inv"])
        err_t, bound_t = _rule(twin.cpu().numpy(), rt)
        _report(name + " (twin)", rt, err_t, bound_t)
        assert err_t <= bound_t and torch.equal(full, twin)
    if "shifts" in c and c["exact"]:
        assert np.abs(got - _closed_form(c)).max() <= r["floor"]
    if c.get("strips"):
        return     # the full-size V = 5 stage: the value check above is what it is for
    # the planar form of the same call, the plain entry, a NULL pair scratch: bit-identical; NaN in output and scratch: ignored
    planar = costvol.build_feature_volume(*(dev[k] for k in VOL_KEYS), c["inv"], pair_layout=False)
    if _is_pair(c):
        assert torch.equal(full, planar)
    plain, ws_null = _raw_volume(c, "plain"), _raw_volume(c, "ws", pair_ws=False)
    assert torch.equal(plain, ws_null) and torch.equal(plain, planar)
    assert torch.equal(_raw_volume(c, "ws", pair_ws=True), full)
    # a non-contiguous src_feat (a channel and column slice of a wider tensor) against its contiguous copy
    wide = torch.full((B, V, Cc + 3, Hs, Ws + 1), float("nan"), device="cuda")
    wide[:, :, 2:2 + Cc, :, :Ws] = dev["feat"]
    view = wide[:, :, 2:2 + Cc, :, :Ws]
    assert not view.is_contiguous()
    assert torch.equal(costvol.build_feature_volume(view, *(dev[k] for k in VOL_KEYS[1:]), c["inv"]), full)


# ---- section 5: the bounds must see a slip -----------------------------------------------------------------------
SLIP_CASES = ("V3-pair-smooth", "V4-pair-smooth", "V3-pair-C32-noise")
VOL_CASES["V3-pair-C32-noise"] = VOL_CASES["V3-pair-B1-C32-D6-inv"]


def _slipped(c, kind):
    s = dict(c)
    if kind == "pp":        # source principal point of view 1 moved by 1/64 pixel: a mis-weighted tap
        s["src_ints"] = c["src_ints"].copy()
        s["src_ints"][:, 1, 0, 2] += F32(1 / 64)
    else:                   # view 1's feature map scaled by 1 + 2^-12: a value-path slip
        s["feat"] = c["feat"].copy()
        s["feat"][:, 1] *= F32(1 + 2.0 ** -12)
    return s


@pytest.mark.parametrize("name", SLIP_CASES)
def test_the_rule_sees_a_slip_in_the_oracle(name):
    """CPU half of the slip test, and the rule's power shown without a GPU: the fp32 ORACLE fed slightly wrong inputs fails the
    rule against the ref64 of the right inputs (and passes on the right ones, by construction with ratio 1).  On the smooth cases
    both slips must be seen; on the white-noise case it is reported which are."""
    c, r = _vol_case(name)
    for kind in ("pp", "scale"):
        s = _slipped(c, kind)
        with np.errstate(all="ignore"):
            bad = oracle.build_feature_volume(*(s[k] for k in VOL_KEYS), bool(s["inv"]))
        err, bound = _rule(bad, r)
        print(f"[costvol cpu slip] {name} {kind}: E_ref {r['e_ref']:.3e}  bound {bound:.3e}  slipped oracle err {err:.3e}  seen {err > bound}")
        if "smooth" in name:
            assert err > bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", SLIP_CASES)
def test_hip_the_rule_sees_a_slip(name):
    """In the spirit of test_the_bounds_see_a_1e4_bias_slip, without touching the kernel: the HIP entry fed slightly wrong inputs
    must FAIL the rule against the ref64 of the right inputs, and pass it on the right ones."""
    c, r = _vol_case(name)
    run = lambda k: costvol.build_feature_volume(*(_cuda(k[n]) for n in VOL_KEYS), k["inv"]).cpu().numpy()
    good, bound = _rule(run(c), r)
    _report(name + " (right inputs)", r, good, bound)
    assert good <= bound
    for kind in ("pp", "scale"):
        bad, _ = _rule(run(_slipped(c, kind)), r)
        print(f"[costvol slip] {name} {kind}: err {bad:.3e} against bound {bound:.3e}: seen {bad > bound}")
        if "smooth" in name:
            assert bad > bound


# ---- section 6: depth regression ---------------------------------------------------------------------------------
CFG_CI = float(make_cfg("configs/dtu_eval.yaml").mvs.ci_scales[0])
#            B   D   H    W   inv    prob       hyp        ci_scale
REG_CASES = {
    "D1-1x1": (1, 1, 1, 1, False, "softmax", "range", CFG_CI),
    "D1-5x7-inv-ci50": (3, 1, 5, 7, True, "softmax", "window", 50.0),
    "D2-5x7-onehot": (1, 2, 5, 7, False, "onehot", "window", CFG_CI),
    "D2-37x45-inv-uniform": (3, 2, 37, 45, True, "uniform", "range", 0.5),
    "D8-37x45-peaked": (3, 8, 37, 45, False, "peaked", "window", CFG_CI),
    "D8-128x160-inv-onehot": (1, 8, 128, 160, True, "onehot", "window", 2.5),
    "D8-5x7-ci0": (3, 8, 5, 7, False, "softmax", "window", 0.0),
    "D8-37x45-ci50": (3, 8, 37, 45, False, "softmax", "window", 50.0),
    "D36-37x45-inv": (3, 36, 37, 45, True, "softmax", "range", CFG_CI),
    "D36-5x7-unnormalised": (1, 36, 5, 7, False, "positive", "range", 2.5),
    "D64-128x160-inv": (1, 64, 128, 160, True, "softmax", "range", CFG_CI),
    "D64-37x45-inv-ci50": (3, 64, 37, 45, True, "uniform", "range", 50.0),
    "D64-1x1-peaked-inv": (3, 64, 1, 1, True, "peaked", "range", 0.5),
    "D192-37x45-unnormalised-inv": (3, 192, 37, 45, True, "positive", "window", CFG_CI),
    "D192-128x160": (3, 192, 128, 160, False, "softmax", "range", 2.5),
    "D192-5x7-onehot-ci0": (1, 192, 5, 7, False, "onehot", "range", 0.0),
}
REG_IDS = list(REG_CASES)


@functools.lru_cache(maxsize=None)
def _reg_case(name):
    B, D, H, W, inv, pk, hk, ci_scale = REG_CASES[name]
    rng = np.random.default_rng(3000 + REG_IDS.index(name))
    hyp = _hyp(rng, B, D, H, W, inv, hk == "window")
    noise = rng.standard_normal((B, D, H, W))
    pick = rng.integers(0, D, (B, 1, H, W))
    if pk in ("softmax", "peaked"):
        e = np.exp((noise * (20 if pk == "peaked" else 1)) - (noise * (20 if pk == "peaked" else 1)).max(1, keepdims=True))
        prob = e / e.sum(1, keepdims=True)
    elif pk == "onehot":
        prob = (np.arange(D).reshape(1, D, 1, 1) == pick).astype(np.float64)
    elif pk == "uniform":
        prob = np.full((B, D, H, W), 1.0 / D)
    else:
        prob = 0.05 + 3 * rng.random((B, D, H, W))
    prob = prob.astype(F32)
    with np.errstate(all="ignore"):
        d64, ci64 = (t.numpy() for t in depth_net.depth_regression(_t64(hyp), _t64(prob), ci_scale, inv))
        d32, ci32 = oracle.depth_regression(hyp, prob, ci_scale, inv)
    ref = dict(hyp=hyp, prob=prob, pick=pick, inv=inv, ci_scale=ci_scale, kind=pk, d64=d64, ci64=ci64, d32=d32, ci32=ci32)
    for k in ("d", "ci"):
        ref["e_" + k] = max_abs(ref[k + "32"], ref[k + "64"])
        ref["floor_" + k] = 8 * _ulp32(float(np.abs(ref[k + "64"]).max()))
    return ref


def _ends(r):
    """What a fully clipped interval is: the first / last hypothesis (their fp32 reciprocals under inv_depth)."""
    e = r["hyp"][:, [0, -1]]
    return (F32(1) / e).astype(F32) if r["inv"] else e


def _check_regression_corners(r, depth, ci):
    if r["ci_scale"] == 50.0:
        assert np.array_equal(ci, _ends(r))
    if r["kind"] == "onehot":
        sel = np.take_along_axis(r["hyp"], r["pick"], 1)
        sel = (F32(1) / sel).astype(F32) if r["inv"] else sel
        assert np.all(np.abs(depth.astype(np.float64) - sel) <= np.spacing(np.abs(sel)))


@pytest.mark.parametrize("name", REG_IDS)
def test_depth_regression_case_referee(name):
    """CPU half: float64 formulation, fp32 oracle, E_ref and the corners (interval on the hypothesis ends at ci_scale 50, the
    selected hypothesis for one-hot probabilities) on the oracle."""
    r = _reg_case(name)
    print(f"[depthreg cpu] {name}: depth E_ref {r['e_d']:.3e} floor {r['floor_d']:.3e}   ci E_ref {r['e_ci']:.3e} floor {r['floor_ci']:.3e}")
    assert np.isfinite(r["d64"]).all() and np.isfinite(r["ci64"]).all() and np.isfinite(r["d32"]).all() and np.isfinite(r["ci32"]).all()
    assert r["d64"].shape == r["d32"].shape == (r["hyp"].shape[0], 1) + r["hyp"].shape[2:]
    assert r["e_d"] <= 1e-5 * np.abs(r["d64"]).max() and r["e_ci"] <= 1e-5 * np.abs(r["ci64"]).max()
    _check_regression_corners(r, r["d32"], r["ci32"])
    if r["kind"] == "onehot":   # var = 0 in exact arithmetic: the 1e-12 clamp decides the half width
        assert np.abs(np.abs(r["ci64"] - r["d64"]).max()) <= max(1.0, r["ci_scale"]) * 1.001e-6 * (np.abs(r["ci64"]).max() ** 2 if r["inv"] else 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REG_IDS)
def test_hip_depth_regression_vs_float64(name):
    r = _reg_case(name)
    d, ci = costvol.depth_regression(_cuda(r["hyp"]), _cuda(r["prob"]), r["ci_scale"], r["inv"])
    d, ci = d.cpu().numpy(), ci.cpu().numpy()
    for k, got in (("d", d), ("ci", ci)):
        err, bound = max_abs(got, r[k + "64"]), max(K_RULE * r["e_" + k], r["floor_" + k])
        ratio = err / r["e_" + k] if r["e_" + k] else float("nan")
        print(f"[depthreg] {name} {'depth' if k == 'd' else 'ci'}: E_ref {r['e_' + k]:.3e}  hip err {err:.3e}  ratio {ratio:.2f}  bound {bound:.3e}")
        assert err <= bound
    _check_regression_corners(r, d, ci)


@pytest.mark.parametrize("name", ["D8-37x45-peaked", "D36-37x45-inv"])
def test_the_rule_sees_a_ci_scale_slip_in_the_oracle(name):
    r = _reg_case(name)
    with np.errstate(all="ignore"):
        _, bad = oracle.depth_regression(r["hyp"], r["prob"], r["ci_scale"] * (1 + 2.0 ** -10), r["inv"])
    err, bound = max_abs(bad, r["ci64"]), max(K_RULE * r["e_ci"], r["floor_ci"])
    print(f"[depthreg cpu slip] {name}: ci_scale (1 + 2^-10): err {err:.3e} against bound {bound:.3e}")
    assert err > bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["D8-37x45-peaked", "D36-37x45-inv"])
def test_hip_the_rule_sees_a_ci_scale_slip(name):
    r = _reg_case(name)
    _, bad = costvol.depth_regression(_cuda(r["hyp"]), _cuda(r["prob"]), r["ci_scale"] * (1 + 2.0 ** -10), r["inv"])
    err, bound = max_abs(bad.cpu().numpy(), r["ci64"]), max(K_RULE * r["e_ci"], r["floor_ci"])
    print(f"[depthreg slip] {name}: ci_scale (1 + 2^-10): err {err:.3e} against bound {bound:.3e}")
    assert err > bound


# ---- section 8: refusals ------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    """NULL arguments, shapes outside what the kernels index and launch grids outside what HIP takes are refused with a status and
    a message before anything is launched: the pointers here are host integers, a launch on them would fail, a refusal never gets
    there.  costvol.py's own ValueErrors likewise need no device."""
    lib = _lib.load()
    fake = 4096
    shape = dict(B=1, V=3, C=8, Hs=8, Ws=8, D=4, Ht=8, Wt=8)

    def vol(entry="ws", null=None, **kw):
        s = dict(shape, **kw)
        ptrs = [None if null == i else fake for i in range(6)]
        tail = [None if null == 6 else fake] + ([None] if entry == "ws" else []) + [None if null == 7 else fake]
        fn = lib.gdb_build_feature_volume_ws if entry == "ws" else lib.gdb_build_feature_volume
        return fn(*ptrs, s["B"], s["V"], s["C"], s["Hs"], s["Ws"], s["D"], s["Ht"], s["Wt"], 0, *tail, None)

    for entry in ("ws", "plain"):
        for i in range(8):
            assert vol(entry, null=i) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error()
        for kw in (dict(Ws=1), dict(B=0), dict(D=0), dict(V=0), dict(C=0), dict(Hs=0), dict(Ht=0), dict(Wt=-1)):
            assert vol(entry, **kw) == _lib.GDB_E_SHAPE and b"shape" in lib.gdb_last_error(), kw
        assert vol(entry, V=_lib.GDB_MAX_VIEWS + 1) == _lib.GDB_E_SHAPE and b"views" in lib.gdb_last_error()
        assert vol(entry, C=65536, Hs=256, Ws=256) == _lib.GDB_E_SHAPE and b"32-bit" in lib.gdb_last_error()
        assert vol(entry, B=32768, D=65536, Ht=1, Wt=1) == _lib.GDB_E_SHAPE and b"launch grid" in lib.gdb_last_error()
        assert vol(entry, Ht=65536, Wt=65536) == _lib.GDB_E_SHAPE and b"launch grid" in lib.gdb_last_error()   # Ht * Wt beyond an int
        assert vol(entry, B=2 ** 31 - 1, D=2 ** 31 - 1, Ht=2 ** 15, Wt=2 ** 15) == _lib.GDB_E_SHAPE and b"launch grid" in lib.gdb_last_error()

    reg = lambda p=(fake,) * 4, B=1, D=4, H=8, W=8: lib.gdb_depth_regression(p[0], p[1], B, D, H, W, 1.0, 0, p[2], p[3], None)
    for i in range(4):
        assert reg(tuple(None if i == j else fake for j in range(4))) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error()
    for kw in (dict(B=0), dict(D=0), dict(H=0), dict(W=-3)):
        assert reg(**kw) == _lib.GDB_E_SHAPE and b"shape" in lib.gdb_last_error()

    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
    a = lambda **kw: [kw.get("feat", z(1, 3, 8, 8, 8)), kw.get("se", z(1, 3, 4, 4)), kw.get("si", z(1, 3, 3, 3)), kw.get("te", z(1, 4, 4)),
                      kw.get("ti", z(1, 3, 3)), kw.get("dv", z(1, 4, 8, 8))]
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.build_feature_volume(*a(), False)
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.build_feature_volume(*a(feat=z(1, 3, 8, 8, 8, dtype=torch.float64)), False)
    for kw in (dict(se=z(1, 2, 4, 4)), dict(si=z(1, 3, 3, 4)), dict(te=z(1, 3, 4)), dict(ti=z(2, 3, 3)), dict(dv=z(2, 4, 8, 8))):
        with pytest.raises(ValueError, match="inconsistent"):
            costvol.build_feature_volume(*a(**kw), False)
    with pytest.raises(ValueError, match="depth_prob shape"):
        costvol.depth_regression(z(1, 4, 8, 8), z(1, 5, 8, 8), 1.0, False)
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.depth_regression(z(1, 4, 8, 8), z(1, 4, 8, 8), 1.0, False)
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.depth_regression(z(1, 4, 8, 8, dtype=torch.float64), z(1, 4, 8, 8, dtype=torch.float64), 1.0, False)

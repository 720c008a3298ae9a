"""The cascade depth net as one library call per stage: gdb_mvs_stage / gdb_mvs_hypotheses (include/gdb_nerf_hip.h),
costvol.MvsStage and the `mvs.hip_cascade` switch of DepthNet.

Rule (tests/test_costvol.py, tests/test_cost_reg_referee.py): referee = the repo's PyTorch formulation (depth_net.py, the branch
DepthNet.forward takes on CPU tensors) on float64 copies of the fp32 inputs; E_ref = max |fp32 CPU formulation - ref64|, no kernel
involved; pass when max |hip - ref64| <= max(4 E_ref, 8 ulp32 of max |ref64|).  K = 4 and the floor are those tests' own.
Every GPU case has a CPU half that proves its inputs and its referee first."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gdb_oracle as oracle
from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, costvol, synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf import depth_net
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d

K_RULE = 4.0
F32 = np.float32
NEW_ENTRIES = ("gdb_mvs_stage_workspace_bytes", "gdb_mvs_stage", "gdb_mvs_hypotheses")


def _ulp32(x):
    return float(np.spacing(F32(abs(x)))) if x else 0.0


def _bound(e_ref, ref64):
    return max(K_RULE * e_ref, 8 * _ulp32(float(np.abs(ref64).max())))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ================================================================================================================
# Without a GPU
# ================================================================================================================
def test_signature_table_and_exports():
    """_lib lists the new entries and the cross-compiled library exports them (load() resolves every listed symbol); the ABI
    version did not move."""
    for name in NEW_ENTRIES:
        assert name in _lib._SIGNATURES and name in _lib.EXPORTS
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert getattr(lib, name).restype is C.c_int
    assert lib.gdb_abi_version() == 7 == _lib.ABI_VERSION
    assert callable(costvol.MvsStage) and callable(costvol.mvs_hypotheses)


def _f7_net(**opts):
    f7 = load_golden("F7_network")
    flat = [x for kv in opts.items() for x in (kv[0], str(kv[1]))]
    net = make_network(make_cfg("configs/dtu_eval.yaml", flat)).eval()
    sd = {k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in f7.items() if k.startswith("sd.")}
    net.load_state_dict(sd, strict=True)
    return f7, net


def test_switch_is_read_and_inert_on_cpu_tensors():
    """mvs.hip_cascade defaults to false; on CPU tensors (and in training mode) DepthNet returns exactly what it returns with the
    switch off: today's code runs."""
    assert make_network(make_cfg("configs/dtu_eval.yaml")).depth_net.hip_cascade is False
    f7, net = _f7_net(**{"mvs.hip_cascade": True})
    d = net.depth_net
    assert d.hip_cascade is True
    cuda_like = type("T", (), {"is_cuda": True, "dtype": torch.float32})()
    half_like = type("T", (), {"is_cuda": True, "dtype": torch.float16})()
    assert d.use_hip_cascade(cuda_like, cuda_like) and not d.use_hip_cascade(cuda_like, torch.zeros(1)) and not d.use_hip_cascade(cuda_like, half_like)
    d.train()
    assert not d.use_hip_cascade(cuda_like)
    d.eval()
    t = lambda k: torch.from_numpy(f7[k])
    src = t("src_images")
    with torch.no_grad():
        ms = [f.unflatten(0, (1, 3)) for f in net.feature_net(src.flatten(0, 1))]
        on = d(src, ms, t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("near_far"))
        d.hip_cascade = False
        off = d(src, ms, t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("near_far"))
    assert len(on) == len(off) == 5 and on[4] == off[4] == []
    for a, b in zip(on[:4], off[:4]):
        assert len(a) == len(b) == d.num_stages
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- the glue restated in float64 numpy ---------------------------------------------------------------------------
def _up64(r, ratio, Ht, Wt, align_corners=False):
    """F.interpolate(r, scale_factor=ratio, mode="bilinear", align_corners=False) on float64, cropped / indexed to (Ht, Wt):
    src = max((dst + 0.5) / ratio - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), weights 1 - frac and frac."""
    r = np.asarray(r, np.float64)
    hr, wr = r.shape[2:]

    def axis(n_out, n_in):
        s = np.maximum((np.arange(n_out) + 0.5) / ratio - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(int), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, s - np.floor(s)
    y0, y1, fy = axis(Ht, hr)
    x0, x1, fx = axis(Wt, wr)
    fy = fy[:, None]
    row = lambda yy: (1 - fx) * r[:, :, yy][..., x0] + fx * r[:, :, yy][..., x1]
    return (1 - fy) * row(y0) + fy * row(y1)


def _steps64(D):
    """get_depth_values draws its steps with torch.linspace(0, 1, D) at the default dtype, float32, whatever the range's dtype:
    linspace's two-sided formula in fp32 (step = 1 / (D - 1); i * step below D // 2, 1 - (D - 1 - i) * step from there on)."""
    if D == 1:
        return np.zeros(1)
    st, i = F32(1) / F32(D - 1), np.arange(D)
    up, down = (st * i.astype(F32)).astype(F32), (F32(1) - (st * (D - 1 - i).astype(F32)).astype(F32)).astype(F32)
    return np.where(i < D // 2, up, down).astype(np.float64)


def _hyp64(search, ratio, D, Ht, Wt, inv):
    s = np.asarray(search, np.float64)
    s = np.broadcast_to(s.reshape(s.shape[0], 2, 1, 1), (s.shape[0], 2, Ht, Wt)) if s[0, 0].size == 1 else _up64(s, ratio, Ht, Wt)
    lo, hi = s[:, :1], s[:, 1:]
    if inv:
        lo, hi = 1.0 / lo, 1.0 / hi
    return lo + (hi - lo) * _steps64(D).reshape(1, D, 1, 1)


def _regress64(hyp, logits, ci_scale, inv):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    mean = (p * hyp).sum(1, keepdims=True)
    var = (p * (hyp - mean) ** 2).sum(1, keepdims=True)
    half = ci_scale * np.sqrt(np.maximum(var, 1e-12))
    first, last = hyp[:, :1], hyp[:, -1:]
    if inv:
        return 1.0 / mean[:, 0], 1.0 / np.concatenate((np.minimum(mean + half, first), np.maximum(mean - half, last)), 1), var
    return mean[:, 0], np.concatenate((np.maximum(mean - half, first), np.minimum(mean + half, last)), 1), var


def _hyp_torch(search, ratio, D, Ht, Wt, inv, dtype, align_corners=False):
    """The repo's formulation as DepthNet.forward strings it together (depth_net.py:132-156)."""
    s = torch.from_numpy(np.ascontiguousarray(search)).to(dtype)
    if s[0, 0].numel() == 1:
        s = s.reshape(s.shape[0], 2, 1, 1)
    else:
        s = F.interpolate(s, scale_factor=ratio, mode="bilinear", align_corners=align_corners)[:, :, :Ht, :Wt]
    return depth_net.get_depth_values(s, D, inv).expand(-1, -1, Ht, Wt).contiguous()


@pytest.mark.parametrize("inv", [False, True])
def test_float64_glue_is_pinned_to_the_fp32_formulation(inv):
    """The float64 restatement above against the repo's own fp32 F.interpolate + get_depth_values + softmax + depth_regression on
    the CPU: they differ by fp32 rounding only."""
    rng = np.random.default_rng(5 + inv)
    mid = (445 + 440 * rng.random((2, 1, 5, 7))).astype(F32)
    search = np.concatenate((mid - F32(20), mid + F32(20)), 1)
    for ratio, (Ht, Wt), D in ((2, (10, 14), 8), (4, (20, 28), 5), (4, (19, 27), 64), (2, (9, 13), 1)):
        h32 = _hyp_torch(search, float(ratio), D, Ht, Wt, inv, torch.float32)
        h64 = _hyp64(search, ratio, D, Ht, Wt, inv)
        assert tuple(h32.shape) == h64.shape
        assert max_abs(h32.numpy(), h64) <= 4 * _ulp32(float(np.abs(h64).max()))
        # at float64 only the steps may differ, by an fp32 ulp (torch's vectorised linspace against the formula above)
        width = float(np.abs(h64[:, -1] - h64[:, 0]).max())
        assert max_abs(_hyp_torch(search, float(ratio), D, Ht, Wt, inv, torch.float64).numpy(), h64) <= 2.0 ** -23 * width + 1e-12 * float(np.abs(h64).max())
        logits = (2 * rng.standard_normal(h64.shape)).astype(F32)
        d32, ci32 = depth_net.depth_regression(h32, torch.softmax(torch.from_numpy(logits), 1), 2.5, inv)
        d64, ci64, _ = _regress64(h64, logits, 2.5, inv)
        assert max_abs(d32[:, 0].numpy(), d64) <= 1e-5 * float(np.abs(d64).max())
        assert max_abs(ci32.numpy(), ci64) <= 1e-5 * float(np.abs(ci64).max())
    nf = np.array([[425.0, 905.0], [300.0, 700.0]], F32)
    assert max_abs(_hyp_torch(nf, 1.0, 8, 3, 5, inv, torch.float32).numpy(), _hyp64(nf, 1.0, 8, 3, 5, inv)) <= 4 * _ulp32(905.0 if not inv else 1 / 300)
    # align_corners=True is something else (the slip test relies on it): neighbouring windows lie hundreds of depth units apart
    wrong = F.interpolate(torch.from_numpy(search).double(), scale_factor=4.0, mode="bilinear", align_corners=True).numpy()
    assert max_abs(wrong, _up64(search, 4, 20, 28)) > 1.0


# ---- hypotheses cases ----------------------------------------------------------------------------------------------
#             B  D    (hr, wr) ratio (Ht, Wt)    inv    kind
HYP_CASES = {
    "bcast-B1-D1-odd": (1, 1, (1, 1), 1, (7, 9), False, "range"),
    "bcast-B3-D8-even-inv": (3, 8, (1, 1), 1, (8, 12), True, "range"),
    "bcast-B1-D64-odd-inv": (1, 64, (1, 1), 1, (15, 23), True, "range"),
    "bcast-B3-D192-even": (3, 192, (1, 1), 1, (8, 12), False, "range"),
    "bcast-B1-D8-flat": (1, 8, (1, 1), 1, (7, 9), False, "flat"),
    "r2-B1-D8-even": (1, 8, (8, 12), 2, (16, 24), False, "window"),
    "r2-B3-D64-odd-inv": (3, 64, (8, 12), 2, (15, 23), True, "window"),
    "r2-B1-D192-even-inv": (1, 192, (5, 7), 2, (10, 14), True, "window"),
    "r2-B3-D1-odd": (3, 1, (5, 7), 2, (9, 13), False, "window"),
    "r2-B1-D8-flat-inv": (1, 8, (5, 7), 2, (10, 14), True, "flat"),
    "r4-B1-D8-even": (1, 8, (8, 12), 4, (32, 48), False, "window"),
    "r4-B3-D8-odd-inv": (3, 8, (8, 12), 4, (31, 45), True, "window"),
    "r4-B1-D64-even-inv": (1, 64, (16, 20), 4, (64, 80), True, "window"),
    "r4-B3-D192-odd": (3, 192, (4, 6), 4, (15, 23), False, "window"),
    "r4-B1-D1-even-inv": (1, 1, (4, 6), 4, (16, 24), True, "window"),
    "r4-B3-D64-flat": (3, 64, (4, 6), 4, (16, 24), False, "flat"),
    "r4-c2-stage1": (1, 8, (64, 80), 4, (256, 320), False, "window"),
}
HYP_IDS = list(HYP_CASES)


@functools.lru_cache(maxsize=None)
def _hyp_case(name):
    B, D, (hr, wr), ratio, (Ht, Wt), inv, kind = HYP_CASES[name]
    rng = np.random.default_rng(4000 + HYP_IDS.index(name))
    if kind == "range":
        search = np.stack((425 + 50 * rng.random(B), 855 + 50 * rng.random(B)), 1).astype(F32).reshape(B, 2, 1, 1)
    else:
        mid = (445 + 440 * rng.random((B, 1, hr, wr))).astype(F32)
        w = F32(0 if kind == "flat" else 20)
        search = np.concatenate((mid - w, mid + w), 1)
    if kind == "flat":
        search[:, 1] = search[:, 0]
    ref64 = _hyp_torch(search, float(ratio), D, Ht, Wt, inv, torch.float64).numpy()
    cpu32 = _hyp_torch(search, float(ratio), D, Ht, Wt, inv, torch.float32).numpy()
    return dict(search=search, ratio=ratio, D=D, Ht=Ht, Wt=Wt, inv=inv, kind=kind, ref64=ref64, cpu32=cpu32, e_ref=max_abs(cpu32, ref64))


def test_hypotheses_case_table_covers_what_it_claims():
    cs = list(HYP_CASES.values())
    for ratio in (1, 2, 4):
        sub = [c for c in cs if c[3] == ratio]
        assert {c[5] for c in sub} == {False, True} and {c[0] for c in sub} == {1, 3} and {c[1] for c in sub} >= {1, 8, 64, 192}
        assert {(c[4][0] % 2, c[4][1] % 2) for c in sub} >= {(0, 0), (1, 1)} and any(c[6] == "flat" for c in sub)
        assert all((c[2] == (1, 1)) == (ratio == 1) for c in sub)


@pytest.mark.parametrize("name", HYP_IDS)
def test_hypotheses_case_referee(name):
    """CPU half: the repo's formulation at float64 agrees with the numpy restatement, the fp32 one is finite, and `flat` ranges
    (lo = hi) give the same value on every plane."""
    c = _hyp_case(name)
    print(f"[hyp cpu] {name}: E_ref {c['e_ref']:.3e}  floor {8 * _ulp32(float(np.abs(c['ref64']).max())):.3e}")
    assert c["ref64"].shape == (c["search"].shape[0], c["D"], c["Ht"], c["Wt"]) and np.isfinite(c["ref64"]).all() and np.isfinite(c["cpu32"]).all()
    width = float(np.abs(c["ref64"][:, -1] - c["ref64"][:, 0]).max())
    assert max_abs(c["ref64"], _hyp64(c["search"], c["ratio"], c["D"], c["Ht"], c["Wt"], c["inv"])) <= 2.0 ** -23 * width + 1e-12 * float(np.abs(c["ref64"]).max())
    if c["kind"] == "flat":
        assert np.ptp(c["ref64"], axis=1).max() <= 1e-12 * float(np.abs(c["ref64"]).max())


#              D  (hr, wr) ratio (Ht, Wt)  inv
EXACT_CASES = [(2, (1, 1), 1, (5, 7), False), (3, (1, 1), 1, (4, 6), True), (5, (1, 1), 1, (7, 9), False), (9, (1, 1), 1, (8, 12), True),
               (17, (1, 1), 1, (3, 3), False), (2, (4, 6), 2, (8, 12), False), (5, (4, 6), 2, (7, 11), False), (3, (4, 6), 4, (16, 24), False),
               (9, (4, 6), 4, (15, 23), False), (33, (3, 5), 4, (12, 20), False)]


def _exact_case(i):
    """Dyadic ranges, D - 1 a power of two: every product and sum of the formula is exact in fp32 (range values are multiples of 16
    below 2^11, the bilinear weights multiples of 1/8, the steps multiples of 1 / (D - 1)); under inv_depth the values are powers of
    two and the range is broadcast, so the reciprocals are exact too."""
    D, (hr, wr), ratio, (Ht, Wt), inv = EXACT_CASES[i]
    rng = np.random.default_rng(4500 + i)
    if inv:
        search = np.stack((2.0 ** rng.integers(5, 8, 2), 2.0 ** rng.integers(8, 11, 2)), 1).astype(F32).reshape(2, 2, 1, 1)
    else:
        lo = 16 * rng.integers(8, 40, (2, 1, hr, wr))
        search = np.concatenate((lo, lo + 16 * rng.integers(1, 40, (2, 1, hr, wr))), 1).astype(F32)
    want = _hyp64(search, ratio, D, Ht, Wt, inv)
    return search, ratio, D, Ht, Wt, inv, want


@pytest.mark.parametrize("i", range(len(EXACT_CASES)))
def test_exact_hypotheses_are_representable(i):
    search, ratio, D, Ht, Wt, inv, want = _exact_case(i)
    assert np.array_equal(want.astype(F32).astype(np.float64), want)
    assert np.array_equal(_hyp_torch(search, float(ratio), D, Ht, Wt, inv, torch.float32).numpy(), want.astype(F32))


# ---- stage cases ---------------------------------------------------------------------------------------------------
CFG = make_cfg("configs/dtu_eval.yaml")
#               stage frame      V  B
STAGE_CASES = {
    "F7-s0-V1-B1": (0, (64, 96), 1, 1),
    "F7-s0-V2-B2": (0, (64, 96), 2, 2),
    "F7-s0-V5-B1": (0, (64, 96), 5, 1),
    "F7-s0-V8-B2": (0, (64, 96), 8, 2),
    "F7-s1-V3-B2": (1, (64, 96), 3, 2),
    "F7-s1-V4-B1": (1, (64, 96), 4, 1),
    "F7-s1-V6-B1": (1, (64, 96), 6, 1),
    "F7-s1-V7-B2": (1, (64, 96), 7, 2),
    "c2-s0-V3-B1": (0, (512, 640), 3, 1),
    "c2-s1-V3-B1": (1, (512, 640), 3, 1),
}
STAGE_IDS = list(STAGE_CASES)
OUT_KEYS = ("volume", "depth", "ci", "vol_range")


def _unet(cin, c, cout, depth, seed=0):
    """Random weights and non-trivial BN statistics, as tests/test_cost_reg.py builds them."""
    torch.manual_seed(seed)
    m = _UNet3d(cin, cout, c, depth).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.8, 1.2)
    return m


def _stage_inputs(name):
    """Cameras as tests/test_costvol.py's general cases build them (synthetic.make_frame, features drawn per case); the intrinsics
    stay UNSCALED: the stage scales them."""
    s, (Ho, Wo), V, B = STAGE_CASES[name]
    lvl = CFG.mvs.vol_levels[s]
    fs, vs = float(CFG.fpn.feat_scales[lvl]), float(CFG.mvs.vol_scales[s])
    Cc, D, inv = int(CFG.fpn.feat_dims[lvl]), int(CFG.mvs.num_depth[s]), bool(CFG.mvs.inv_depth[s])
    seed = 100 + STAGE_IDS.index(name)
    rng = np.random.default_rng(5000 + seed)
    fr = synthetic.make_frame(Ho, Wo, V=V, B=B, seed=seed, feat_dim=1, voxel_dim=1, num_depth=1)
    Hs, Ws, Ht, Wt = int(Ho * fs), int(Wo * fs), int(Ho * vs), int(Wo * vs)
    feat = rng.standard_normal((B, V, Cc, Hs, Ws), dtype=F32)
    if s == 0:
        search, ratio = np.broadcast_to(np.array([425.0, 905.0], F32), (B, 2)).copy(), 1.0
    else:   # the previous stage's interval at its resolution: per-pixel windows of +-20 as in fixture F8
        ratio = vs / float(CFG.mvs.vol_scales[s - 1])
        hr, wr = int(Ho * CFG.mvs.vol_scales[s - 1]), int(Wo * CFG.mvs.vol_scales[s - 1])
        mid = (445 + 440 * rng.random((B, 1, hr, wr))).astype(F32)
        search = np.concatenate((mid - F32(20), mid + F32(20)), 1)
    return dict(stage=s, feat=feat, src_exts=fr["src_exts"], src_ints=fr["src_ints"], tar_ext=fr["tar_ext"], tar_int=fr["tar_int"], fs=fs, vs=vs,
                search=search, ratio=ratio, D=D, Ht=Ht, Wt=Wt, inv=inv, ci_scale=float(CFG.mvs.ci_scales[s]),
                unet=_unet(Cc, int(CFG.fpn.base_channels), int(CFG.mvs.voxel_dim), 2 if s == 0 else 3, seed=seed))


def _stage_torch(c, dtype, unet=None):
    """One stage exactly as DepthNet.forward's PyTorch branch runs it (depth_net.py:133-156)."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dtype)
    Ks, Kt = t("src_ints").clone(), t("tar_int").clone()   # (.to() of an fp32 array shares its memory: the case's inputs stay unscaled)
    Ks[..., :2, :] *= c["fs"]
    Kt[:, :2, :] *= c["vs"]
    hyp = _hyp_torch(c["search"], c["ratio"], c["D"], c["Ht"], c["Wt"], c["inv"], dtype)
    m = copy.deepcopy(unet if unet is not None else c["unet"]).to(dtype)
    with torch.no_grad():
        cost = depth_net.build_feature_volume(t("feat"), t("src_exts"), Ks, t("tar_ext"), Kt, hyp, c["inv"])
        volume, prob = m(cost)
        depth, ci = depth_net.depth_regression(hyp, prob, c["ci_scale"], c["inv"])
        var = (prob * (hyp - (prob * hyp).sum(1, keepdim=True)).square()).sum(1)
    return dict(volume=volume.numpy(), depth=depth.squeeze(1).numpy(), ci=ci.numpy(), vol_range=hyp[:, [0, -1]].numpy(), var=var.numpy(),
                hyp=hyp.numpy(), Ks=Ks.numpy(), Kt=Kt.numpy())


def _excluded_fraction(c, r64):
    """tests/test_costvol.py's exclusion rule on float64 alone: some view's z below 1e-3 of the plane depth."""
    B = c["feat"].shape[0]
    depth = 1.0 / r64["hyp"] if c["inv"] else r64["hyp"]
    f = lambda k: np.asarray(c[k], np.float64)
    P_tar = np.zeros((B, 4, 4)); P_tar[:, :3] = r64["Kt"] @ f("tar_ext")[:, :3]; P_tar[:, 3, 3] = 1
    Hm = (r64["Ks"] @ f("src_exts")[..., :3, :]) @ np.linalg.inv(P_tar)[:, None]
    xs, ys = np.meshgrid(np.arange(c["Wt"]) + 0.5, np.arange(c["Ht"]) + 0.5, indexing="xy")
    rz = Hm[..., 2, 0, None, None] * xs + Hm[..., 2, 1, None, None] * ys + Hm[..., 2, 2, None, None]
    z = rz[:, :, None] * depth[:, None] + Hm[..., 2, 3, None, None, None]
    return float(((z < 1e-3 * depth[:, None]).any(1) | ~np.isfinite(z).all(1)).mean())


@functools.lru_cache(maxsize=None)
def _stage_case(name):
    c = _stage_inputs(name)
    r64, r32 = _stage_torch(c, torch.float64), _stage_torch(c, torch.float32)
    c["ref64"], c["cpu32"] = r64, r32
    c["e_ref"] = {k: max_abs(r32[k], r64[k]) for k in OUT_KEYS}
    c["excluded"] = _excluded_fraction(c, r64)
    return c


def test_stage_case_table_covers_what_it_claims():
    assert {v[2] for v in STAGE_CASES.values()} == set(range(1, 9)) and {v[3] for v in STAGE_CASES.values()} == {1, 2}
    assert {(v[0], v[1]) for v in STAGE_CASES.values()} == {(0, (64, 96)), (1, (64, 96)), (0, (512, 640)), (1, (512, 640))}
    shapes = {n: (_stage_inputs(n)["feat"].shape[2:], (_stage_inputs(n)["D"], _stage_inputs(n)["Ht"], _stage_inputs(n)["Wt"])) for n in ("F7-s0-V1-B1", "F7-s1-V4-B1")}
    assert shapes == {"F7-s0-V1-B1": ((32, 16, 24), (64, 8, 12)), "F7-s1-V4-B1": ((16, 32, 48), (8, 32, 48))}


@pytest.mark.parametrize("name", [n for n in STAGE_IDS if n.startswith("F7")])
def test_stage_case_referee(name):
    """CPU half of the F7-shape stage cases (the c2 ones run the same code; their float64 U-Nets are left to the GPU test): no
    voxel is outside the referee's domain, the float64 variance stays well away from the 1e-12 clamp, outputs are finite."""
    c = _stage_case(name)
    print(f"[stage cpu] {name}: E_ref {c['e_ref']}  excluded {c['excluded']}  min var64 {c['ref64']['var'].min():.3e}")
    assert c["excluded"] == 0.0
    assert c["ref64"]["var"].min() >= 1e4 * 1e-12
    for k in OUT_KEYS:
        assert np.isfinite(c["ref64"][k]).all() and np.isfinite(c["cpu32"][k]).all()
    assert c["ref64"]["depth"].shape == (c["feat"].shape[0], c["Ht"], c["Wt"])


def _run_stage(c, unet=None, workspace=None, **slip):
    """costvol.MvsStage on the case's inputs; `slip` overrides single arguments."""
    m = (unet if unet is not None else c["unet"])
    reg = costvol.CostReg(copy.deepcopy(m).cuda())
    a = dict(fs=c["fs"], vs=c["vs"], search=c["search"], ratio=c["ratio"], ci_scale=c["ci_scale"])
    a.update(slip)
    out = costvol.MvsStage(reg)(_cuda(c["feat"]), _cuda(c["src_exts"]), _cuda(c["src_ints"]), _cuda(c["tar_ext"]), _cuda(c["tar_int"]), a["fs"],
                                a["vs"], _cuda(a["search"]), a["ratio"], c["D"], c["Ht"], c["Wt"], c["inv"], a["ci_scale"], workspace=workspace)
    torch.cuda.synchronize()
    return dict(zip(OUT_KEYS, out))


# ================================================================================================================
# On the MI355X
# ================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("name", HYP_IDS)
def test_hip_hypotheses_vs_float64(name):
    c = _hyp_case(name)
    got = costvol.mvs_hypotheses(_cuda(c["search"]), c["ratio"], c["D"], c["Ht"], c["Wt"], c["inv"]).cpu().numpy()
    assert got.shape == c["ref64"].shape and np.isfinite(got).all()     # every element is compared: nothing is excluded
    err, bound = max_abs(got, c["ref64"]), _bound(c["e_ref"], c["ref64"])
    print(f"[hyp] {name}: E_ref {c['e_ref']:.3e}  hip err {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    # the (B, 2) form of a broadcast range is the (B, 2, 1, 1) one
    if c["search"][0, 0].size == 1:
        assert np.array_equal(costvol.mvs_hypotheses(_cuda(c["search"].reshape(-1, 2)), 1.0, c["D"], c["Ht"], c["Wt"], c["inv"]).cpu().numpy(), got)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(EXACT_CASES)))
def test_hip_hypotheses_exact_on_dyadic_ranges(i):
    search, ratio, D, Ht, Wt, inv, want = _exact_case(i)
    got = costvol.mvs_hypotheses(_cuda(search), ratio, D, Ht, Wt, inv).cpu().numpy()
    assert np.array_equal(got, want.astype(F32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGE_IDS)
def test_hip_stage_vs_float64(name):
    """volume, depth, ci and vol_range of one gdb_mvs_stage call against the float64 stage (sweep -> _UNet3d.double() -> regression)
    under the rule; no voxel is excluded (asserted: the exclusion rule excludes 0 on these cases)."""
    c = _stage_case(name)
    assert c["excluded"] == 0.0 and c["ref64"]["var"].min() >= 1e4 * 1e-12
    got = _run_stage(c)
    fails = []
    for k in OUT_KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == c["ref64"][k].shape and np.isfinite(g).all()
        err, bound = max_abs(g, c["ref64"][k]), _bound(c["e_ref"][k], c["ref64"][k])
        print(f"[stage] {name} {k}: E_ref {c['e_ref'][k]:.3e}  hip err {err:.3e}  ratio {err / c['e_ref'][k] if c['e_ref'][k] else float('nan'):.2f}  bound {bound:.3e}")
        if err > bound:
            fails.append(k)
    assert not fails


def _flat_unet(s, tap=None, a=-4.0):
    """A U-Net whose activations are constant: zero convolutions under BatchNorm(weight 1, bias 1, mean 0, var 1) give 1 after every
    layer and 2 after every skip add, in all 8 channels.  With a zero prob head the logits are constant.  With `tap` = 0 / 2 the
    prob head reads only the plane before / after (kz = 0 / 2, centre of the 3 x 3): a * 2 * 8 = -64 everywhere except on the first
    / last plane, where that neighbour is the zero padding and the logit is 0: one plane dominant by 64."""
    m = _unet(int(CFG.fpn.feat_dims[CFG.mvs.vol_levels[s]]), int(CFG.fpn.base_channels), int(CFG.mvs.voxel_dim), 2 if s == 0 else 3)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
                mod.weight.zero_()
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.weight.fill_(1.0); mod.bias.fill_(1.0); mod.running_mean.zero_(); mod.running_var.fill_(1.0 - mod.eps)
        if tap is not None:
            m.prob_head.weight[0, :, tap, 1, 1] = a
    return m


@pytest.mark.parametrize("name", ["F7-s0-V2-B2", "F7-s1-V3-B2"])
def test_flat_unet_gives_the_logits_it_claims(name):
    """CPU half of the closed-form regressions: the module itself, at float64, yields constant logits / one plane 64 above the rest."""
    c = _stage_inputs(name)
    x = torch.rand(1, c["feat"].shape[2], c["D"], c["Ht"], c["Wt"], dtype=torch.float64)
    for tap, plane in ((None, None), (0, 0), (2, c["D"] - 1)):
        m = _flat_unet(c["stage"], tap).double()
        with torch.no_grad():
            assert float((m.conv0(x) - 1).abs().max()) <= 1e-6       # (1 / sqrt(var + eps) is 1 up to fp32 rounding of the buffers)
            _, prob = m(x)
        logp = prob.log()
        if tap is None:
            assert float((prob - 1.0 / c["D"]).abs().max()) <= 1e-12
        else:
            others = [d for d in range(c["D"]) if d != plane]
            assert float((logp[:, plane:plane + 1] - logp[:, others]).min()) >= 60.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["F7-s0-V2-B2", "F7-s1-V3-B2"])
def test_hip_stage_degenerate_regressions_closed_form(name):
    """Constant logits: depth is the mean hypothesis.  Bound: the kernel sums D products (1 / D) * hyp_d in fp32, each term and
    each partial sum rounded once: at most 2 D roundings of relative size 2^-24 on values below max |hyp|, plus the referee
    rule's own floor of 8 ulp.  One plane dominant by 64: exp(-64) * hyp is far below an ulp of the dominant term, so depth is that
    hypothesis to the floor, the variance falls under the 1e-12 clamp, and ci lies inside [first, last]."""
    c = _stage_inputs(name)
    hyp = _hyp64(c["search"], c["ratio"], c["D"], c["Ht"], c["Wt"], c["inv"])
    top = float(np.abs(hyp).max())
    got = _run_stage(c, unet=_flat_unet(c["stage"]))
    mean = hyp.mean(1)
    bound = 2 * c["D"] * 2.0 ** -24 * top + 8 * _ulp32(top)
    want = mean
    if c["inv"]:   # depth = 1 / mean: the error of the mean divided by mean^2, and the reciprocal's own rounding inside the floor
        want = 1.0 / mean
        bound = bound / float(np.abs(mean).min()) ** 2 + 8 * _ulp32(float(np.abs(want).max()))
    err = max_abs(got["depth"].cpu().numpy(), want)
    print(f"[stage closed form] {name} constant logits: err {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    assert max_abs(got["vol_range"].cpu().numpy(), hyp[:, [0, -1]]) <= 8 * _ulp32(top)
    for tap, plane in ((0, 0), (2, c["D"] - 1)):
        got = _run_stage(c, unet=_flat_unet(c["stage"], tap))
        sel = 1.0 / hyp[:, plane] if c["inv"] else hyp[:, plane]
        err, floor = max_abs(got["depth"].cpu().numpy(), sel), 8 * _ulp32(float(np.abs(sel).max()))
        print(f"[stage closed form] {name} plane {plane} dominant: err {err:.3e}  floor {floor:.3e}")
        assert err <= floor
        ci, vr = got["ci"].cpu().numpy().astype(np.float64), got["vol_range"].cpu().numpy().astype(np.float64)
        ends = np.sort(1.0 / vr if c["inv"] else vr, axis=1)
        slack = 2 * np.spacing(np.abs(ends).astype(F32)).astype(np.float64)    # the fp32 reciprocal of an end, under inv_depth
        assert (ci[:, 0] >= ends[:, 0] - slack[:, 0]).all() and (ci[:, 1] <= ends[:, 1] + slack[:, 1]).all() and (ci[:, 0] <= ci[:, 1]).all()


SLIP_CASE = "F7-s1-V3-B2"


def _slips(c):
    up_wrong = F.interpolate(torch.from_numpy(c["search"]), scale_factor=c["ratio"], mode="bilinear", align_corners=True).numpy()
    return {"feat_scale (1 + 2^-10)": dict(fs=c["fs"] * (1 + 2.0 ** -10)),
            "range upsampled with align_corners=True": dict(search=up_wrong, ratio=1.0),   # handed over at target size: ratio 1 is the identity
            "ci_scale (1 + 2^-8)": dict(ci_scale=c["ci_scale"] * (1 + 2.0 ** -8))}


@pytest.mark.gpu
def test_hip_stage_rule_sees_slips():
    """The stage run on inputs that carry a slip must FAIL the rule against the referee of the right inputs, and pass on the right
    ones.  The range slip: the interval upsampled by torch with align_corners=True and handed to the stage at target size (ratio
    1 reproduces it exactly, checked through gdb_mvs_hypotheses first)."""
    c = _stage_case(SLIP_CASE)
    ident = costvol.mvs_hypotheses(_cuda(_slips(c)["range upsampled with align_corners=True"]["search"]), 1.0, 1, c["Ht"], c["Wt"], False).cpu().numpy()
    assert np.array_equal(ident[:, 0], _slips(c)["range upsampled with align_corners=True"]["search"][:, 0])
    good = _run_stage(c)
    for k in OUT_KEYS:
        assert max_abs(good[k].cpu().numpy(), c["ref64"][k]) <= _bound(c["e_ref"][k], c["ref64"][k])
    for kind, slip in _slips(c).items():
        bad = _run_stage(c, **slip)
        seen = {}
        for k in OUT_KEYS:
            err, bound = max_abs(bad[k].cpu().numpy(), c["ref64"][k]), _bound(c["e_ref"][k], c["ref64"][k])
            seen[k] = err > bound
            print(f"[stage slip] {kind} {k}: err {err:.3e} against bound {bound:.3e}: seen {err > bound}")
        assert seen["ci"]
        if not kind.startswith("ci_scale"):
            assert seen["volume"] and seen["depth"]


@pytest.mark.gpu
def test_hip_stage_is_deterministic_and_ignores_the_workspace():
    c = _stage_inputs("F7-s1-V3-B2")
    a = _run_stage(c)
    b = _run_stage(c)
    reg = costvol.CostReg(c["unet"])
    B, V, Cc, Hs, Ws = c["feat"].shape
    n = costvol.MvsStage(reg).workspace_bytes(B, V, Cc, Hs, Ws, c["D"], c["Ht"], c["Wt"])
    ws = torch.full(((n + 3) // 4,), float("nan"), device="cuda")
    w = _run_stage(c, workspace=ws)
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], w[k]) and bool(torch.isfinite(a[k]).all())
    with pytest.raises(ValueError, match="workspace"):
        _run_stage(c, workspace=ws[:16])


# ---- the cascade ---------------------------------------------------------------------------------------------------
def _depth_net_inputs(kind):
    """F7's own inputs and weights, or the c2 (512 x 640) frame with random weights; features from the network's own FPN."""
    opts = {"mvs.hip_cost_reg": True, "fpn.hip_feature_net": True, "mvs.hip_cascade": True}
    if kind == "F7":
        f7, net = _f7_net(**opts)
        fr = {k: f7[k] for k in ("src_images", "src_exts", "src_ints", "tar_ext", "tar_int", "near_far")}
    else:
        torch.manual_seed(0)
        net = make_network(make_cfg("configs/dtu_eval.yaml", [x for kv in opts.items() for x in (kv[0], str(kv[1]))])).eval()
        fr = synthetic.make_frame(512, 640, V=3, seed=0)
    net = net.cuda()
    t = {k: _cuda(np.asarray(fr[k], F32)) for k in ("src_images", "src_exts", "src_ints", "tar_ext", "tar_int", "near_far")}
    with torch.no_grad():
        ms = [f.unflatten(0, t["src_images"].shape[:2]) for f in net.feature_net(t["src_images"].flatten(0, 1))]
    return net.depth_net, t, ms


def _depth_net_call(d, t, ms):
    with torch.no_grad():
        return d(t["src_images"], ms, t["src_exts"], t["src_ints"], t["tar_ext"], t["tar_int"], t["near_far"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["F7", "c2"])
def test_hip_cascade_vs_float64_depth_net(kind):
    """DepthNet.forward with mvs.hip_cascade (hip_cost_reg and hip_feature_net on as well) against the float64 DepthNet on the CPU,
    per stage and per output under the rule; E_ref from the fp32 DepthNet on the CPU.  The distance to the switch-off path is
    printed, not used."""
    d, t, ms = _depth_net_inputs(kind)
    on = _depth_net_call(d, t, ms)
    d.hip_cascade = False
    off = _depth_net_call(d, t, ms)
    d.hip_cascade = True
    torch.cuda.synchronize()
    cpu = {dt: _depth_net_call(copy.deepcopy(d).cpu().to(dt), {k: v.cpu().to(dt) for k, v in t.items()}, [m.cpu().to(dt) for m in ms])
           for dt in (torch.float32, torch.float64)}
    fails = []
    for o, key in enumerate(("depth", "ci", "vol_range", "volume")):
        for s in range(d.num_stages):
            ref64, got = cpu[torch.float64][o][s].numpy(), on[o][s].cpu().numpy()
            assert got.shape == ref64.shape and np.isfinite(got).all()
            e_ref = max_abs(cpu[torch.float32][o][s].numpy(), ref64)
            err, bound = max_abs(got, ref64), _bound(e_ref, ref64)
            print(f"[cascade] {kind} stage {s} {key}: E_ref {e_ref:.3e}  hip err {err:.3e}  bound {bound:.3e}  |on - off| {max_abs(got, off[o][s].cpu().numpy()):.3e}")
            if err > bound:
                fails.append((s, key))
    assert on[4] == [] and not fails


@pytest.mark.gpu
def test_hip_cascade_is_deterministic_and_never_syncs():
    d, t, ms = _depth_net_inputs("F7")
    a = _depth_net_call(d, t, ms)          # packs and uploads the weights
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = _depth_net_call(d, t, ms)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for x, y in zip(a[:4], b[:4]):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


@pytest.mark.gpu
def test_hip_cascade_is_one_stage_call_per_stage(monkeypatch):
    d, t, ms = _depth_net_inputs("F7")
    calls = []
    orig = costvol.MvsStage.__call__
    monkeypatch.setattr(costvol.MvsStage, "__call__", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    monkeypatch.setattr(costvol, "build_feature_volume", lambda *a, **k: pytest.fail("the sweep entry was called"))
    monkeypatch.setattr(costvol, "depth_regression", lambda *a, **k: pytest.fail("the regression entry was called"))
    _depth_net_call(d, t, ms)
    assert len(calls) == d.num_stages


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["F7_network", "F7b_network_nerf_eval", "F7c_network_render_scale"])
def test_network_forward_with_hip_cascade_matches_reference(fixture):
    """Whole Network.forward with every switch on against F7 / F7b / F7c, the bounds of
    tests/test_cost_reg.py::test_network_forward_with_hip_cost_reg_matches_reference."""
    f7 = load_golden("F7_network")
    fx = f7 if fixture == "F7_network" else load_golden(fixture)
    opts = ["mvs.hip_cost_reg", "True", "fpn.hip_feature_net", "True", "mvs.hip_cascade", "True"]
    net = make_network(make_cfg(str(fx["yaml"]) if "yaml" in fx else "configs/dtu_eval.yaml", opts)).eval()
    net.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in f7.items() if k.startswith("sd.")},
                        strict=True)
    net = net.cuda()
    assert net.depth_net.hip_cascade
    fxb = dict(fx); fxb["src_images"] = fx["src_images"].astype(np.float32)
    tt = lambda k: torch.from_numpy(fxb[k]).cuda()
    batch = {"src_views": {"rgb": tt("src_images"), "extrinsics": tt("src_exts"), "intrinsics": tt("src_ints")},
             "tar_views": {"extrinsics": tt("tar_ext"), "intrinsics": tt("tar_int")}, "near_far": tt("near_far")}
    if "render_scale" in fx and float(fx["render_scale"]) != 1.0:
        batch["render_scale"] = torch.tensor([float(fx["render_scale"])], device="cuda")
    with torch.no_grad():
        ret, mvs_depths, blend = net(batch)
    e = max_abs(ret["rgb"].cpu().numpy(), fx["rgb"])
    print(f"{fixture} with the cascade on the library: max |rgb - reference| = {e:.3e}")
    assert e <= 5e-4
    assert max_abs(ret["mvs_depth"].cpu().numpy(), fx["mvs_depth"]) <= 1e-3 * float(np.abs(fx["mvs_depth"]).max())
    H, W = fx["rgb"].shape[2:]
    gt = np.clip(np.transpose(fx["rgb"][0], (1, 2, 0)) + np.random.default_rng(1).normal(0, 0.03, (H, W, 3)), 0, 1)
    d_psnr = abs(oracle.psnr(gt, np.transpose(ret["rgb"][0].cpu().numpy(), (1, 2, 0))) - oracle.psnr(gt, np.transpose(fx["rgb"][0], (1, 2, 0))))
    assert d_psnr <= 0.05


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    """Host integers stand in for device pointers: a launch on them would fail, a refusal never gets there."""
    lib = _lib.load()
    fake, n = 4096, C.c_size_t()
    shape = dict(B=1, V=3, C=32, Hs=16, Ws=24, D=64, Ht=8, Wt=12)
    unet = (2, 32, 8, 8)

    def nbytes(u=unet, **kw):
        s = dict(shape, **kw)
        return lib.gdb_mvs_stage_workspace_bytes(s["B"], s["V"], s["C"], s["Hs"], s["Ws"], s["D"], s["Ht"], s["Wt"], *u, C.byref(n))

    assert nbytes() == _lib.GDB_OK
    need = n.value
    cr = C.c_size_t()
    assert lib.gdb_cost_reg_workspace_bytes(2, 32, 8, 8, 1, 64, 8, 12, C.byref(cr)) == _lib.GDB_OK
    al = lambda x: (x + 63) // 64 * 64
    assert need == 4 * (al(3 * 12) + al(3 * 32 * 16 * 24) + al(32 * 64 * 8 * 12) + al(64 * 8 * 12)) + cr.value
    assert nbytes(V=5) == _lib.GDB_OK and n.value == need - 4 * al(3 * 32 * 16 * 24) - 4 * al(36) + 4 * al(60)   # no pair copy beyond 4 views
    for kw in (dict(B=0), dict(V=0), dict(Ws=1), dict(D=0), dict(Ht=0), dict(V=9), dict(D=1024), dict(D=62), dict(Wt=10)):
        assert nbytes(**kw) == _lib.GDB_E_SHAPE, kw
    assert nbytes(u=(2, 16, 8, 8)) == _lib.GDB_E_BADARG and b"channels" in lib.gdb_last_error()
    assert nbytes(u=(4, 32, 8, 8)) == _lib.GDB_E_BADARG

    def stage(null=None, ws=need, hr=1, wr=1, ratio=1.0, u=unet, **kw):
        s = dict(shape, **kw)
        p = [None if null == i else fake for i in range(12)]
        return lib.gdb_mvs_stage(p[0], p[1], p[2], p[3], p[4], 0.25, 0.125, p[5], hr, wr, ratio, s["B"], s["V"], s["C"], s["Hs"], s["Ws"], s["D"],
                                 s["Ht"], s["Wt"], 1, 2.5, *u, p[6], p[7], ws, p[8], p[9], p[10], p[11], None)

    for i in range(12):
        assert stage(null=i) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error()
    assert stage(ws=need - 4) == _lib.GDB_E_WORKSPACE and b"workspace" in lib.gdb_last_error()
    assert stage(Wt=10) == _lib.GDB_E_SHAPE and stage(V=9) == _lib.GDB_E_SHAPE and stage(u=(2, 16, 8, 8)) == _lib.GDB_E_BADARG
    assert stage(hr=0) == _lib.GDB_E_SHAPE
    for ratio in (0.0, -2.0, float("nan"), float("inf")):
        assert stage(hr=2, wr=3, ratio=ratio) == _lib.GDB_E_BADARG and b"ratio" in lib.gdb_last_error()
    assert stage(hr=2, wr=3, ratio=1e-12) == _lib.GDB_E_SHAPE

    hyp = lambda p=(fake, fake), hr=1, wr=1, ratio=1.0, B=1, D=4, Ht=8, Wt=8: lib.gdb_mvs_hypotheses(p[0], hr, wr, ratio, B, D, Ht, Wt, 0, p[1], None)
    assert hyp((None, fake)) == _lib.GDB_E_BADARG and hyp((fake, None)) == _lib.GDB_E_BADARG
    for kw in (dict(B=0), dict(D=0), dict(Ht=0), dict(Wt=-1), dict(hr=0), dict(wr=-1)):
        assert hyp(**kw) == _lib.GDB_E_SHAPE, kw
    assert hyp(hr=2, wr=2, ratio=0.0) == _lib.GDB_E_BADARG

    z = torch.zeros
    reg = costvol.CostReg(_unet(32, 8, 8, 2))
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.MvsStage(reg)(z(1, 3, 32, 16, 24), z(1, 3, 4, 4), z(1, 3, 3, 3), z(1, 4, 4), z(1, 3, 3), 0.25, 0.125, z(1, 2), 1.0, 64, 8, 12, True, 2.5)
    with pytest.raises(ValueError, match="inconsistent"):
        costvol.MvsStage(reg)(z(1, 3, 32, 16, 24), z(1, 2, 4, 4), z(1, 3, 3, 3), z(1, 4, 4), z(1, 3, 3), 0.25, 0.125, z(1, 2), 1.0, 64, 8, 12, True, 2.5)
    with pytest.raises(ValueError, match="float32 CUDA"):
        costvol.mvs_hypotheses(z(1, 2), 1.0, 8, 4, 4, False)

"""The forward of the operator mirrors (gdb_build_rays, gdb_sample, gdb_encode, gdb_mlp, gdb_render_weights, gdb_accumulate,
gdb_composite) against the CPU restatement `gdb_oracle_torch` in float64.  Runs on a real MI355X: `pytest -m gpu`.

Rule (the project's own), per tensor and per channel group, elementwise, no element excluded:
    |hip - ref64| <= 4 max(E32, 8 fp32 ulp of max |ref64|),     E32 = max |float32 CPU restatement - ref64|.
ref64 is the restatement in float64 on float64 copies of exactly the float32 arrays the kernel was given; the float32 restatement runs
on the same arrays.  Every operator is refereed at its own boundary: from `encode` onward the inputs are the HIP outputs of the operator
before it, so no operator hides behind its predecessor; only the chained test lets errors compound.  The kernel never enters the bound,
and every ref64 value is asserted finite.

Groups.  Where one tensor holds channels of different kinds they are refereed apart (encode: per-ray RGB, mip feature, direction code;
the voxel feature in four channel pairs; the MLP's blended channels and its feat_head).  `ball_radii` is split in two by conditioning:
its factor sqrt(1 / cos^2 - 1) cancels for the few bundles around the principal point, and those alone would set the tensor's E32.  The
split is made from ref64 alone: tan^2 = 1 / cos^2 - 1 of the float64 bundle axis below or above 1 / 64.  Both groups are held to the rule;
no element belongs to none (asserted).

Integer outputs (samples_per_bundle, indices, samples_per_batch, total) are exact against the float32 restatement, with one exception: a
bundle whose float64 `ceil` argument lies within 1e-4 of an integer may take either neighbour.  At most 1 % of a case's bundles may be
such (asserted; the seeds below were chosen on the CPU to stay within it).  The continuous outputs are then refereed with HIP's counts as
data (`gdb_oracle_torch.sample_bundles_counted`).

`sample` takes no ray arrays - the kernel forms its rays from the target camera - so its inputs are the frame's: both restatements run
build_rays -> sample_bundles_counted from tar_ext / tar_int in their own dtype.

The composite's tensors are split likewise, from ref64's opacity: bundles whose weights sum to 1, bundles under the 1e-6 clamp of the
normalising denominator, and bundles without any weight, which must come out as exact zeros (`render_tensors`).  Under inv_depth the depth of a bundle without any weight is 1 / 0: there is no finite
referee, so such a bundle is held exactly instead - +inf in HIP, ref64 and the float32 restatement alike, asserted.

Two calls of every entry are bit-identical (asserted in each test).  Observed E32, error and error / bound per case and tensor:
profiles/forward_referee/referee_observed.txt (rewritten by a run of this file)."""
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
from test_position_backward_referee import CASES as ENCODE_CAMERAS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "forward_referee", "referee_observed.txt")
K_RULE, FLOOR_ULPS = 4.0, 8.0
COUNT_MARGIN, COUNT_CAP = 1e-4, 0.01
NEAR_AXIS_TAN2 = 1.0 / 64.0
NUM_DEPTH = 64   # HotPathEngine's default global_num_depth


# ---- referee -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)   # the restatement allocates its tables with the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def both(fn):
    """fn(c) -> {name: tensor}, c the conversion of an array to the run's dtype: run on the CPU in float64, then in float32
    -> (ref64, ref32), float64 numpy."""
    out = []
    for dt in (torch.float64, torch.float32):
        with default_dtype(dt), torch.no_grad():
            res = fn(lambda a, dt=dt: torch.tensor(np.asarray(a), dtype=dt))
            out.append({k: v.double().numpy() for k, v in res.items()})
    return out


def rule(got, ref64, ref32, groups=None):
    """The rule on one tensor -> [(group label, E32, err, bound)].  groups: {label: boolean mask, broadcastable}, made from ref64 alone;
    every element must lie in one."""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    assert np.isfinite(ref64).all()
    if groups is None:
        groups = {"": np.ones(ref64.shape, bool)}
    covered, rows = np.zeros(ref64.shape, bool), []
    for label, m in groups.items():
        m = np.broadcast_to(m, ref64.shape)
        covered |= m
        if not m.any():
            continue
        e32 = float(np.abs(ref32[m] - ref64[m]).max())
        bound = K_RULE * max(e32, FLOOR_ULPS * float(np.spacing(np.float32(np.abs(ref64[m]).max()))))
        err = float(np.abs(got[m] - ref64[m]).max()) if np.isfinite(got[m]).all() else float("inf")
        rows.append((label, e32, err, bound))
    assert covered.all(), "an element lies in no group"
    return rows


_observed = {}


def check(case, tensors):
    """tensors: {name: (hip, ref64, ref32[, groups])}.  Prints each figure, records it, then asserts the rule for every tensor."""
    fails = []
    for name, t in tensors.items():
        for label, e32, err, bound in rule(*t):
            ratio = err / bound if bound else (0.0 if err == 0.0 else float("inf"))
            key = (case, name + (":" + label if label else ""))
            line = f"[forward referee] {key[0]} {key[1]}: E32 {e32:.3e}, err {err:.3e}, err/bound {ratio:.3f}"
            print(line)
            _observed[key] = line
            if not err <= bound:
                fails.append(line)
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        old = {}
        if os.path.exists(OBSERVED):
            for l in open(OBSERVED):
                if l.startswith("[forward referee]"):
                    old[tuple(l.rstrip(":\n").split()[2:4])] = l.rstrip("\n")
        old.update({(k[0], k[1] + ":"): v for k, v in _observed.items()})
        with open(OBSERVED, "w") as f:
            f.write("# E32 = max |fp32 CPU restatement - ref64|, err = max |hip - ref64|, bound = 4 * max(E32, 8 ulp32 of max |ref64|); "
                    "tests/test_forward_referee.py\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError:
        pass
    assert not fails, "\n".join(fails)


# ---- frames --------------------------------------------------------------------------------------------------------------------
def posed(fr):
    """`synthetic` gives identity, centred target cameras only: a target off the origin, rolled, looking off the scene's axis, with
    fx != fy and the principal point off the image centre."""
    fr = dict(fr)
    B = fr["tar_ext"].shape[0]
    ext, K = np.empty((B, 4, 4), np.float32), fr["tar_int"].copy()
    for bi in range(B):
        E = synthetic.look_at_w2c(np.array([35.0 + 12.0 * bi, -20.0, 15.0]), np.array([10.0, 5.0 - 9.0 * bi, 650.0])).astype(np.float64)
        a = 0.2 + 0.1 * bi
        roll = np.eye(4)
        roll[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        ext[bi] = (roll @ E).astype(np.float32)
    K[:, 0, 0] *= np.float32(1.1)
    K[:, 1, 1] *= np.float32(0.9)
    K[:, 0, 2] += np.float32(2.75)
    K[:, 1, 2] -= np.float32(1.5)
    fr["tar_ext"], fr["tar_int"] = ext, K
    return fr


POSED = dict(Ho=24, Wo=40, V=2, B=2, seed=3)


def posed_frame(b=2):
    return posed(synthetic.make_frame(POSED["Ho"], POSED["Wo"], V=POSED["V"], B=POSED["B"], bundle_size=b, seed=POSED["seed"]))


# ---- HIP side ------------------------------------------------------------------------------------------------------------------
def cu(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def npy(t):
    return t.detach().cpu().numpy()


def cuda_frame(fr):
    return {k: cu(fr[k]) for k in FRAME_KEYS}


def engine(fr=None, w=None, **cfg):
    eng = HotPathEngine(**cfg)
    if w is not None:
        eng.load_weights(w)
    if fr is not None:
        eng.prepare(cuda_frame(fr))
    return eng


def twice(fn):
    """Two calls of an entry: bit-identical (NaN-prefilled rows included) -> the first result as a tuple of numpy arrays."""
    a, b = (tuple(npy(t) for t in fn()) for _ in range(2))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    return a


def raw_encode(eng, xyz, uvd, ball, spb, total, rfd, vox):
    """gdb_encode into the caller's (prefilled) outputs: `engine.encode` allocates its own."""
    f = eng._need_frame()
    eng._need_pyr32()
    _lib.check(eng.lib.gdb_encode(C.byref(eng.cfg), C.byref(f), eng._ws.data_ptr(), xyz.data_ptr(), uvd.data_ptr(), ball.data_ptr(),
                                  spb.data_ptr(), total.data_ptr(), xyz.shape[0], rfd.data_ptr(), vox.data_ptr(), eng._stream()))


def raw_mlp(eng, vox, rfd, total, sigma, feat):
    _lib.check(eng.lib.gdb_mlp(C.byref(eng.cfg), eng.weights.data_ptr(), rfd.shape[0], vox.data_ptr(), rfd.data_ptr(), total.data_ptr(),
                               rfd.shape[1], sigma.data_ptr(), feat.data_ptr(), eng._stream()))


# ---- build_rays ----------------------------------------------------------------------------------------------------------------
RAY_KEYS = ("rays_d", "uv", "rays_o", "z_axis", "tar_pixel_radius")
RAY_CASES = {
    "32x48_B2": lambda: synthetic.make_frame(32, 48, V=3, B=2, seed=1),
    "posed_24x40_B2": posed_frame,
    "10x14": lambda: synthetic.make_frame(10, 14, V=2, seed=4),
}


def rays_ref(fr):
    Ho, Wo = fr["src_images"].shape[-2:]
    return both(lambda c: oracle_t.build_rays(c(fr["tar_ext"]), c(fr["tar_int"]), Ho, Wo))


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_build_rays(name):
    fr = RAY_CASES[name]()
    eng = engine(fr)
    got = dict(zip(RAY_KEYS, twice(lambda: [eng.build_rays()[k] for k in RAY_KEYS])))
    r64, r32 = rays_ref(fr)
    check("build_rays/" + name, {k: (got[k], r64[k], r32[k]) for k in RAY_KEYS})


# ---- sample --------------------------------------------------------------------------------------------------------------------
# name: (Ho, Wo, B, bundle_size, S_max, adaptive, inv_depth, seed); "posed": the frame of posed_frame()
SAMPLE_CASES = {
    "ada3": (32, 48, 2, 2, 3, True, False, 1),
    "ada6_inv": (32, 48, 2, 2, 6, True, True, 1),
    "fix2_inv": (32, 48, 2, 2, 2, False, True, 1),
    "fix12": (32, 48, 2, 2, 12, False, False, 1),
    "ada3_bundle_1": (16, 24, 1, 1, 3, True, False, 7),
    "ada3_bundle_4": (32, 64, 1, 4, 3, True, False, 2),
    "ada6_bundle_4_inv": (32, 64, 1, 4, 6, True, True, 2),
    "one_scan_block_64x64": (64, 64, 1, 2, 3, True, False, 5),          # 1024 bundles: exactly one SCAN_BLOCK
    "two_scan_blocks_64x66": (64, 66, 1, 2, 3, True, False, 6),         # 1056: two blocks, the second nearly empty
    "batch_ends_mid_block_32x64_B2": (32, 64, 2, 2, 3, True, False, 8),  # 1024 over two batch items: the per_batch end falls mid-block
    "posed_ada3": "posed",
    "posed_ada6_inv": "posed",
}


def sample_setup(name):
    cfg = SAMPLE_CASES[name]
    if cfg == "posed":
        S, inv = (6, True) if name.endswith("inv") else (3, False)
        return posed_frame(), 2, S, True, inv
    Ho, Wo, B, b, S, adaptive, inv, seed = cfg
    return synthetic.make_frame(Ho, Wo, V=2, B=B, bundle_size=b, seed=seed), b, S, adaptive, inv


def ceil_args64(fr, inv):
    """The argument of the adaptive count's ceil (bundle_sampler.py:179), float64 from the float32 frame, per bundle."""
    dr, nf = fr["depth_range"].astype(np.float64), fr["near_far"].astype(np.float64)
    if inv:
        dr, nf = 1.0 / dr, 1.0 / nf
    miniv = np.abs(nf[:, 1] - nf[:, 0]) / NUM_DEPTH
    return (np.abs(dr[:, 1] - dr[:, 0]) / miniv[:, None, None]).reshape(-1)


def check_counts(fr, cnt_hip, b, S, adaptive, inv):
    """HIP's counts against the float32 restatement's: exact, but for a bundle whose float64 ceil argument is within COUNT_MARGIN of
    an integer (either neighbour); at most COUNT_CAP of the bundles may be such."""
    Ho, Wo = fr["src_images"].shape[-2:]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    s32 = oracle_t.sample_bundles(oracle_t.build_rays(t(fr["tar_ext"]), t(fr["tar_int"]), Ho, Wo), t(fr["depth_range"]), t(fr["vol_range"]),
                                  t(fr["near_far"][:, 0]), t(fr["near_far"][:, 1]), b, S, NUM_DEPTH, inv, adaptive)
    cnt32 = s32["samples_per_bundle"].numpy().astype(np.int64)
    arg = ceil_args64(fr, inv)
    near = (np.abs(arg - np.rint(arg)) < COUNT_MARGIN) if adaptive else np.zeros(arg.shape, bool)
    assert near.mean() <= COUNT_CAP, (int(near.sum()), near.size)
    assert cnt_hip.shape == cnt32.shape and np.array_equal(cnt_hip[~near], cnt32[~near])
    r = np.rint(arg[near])
    assert ((cnt_hip[near] == np.clip(r, 1, S)) | (cnt_hip[near] == np.clip(r + 1, 1, S))).all()
    return s32, bool((cnt_hip == cnt32).all())


def sample_ref(fr, cnt, b, inv):
    """build_rays -> sample_bundles_counted in both dtypes, plus tan^2 of the bundle axis per sample (the grouping of ball_radii)."""
    Ho, Wo = fr["src_images"].shape[-2:]
    cnt = torch.as_tensor(np.asarray(cnt), dtype=torch.int64)

    def run(c):
        rays = oracle_t.build_rays(c(fr["tar_ext"]), c(fr["tar_int"]), Ho, Wo)
        s = oracle_t.sample_bundles_counted(rays, c(fr["depth_range"]), c(fr["vol_range"]), b, inv, cnt)
        bidx = s["indices"] // ((Ho // b) * (Wo // b))
        axis = s["rays_xyz"].mean(dim=-1) - rays["rays_o"][bidx]
        cos = (axis * rays["z_axis"][bidx]).sum(-1) / axis.norm(dim=-1)
        return dict(s, tan2=1.0 / (cos * cos) - 1.0)
    return both(run)


def sample_tensors(got, r64, r32, n):
    near = r64["tan2"] < NEAR_AXIS_TAN2
    t = {k: (got[k][:n], r64[k], r32[k]) for k in ("z_vals", "rays_xyz")}
    t["uvd_uv"] = (got["uvd"][:n, :2], r64["uvd"][:, :2], r32["uvd"][:, :2])
    t["uvd_d"] = (got["uvd"][:n, 2], r64["uvd"][:, 2], r32["uvd"][:, 2])
    t["ball_radii"] = (got["ball_radii"][:n], r64["ball_radii"], r32["ball_radii"], {"near_axis": near, "off_axis": ~near})
    return t


SAMPLE_OUT = ("rays_xyz", "uvd", "z_vals", "ball_radii", "indices", "samples_per_batch", "samples_per_bundle", "total")


def hip_sample(eng):
    """-> engine.sample() as numpy, the rows at and past `total` dropped from what is compared across two calls (they are not written)."""
    def run():
        s = eng.sample()
        n = int(s["total"].item())
        return [s[k][:n] if s[k].shape[0] == s["rays_xyz"].shape[0] else s[k] for k in SAMPLE_OUT]
    return dict(zip(SAMPLE_OUT, twice(run)))


@pytest.mark.parametrize("name", list(SAMPLE_CASES))
def test_sample(name):
    fr, b, S, adaptive, inv = sample_setup(name)
    eng = engine(fr, bundle_size=b, max_num_samples=S, is_adaptive=adaptive, inv_depth=inv)
    got = hip_sample(eng)
    n, cnt = int(got["total"][0]), got["samples_per_bundle"].astype(np.int64)
    s32, same_counts = check_counts(fr, cnt, b, S, adaptive, inv)
    r64, r32 = sample_ref(fr, cnt, b, inv)
    # the integer outputs follow from the counts, exactly
    assert n == cnt.sum() == r64["z_vals"].shape[0]
    assert np.array_equal(got["indices"], r32["indices"].astype(np.int64))
    assert np.array_equal(got["samples_per_batch"], r32["samples_per_batch"].astype(np.int64))
    if same_counts:   # ... and are the float32 restatement's own
        assert np.array_equal(got["indices"], s32["indices"].numpy()) and np.array_equal(got["samples_per_batch"], s32["samples_per_batch"].numpy())
    if "scan_block" in name or "mid_block" in name:
        nb = cnt.size
        assert nb == {"one_scan_block_64x64": 1024, "two_scan_blocks_64x66": 1056, "batch_ends_mid_block_32x64_B2": 1024}[name]
    check("sample/" + name, sample_tensors(got, r64, r32, n))


# ---- encode --------------------------------------------------------------------------------------------------------------------
# name: (Ho, Wo, V, B, bundle_size, seed, src_focal_scale, inv_depth, mip levels built)
ENCODE_CASES = dict(ENCODE_CAMERAS)
ENCODE_CASES["eight_views_16x24"] = (16, 24, 8, 1, 2, 13, (1.0, 2.5, 6.0, 12.0, 1.5, 3.0, 1.0, 4.0), False, 2)
ENCODE_CASES["out_of_frame"] = (32, 64, 3, 1, 2, 11, (2.0, 1.0, 3.5), False, 3)
ENC_IN = ("rays_xyz", "uvd", "ball_radii")
_enc = {}


def encode_inputs(name):
    """Frame, prepared engine and the valid rows of HIP's own sample() (the arrays `encode` is given): built once, read-only."""
    if name not in _enc:
        Ho, Wo, V, B, b, seed, fs, inv, levels = ENCODE_CASES[name]
        fr = synthetic.make_frame(Ho, Wo, V=V, B=B, bundle_size=b, scene="dtu", seed=seed, src_focal_scale=fs)
        eng = engine(bundle_size=b, inv_depth=inv)
        assert eng.prepare(cuda_frame(fr)) == levels
        s = eng.sample()
        n = int(s["total"].item())
        smp = {k: npy(s[k])[:n].copy() for k in ENC_IN}
        if name == "out_of_frame":
            smp["uvd"][:, 2] *= np.float32(4.0)   # depth coordinates past the volume's faces (border)
        _enc[name] = dict(fr=fr, eng=eng, smp=smp, spb=npy(s["samples_per_batch"]), n=n, b=b)
    c = _enc[name]
    c["eng"].prepare(cuda_frame(c["fr"]))
    return c


def encode_ref(fr, smp, spb, b):
    Ho, Wo = fr["src_images"].shape[-2:]

    def run(c):
        s = {k: c(smp[k]) for k in ENC_IN}
        s["samples_per_batch"] = torch.as_tensor(np.asarray(spb), dtype=torch.int64)
        rfd, vox = oracle_t.encode(c(fr["src_images"]), c(fr["img_feat"]), c(fr["feat_volume"]), s, c(fr["src_exts"]), c(fr["src_ints"]),
                                   c(fr["tar_ext"]), b, Ho, Wo, 3)
        return {"rfd": rfd, "vox": vox}
    return both(run)


def encode_tensors(rfd, vox, r64, r32, b):
    k = 3 * b * b
    t = {}
    for name, sl in (("rgb", slice(0, k)), ("mip_feature", slice(k, k + 19)), ("dir_code", slice(k + 19, k + 23))):
        t[name] = (rfd[..., sl], r64["rfd"][..., sl], r32["rfd"][..., sl])
    for g in range(4):
        t[f"vox_{2 * g}{2 * g + 1}"] = (vox[:, 2 * g:2 * g + 2], r64["vox"][:, 2 * g:2 * g + 2], r32["vox"][:, 2 * g:2 * g + 2])
    return t


def hip_encode(c, smp=None, spb=None):
    smp, spb = c["smp"] if smp is None else smp, c["spb"] if spb is None else spb
    n = smp["rays_xyz"].shape[0]
    return twice(lambda: c["eng"].encode(cu(smp["rays_xyz"]), cu(smp["uvd"]), cu(smp["ball_radii"]), cu(spb, torch.int64),
                                         torch.tensor([n], dtype=torch.int64, device="cuda")))


@pytest.mark.parametrize("name", list(ENCODE_CASES))
def test_encode(name):
    c = encode_inputs(name)
    fr, smp, b = c["fr"], c["smp"], c["b"]
    if name == "out_of_frame":   # the case is what it says: source pixels outside the image, depth coordinates outside [-1, 1]
        Ho, Wo = fr["src_images"].shape[-2:]
        pts = np.transpose(smp["rays_xyz"].astype(np.float64), (0, 2, 1)).reshape(-1, 3)
        cam = np.einsum("vij,nj->vni", fr["src_exts"][0].astype(np.float64)[:, :3, :3], pts) + fr["src_exts"][0].astype(np.float64)[:, None, :3, 3]
        im = np.einsum("vij,vnj->vni", fr["src_ints"][0].astype(np.float64), cam)
        px, py = im[..., 0] / im[..., 2], im[..., 1] / im[..., 2]
        outside = (px < 0) | (px > Wo) | (py < 0) | (py > Ho)
        assert 0.05 < outside.mean() < 0.95 and (im[..., 2] > 1.0).all()
        assert 0.02 < (np.abs(smp["uvd"][:, 2]) > 1).mean() < 0.9
    rfd, vox = hip_encode(c)
    r64, r32 = encode_ref(fr, smp, c["spb"], b)
    check("encode/" + name, encode_tensors(rfd, vox, r64, r32, b))


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_encode_block_edges_and_rows_past_total(n):
    """total = n < n_alloc = n + 40, n on either side of k_encode_views' 128-wide blocks (k_encode_vox: 256 threads, one per (sample,
    channel)).  NaN in the input rows past the total; rows at and past the total of NaN-prefilled outputs stay NaN."""
    c = encode_inputs("levels_0_1_2")
    na, V, P = n + 40, c["fr"]["src_images"].shape[1], c["eng"].P
    smp = {k: c["smp"][k][:na].copy() for k in ENC_IN}
    head = {k: smp[k][:n].copy() for k in ENC_IN}
    for a in smp.values():
        a[n:] = np.nan
    spb, total = cu([n], torch.int64), cu([n], torch.int64)

    def run():
        rfd, vox = torch.full((V, na, P), float("nan"), device="cuda"), torch.full((na, 8), float("nan"), device="cuda")
        raw_encode(c["eng"], cu(smp["rays_xyz"]), cu(smp["uvd"]), cu(smp["ball_radii"]), spb, total, rfd, vox)
        return rfd, vox
    rfd, vox = twice(run)
    assert np.isnan(rfd[:, n:]).all() and np.isnan(vox[n:]).all()
    r64, r32 = encode_ref(c["fr"], head, [n], c["b"])
    check(f"encode/total_{n}_of_{na}", encode_tensors(rfd[:, :n], vox[:n], r64, r32, c["b"]))
    whole_rfd, whole_vox = hip_encode(c, head, [n])   # n_alloc = n: the same rows, bit for bit
    assert np.array_equal(whole_rfd, rfd[:, :n]) and np.array_equal(whole_vox, vox[:n])


SOFTPLUS_SCALE = 64.0


# ---- mlp -----------------------------------------------------------------------------------------------------------------------
_mlp_in = {}


def weights(seed=1):
    return synthetic.make_nerf_weights(seed=seed)


def mlp_inputs(V, Ho=16, Wo=24):
    """(vox_feat, rgbs_feat_dir) as HIP's own sample() -> encode() gives them on a V-view frame: the arrays `mlp` is given."""
    if (V, Ho, Wo) not in _mlp_in:
        fs = (1.0, 2.5, 6.0, 12.0, 1.5, 3.0, 1.0, 4.0)[:V]
        fr = synthetic.make_frame(Ho, Wo, V=V, seed=20 + V, src_focal_scale=fs)
        eng = engine(fr)
        s = eng.sample()
        n = int(s["total"].item())
        rfd, vox = eng.encode(*(s[k][:n].contiguous() for k in ENC_IN), s["samples_per_batch"], s["total"])
        _mlp_in[(V, Ho, Wo)] = (npy(vox), npy(rfd))
    return _mlp_in[(V, Ho, Wo)]


def mlp_ref(w, vox, rfd, viewdir=True):
    def run(c):
        sigma, feat = oracle_t.nerf_mlp({k: c(v) for k, v in w.items()}, c(vox), c(rfd), 16, viewdir)
        return {"sigma": sigma, "feat": feat}
    return both(run)


def mlp_tensors(sigma, feat, r64, r32):
    q = feat.shape[1] - 8
    return {"sigma": (sigma, r64["sigma"], r32["sigma"]), "feat_blend": (feat[:, :q], r64["feat"][:, :q], r32["feat"][:, :q]),
            "feat_head": (feat[:, q:], r64["feat"][:, q:], r32["feat"][:, q:])}


def referee_mlp(case, w, vox, rfd, viewdir=True):
    eng = engine(w=w, viewdir_agg=viewdir)
    sigma, feat = twice(lambda: eng.mlp(cu(vox), cu(rfd)))
    r64, r32 = mlp_ref(w, vox, rfd, viewdir)
    check("mlp/" + case, mlp_tensors(sigma, feat, r64, r32))
    return r64


@pytest.mark.parametrize("viewdir", [True, False], ids=["viewdir", "noviewdir"])
@pytest.mark.parametrize("V", range(2, 9))
def test_mlp_views(V, viewdir):
    vox, rfd = mlp_inputs(V)
    assert rfd.shape[0] == V and 100 <= rfd.shape[1] <= 300
    referee_mlp(f"V{V}_{'viewdir' if viewdir else 'noviewdir'}", weights(), vox, rfd, viewdir)


@pytest.mark.parametrize("n", [1, 127, 128, 129, None], ids=lambda n: "all" if n is None else str(n))
def test_mlp_block_edges(n):
    """n on either side of k_mlp's 128-wide blocks, and the ~2k samples of a 48 x 64 frame."""
    vox, rfd = mlp_inputs(3, 48, 64)
    assert 1500 <= rfd.shape[1] <= 2500
    if n is not None:
        vox, rfd = vox[:n], np.ascontiguousarray(rfd[:, :n])
    referee_mlp(f"n_{rfd.shape[1]}", weights(), vox, rfd)


def test_mlp_rows_past_total_are_untouched():
    vox, rfd = mlp_inputs(3, 48, 64)
    n, na = 129, 169
    vox, rfd = vox[:na].copy(), np.ascontiguousarray(rfd[:, :na])
    head = (vox[:n].copy(), np.ascontiguousarray(rfd[:, :n]))
    vox[n:], rfd[:, n:] = np.nan, np.nan
    w = weights()
    eng = engine(w=w)

    def run():
        sigma, feat = torch.full((na,), float("nan"), device="cuda"), torch.full((na, eng.Q), float("nan"), device="cuda")
        raw_mlp(eng, cu(vox), cu(rfd), cu([n], torch.int64), sigma, feat)
        return sigma, feat
    sigma, feat = twice(run)
    assert np.isnan(sigma[n:]).all() and np.isnan(feat[n:]).all()
    r64, r32 = mlp_ref(w, *head)
    check(f"mlp/total_{n}_of_{na}", mlp_tensors(sigma[:n], feat[:n], r64, r32))


@pytest.mark.parametrize("scale", [8.0, 0.125], ids=["x8", "x1_8"])
def test_mlp_scaled_inputs(scale):
    vox, rfd = mlp_inputs(3)
    referee_mlp(f"inputs_x{scale:g}", weights(), vox * np.float32(scale), rfd * np.float32(scale))


def test_mlp_softplus_both_ends():
    """sigma.0 scaled so that its pre-activations reach past +-20: the linear branch of softplus (threshold 20) and its underflowing end."""
    vox, rfd = mlp_inputs(3, 48, 64)
    w = weights()
    w["sigma.0.weight"], w["sigma.0.bias"] = w["sigma.0.weight"] * np.float32(SOFTPLUS_SCALE), w["sigma.0.bias"] * np.float32(SOFTPLUS_SCALE)
    r64 = referee_mlp("softplus_ends", w, vox, rfd)
    # softplus(x) > 20 <=> x > 20 (there it is x itself);  softplus(x) < exp(-20) <=> x < -20
    assert r64["sigma"].max() > 20.0 and 0.0 <= r64["sigma"].min() < np.exp(-20.0)


# ---- render_weights, accumulate, composite -------------------------------------------------------------------------------------
def drawn_segments(inv_depth, seed=31):
    """Bundles of 1 .. 16 (GDB_MAX_SAMPLES) samples, three rounds: plain; sigma exactly 0 (even lengths) or so small that the weights'
    sum, 0.5e-6 .. 0.9e-6, stays below the 1e-6 clamp of the normalising denominator (odd lengths); one sample of each bundle with
    sigma > 50.  An empty bundle follows every bundle."""
    rng = np.random.default_rng(seed)
    lens, sig = [], []
    for rnd in range(3):
        for L in range(1, 17):
            s = np.exp(rng.normal(-0.5, 1.5, L))
            if rnd == 1:
                if L % 2:
                    s = rng.uniform(0.5e-6 / L, 0.9e-6 / L, L)
                else:
                    s = np.zeros(L)
            if rnd == 2:
                s[rng.integers(L)] = 50.0 + 30.0 * rng.random()
            lens += [L, 0]
            sig.append(s)
    lens = np.asarray(lens)
    idx = np.repeat(np.arange(lens.size), lens)
    n = idx.size
    first = np.cumsum(lens) - lens
    z = 425.0 + 480.0 * (np.arange(n) - first[idx] + rng.random(n)) / lens[idx]
    return dict(sigma=np.concatenate(sig).astype(np.float32), feat=rng.standard_normal((n, 39)).astype(np.float32), z_vals=z.astype(np.float32),
                indices=idx.astype(np.int64), n_bundles=int(lens.size), inv_depth=inv_depth)


def composite_ref(sigma, feat, z, idx, nb, inv, den_floor=1e-6):
    wgt = oracle_t.render_weights(sigma, idx, nb, den_floor)
    return dict(zip(("bundle_feat", "depth", "opacity"), oracle_t.accumulate(wgt, feat, z, idx, nb, inv)), weights=wgt)


def render_tensors(got, r64, r32, idx, nb):
    """The tensors of `got` in three groups of bundles, split by ref64 alone: a bundle whose float64 weights sum to 1 (normalised); one
    where they sum to less - the denominator sat on its 1e-6 clamp: there the weights are alpha / 1e-6 with alpha = 1 - exp(-sigma) of a
    sigma below 1e-6, whose float32 rounding alone is a few per cent of the weight, and those few bundles would set the E32 of every
    tensor of the case; and a bundle without any weight (empty, or sigma = 0 throughout), where E32 = 0 and the rule asks for exact
    zeros."""
    total = r64["opacity"] if "opacity" in r64 else np.bincount(idx, weights=r64["weights"], minlength=nb)
    under = total < 0.999
    if "depth" in got:
        # under inv_depth a bundle without any weight (empty, or sigma = 0 throughout) has the depth 1 / 0: no finite referee.  Those
        # bundles - named by ref64 alone - are not left out but held exactly: +inf on every side; the rule then sees a 0 in their place.
        dead = ~np.isfinite(r64["depth"])
        assert not (dead & (total != 0)).any()
        assert all(np.array_equal(a[dead], np.full(int(dead.sum()), np.inf)) for a in (got["depth"], r64["depth"], r32["depth"]))
        got, r64, r32 = ({**d, "depth": np.where(dead, 0.0, d["depth"])} for d in (got, r64, r32))
    shape = {"weights": lambda m: m[idx], "bundle_feat": lambda m: m[:, None], "depth": lambda m: m, "opacity": lambda m: m}
    groups = {"no_weight": total == 0, "under_clamp": under & (total != 0), "normalised": ~under}
    return {k: (v, r64[k], r32[k], {g: shape[k](m) for g, m in groups.items()}) for k, v in got.items()}


RENDER_CASES = {"F5_dtu": lambda: load_golden("F5_render_dtu"), "F5_nerfinv": lambda: load_golden("F5_render_nerfinv"),
                "F5_mips": lambda: load_golden("F5_render_mips"), "segments_1_16": lambda: drawn_segments(False),
                "segments_1_16_inv_depth": lambda: drawn_segments(True)}


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_render_weights_accumulate_composite(name):
    fx = RENDER_CASES[name]()
    inv, nb = bool(fx["inv_depth"]), int(fx["n_bundles"])
    sigma, feat, z, idx = (np.ascontiguousarray(fx[k]) for k in ("sigma", "feat", "z_vals", "indices"))
    if name.startswith("segments"):
        cnt = np.bincount(idx, minlength=nb)
        assert set(range(1, 17)) <= set(cnt.tolist()) and (cnt == 0).sum() == 48 and (sigma == 0).sum() == 72 and (sigma > 50).sum() >= 16
    eng = engine(inv_depth=inv)
    it = torch.as_tensor(idx, dtype=torch.int64)
    d_sigma, d_feat, d_z, d_idx = cu(sigma), cu(feat), cu(z), cu(idx, torch.int64)
    names = ("bundle_feat", "depth", "opacity")
    # render_weights
    w_hip, = twice(lambda: [eng.render_weights(d_sigma, d_idx, nb)])
    r64, r32 = both(lambda c: {"weights": oracle_t.render_weights(c(sigma), it, nb)})
    check("render_weights/" + name, render_tensors({"weights": w_hip}, r64, r32, idx, nb))
    # accumulate, given HIP's weights; under inv_depth the caller hands over 1 / z and inverts the depth (Network.render_bundles)
    d_w = cu(w_hip)
    z_in = npy(1.0 / d_z) if inv else z
    fm, dm, om = twice(lambda: eng.accumulate(d_w, d_feat, cu(z_in), d_idx, nb))
    r64, r32 = both(lambda c: dict(zip(names, oracle_t.accumulate(c(w_hip), c(feat), c(z_in), it, nb, False))))
    check("accumulate/" + name, render_tensors(dict(zip(names, (fm, dm, om))), r64, r32, idx, nb))
    # composite: both in one entry, refereed as a whole from sigma
    w2, bf, depth, opac = twice(lambda: eng.composite(d_sigma, d_feat, d_z, d_idx, nb))
    r64, r32 = both(lambda c: composite_ref(c(sigma), c(feat), c(z), it, nb, inv))
    check("composite/" + name, render_tensors(dict(zip(("weights",) + names, (w2, bf, depth, opac))), r64, r32, idx, nb))
    # ... and is render_weights followed by accumulate, bit for bit
    dm_final = npy(1.0 / cu(dm)) if inv else dm
    assert np.array_equal(w2, w_hip) and np.array_equal(bf, fm) and np.array_equal(opac, om) and np.array_equal(depth, dm_final)


# ---- the chained mirrors -------------------------------------------------------------------------------------------------------
# name: (S_max, adaptive, make_frame keywords)
CHAIN_CASES = {"ada3": (3, True, {}), "fix6": (6, False, {}), "ada3_smooth_features": (3, True, dict(smooth_feat=5, smooth_vol=3))}


@pytest.mark.parametrize("name", list(CHAIN_CASES))
def test_chained_mirrors(name):
    """engine.render_unfused() against the float64 chain build_rays -> sample (HIP's counts) -> encode -> render_bundles on the frame,
    with the float32 chain's own E32: the one place where the operators' errors may compound."""
    S, adaptive, kw = CHAIN_CASES[name]
    fr, w = synthetic.make_frame(64, 80, V=3, seed=21, **kw), weights(3)
    Ho, Wo = fr["src_images"].shape[-2:]
    eng = engine(fr, w, max_num_samples=S, is_adaptive=adaptive)
    cnt = npy(eng.sample()["samples_per_bundle"]).astype(np.int64)
    check_counts(fr, cnt, 2, S, adaptive, False)
    bf, depth, opac = twice(eng.render_unfused)
    ct = torch.as_tensor(cnt)

    def run(c):
        rays = oracle_t.build_rays(c(fr["tar_ext"]), c(fr["tar_int"]), Ho, Wo)
        s = oracle_t.sample_bundles_counted(rays, c(fr["depth_range"]), c(fr["vol_range"]), 2, False, ct)
        rfd, vox = oracle_t.encode(c(fr["src_images"]), c(fr["img_feat"]), c(fr["feat_volume"]), s, c(fr["src_exts"]), c(fr["src_ints"]),
                                   c(fr["tar_ext"]), 2, Ho, Wo, 3)
        return dict(zip(("bundle_feat", "depth", "opacity"), oracle_t.render_bundles({k: c(v) for k, v in w.items()}, rfd, vox, s["z_vals"],
                                                                                     s["indices"], cnt.size, False)))
    r64, r32 = both(run)
    check("chain/" + name, {k: (v, r64[k], r32[k]) for k, v in (("bundle_feat", bf), ("depth", depth), ("opacity", opac))})

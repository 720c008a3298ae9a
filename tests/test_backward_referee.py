"""The HIP backward of the radiance MLP and of the normalised alpha composite against float64 autograd of the CPU restatement
(`gdb_oracle_torch.nerf_mlp` / `render_bundles`).  Runs on a real MI355X: `pytest -m gpu`.

Rule, per gradient tensor, elementwise, no element excluded:  |hip - ref64| <= 4 E32,  E32 = max |float32 CPU autograd of the same
restatement - ref64|, floored at 8 fp32 ulp of max |ref64|.  The kernel is not involved in the bound.

ReLU kinks: a sample with a ReLU pre-activation within 1e-5 of 0 (float64) has no fp32 answer to referee (the derivative jumps).
Such a sample's bundle is removed from the inputs of BOTH sides (a sample is its own bundle where a case has no bundles); at most
5 % of a case's samples may go, asserted.  The generated large case draws its 1 % jitter from seed 0.

Observed |hip - ref64| / bound per case and tensor: profiles/backward/referee_observed.txt (rewritten by a run of this file).

The Network test runs a 32 x 64 frame: the cost-regularisation U-Net of the depth net refuses 32 x 40 (its skip connections need the
coarse stage's width divisible by 8); the chain test, which needs no depth net, runs 32 x 40.  Its random initialisation is seed 109,
picked on the CPU alone (the float64 pre-activations of the restatement on the oracle's own sample / encode; float32 autograd of the
restatement and of the PyTorch decoder on the oracle's bundle features): 48 of 1536 samples leave with their bundles, and no
gradient is identically zero in torch itself.  A freshly initialised head has pre-activations of order 0.1 and every kink sample
takes its bundle's three samples along: seeds 0 .. 39 lose 3.3 % to 15 %, most of them more than the cap.  And at many seeds a ReLU
behind a single unit is dead on every sample of so small a frame - the view score of `agg_w_fc` (seeds 4, 30, 44), the blend score of
`weight.2` (45, 68, 75, 95: `weight.0` and `weight.2` then get an exactly zero gradient), a squeeze-excitation unit of the decoder
(10) - which is the network's arithmetic, not the kernels'.  Seeds 70, 91, 103, 104, 105, 109 and 149 pass both; 109 loses fewest.
"""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gdb_oracle_torch as oracle_t
from conftest import FRAME_KEYS, load_golden, nerf_weights_of
from gdb_nerf_amd import synthetic
from gdb_nerf_amd.engine import NERF_KEYS, HotPathEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "backward", "referee_observed.txt")
KINK, CAP = 1e-5, 0.05
PARAM_KEYS = [k + s for k in NERF_KEYS for s in (".weight", ".bias")]


# ---- referee ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)   # the restatement allocates its tables with the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def relu_preacts64(w, vox, x, viewdir):
    """Smallest |ReLU pre-activation| per sample, float64 (nerf.py:58-115)."""
    W = lambda k: torch.as_tensor(w[k + ".weight"], dtype=torch.float64)
    Bi = lambda k: torch.as_tensor(w[k + ".bias"], dtype=torch.float64)
    vox, x = torch.as_tensor(vox, dtype=torch.float64), torch.as_tensor(x, dtype=torch.float64)
    tail = x[..., -23:]
    g, pre = tail[..., :19], []
    if viewdir:
        vp = tail[..., 19:] @ W("view_fc.0").T + Bi("view_fc.0")
        g = g + vp.clamp(min=0)
        pre.append(vp.abs().amin(-1).amin(0))
    var, mean = torch.var_mean(g, dim=0, keepdim=True)
    A = torch.cat((g, var.expand_as(g), mean.expand_as(g)), -1) @ W("global_fc.0").T + Bi("global_fc.0")
    G = A.clamp(min=0)
    sp = G @ W("agg_w_fc.0").T + Bi("agg_w_fc.0")
    a = torch.softmax(sp.clamp(min=0), 0)
    fcp = (G * a).sum(0) @ W("fc.0").T + Bi("fc.0")
    h = torch.cat((vox, fcp.clamp(min=0)), -1)
    lp = h @ W("lr0.0").T + Bi("lr0.0")
    xx = lp.clamp(min=0)
    V = x.shape[0]
    hid = torch.cat((xx.expand(V, -1, -1), h.expand(V, -1, -1), tail), -1) @ W("weight.0").T + Bi("weight.0")
    up = hid.clamp(min=0) @ W("weight.2").T + Bi("weight.2")
    fhp = xx @ W("feat_head.0").T + Bi("feat_head.0")
    pre += [A.abs().amin(-1).amin(0), sp.abs().amin(-1).amin(0), fcp.abs().amin(-1), lp.abs().amin(-1), hid.abs().amin(-1).amin(0),
            up.abs().amin(-1).amin(0), fhp.abs().amin(-1)]
    return torch.stack(pre).amin(0).numpy()


def keep_mask(w, vox, x, viewdir, indices=None):
    """Samples that stay: none of their bundle's samples sits on a ReLU kink.  Asserts the 5 % cap."""
    bad = relu_preacts64(w, vox, x, viewdir) < KINK
    if indices is not None:
        bad = np.isin(indices, np.unique(indices[bad]))
    assert bad.mean() <= CAP, f"{bad.sum()} of {bad.size} samples removed"
    return ~bad


def mlp_ref(w, vox, x, g_sigma, g_feat, dtype, viewdir):
    """Autograd of the restatement on the CPU in `dtype` -> {tensor name: gradient as float64 numpy}."""
    with default_dtype(dtype):
        wt = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in w.items() if viewdir or not k.startswith("view_fc")}
        vt, xt = torch.tensor(vox, dtype=dtype, requires_grad=True), torch.tensor(x, dtype=dtype, requires_grad=True)
        sigma, feat = oracle_t.nerf_mlp(wt, vt, xt, 16, viewdir)
        loss = (sigma * torch.tensor(g_sigma, dtype=dtype)).sum() + (feat * torch.tensor(g_feat, dtype=dtype)).sum()
        loss.backward()
    out = {k: t.grad.double().numpy() for k, t in wt.items()}
    out["vox"], out["rfd"] = vt.grad.double().numpy(), xt.grad.double().numpy()
    return out


def bundles_ref(w, vox, x, z, idx, nb, inv_depth, gF, gD, gO, dtype, viewdir=True, mlp_out=None):
    """Autograd of `render_bundles` for the loss gF . feat + gD . depth + gO . opacity.  mlp_out = (sigma, feat): the composite alone
    (the restatement's MLP call is answered with these leaves), gradients of sigma and feat."""
    with default_dtype(dtype):
        c = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
        it = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
        if mlp_out is not None:
            leaves = {"sigma": c(mlp_out[0]).requires_grad_(), "feat": c(mlp_out[1]).requires_grad_()}
            saved, oracle_t.nerf_mlp = oracle_t.nerf_mlp, lambda *a, **k: (leaves["sigma"], leaves["feat"])
            try:
                f, d, o = oracle_t.render_bundles(None, None, None, c(z), it, nb, inv_depth)
            finally:
                oracle_t.nerf_mlp = saved
        else:
            leaves = {k: c(v).requires_grad_() for k, v in w.items() if viewdir or not k.startswith("view_fc")}
            leaves["vox"], leaves["rfd"] = c(vox).requires_grad_(), c(x).requires_grad_()
            f, d, o = oracle_t.render_bundles({k: leaves[k] for k in leaves if k not in ("vox", "rfd")}, leaves["rfd"], leaves["vox"], c(z), it,
                                              nb, inv_depth, 16, viewdir)
        ((f * c(gF)).sum() + (d * c(gD)).sum() + (o * c(gO)).sum()).backward()
    return {k: (torch.zeros_like(t) if t.grad is None else t.grad).double().numpy() for k, t in leaves.items()}


_observed = {}


def check_rule(case, hip, ref64, ref32):
    """hip, ref64, ref32: {name: array}.  Prints each figure, records it, then asserts the rule for every tensor."""
    fails = []
    for name, r64 in ref64.items():
        h = np.asarray(hip[name], np.float64)
        assert h.shape == r64.shape, (case, name, h.shape, r64.shape)
        top = float(np.abs(r64).max()) if r64.size else 0.0
        e32 = float(np.abs(ref32[name] - r64).max()) if r64.size else 0.0
        bound = 4.0 * max(e32, 8.0 * float(np.spacing(np.float32(top))))
        err = float(np.abs(h - r64).max()) if r64.size else 0.0
        if not np.isfinite(h).all():
            err = float("inf")
        line = f"{case:28s} {name:22s} err {err:.3e}  bound {bound:.3e}  err/bound {err / bound if bound else 0.0:.3f}  max|ref64| {top:.3e}"
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
            f.write("# |hip - ref64| per gradient tensor against the bound 4 * max(E32, 8 ulp of max |ref64|); tests/test_backward_referee.py\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError:
        pass
    assert not fails, "\n".join(fails)


# ---- HIP side ----------------------------------------------------------------------------------------------------------------
def cu(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def npy(t):
    return t.detach().cpu().numpy()


def hip_mlp_grads(eng, vox, x, g_sigma, g_feat, viewdir, total=None, need_vox=True, need_rfd=True):
    gp, gv, gx = eng.mlp_backward(cu(vox), cu(x), cu(g_sigma), cu(g_feat), total=total, need_vox=need_vox, need_rfd=need_rfd)
    gp = npy(gp)
    out = {}
    for key, (off, shp) in zip(PARAM_KEYS, eng.packed_grad_slices()[0]):
        if viewdir or not key.startswith("view_fc"):
            out[key] = gp[off:off + int(np.prod(shp))].reshape(shp)
    out["vox"], out["rfd"] = (None if gv is None else npy(gv)), (None if gx is None else npy(gx))
    return out, gp


def mlp_case(name):
    fx = load_golden(name)
    viewdir = name != "F3_nerf_noviewdir"
    w = nerf_weights_of(fx)
    keep = keep_mask(w, fx["vox_feat"], fx["rgbs_feat_dir"], viewdir)
    return w, np.ascontiguousarray(fx["vox_feat"][keep]), np.ascontiguousarray(fx["rgbs_feat_dir"][:, keep]), viewdir


def upstream(n, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, cols)).astype(np.float32)


def engine(w, viewdir=True, **cfg):
    eng = HotPathEngine(viewdir_agg=viewdir, **cfg)
    eng.load_weights(w)
    return eng


@pytest.mark.parametrize("name", ["F3_nerf_V2", "F3_nerf_V3", "F3_nerf_V5", "F3_nerf_noviewdir"])
def test_mlp_backward_on_the_fixtures(name):
    w, vox, x, viewdir = mlp_case(name)
    gs, gf = upstream(vox.shape[0], x.shape[2] - 4 + 8, 1)
    hip, _ = hip_mlp_grads(engine(w, viewdir), vox, x, gs, gf, viewdir)
    check_rule(name, hip, mlp_ref(w, vox, x, gs, gf, torch.float64, viewdir), mlp_ref(w, vox, x, gs, gf, torch.float32, viewdir))


def test_mlp_backward_one_sample():
    w, vox, x, viewdir = mlp_case("F3_nerf_V3")
    vox, x = vox[:1], np.ascontiguousarray(x[:, :1])
    gs, gf = upstream(1, x.shape[2] + 4, 2)
    hip, _ = hip_mlp_grads(engine(w), vox, x, gs, gf, True)
    check_rule("one_sample", hip, mlp_ref(w, vox, x, gs, gf, torch.float64, True), mlp_ref(w, vox, x, gs, gf, torch.float32, True))


def test_mlp_backward_two_tiles_per_workgroup_and_a_single_sample_tile():
    """N = 2 * partials * tile + 1: every workgroup accumulates at least two tiles, the last tile holds one sample.  F3_nerf_V3's rows
    tiled, with a 1 % multiplicative jitter from seed 0; kink samples are dropped before the first N are taken."""
    fx = load_golden("F3_nerf_V3")
    w = nerf_weights_of(fx)
    eng = engine(w)
    _, parts, tile = eng.mlp_backward_layout(3, 1 << 24)
    N = 2 * parts * tile + 1
    assert eng.mlp_backward_layout(3, N)[1] == parts
    rng = np.random.default_rng(0)
    M = N + N // 10
    rep = -(-M // fx["vox_feat"].shape[0])
    vox = np.tile(fx["vox_feat"], (rep, 1))[:M]
    x = np.tile(fx["rgbs_feat_dir"], (1, rep, 1))[:, :M]
    vox = (vox * (1 + 0.01 * rng.standard_normal(vox.shape))).astype(np.float32)
    x = (x * (1 + 0.01 * rng.standard_normal(x.shape))).astype(np.float32)
    keep = np.flatnonzero(keep_mask(w, vox, x, True))[:N]
    assert keep.size == N and (keep[-1] + 1 - N) <= CAP * (keep[-1] + 1)
    vox, x = np.ascontiguousarray(vox[keep]), np.ascontiguousarray(x[:, keep])
    gs, gf = upstream(N, x.shape[2] + 4, 3)
    hip, _ = hip_mlp_grads(eng, vox, x, gs, gf, True)
    check_rule("two_tiles_plus_one", hip, mlp_ref(w, vox, x, gs, gf, torch.float64, True), mlp_ref(w, vox, x, gs, gf, torch.float32, True))


def test_mlp_backward_total_below_n_alloc_and_null_outputs():
    w, vox, x, _ = mlp_case("F3_nerf_V3")
    N = vox.shape[0]
    n = N - 37
    gs, gf = upstream(N, x.shape[2] + 4, 4)
    ref64 = mlp_ref(w, vox[:n], x[:, :n], gs[:n], gf[:n], torch.float64, True)
    ref32 = mlp_ref(w, vox[:n], x[:, :n], gs[:n], gf[:n], torch.float32, True)
    vox, x, gs, gf = vox.copy(), x.copy(), gs.copy(), gf.copy()
    vox[n:], x[:, n:], gs[n:], gf[n:] = np.nan, np.nan, np.nan, np.nan
    eng = engine(w)
    hip, packed = hip_mlp_grads(eng, vox, x, gs, gf, True, total=torch.tensor([n], device="cuda"))
    assert not hip["vox"][n:].any() and not hip["rfd"][:, n:].any()        # tail rows: zeros, whatever the inputs hold
    hip["vox"], hip["rfd"] = hip["vox"][:n], hip["rfd"][:, :n]
    check_rule("total_below_n_alloc", hip, ref64, ref32)
    none, packed2 = hip_mlp_grads(eng, vox, x, gs, gf, True, total=torch.tensor([n], device="cuda"), need_vox=False, need_rfd=False)
    assert none["vox"] is None and none["rfd"] is None and np.array_equal(packed, packed2)


# ---- composite ----------------------------------------------------------------------------------------------------------------
def hand_built():
    """Bundle 0 empty; 1 one sample; 2 eight samples (max_num_samples 8); 3 all sigma 1e-9 (the clamp is active: no derivative through
    the sum); 4 sigma 100 first (1 - alpha underflows); 5 empty."""
    rng = np.random.default_rng(5)
    counts = [0, 1, 8, 3, 4, 0]
    idx = np.repeat(np.arange(6), counts).astype(np.int64)
    sigma = rng.uniform(0.05, 2.0, idx.size).astype(np.float32)
    sigma[idx == 3] = 1e-9
    sigma[np.flatnonzero(idx == 4)[0]] = 100.0
    feat = rng.standard_normal((idx.size, 5)).astype(np.float32)
    z = np.sort(rng.uniform(2.0, 6.0, idx.size)).astype(np.float32)
    return {"sigma": sigma, "feat": feat, "z_vals": z, "indices": idx, "n_bundles": 6, "inv_depth": 0}


def composite_case(tag):
    fx = hand_built() if tag == "hand_built" else load_golden("F5_render_" + tag)
    return (np.asarray(fx["sigma"], np.float32), np.asarray(fx["feat"], np.float32), np.asarray(fx["z_vals"], np.float32),
            np.asarray(fx["indices"], np.int64), int(fx["n_bundles"]), bool(fx["inv_depth"]))


@pytest.mark.parametrize("tag", ["dtu", "nerfinv", "hand_built"])
def test_composite_backward_pieces_and_chain(tag):
    from gdb_nerf_amd.networks.gdb_nerf.network import Network
    sigma, feat, z, idx, nb, inv = composite_case(tag)
    n, ch = feat.shape
    rng = np.random.default_rng(6)
    eng = HotPathEngine(inv_depth=inv, max_num_samples=8)
    zz = (1.0 / z).astype(np.float32) if inv else z   # what Network.render_bundles hands the composite

    # piece 1, render weights: loss = sum g_w w is the restatement's feature map of the one-column feature g_w, summed
    g_w = rng.standard_normal(n).astype(np.float32)
    hip = {"sigma": npy(eng.render_weights_backward(cu(sigma), cu(idx, torch.int64), nb, cu(g_w)))}
    args = (None, None, None, zz, idx, nb, False, np.ones((nb, 1)), np.zeros(nb), np.zeros(nb))
    r64, r32 = (bundles_ref(*args, dt, mlp_out=(sigma, g_w[:, None])) for dt in (torch.float64, torch.float32))
    check_rule(f"render_weights_{tag}", hip, {"sigma": r64["sigma"]}, {"sigma": r32["sigma"]})

    # piece 2, accumulate: g_feat from the restatement (its own weights); g_weights from the three-term sum in float64
    gF, gZ, gO = rng.standard_normal((nb, ch)).astype(np.float32), rng.standard_normal(nb).astype(np.float32), rng.standard_normal(nb).astype(np.float32)
    w_hip = eng.render_weights(cu(sigma), cu(idx, torch.int64), nb)
    g_wa, g_fa = eng.accumulate_backward(w_hip, cu(feat), cu(zz), cu(idx, torch.int64), nb, cu(gF), cu(gZ), cu(gO))
    args = (None, None, None, zz, idx, nb, False, gF, gZ, gO)
    r64, r32 = (bundles_ref(*args, dt, mlp_out=(sigma, feat)) for dt in (torch.float64, torch.float32))
    gw64 = (gF.astype(np.float64)[idx] * feat).sum(1) + gZ.astype(np.float64)[idx] * zz + gO[idx]
    gw32 = ((gF[idx] * feat).sum(1, dtype=np.float32) + gZ[idx] * zz + gO[idx]).astype(np.float64)
    check_rule(f"accumulate_{tag}", {"feat": npy(g_fa), "weights": npy(g_wa)}, {"feat": r64["feat"], "weights": gw64},
               {"feat": r32["feat"], "weights": gw32})

    # the chain, through Network.render_bundles (torch's 1/z and 1/depth around the calls when inv_depth)
    st, ft = cu(sigma).requires_grad_(), cu(feat).requires_grad_()
    stub = SimpleNamespace(nerf=lambda vox, rfd: (st, ft), inv_depth=inv)
    f, d, o = Network.render_bundles(stub, None, None, cu(z), cu(idx, torch.int64), torch.empty(nb))
    ((f * cu(gF)).sum() + (d * cu(gZ)).sum() + (o * cu(gO)).sum()).backward()
    if tag == "hand_built":
        d_ok = np.isfinite(npy(d))   # an empty or fully clamped bundle has no depth under inv_depth; not the case here
        assert d_ok.all()
    args = (None, None, None, z, idx, nb, inv, gF, gZ, gO)
    r64, r32 = (bundles_ref(*args, dt, mlp_out=(sigma, feat)) for dt in (torch.float64, torch.float32))
    check_rule(f"composite_chain_{tag}", {"sigma": npy(st.grad), "feat": npy(ft.grad)}, r64, r32)

    # determinism
    a = eng.render_weights_backward(cu(sigma), cu(idx, torch.int64), nb, cu(g_w))
    assert np.array_equal(npy(a), hip["sigma"])
    b = eng.accumulate_backward(w_hip, cu(feat), cu(zz), cu(idx, torch.int64), nb, cu(gF), cu(gZ), cu(gO))
    assert np.array_equal(npy(b[0]), npy(g_wa)) and np.array_equal(npy(b[1]), npy(g_fa))


# ---- chain on real samples ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_samples():
    """A 32 x 40 synthetic frame through engine.sample -> encode, with the bundles of kink samples removed."""
    frame = synthetic.make_frame(32, 40, V=3, scene="dtu", seed=11)
    w = synthetic.make_nerf_weights(seed=3)
    eng = engine(w)
    eng.prepare({k: torch.from_numpy(np.ascontiguousarray(frame[k])).cuda() for k in FRAME_KEYS})
    s = eng.sample()
    rfd, vox = eng.encode(s["rays_xyz"], s["uvd"], s["ball_radii"], s["samples_per_batch"], s["total"])
    n = int(s["total"].item())
    rfd, vox, z, idx = npy(rfd)[:, :n], npy(vox)[:n], npy(s["z_vals"])[:n], npy(s["indices"])[:n]
    keep = keep_mask(w, vox, rfd, True, idx)
    return w, np.ascontiguousarray(rfd[:, keep]), np.ascontiguousarray(vox[keep]), z[keep], idx[keep], eng.n_bundles


def test_chain_on_real_samples(real_samples):
    from gdb_nerf_amd.networks.gdb_nerf.nerf import NeRF
    from gdb_nerf_amd.networks.gdb_nerf.network import Network
    w, rfd, vox, z, idx, nb = real_samples
    rng = np.random.default_rng(8)
    gF, gD, gO = rng.standard_normal((nb, 35 - 4 + 8)).astype(np.float32), rng.standard_normal(nb).astype(np.float32), rng.standard_normal(nb).astype(np.float32)
    gD *= 1e-2   # depths are O(500) scene units
    hips = []
    for _ in range(2):
        nerf = NeRF().cuda()
        nerf.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()})
        rt, vt = cu(rfd).requires_grad_(), cu(vox).requires_grad_()
        f, d, o = Network.render_bundles(SimpleNamespace(nerf=nerf, inv_depth=False), rt, vt, cu(z), cu(idx, torch.int64), torch.empty(nb))
        assert f.grad_fn is not None
        ((f * cu(gF)).sum() + (d * cu(gD)).sum() + (o * cu(gO)).sum()).backward()
        hip = {k: npy(p.grad) for k, p in nerf.named_parameters()}
        hip["vox"], hip["rfd"] = npy(vt.grad), npy(rt.grad)
        hips.append(hip)
    assert set(hips[0]) == set(PARAM_KEYS) | {"vox", "rfd"}
    for k in hips[0]:
        assert np.array_equal(hips[0][k], hips[1][k]), k   # no atomics: bit-identical from run to run
    args = (w, vox, rfd, z, idx, nb, False, gF, gD, gO)
    check_rule("chain_32x40", hips[0], bundles_ref(*args, torch.float64), bundles_ref(*args, torch.float32))


def test_mlp_backward_is_deterministic():
    w, vox, x, _ = mlp_case("F3_nerf_V5")
    gs, gf = upstream(vox.shape[0], x.shape[2] + 4, 9)
    eng = engine(w)
    a, pa = hip_mlp_grads(eng, vox, x, gs, gf, True)
    b, pb = hip_mlp_grads(eng, vox, x, gs, gf, True)
    assert np.array_equal(pa, pb) and np.array_equal(a["vox"], b["vox"]) and np.array_equal(a["rfd"], b["rfd"])


# ---- Network ----------------------------------------------------------------------------------------------------------------
def test_network_mirrors_trains_the_radiance_head_and_the_decoder():
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    fr = synthetic.make_frame(32, 64, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    batch = {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
             "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}
    torch.manual_seed(109)
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False"])).eval().cuda()
    w = {k: npy(v) for k, v in net.nerf.state_dict().items()}
    seen = {}
    inner = net.render_bundles

    def render_bundles(rfd, vox, z, idx, per_bundle):
        # the bundles of kink samples leave the inputs of both sides; autograd's own upstream gradients are captured by hooks
        keep = torch.from_numpy(keep_mask(w, npy(vox), npy(rfd), True, npy(idx))).cuda()
        rfd, vox, z, idx = rfd[:, keep].contiguous(), vox[keep].contiguous(), z[keep].contiguous(), idx[keep].contiguous()
        f, d, o = inner(rfd, vox, z, idx, per_bundle)
        seen.update(rfd=npy(rfd), vox=npy(vox), z=npy(z), idx=npy(idx), nb=per_bundle.shape[0], up={})
        for name, out in (("f", f), ("d", d), ("o", o)):
            if out.requires_grad:
                # (an output of the composite that the loss does not reach sees an undefined gradient: None)
                out.register_hook(lambda g, name=name: None if g is None else seen["up"].__setitem__(name, npy(g)))
        return f, d, o

    net.render_bundles = render_bundles
    ret = net(batch)[0]
    before = ret["rgb"].detach().clone()
    ret["rgb"].square().mean().backward()
    for k, p in net.named_parameters():
        if k.startswith(("nerf.", "upsampler.")):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k
        else:
            assert k.startswith(("feature_net.", "depth_net.")) and p.grad is None, k
    nb = seen["nb"]
    gF = seen["up"]["f"]
    gD, gO = seen["up"].get("d", np.zeros(nb, np.float32)), seen["up"].get("o", np.zeros(nb, np.float32))
    args = (w, seen["vox"], seen["rfd"], seen["z"], seen["idx"], nb, bool(net.inv_depth), gF, gD, gO)
    r64, r32 = bundles_ref(*args, torch.float64), bundles_ref(*args, torch.float32)
    hip = {k: npy(p.grad) for k, p in net.nerf.named_parameters()}
    check_rule("network_mirrors_32x64", hip, {k: r64[k] for k in hip}, {k: r32[k] for k in hip})
    torch.optim.SGD(net.parameters(), lr=1e-2).step()
    with torch.no_grad():
        after = net(batch)[0]["rgb"]
    assert not torch.equal(before, after)   # the re-pack saw the optimiser's update

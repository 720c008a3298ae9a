"""The feature pyramid network (networks/gdb_nerf/feature_net.py) on the HIP library: gdb_fpn and friends (include/gdb_nerf_hip.h),
fpn.FeaturePyramid and the `fpn.hip_feature_net` switch of FeatureNet / Network.  CPU: the packed layout, the refusals and the
switch's plumbing against the built library.  GPU: the PyTorch module (float64 on the CPU and fp32 on the GPU), fixture F7 and the
whole network."""
import ctypes as C

import numpy as np
import pytest
import torch

import gdb_oracle as oracle
from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, fpn
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf.feature_net import FeatureNet

MASKS = {(0,): 1, (0, 1): 3, (0, 1, 2): 7}


def _fpn(c=8, outs=(32, 16, 8), seed=0):
    """A FeatureNet with random weights and non-trivial BN statistics (as tests/golden/make_golden_network.py:36-41)."""
    torch.manual_seed(seed)
    m = FeatureNet(c, outs).eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.2, 0.2)
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.8, 1.2)
    return m


def _layers(c, outs):
    """The packed layout of include/gdb_nerf_hip.h restated: per layer (name, ks, cin, cout, kind, T, E, K, zs, w_off, ep_off)."""
    spec = [("conv0.0", 3, 3, c, "bn"), ("conv0.1", 3, c, c, "bn"), ("conv1.0", 5, c, 2 * c, "bn"), ("conv1.1", 3, 2 * c, 2 * c, "bn"),
            ("conv2.0", 5, 2 * c, 4 * c, "bn"), ("conv2.1", 3, 4 * c, 4 * c, "bn"), ("out0", 1, 4 * c, outs[0], "bias"),
            ("inner1", 1, 2 * c, 4 * c, "bias"), ("inner2", 1, c, 4 * c, "bias"), ("out1", 3, 4 * c, outs[1], "none"),
            ("out2", 3, 4 * c, outs[2], "none")]
    out, o = [], 0
    for name, ks, ci, co, kind in spec:
        zs = 2 if (ks == 3 and co == 8 and name not in ("conv1.0", "conv2.0")) else 1
        if name == "conv0.0":
            E, K, T = 1, 1, (9 * (4 if zs == 2 else 3) + 3) // 4
        else:
            E = 4 if ci % 16 == 0 else 2
            K, T = ci // (4 * E), (12 if zs == 2 else ks * ks)
        rows = zs * co
        w_off = o
        o = (o + ((rows + 15) // 16) * T * K * 64 * E + 63) // 64 * 64
        ep_off = o
        o = (o + {"bn": 4 * co, "bias": co, "none": 0}[kind] + 63) // 64 * 64
        out.append(dict(name=name, ks=ks, cin=ci, cout=co, kind=kind, rows=rows, T=T, E=E, K=K, zs=zs, w_off=w_off, ep_off=ep_off))
    return out, o


def _pack(m, c, outs):
    lib = _lib.load()
    sd = m.state_dict()
    arrs = [np.ascontiguousarray(sd[k].numpy(), dtype=np.float32) for k in fpn.fpn_keys()] + [np.array([1e-5], np.float32)]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    n = C.c_size_t()
    _lib.check(lib.gdb_fpn_packed_floats(c, *outs, C.byref(n)))
    host = np.full(n.value, np.nan, np.float32)
    _lib.check(lib.gdb_pack_fpn_weights(c, *outs, ptrs, host.ctypes.data))
    return host, n.value


@pytest.mark.parametrize("c,outs", [(8, (32, 16, 8)), (8, (16, 16, 8)), (16, (32, 16, 8))])
def test_packed_layout_round_trip(c, outs):
    m = _fpn(c, outs)
    host, n = _pack(m, c, outs)
    layers, total = _layers(c, outs)
    assert n == total and np.isfinite(host).all()     # packed_floats agrees with what the packer writes (every float written)
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(c + sum(outs))
    for L in layers:
        W = sd[L["name"] + (".0.weight" if L["kind"] == "bn" else ".weight")]
        for _ in range(300):
            mt = int(rng.integers(0, (L["rows"] + 15) // 16)); tap = int(rng.integers(0, L["T"])); cc = int(rng.integers(0, L["K"]))
            lane = int(rng.integers(0, 64)); e = int(rng.integers(0, L["E"]))
            got = host[L["w_off"] + (((mt * L["T"] + tap) * L["K"] + cc) * 64 + lane) * L["E"] + e]
            row, kq = 16 * mt + (lane & 15), lane >> 4
            s, co = (row // 8, row % 8) if L["zs"] == 2 else (0, row)
            if L["name"] == "conv0.0":
                R = 4 if L["zs"] == 2 else 3
                k = 4 * tap + kq
                ci, ky, kx = k // (3 * R), (k // 3) % R - s, k % 3
                valid = k < 9 * R
            else:
                ci = 4 * L["E"] * cc + L["E"] * kq + e
                ky, kx = (tap // 3 - s, tap % 3) if L["zs"] == 2 else (tap // L["ks"], tap % L["ks"])
                valid = True
            want = W[co, ci, ky, kx] if valid and row < L["rows"] and 0 <= ky < L["ks"] else 0.0
            assert got == np.float32(want), (L["name"], mt, tap, cc, lane, e)
        co = L["cout"]
        if L["kind"] == "bn":
            ep = host[L["ep_off"]:L["ep_off"] + 4 * co].reshape(4, co)
            p = L["name"] + ".1."
            assert np.array_equal(ep[0], (1.0 / np.sqrt(sd[p + "running_var"] + np.float32(1e-5))).astype(np.float32))
            assert np.array_equal(ep[1], sd[p + "running_mean"]) and np.array_equal(ep[2], sd[p + "weight"]) and np.array_equal(ep[3], sd[p + "bias"])
        elif L["kind"] == "bias":
            assert np.array_equal(host[L["ep_off"]:L["ep_off"] + co], sd[L["name"] + ".bias"])


def test_refusals_come_before_any_launch():
    """Bad channel counts, a NULL output whose level is asked for, an empty mask, a bad shape and a short workspace are refused with a
    status and a message; the device pointers are never touched (they are not even device memory here)."""
    lib = _lib.load()
    n = C.c_size_t()
    for c, outs in ((12, (32, 16, 8)), (40, (32, 16, 8)), (0, (32, 16, 8)), (8, (36, 16, 8)), (8, (32, 72, 8)), (8, (32, 16, 4))):
        assert lib.gdb_fpn_packed_floats(c, *outs, C.byref(n)) == _lib.GDB_E_BADARG, (c, outs)
    assert b"out_channels[2]" in lib.gdb_last_error() and b"64" in lib.gdb_last_error()
    assert lib.gdb_fpn_packed_floats(40, 32, 16, 8, C.byref(n)) == _lib.GDB_E_BADARG and b"at most 32" in lib.gdb_last_error()
    assert lib.gdb_fpn_workspace_bytes(8, 32, 16, 8, 3, 64, 96, 0, C.byref(n)) == _lib.GDB_E_BADARG
    assert b"level_mask" in lib.gdb_last_error()
    assert lib.gdb_fpn_workspace_bytes(8, 32, 16, 8, 3, 64, 96, 8, C.byref(n)) == _lib.GDB_E_BADARG
    assert lib.gdb_fpn_workspace_bytes(8, 32, 16, 8, 0, 64, 96, 7, C.byref(n)) == _lib.GDB_E_SHAPE
    assert lib.gdb_fpn_workspace_bytes(8, 32, 16, 8, 3, 64, 0, 7, C.byref(n)) == _lib.GDB_E_SHAPE

    def ws(N, H, W, mask, c=8):
        _lib.check(lib.gdb_fpn_workspace_bytes(c, 32, 16, 8, N, H, W, mask, C.byref(n)))
        return n.value
    assert ws(1, 1, 1, 7) > 0 and ws(2, 63, 95, 7) > ws(1, 63, 95, 7) and ws(1, 128, 96, 7) > ws(1, 64, 96, 7)
    assert ws(3, 512, 640, 3) < ws(3, 512, 640, 7) and ws(3, 512, 640, 1) < ws(3, 512, 640, 3) and ws(3, 64, 96, 7, c=16) > ws(3, 64, 96, 7)
    # channel-last intermediates: conv0.0 / conv0 (8 ch), conv1.0 / conv1 (16 ch at half), conv2.0 / conv2 (32 ch at quarter); I1 (32 ch
    # at half) for levels 1 and 2; level 2 adds I2 (32 ch at full) and conv0.0's output moves into it
    r64 = lambda f: (f + 63) // 64 * 64
    N, H, W, h, w, q, wq = 2, 63, 95, 32, 48, 16, 24
    assert ws(N, H, W, 1) == 4 * (2 * r64(N * H * W * 8) + 2 * r64(N * h * w * 16) + 2 * r64(N * q * wq * 32))
    assert ws(N, H, W, 7) == 4 * (r64(N * H * W * 8) + 2 * r64(N * h * w * 16) + 2 * r64(N * q * wq * 32) + r64(N * h * w * 32) + r64(N * H * W * 32))
    need = ws(N, H, W, 7)
    fake = 4096   # not device memory: a launch would fail, a refusal never gets there
    call = lambda c=8, mask=7, wsb=need, l0=fake, l1=fake, l2=fake, img=fake, H=H: lib.gdb_fpn(
        c, 32, 16, 8, img, N, H, W, fake, mask, fake, wsb, l0, l1, l2, None)
    assert call(c=12) == _lib.GDB_E_BADARG
    assert call(l2=None) == _lib.GDB_E_BADARG and b"level 2" in lib.gdb_last_error()
    assert call(l1=None) == _lib.GDB_E_BADARG and call(l0=None) == _lib.GDB_E_BADARG
    assert call(mask=0) == _lib.GDB_E_BADARG
    assert call(H=0) == _lib.GDB_E_SHAPE
    assert call(img=None) == _lib.GDB_E_BADARG
    assert call(wsb=need - 4) == _lib.GDB_E_WORKSPACE and b"workspace" in lib.gdb_last_error()


def test_switch_plumbing(monkeypatch):
    """fpn.hip_feature_net is read from the config (default off); the PyTorch module runs whenever the switch is off, the tensor is on
    the CPU or the net is in training mode, and FeaturePyramid only when all three allow it.  Network asks for the levels it reads."""
    assert make_network(make_cfg("configs/dtu_eval.yaml")).feature_net.hip is False
    cfg = make_cfg("configs/dtu_eval.yaml", ["fpn.hip_feature_net", "True"])
    assert cfg.fpn.hip_feature_net is True
    net = make_network(cfg).eval()
    f = net.feature_net
    assert f.hip is True
    cuda_like = type("T", (), {"is_cuda": True, "dtype": torch.float32})()
    assert f.use_hip(cuda_like) and not f.use_hip(torch.zeros(1))
    f.train()
    assert not f.use_hip(cuda_like)
    f.eval()
    f.hip = False
    assert not f.use_hip(cuda_like)
    assert not make_network(make_cfg("configs/dtu_eval.yaml")).eval().feature_net.use_hip(cuda_like)

    calls = {"module": 0, "hip": []}
    monkeypatch.setattr(fpn.FeaturePyramid, "__call__", lambda self, x, levels=(0, 1, 2): (calls["hip"].append(tuple(levels)), [None] * 3)[1])
    orig = f.conv0.forward
    def conv0(x):
        calls["module"] += 1
        return orig(x)
    monkeypatch.setattr(f.conv0, "forward", conv0)
    x = torch.rand(2, 3, 16, 24)
    for switch, train in ((True, False), (False, False), (True, True)):
        f.hip = switch
        f.train(train)
        calls.update(module=0, hip=[])
        with torch.no_grad():
            out = f(x, levels=(0,))
        assert calls == {"module": 1, "hip": []} and all(o is not None for o in out), (switch, train)   # levels ignored: all three
    # a CUDA-like input in eval mode with the switch on takes FeaturePyramid and not the module
    f.eval(); f.hip = True
    calls.update(module=0, hip=[])
    monkeypatch.setattr(f, "use_hip", lambda x: True)
    assert f(x, levels={1, 0}) == [None] * 3 and f(x) == [None] * 3
    assert calls == {"module": 0, "hip": [(0, 1), (0, 1, 2)]}

    # Network.forward asks for set(vol_levels) | {feat_level}: {0, 1} under dtu_eval.yaml, {0} under F7d's opts (bundle_size 4)
    assert net.fpn_levels == (0, 1)
    f7d = make_network(make_cfg("configs/dtu_eval.yaml", [str(x) for x in load_golden("F7d_network_bundle4")["opts"]] + ["fpn.hip_feature_net", "True"]))
    assert f7d.fpn_levels == (0,)
    seen = []
    f7 = load_golden("F7_network")
    t = lambda k: torch.from_numpy(f7[k])
    batch = {"src_views": {"rgb": t("src_images").float(), "extrinsics": t("src_exts"), "intrinsics": t("src_ints")},
             "tar_views": {"extrinsics": t("tar_ext"), "intrinsics": t("tar_int")}, "near_far": t("near_far")}
    class Stop(Exception):
        pass

    def spy(x, levels=None):
        seen.append(levels)
        raise Stop   # the rest of the forward needs the GPU
    plain = make_network(make_cfg("configs/dtu_eval.yaml")).eval()
    monkeypatch.setattr(plain.feature_net, "forward", spy)
    with pytest.raises(Stop), torch.no_grad():
        plain(batch)
    assert seen == [(0, 1)]


def test_network_refuses_a_feature_net_the_library_is_not_built_for():
    with pytest.raises(ValueError, match="base_channels 12"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["fpn.hip_feature_net", "True", "fpn.base_channels", "12"]))
    with pytest.raises(ValueError, match="at most 64"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["fpn.hip_feature_net", "True", "fpn.feat_dims", "[128, 16, 8]"]))
    make_network(make_cfg("configs/dtu_eval.yaml", ["fpn.base_channels", "12"]))   # the switch off: the module, as before


def test_feature_pyramid_refuses_mixed_eps():
    m = _fpn()
    m.conv1[0][1].eps = 1e-3
    with pytest.raises(ValueError, match="eps"):
        fpn.FeaturePyramid(m)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _err(got, ref):
    scale = max(1.0, float(ref.abs().max()))
    return float((got.double() - ref.double()).abs().max()) / scale


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", [(2, 64, 96), (5, 64, 96), (2, 63, 95), (5, 63, 95), (2, 512, 640), (5, 512, 640), (2, 1200, 1600),
                                   (5, 1200, 1600)])
def test_hip_fpn_matches_module(N, H, W):
    """Every level each mask produces against the module: float64 on the CPU up to 512 x 640 at N = 2 (bound 5e-6 of max(1, max |ref|)),
    fp32 on the GPU at every size (1e-5).  Observed on MI355X: <= 3.8e-7 against float64, <= 5.0e-7 against the fp32 module (level 2 at
    1200 x 1600; levels 0 / 1 <= 9e-8 / 2.9e-7)."""
    m = _fpn(seed=H + W)
    torch.manual_seed(N)
    x = torch.rand(N, 3, H, W) * 2.0 - 0.5
    refs64 = None
    if N == 2 and H * W <= 512 * 640:
        with torch.no_grad():
            refs64 = m.double()(x.double())
        m.float()
    m = m.cuda()
    xc = x.cuda()
    with torch.no_grad():
        refs32 = m(xc)
    pyr = fpn.FeaturePyramid(m)
    for levels, mask in MASKS.items():
        with torch.no_grad():
            outs = pyr(xc, levels)
        torch.cuda.synchronize()
        for l in range(3):
            if l not in levels:
                assert outs[l] is None
                continue
            assert outs[l].shape == refs32[l].shape, (levels, l)
            e32 = _err(outs[l], refs32[l])
            msg = f"fpn N={N} {H}x{W} mask {mask} level {l}: vs fp32 module {e32:.2e}"
            if refs64 is not None:
                e64 = _err(outs[l].cpu(), refs64[l])
                msg += f", vs float64 module {e64:.2e}"
                assert e64 <= 5e-6, msg
            print(msg)
            assert e32 <= 1e-5, msg


def _state_dict(fx):
    return {k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in fx.items() if k.startswith("sd.")}


@pytest.mark.gpu
def test_f7_feat_l1_through_hip_fpn():
    """F7's feat_l1 (the reference FPN's own level 1 on F7's source images) through FeaturePyramid with F7's weights: the CPU bound of
    test_network_surface.py."""
    f7 = load_golden("F7_network")
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["fpn.hip_feature_net", "True"])).eval()
    net.load_state_dict(_state_dict(f7), strict=True)
    net = net.cuda()
    src = torch.from_numpy(f7["src_images"]).float().cuda().flatten(0, 1)
    with torch.no_grad():
        out = net.feature_net(src, levels=(1,))
    assert out[0] is None and out[2] is None
    e = max_abs(out[1].cpu().numpy(), f7["feat_l1"])
    print(f"F7 feat_l1 through the HIP FPN: max abs err {e:.3e}")
    assert e <= 1e-5


def _run_network(fx, sd_fx, opts):
    net = make_network(make_cfg(str(fx["yaml"]) if "yaml" in fx else "configs/dtu_eval.yaml", opts)).eval()
    net.load_state_dict(_state_dict(sd_fx), strict=True)
    net = net.cuda()
    fxb = dict(fx); fxb["src_images"] = fx["src_images"].astype(np.float32)
    tt = lambda k: torch.from_numpy(fxb[k]).cuda()
    batch = {"src_views": {"rgb": tt("src_images"), "extrinsics": tt("src_exts"), "intrinsics": tt("src_ints")},
             "tar_views": {"extrinsics": tt("tar_ext"), "intrinsics": tt("tar_int")}, "near_far": tt("near_far")}
    if "render_scale" in fx and float(fx["render_scale"]) != 1.0:
        batch["render_scale"] = torch.tensor([float(fx["render_scale"])], device="cuda")
    calls = []
    orig = fpn.FeaturePyramid.__call__
    fpn.FeaturePyramid.__call__ = lambda self, x, levels=(0, 1, 2): (calls.append(tuple(levels)), orig(self, x, levels))[1]
    try:
        with torch.no_grad():
            ret, _, _ = net(batch)
    finally:
        fpn.FeaturePyramid.__call__ = orig
    assert calls == [net.fpn_levels]
    return ret


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,cost_reg", [("F7_network", False), ("F7b_network_nerf_eval", False), ("F7c_network_render_scale", False),
                                              ("F7d_network_bundle4", False), ("F7_network", True)])
def test_network_forward_with_hip_fpn_matches_reference(fixture, cost_reg):
    """Whole Network.forward with fpn.hip_feature_net (and mvs.hip_cost_reg) against F7 / F7b / F7c / F7d, the bounds of
    test_network_forward_with_hip_cost_reg_matches_reference."""
    f7 = load_golden("F7_network")
    fx = f7 if fixture == "F7_network" else load_golden(fixture)
    opts = ["fpn.hip_feature_net", "True", "mvs.hip_cost_reg", str(cost_reg)]
    if fixture == "F7d_network_bundle4":
        ret = _run_network(fx, fx, [str(x) for x in fx["opts"]] + opts)
    else:
        ret = _run_network(fx, f7, opts)
    e = max_abs(ret["rgb"].cpu().numpy(), fx["rgb"])
    print(f"{fixture} with the HIP FPN{' and U-Nets' if cost_reg else ''}: max |rgb - reference| = {e:.3e}")
    assert e <= 5e-4
    assert max_abs(ret["mvs_depth"].cpu().numpy(), fx["mvs_depth"]) <= 1e-3 * float(np.abs(fx["mvs_depth"]).max())
    H, W = fx["rgb"].shape[2:]
    gt = np.clip(np.transpose(fx["rgb"][0], (1, 2, 0)) + np.random.default_rng(1).normal(0, 0.03, (H, W, 3)), 0, 1)
    d_psnr = abs(oracle.psnr(gt, np.transpose(ret["rgb"][0].cpu().numpy(), (1, 2, 0))) - oracle.psnr(gt, np.transpose(fx["rgb"][0], (1, 2, 0))))
    assert d_psnr <= 0.05


@pytest.mark.gpu
def test_hip_fpn_is_deterministic_and_ignores_the_workspace():
    m = _fpn(seed=3).cuda()
    x = torch.rand(2, 3, 63, 95, device="cuda")
    pyr = fpn.FeaturePyramid(m)
    a = pyr(x)
    b = pyr(x)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.gdb_fpn_workspace_bytes(*pyr.channels, 2, 63, 95, 7, C.byref(n)))
    ws = torch.full(((n.value + 3) // 4,), float("nan"), device="cuda")
    outs = [torch.full_like(t, float("nan")) for t in a]
    _lib.check(lib.gdb_fpn(*pyr.channels, x.data_ptr(), 2, 63, 95, pyr.pack(x.device).data_ptr(), 7, ws.data_ptr(), n.value,
                           outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, outs))


@pytest.mark.gpu
def test_hip_fpn_follows_new_weights_and_buffers():
    """`p.data = ...`, an in-place change to a running_var buffer and load_state_dict all reach the next forward."""
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["fpn.hip_feature_net", "True"])).eval().cuda()
    f = net.feature_net
    x = torch.rand(3, 3, 64, 96, device="cuda")

    def check(prev):
        with torch.no_grad():
            got = f(x)
            f.hip = False
            ref = f(x)
            f.hip = True
        assert prev is None or not torch.equal(prev[2], got[2])
        for g, r in zip(got, ref):
            assert _err(g, r) <= 1e-5
        return got

    o = check(None)
    f.out2.weight.data = torch.randn_like(f.out2.weight) * 0.1
    o = check(o)
    with torch.no_grad():
        f.conv0[1][1].running_var.mul_(3.0)
    o = check(o)
    f.load_state_dict(_fpn(seed=11).state_dict())
    check(o)

"""The cascade's cost-regularisation 3-D U-Nets (networks/gdb_nerf/cost_reg_net.py:24-54) on the HIP library: gdb_cost_reg and
friends (include/gdb_nerf_hip.h), costvol.CostReg and the `mvs.hip_cost_reg` switch of DepthNet.  CPU: the packed layout, the
refusals and the switch's plumbing against the built library.  GPU: the PyTorch module, fixture F7 and the whole network."""
import ctypes as C

import numpy as np
import pytest
import torch

import gdb_oracle as oracle
from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, costvol
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d


def _unet(cin, c, cout, depth, seed=0):
    """A U-Net with random weights and non-trivial BN statistics (as tests/golden/make_golden_network.py:36-41)."""
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


def _layers(depth, cin, c, cout):
    """The packed layout of include/gdb_nerf_hip.h restated: per layer (name, kind, cin, rows, T, E, nc, w_off, ep_off, cout)."""
    spec = [("conv0", "s1", cin, c)]
    n = 1
    for lvl in range(depth):
        spec += [(f"conv{n}", "s2", c << lvl, c << (lvl + 1)), (f"conv{n + 1}", "s1", c << (lvl + 1), c << (lvl + 1))]
        n += 2
    for lvl in reversed(range(depth)):
        spec.append((f"conv{n}", "up", c << (lvl + 1), c << lvl))
        n += 1
    spec.append(("heads", "heads", c, cout))
    out, o = [], 0
    for i, (name, kind, ci, co) in enumerate(spec):
        nc = i == 0
        zs = 2 if (kind == "s1" and co == 8) else 1
        T = 36 if zs == 2 else 27
        E = 4 if (nc or ci % 16 == 0) else 2
        K = (ci + 15) // 16 if nc else ci // (4 * E)
        rows = co + 1 if kind == "heads" else zs * co
        nmt = (rows + 15) // 16
        w_off = o
        o += nmt * T * K * 64 * E
        ep_off = o
        o += 0 if kind == "heads" else 4 * co
        o = (o + 63) // 64 * 64
        out.append(dict(name=name, kind=kind, cin=ci, cout=co, rows=rows, T=T, E=E, K=K, nc=nc, zs=zs, w_off=w_off, ep_off=ep_off))
    return out, o


def _pack(m, depth, cin, c, cout):
    lib = _lib.load()
    sd = m.state_dict()
    arrs = [np.ascontiguousarray(sd[k].numpy(), dtype=np.float32) for k in costvol.cost_reg_keys(depth)] + [np.array([1e-5], np.float32)]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    n = C.c_size_t()
    _lib.check(lib.gdb_cost_reg_packed_floats(depth, cin, c, cout, C.byref(n)))
    host = np.full(n.value, np.nan, np.float32)
    _lib.check(lib.gdb_pack_cost_reg_weights(depth, cin, c, cout, ptrs, host.ctypes.data))
    return host, n.value


@pytest.mark.parametrize("depth,cin,c,cout", [(2, 32, 8, 8), (3, 16, 8, 8), (3, 16, 16, 4)])
def test_packed_layout_round_trip(depth, cin, c, cout):
    m = _unet(cin, c, cout, depth)
    host, n = _pack(m, depth, cin, c, cout)
    layers, total = _layers(depth, cin, c, cout)
    assert n == total and np.isfinite(host).all()     # packed_floats agrees with what the packer writes (every float written)
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(depth + cin + c)
    for L in layers:
        for _ in range(200):
            mt = int(rng.integers(0, (L["rows"] + 15) // 16)); tap = int(rng.integers(0, L["T"])); cc = int(rng.integers(0, L["K"]))
            lane = int(rng.integers(0, 64)); e = int(rng.integers(0, L["E"]))
            got = host[L["w_off"] + (((mt * L["T"] + tap) * L["K"] + cc) * 64 + lane) * L["E"] + e]
            row, kq = 16 * mt + (lane & 15), lane >> 4
            ci = 16 * cc + 4 * e + kq if L["nc"] else 4 * L["E"] * cc + L["E"] * kq + e
            if ci >= L["cin"] or row >= L["rows"]:
                want = 0.0
            elif L["kind"] == "heads":
                want = sd["feat_head.weight"][row, ci].reshape(-1)[tap] if row < cout else sd["prob_head.weight"][0, ci].reshape(-1)[tap]
            elif L["zs"] == 2:
                s, co, kz = row // L["cout"], row % L["cout"], tap // 9 - row // L["cout"]
                want = sd[L["name"] + ".0.weight"][co, ci, kz].reshape(-1)[tap % 9] if 0 <= kz <= 2 else 0.0
            elif L["kind"] == "up":   # ConvTranspose3d weights are (cin, cout, 3, 3, 3)
                want = sd[L["name"] + ".0.weight"][ci, row].reshape(-1)[tap]
            else:
                want = sd[L["name"] + ".0.weight"][row, ci].reshape(-1)[tap]
            assert got == np.float32(want), (L["name"], mt, tap, cc, lane, e)
        if L["kind"] != "heads":
            co = L["cout"]
            ep = host[L["ep_off"]:L["ep_off"] + 4 * co].reshape(4, co)
            p = L["name"] + ".1."
            assert np.array_equal(ep[0], (1.0 / np.sqrt(sd[p + "running_var"] + np.float32(1e-5))).astype(np.float32))
            assert np.array_equal(ep[1], sd[p + "running_mean"]) and np.array_equal(ep[2], sd[p + "weight"]) and np.array_equal(ep[3], sd[p + "bias"])


def test_refusals_come_before_any_launch():
    """Bad depth / channels, a volume not divisible by 2^depth and a short workspace are refused with a status and a message; the
    device pointers are never touched (they are not even device memory here)."""
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.gdb_cost_reg_packed_floats(4, 16, 8, 8, C.byref(n)) == _lib.GDB_E_BADARG
    assert b"depth" in lib.gdb_last_error()
    assert lib.gdb_cost_reg_packed_floats(3, 12, 8, 8, C.byref(n)) == _lib.GDB_E_BADARG
    assert lib.gdb_cost_reg_packed_floats(3, 16, 8, 16, C.byref(n)) == _lib.GDB_E_BADARG
    assert lib.gdb_cost_reg_workspace_bytes(3, 16, 8, 8, 1, 8, 32, 44, C.byref(n)) == _lib.GDB_E_SHAPE
    assert b"2^depth" in lib.gdb_last_error()
    assert lib.gdb_cost_reg_workspace_bytes(2, 32, 8, 8, 1, 62, 8, 12, C.byref(n)) == _lib.GDB_E_SHAPE
    assert lib.gdb_cost_reg_workspace_bytes(2, 32, 8, 8, 1, 64, 8, 12, C.byref(n)) == _lib.GDB_OK
    need = n.value
    assert need == 4 * (64 * 8 * 12 * 8 + 2 * 32 * 4 * 6 * 16 + 2 * 16 * 2 * 3 * 32)
    fake = 4096   # not device memory: a launch would fail, a refusal never gets there
    assert lib.gdb_cost_reg(5, 32, 8, 8, fake, 1, 64, 8, 12, fake, fake, need, fake, fake, None) == _lib.GDB_E_BADARG
    assert lib.gdb_cost_reg(2, 32, 8, 8, fake, 1, 64, 8, 10, fake, fake, need, fake, fake, None) == _lib.GDB_E_SHAPE
    assert lib.gdb_cost_reg(2, 32, 8, 8, fake, 1, 64, 8, 12, fake, fake, need - 4, fake, fake, None) == _lib.GDB_E_WORKSPACE
    assert b"workspace" in lib.gdb_last_error()
    assert lib.gdb_cost_reg(2, 32, 8, 8, None, 1, 64, 8, 12, fake, fake, need, fake, fake, None) == _lib.GDB_E_BADARG


def test_depth_net_switch_plumbing(monkeypatch):
    """mvs.hip_cost_reg is read from the config (default off); the PyTorch module runs whenever the switch is off, the tensors are
    on the CPU or the net is in training mode, and CostReg only when all three allow it."""
    assert make_network(make_cfg("configs/dtu_eval.yaml")).depth_net.hip_cost_reg is False
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["mvs.hip_cost_reg", "True"])).eval()
    d = net.depth_net
    assert d.hip_cost_reg is True
    cuda_like = type("T", (), {"is_cuda": True, "dtype": torch.float32})()
    assert d.use_hip_cost_reg(cuda_like) and not d.use_hip_cost_reg(torch.zeros(1))
    d.train()
    assert not d.use_hip_cost_reg(cuda_like)
    d.eval()
    d.hip_cost_reg = False
    assert not d.use_hip_cost_reg(cuda_like)
    assert not make_network(make_cfg("configs/dtu_eval.yaml")).eval().depth_net.use_hip_cost_reg(cuda_like)

    calls = {"module": 0, "hip": 0}
    class Spy(costvol.CostReg):
        def __call__(self, cost):
            calls["hip"] += 1
            return super().__call__(cost)
    monkeypatch.setattr(costvol, "CostReg", Spy)
    for reg in d.cost_regs:
        orig = reg.forward
        def fwd(x, _orig=orig):
            calls["module"] += 1
            return _orig(x)
        monkeypatch.setattr(reg, "forward", fwd)
    f7 = load_golden("F7_network")
    t = lambda k: torch.from_numpy(f7[k])
    src = t("src_images")
    with torch.no_grad():
        ms = [f.unflatten(0, (1, 3)) for f in net.feature_net(src.flatten(0, 1))]
        for switch, train in ((True, False), (False, False), (True, True)):
            d.hip_cost_reg = switch
            d.train(train)
            calls.update(module=0, hip=0)
            d(src, ms, t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("near_far"))   # CPU tensors
            assert calls == {"module": 2, "hip": 0}, (switch, train, calls)
    # on a CUDA-like input with the switch on in eval mode the HIP path is taken and the module is not called
    d.eval(); d.hip_cost_reg = True
    calls.update(module=0, hip=0)
    monkeypatch.setattr(Spy, "__call__", lambda self, cost: (calls.__setitem__("hip", calls["hip"] + 1), (None, None))[1])
    d._cost_reg(0, torch.zeros(1), cuda_like)
    assert calls == {"module": 0, "hip": 1}


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _check_vs_module(m, cost, tag):
    reg = costvol.CostReg(m)
    with torch.no_grad():
        v_ref, p_ref = m(cost)
        v, p = reg(cost)
    torch.cuda.synchronize()
    assert v.shape == v_ref.shape and p.shape == p_ref.shape
    ev = float((v - v_ref).abs().max()); ep = float((p - p_ref).abs().max())
    scale = max(1.0, float(v_ref.abs().max()))
    print(f"cost reg {tag}: volume max abs err {ev:.3e} (values up to {scale:.2f}), prob max abs err {ep:.3e}")
    assert ev <= 5e-6 * scale and ep <= 5e-7   # (issue bounds 2e-5 / 1e-6; observed <= 1.2e-6 / 1.1e-7 on MI355X)
    return reg, v, p


@pytest.mark.gpu
@pytest.mark.parametrize("depth,cin,D,H,W", [(2, 32, 64, 8, 12), (3, 16, 8, 32, 48), (2, 32, 64, 64, 80), (3, 16, 8, 256, 320)])
def test_hip_cost_reg_matches_module(depth, cin, D, H, W):
    """Both U-Nets at the F7 stage shapes and the c2 (512 x 640) stage shapes, B = 2, random weights and BN statistics."""
    m = _unet(cin, 8, 8, depth, seed=depth).cuda()
    torch.manual_seed(1)
    cost = torch.rand(2, cin, D, H, W, device="cuda") * 2.0
    _check_vs_module(m, cost, f"depth {depth} {cin}x{D}x{H}x{W}")


@pytest.mark.gpu
def test_hip_cost_reg_is_deterministic_and_ignores_the_workspace():
    m = _unet(16, 8, 8, 3, seed=5).cuda()
    cost = torch.rand(2, 16, 8, 32, 48, device="cuda")
    reg, v0, p0 = _check_vs_module(m, cost, "determinism")
    v1, p1 = reg(cost)
    assert torch.equal(v0, v1) and torch.equal(p0, p1)
    lib = _lib.load()
    n = C.c_size_t()
    _lib.check(lib.gdb_cost_reg_workspace_bytes(3, 16, 8, 8, 2, 8, 32, 48, C.byref(n)))
    ws = torch.full(((n.value + 3) // 4,), float("nan"), device="cuda")
    v2, p2 = torch.full_like(v0, float("nan")), torch.full_like(p0, float("nan"))
    _lib.check(lib.gdb_cost_reg(3, 16, 8, 8, cost.data_ptr(), 2, 8, 32, 48, reg.pack(cost.device).data_ptr(), ws.data_ptr(), n.value,
                                v2.data_ptr(), p2.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(v0, v2) and torch.equal(p0, p2)


@pytest.mark.gpu
def test_hip_cost_reg_follows_new_weights_and_buffers():
    """load_state_dict of new weights and an in-place change to a running_var buffer both reach the next forward."""
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["mvs.hip_cost_reg", "True"])).eval().cuda()
    d = net.depth_net
    m = d.cost_regs[1]
    cost = torch.rand(1, 16, 8, 32, 48, device="cuda")
    v0, _ = d._cost_reg(1, cost, cost)
    m.load_state_dict(_unet(16, 8, 8, 3, seed=7).state_dict())
    v1, p1 = d._cost_reg(1, cost, cost)
    with torch.no_grad():
        v_ref, p_ref = m(cost)
    assert not torch.equal(v0, v1) and float((v1 - v_ref).abs().max()) <= 5e-6 * max(1.0, float(v_ref.abs().max()))
    with torch.no_grad():
        m.conv2[1].running_var.mul_(3.0)
        v_ref, p_ref = m(cost)
    v2, p2 = d._cost_reg(1, cost, cost)
    assert not torch.equal(v1, v2)
    assert float((v2 - v_ref).abs().max()) <= 5e-6 * max(1.0, float(v_ref.abs().max())) and float((p2 - p_ref).abs().max()) <= 5e-7


def _state_dict(fx):
    return {k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in fx.items() if k.startswith("sd.")}


def _net(fx, yaml="configs/dtu_eval.yaml", **opts):
    flat = [x for kv in {"mvs.hip_cost_reg": True, **opts}.items() for x in (kv[0], str(kv[1]))]
    net = make_network(make_cfg(yaml, flat)).eval()
    net.load_state_dict(_state_dict(fx), strict=True)
    return net.cuda()


@pytest.mark.gpu
def test_depth_net_with_hip_cost_reg_matches_reference():
    """Fixture F7 (the reference's own DepthNet outputs) through DepthNet with mvs.hip_cost_reg, the bounds of
    test_cnns_match_reference_on_cpu."""
    f7 = load_golden("F7_network")
    net = _net(f7)
    t = lambda k: torch.from_numpy(f7[k]).cuda()
    calls = []
    orig = costvol.CostReg.__call__
    with torch.no_grad():
        costvol.CostReg.__call__ = lambda self, cost: (calls.append(1), orig(self, cost))[1]
        try:
            src = t("src_images")
            ms = [f.unflatten(0, (1, 3)) for f in net.feature_net(src.flatten(0, 1))]
            d, rng, vrng, vol, _ = net.depth_net(src, ms, t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("near_far"))
        finally:
            costvol.CostReg.__call__ = orig
    assert len(calls) == 2
    assert max_abs(d[0].cpu().numpy(), f7["mvs_depth0"]) <= 1e-3 * float(np.abs(f7["mvs_depth0"]).max())
    assert max_abs(rng[-1].cpu().numpy(), f7["depth_range"]) <= 1e-4 * float(np.abs(f7["depth_range"]).max())
    assert max_abs(vrng[-1].cpu().numpy(), f7["vol_range"]) <= 1e-4 * float(np.abs(f7["vol_range"]).max())
    e = max_abs(vol[-1].cpu().numpy(), f7["feat_volume"])
    print(f"F7 feat_volume through the HIP U-Nets: max abs err {e:.3e}")
    assert e <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["F7_network", "F7b_network_nerf_eval", "F7c_network_render_scale"])
def test_network_forward_with_hip_cost_reg_matches_reference(fixture):
    """Whole Network.forward with mvs.hip_cost_reg against F7 / F7b / F7c, the bounds of test_network_forward_matches_reference."""
    f7 = load_golden("F7_network")
    fx = f7 if fixture == "F7_network" else load_golden(fixture)
    net = _net(f7, str(fx["yaml"]) if "yaml" in fx else "configs/dtu_eval.yaml")
    fxb = dict(fx); fxb["src_images"] = fx["src_images"].astype(np.float32)
    tt = lambda k: torch.from_numpy(fxb[k]).cuda()
    batch = {"src_views": {"rgb": tt("src_images"), "extrinsics": tt("src_exts"), "intrinsics": tt("src_ints")},
             "tar_views": {"extrinsics": tt("tar_ext"), "intrinsics": tt("tar_int")}, "near_far": tt("near_far")}
    if "render_scale" in fx and float(fx["render_scale"]) != 1.0:
        batch["render_scale"] = torch.tensor([float(fx["render_scale"])], device="cuda")
    with torch.no_grad():
        ret, mvs_depths, blend = net(batch)
    e = max_abs(ret["rgb"].cpu().numpy(), fx["rgb"])
    print(f"{fixture} with the HIP U-Nets: max |rgb - reference| = {e:.3e}")
    assert e <= 5e-4
    assert max_abs(ret["mvs_depth"].cpu().numpy(), fx["mvs_depth"]) <= 1e-3 * float(np.abs(fx["mvs_depth"]).max())
    H, W = fx["rgb"].shape[2:]
    gt = np.clip(np.transpose(fx["rgb"][0], (1, 2, 0)) + np.random.default_rng(1).normal(0, 0.03, (H, W, 3)), 0, 1)
    d_psnr = abs(oracle.psnr(gt, np.transpose(ret["rgb"][0].cpu().numpy(), (1, 2, 0))) - oracle.psnr(gt, np.transpose(fx["rgb"][0], (1, 2, 0))))
    assert d_psnr <= 0.05

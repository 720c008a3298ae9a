"""The stage render's library surface without a GPU: the header, the export list and the build recipe; every refusal of the entries
(made on the host, before any launch: the pointers handed over here are never dereferenced); the pack -> unpack round trip of the 16
tensors; the build-time properties of gdb_stage_nerf.hip; the switches of the depth net."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gdb_nerf_amd import _lib, build
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks.gdb_nerf import depth_net as dn

ENTRIES = ("gdb_stage_nerf_packed_floats", "gdb_pack_stage_nerf_weights", "gdb_unpack_stage_nerf_grads", "gdb_stage_nerf_layout",
           "gdb_stage_nerf", "gdb_stage_nerf_backward")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_header_exports_and_build_recipe(lib):
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(gdb_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "train-time stage render" in hdr and "(ABI v7, added" in hdr[hdr.index("train-time stage render") - 200:hdr.index("train-time stage render") + 400]
    assert lib.gdb_abi_version() == 7 == _lib.ABI_VERSION   # additions only
    assert "gdb_stage_nerf.hip" in build.SOURCES and build.CONTRACT["gdb_stage_nerf.hip"] == "off"
    for untouched in ("gdb_mlp.hip", "gdb_backward.hip"):
        assert "gdb_stage" not in open(os.path.join(build.CSRC, untouched)).read()


def test_every_refusal_comes_before_a_launch(lib):
    n, out = C.c_size_t(), (C.c_size_t * 3)()
    ok = (32, 8, 64, 1)
    assert lib.gdb_stage_nerf_packed_floats(*ok, C.byref(n)) == _lib.GDB_OK and n.value % 64 == 0 and n.value >= 64 * 127 + 32 * 105
    assert lib.gdb_stage_nerf_packed_floats(*ok, None) == _lib.GDB_E_BADARG
    for net in ((24, 8, 64, 1), (0, 8, 64, 1), (32, 4, 64, 1), (32, 8, 32, 1), (32, 8, 64, 2)):
        assert lib.gdb_stage_nerf_packed_floats(*net, C.byref(n)) == _lib.GDB_E_BADARG, net
        assert lib.gdb_stage_nerf_layout(*net, 3, 8, 100, out) == _lib.GDB_E_BADARG, net
    for feat in (8, 16, 32):
        assert lib.gdb_stage_nerf_layout(feat, 8, 64, 1, 3, 8, 5120, out) == _lib.GDB_OK
        assert out[1] == 256 and out[2] == 2 and out[0] == 4 * 256 * [n2 for n2 in [C.c_size_t()] if not lib.gdb_stage_nerf_packed_floats(feat, 8, 64, 1, C.byref(n2))][0].value
    assert lib.gdb_stage_nerf_layout(*ok, 3, 8, 5120, None) == _lib.GDB_E_BADARG
    assert lib.gdb_stage_nerf_layout(*ok, 1, 8, 100, out) == _lib.GDB_E_SHAPE and "V=1" in lib.gdb_last_error().decode()   # as gdb_mlp_backward_layout
    for V, S, rays in ((9, 8, 100), (0, 8, 100), (3, 0, 100), (3, 17, 100), (3, 8, 0), (3, 8, -4), (3, 8, 2 ** 31 // 8), (8, 16, 10), (5, 13, 10)):
        assert lib.gdb_stage_nerf_layout(*ok, V, S, rays, out) == _lib.GDB_E_SHAPE, (V, S, rays)
    # rays per tile: whole rays, <= 16 samples, <= 64 (view, sample) rows with a view's block padded to four samples
    for V, S, rpt in ((3, 8, 2), (2, 3, 5), (8, 1, 8), (5, 8, 1), (2, 16, 1), (4, 16, 1), (8, 8, 1), (2, 1, 16), (3, 5, 3), (6, 5, 1)):
        assert lib.gdb_stage_nerf_layout(*ok, V, S, 10 ** 6, out) == _lib.GDB_OK and out[2] == rpt and out[1] == 256, (V, S, out[2])
    assert lib.gdb_stage_nerf_layout(*ok, 3, 8, 7, out) == _lib.GDB_OK and out[1] == 4        # four tiles, four workgroups
    p = C.c_void_p(4096)
    fwd = lambda packed=p, vox=p, img=p, out_=p, V=3, S=8, rays=10, net=ok: lib.gdb_stage_nerf(*net, packed, V, S, vox, img, rays, out_, None, None, None)
    assert fwd(packed=None) == fwd(vox=None) == fwd(img=None) == fwd(out_=None) == _lib.GDB_E_BADARG
    assert fwd(V=1) == fwd(S=17) == fwd(rays=0) == fwd(V=8, S=16) == _lib.GDB_E_SHAPE and fwd(net=(24, 8, 64, 1)) == _lib.GDB_E_BADARG
    bwd = lambda packed=p, g=p, gp=p, ws=p, nbytes=1 << 30, V=3, S=8, rays=10: lib.gdb_stage_nerf_backward(*ok, packed, V, S, p, p, rays, g, gp, None, None, ws, nbytes, None)
    assert bwd(packed=None) == bwd(g=None) == bwd(gp=None) == bwd(ws=None) == _lib.GDB_E_BADARG
    assert bwd(V=1) == bwd(rays=0) == _lib.GDB_E_SHAPE
    assert lib.gdb_stage_nerf_layout(*ok, 3, 8, 10, out) == _lib.GDB_OK
    assert bwd(nbytes=out[0] - 1) == _lib.GDB_E_WORKSPACE and "workspace" in lib.gdb_last_error().decode()


@pytest.mark.parametrize("feat_dim,agg", [(32, True), (16, True), (8, False)])
def test_pack_unpack_round_trip(lib, feat_dim, agg):
    from gdb_nerf_amd import stage_nerf
    nerf = dn._AuxStageNerf(64, 8, feat_dim, agg)
    params = stage_nerf.stage_params(nerf)
    assert len(params) == 16 and (params[0] is None) == (not agg)
    holder = stage_nerf.StageNerf(nerf)
    host = [None if p is None else np.ascontiguousarray(p.detach().numpy()) for p in params]
    arr = (C.c_void_p * 16)(*[None if h is None else h.ctypes.data for h in host])
    packed = np.full(holder.floats, np.nan, dtype=np.float32)
    net = (feat_dim, 8, 64, int(agg))
    assert lib.gdb_pack_stage_nerf_weights(*net, arr, C.c_void_p(packed.ctypes.data)) == _lib.GDB_OK
    back = [None if h is None else np.full_like(h, np.nan) for h in host]
    arr2 = (C.c_void_p * 16)(*[None if b is None else b.ctypes.data for b in back])
    assert lib.gdb_unpack_stage_nerf_grads(*net, C.c_void_p(packed.ctypes.data), arr2) == _lib.GDB_OK
    used = np.zeros(holder.floats, dtype=bool)
    for h, b, o in zip(host, back, holder.offsets):
        if h is None:
            assert o is None
            continue
        assert np.array_equal(h, b) and o % 4 == 0 and not used[o:o + h.size].any()
        assert np.array_equal(packed[o:o + h.size], h.reshape(-1))
        used[o:o + h.size] = True
    assert np.all(packed[~used] == 0.0)       # pad slots, and view_fc's slots without viewdir_agg
    if not agg:
        assert holder.offsets[2] >= (feat_dim + 3) * 5 and not used[:holder.offsets[2]].any()
    if agg:   # a missing tensor is refused
        arr[5] = None
        assert lib.gdb_pack_stage_nerf_weights(*net, arr, C.c_void_p(packed.ctypes.data)) == _lib.GDB_E_BADARG
    assert lib.gdb_pack_stage_nerf_weights(*net, None, C.c_void_p(packed.ctypes.data)) == _lib.GDB_E_BADARG


def test_stage_kernels_use_no_private_memory_and_fit_the_lds(lib):
    path = os.path.join(build.CSRC, "obj", "resource_usage.json")
    if "gdb_stage_nerf.hip" not in json.load(open(path)):
        build.build(force=True)
    usage = json.load(open(path))["gdb_stage_nerf.hip"]
    kernels = [k for k in usage if "k_stage_nerf" in k]
    assert len(kernels) == 6 and any("k_stage_reduce" in k for k in usage)      # feat_dim 8 / 16 / 32, forward and backward
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0 and u["lds_bytes"] <= 160 * 1024, (name, u)


def test_the_switches_of_the_depth_net():
    cfg = lambda *o: make_cfg("configs/dtu_pretrain.yaml", list(o))
    assert dn.DepthNet(cfg()).hip_stage_render is False
    assert dn.DepthNet(cfg("mvs.hip_stage_render", "True")).hip_stage_render is True
    with pytest.raises(ValueError, match="stage_render"):
        dn.DepthNet(cfg("mvs.hip_stage_render", "True", "mvs.stage_render", "False"))
    with pytest.raises(ValueError, match="stage_render"):
        dn.DepthNet(make_cfg("configs/dtu_eval.yaml", ["mvs.hip_stage_render", "True"]))


def test_cpu_tensors_take_the_torch_path_under_the_hip_switch_and_the_entries_refuse_them():
    from gdb_nerf_amd import stage_nerf
    from test_stage_render import run_depth_net, tiny_frame
    t, feats = tiny_frame()
    on, off = dn.DepthNet(make_cfg("configs/dtu_pretrain.yaml", ["mvs.hip_stage_render", "True"])), dn.DepthNet(make_cfg("configs/dtu_pretrain.yaml"))
    off.load_state_dict(on.state_dict())
    on.train(), off.train()
    with torch.no_grad():
        assert torch.equal(run_depth_net(on, t, feats)[4][0], run_depth_net(off, t, feats)[4][0])
    assert on._hip_nerfs == {}
    holder = stage_nerf.StageNerf(on.nerfs[0])
    with pytest.raises(ValueError, match="CUDA"):
        holder.forward(torch.zeros(holder.floats), torch.zeros(8, 8), torch.zeros(8, 3, 39), 8)

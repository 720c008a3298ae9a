"""The backward entries' surface without a GPU: header and bindings agree, the gradient unpacker inverts the weight packer, the
layout call refuses what the kernel is not built for, the kernels keep out of private memory, and the autograd Functions are
entered only for CUDA tensors under grad mode."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from gdb_nerf_amd import _lib, build
from gdb_nerf_amd.engine import NERF_KEYS, HotPathEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gdb_mlp_backward_layout", "gdb_mlp_backward", "gdb_unpack_weight_grads", "gdb_render_weights_backward",
           "gdb_accumulate_backward")
SHAPES = {"view_fc.0": (19, 4), "global_fc.0": (32, 57), "agg_w_fc.0": (1, 32), "fc.0": (16, 32), "lr0.0": (64, 24),
          "sigma.0": (1, 64), "weight.0": (64, 111), "weight.2": (1, 64), "feat_head.0": (8, 64)}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _cfg(viewdir=True):
    return _lib.GdbConfig(2, 3, 1, 0, 64, 3, 16, 8, 64, int(viewdir))


def test_header_declares_the_backward_entries_and_bindings_match(lib):
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(gdb_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.gdb_abi_version() == 7   # additions only


@pytest.mark.parametrize("viewdir", [True, False])
def test_unpack_inverts_pack_bit_for_bit(lib, viewdir):
    rng = np.random.default_rng(7)
    cfg = _cfg(viewdir)
    tensors = []
    for key in NERF_KEYS:
        tensors += [rng.standard_normal(SHAPES[key]).astype(np.float32), rng.standard_normal(SHAPES[key][0]).astype(np.float32)]
    n = C.c_size_t()
    _lib.check(lib.gdb_packed_weight_floats(C.byref(cfg), C.byref(n)))
    packed = np.full(n.value, np.nan, np.float32)
    ptrs = (C.c_void_p * 18)(*[t.ctypes.data for t in tensors])
    if not viewdir:
        ptrs[0] = ptrs[1] = None
    _lib.check(lib.gdb_pack_weights(C.byref(cfg), ptrs, packed.ctypes.data))
    outs = [np.full_like(t, np.nan) for t in tensors]
    optrs = (C.c_void_p * 18)(*[t.ctypes.data for t in outs])
    if not viewdir:
        optrs[0] = optrs[1] = None
    _lib.check(lib.gdb_unpack_weight_grads(C.byref(cfg), packed.ctypes.data, optrs))
    for i, (a, b) in enumerate(zip(tensors, outs)):
        if i < 2 and not viewdir:
            continue
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), i
    # the Python view of the same layout (what the autograd Function slices on the device)
    slices, n_fp32 = HotPathEngine.packed_grad_slices()
    assert n_fp32 <= n.value and len(slices) == 18
    for i, ((off, shp), a) in enumerate(zip(slices, tensors)):
        if i < 2 and not viewdir:
            assert not packed[off:off + a.size].any()   # view_fc's slots stay zero
            continue
        assert tuple(shp) == a.shape
        assert np.array_equal(packed[off:off + a.size].reshape(shp).view(np.uint32), a.view(np.uint32)), i


def test_layout_refuses_what_the_kernel_is_not_built_for(lib):
    cfg, out = _cfg(), (C.c_size_t * 3)()
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), 1, 100, out) == _lib.GDB_E_SHAPE
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), _lib.GDB_MAX_VIEWS + 1, 100, out) == _lib.GDB_E_SHAPE
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), 3, 0, out) == _lib.GDB_E_SHAPE
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), 3, 100, None) == _lib.GDB_E_BADARG
    for V in (2, _lib.GDB_MAX_VIEWS):
        assert lib.gdb_mlp_backward_layout(C.byref(cfg), V, 1, out) == _lib.GDB_OK
        assert (out[1], out[0]) == (1, 4 * HotPathEngine.packed_grad_slices()[1]) and out[2] >= 1
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), 3, 1 << 24, out) == _lib.GDB_OK
    parts, tile = out[1], out[2]
    assert lib.gdb_mlp_backward_layout(C.byref(cfg), 3, 2 * parts * tile + 1, out) == _lib.GDB_OK
    assert out[1] == parts and out[0] == 4 * HotPathEngine.packed_grad_slices()[1] * parts   # a persistent grid: one partial per workgroup


def test_backward_kernels_use_no_private_memory(lib):
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json")))["gdb_backward.hip"]
    names = " ".join(usage)
    for k in ("k_mlp_bwd", "k_mlp_bwd_reduce", "k_render_weights_bwd", "k_accumulate_bwd"):
        assert k in names, k
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0, (name, u)


class _Entered(Exception):
    pass


def _raise(*a, **k):
    raise _Entered()


def test_functions_are_not_entered_for_cpu_tensors_or_without_grad_mode(lib, monkeypatch):
    """Only CUDA tensors under grad mode take the autograd Functions; everything else is the call path of before (which, for CPU
    tensors, is the engine's own refusal)."""
    from gdb_nerf_amd.networks.gdb_nerf import nerf as nerf_mod, utils
    monkeypatch.setattr(nerf_mod.MLPFunction, "apply", _raise)
    monkeypatch.setattr(utils.RenderWeightsFunction, "apply", _raise)
    monkeypatch.setattr(utils.AccumulateFunction, "apply", _raise)
    m = nerf_mod.NeRF()
    vox, rfd = torch.zeros(4, 8, requires_grad=True), torch.zeros(3, 4, 35, requires_grad=True)
    sigma, feat = torch.zeros(4, requires_grad=True), torch.zeros(4, 31, requires_grad=True)
    idx, z = torch.zeros(4, dtype=torch.int64), torch.ones(4)
    calls = (lambda: m(vox, rfd), lambda: utils.render_weight_from_density(sigma, idx, 2),
             lambda: utils.accumulate_value_along_rays(feat, z, sigma, idx, 2))
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            for call in calls:
                with pytest.raises(Exception) as e:   # CPU tensors: the engine refuses them, as before
                    call()
                assert not isinstance(e.value, _Entered)
    # ... and the gate itself
    assert not utils._wants_grad(sigma)
    assert len(m._mlp_params()) == 18 and len(nerf_mod.NeRF(viewdir_agg=False)._mlp_params()) == 16

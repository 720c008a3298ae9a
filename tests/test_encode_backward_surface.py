"""The surface of the encode backward without a GPU: header, bindings and library agree on the two entries, the layout call refuses
what the kernels are not built for and reports the fixed-point rule F = min(40, 62 - ceil(log2(8 n_alloc))), the kernels keep out of
private memory, `EncodeFunction` is entered only with the switch on, under grad mode, for CUDA tensors that require grad, and
`nerf.encode_grad` without the operator mirrors is refused."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from gdb_nerf_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gdb_encode_backward_layout", "gdb_encode_backward")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _cfg(S=3):
    return _lib.GdbConfig(2, S, 1, 0, 64, 3, 16, 8, 64, 1)


def _shape(B=1, V=3, H=600, W=600, D=8):
    f = _lib.GdbFrame()
    f.B, f.V, f.Ho, f.Wo, f.H, f.W, f.D = B, V, 2 * H, 2 * W, H, W, D
    return f


def test_header_bindings_and_library_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(gdb_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.gdb_abi_version() == 7   # additions only
    assert "gdb_encode, the fused entries and the decoder have no backward" not in hdr


def _ceil_log2(x):
    return (x - 1).bit_length()


def test_layout_refusals_and_the_fixed_point_rule(lib):
    cfg, f, out = _cfg(), _shape(), (C.c_size_t * 4)()
    n_max = f.B * f.H * f.W * cfg.max_num_samples
    assert n_max >= 1 << 20
    for bad in (0, -1, n_max + 1):
        assert lib.gdb_encode_backward_layout(C.byref(cfg), C.byref(f), bad, out) == _lib.GDB_E_SHAPE
    assert lib.gdb_encode_backward_layout(C.byref(cfg), C.byref(f), 1, None) == _lib.GDB_E_BADARG
    expect = {1: 40, 1 << 20: 39, n_max: 62 - _ceil_log2(8 * n_max)}
    assert expect[n_max] == 38
    for n, F in expect.items():
        assert lib.gdb_encode_backward_layout(C.byref(cfg), C.byref(f), n, out) == _lib.GDB_OK
        assert out[1] == F == min(40, 62 - _ceil_log2(8 * n)), (n, out[1])
        assert (8 * n) << out[1] <= 1 << 62   # 8 n contributions of 2^F stay inside int64
    # the accumulators: int64, the pyramid's texels x 20 channels per (batch, view), the volume's voxels x C_v; 256-byte aligned regions
    lay = (C.c_size_t * 7)()
    assert lib.gdb_pyramid_layout(C.byref(cfg), C.byref(f), lay) == _lib.GDB_OK
    pyr, vol = 8 * lay[1] * f.B * f.V, 8 * f.B * f.D * f.H * f.W * 8
    assert out[2] % 256 == 0 and out[3] % 256 == 0 and out[3] >= out[2] + pyr and out[0] >= out[3] + vol
    # the entry itself: both outputs NULL is refused before anything is launched (no device needed to be told so)
    one = C.c_void_p(256)
    rc = lib.gdb_encode_backward(C.byref(cfg), C.byref(f), one, one, one, one, one, one, 1, one, one, None, None, one, out[0], None)
    assert rc == _lib.GDB_E_BADARG


def test_the_new_file_is_built_with_contraction_off_and_uses_no_private_memory(lib):
    assert "gdb_encode_backward.hip" in build.SOURCES and build.CONTRACT["gdb_encode_backward.hip"] == "off"
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json")))["gdb_encode_backward.hip"]
    names = " ".join(usage)
    for k in ("k_encbwd_max", "k_encbwd_vol", "k_encbwd_tex", "k_encbwd_fold_vol", "k_encbwd_fold_img"):
        assert k in names, k
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0, (name, u)


class _Entered(Exception):
    pass


def _raise(*a, **k):
    raise _Entered()


class _CudaLike:
    """Just enough of a tensor for `BundleSampler.encode` to reach its gate: claims to live on the GPU and to require grad."""
    is_cuda, requires_grad = True, True
    device = torch.device("cpu")

    def __init__(self, *shape):
        self.shape = shape

    def contiguous(self):
        return self

    float = detach = contiguous

    def to(self, *a, **k):
        return self

    __getitem__ = to


def _encode_args(make):
    B, V, H, W = 1, 3, 4, 6
    return (make(B, V, 3, 2 * H, 2 * W), make(B, V, 19, H, W), make(B, 8, 4, H, W), make(5, 3, 4), make(5, 3), make(5),
            make(B, V, 4, 4), make(B, V, 3, 3), make(B, 4, 4), torch.tensor([5]))


def test_encode_function_is_entered_only_behind_all_three_conditions(lib, monkeypatch):
    from gdb_nerf_amd.networks.gdb_nerf import bundle_sampler as bs
    monkeypatch.setattr(bs.EncodeFunction, "apply", _raise)
    cpu = lambda *shape: torch.zeros(*shape, requires_grad=True)
    cases = [("switch off", False, True, _CudaLike), ("grad mode off", True, False, _CudaLike), ("CPU tensors", True, True, cpu)]
    for what, switch, grad, make in cases:
        s = bs.BundleSampler(64, 3, encode_grad=switch)
        assert s.encode_grad is switch
        with torch.set_grad_enabled(grad):
            with pytest.raises(Exception) as e:   # today's calls: the engine refuses what is not a CUDA tensor
                s.encode(*_encode_args(make))
        assert not isinstance(e.value, _Entered), what
    assert bs.BundleSampler(64, 3).encode_grad is False   # the default
    # ... and the gate opens when all three hold (without this the cases above would pass with any gate)
    with torch.enable_grad(), pytest.raises(_Entered):
        bs.BundleSampler(64, 3, encode_grad=True).encode(*_encode_args(_CudaLike))


def test_encode_grad_without_the_operator_mirrors_is_refused(lib):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    with pytest.raises(ValueError, match="encode_grad"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.encode_grad", "True"]))
    with pytest.raises(ValueError, match="encode_grad"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.encode_grad", "True", "nerf.hot_path", "fused"]))
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.encode_grad", "True", "nerf.hot_path", "mirrors"]))
    assert net.encode_grad is True and net.sampler.encode_grad is True
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors"]))
    assert net.encode_grad is False and net.sampler.encode_grad is False

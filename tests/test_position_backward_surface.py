"""The surface of the position backward without a GPU: header, bindings and library agree on `gdb_encode_position_backward` and
`gdb_sample_backward` (ABI 7, additions only), both refuse bad arguments before any launch, the new translation unit is built with
contraction off and keeps out of private memory, `SampleFunction` / `EncodeFunction` are entered only with `position_grad` on, under
grad mode, for CUDA tensors that require grad, and `nerf.position_grad` without the operator mirrors is refused."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from gdb_nerf_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gdb_encode_position_backward", "gdb_sample_backward")
SRC = "gdb_position_backward.hip"


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _cfg(S=3):
    return _lib.GdbConfig(2, S, 1, 0, 64, 3, 16, 8, 64, 1)


def _frame(B=1, V=3, H=8, W=12, D=8, ptrs=True):
    f = _lib.GdbFrame()
    f.B, f.V, f.Ho, f.Wo, f.H, f.W, f.D = B, V, 2 * H, 2 * W, H, W, D
    if ptrs:   # never dereferenced: every call below is refused on the host
        for name, _ in _lib.GdbFrame._fields_[7:]:
            setattr(f, name, 256)
    return f


def test_header_bindings_and_library_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(gdb_\w+)\s*\(", hdr, flags=re.M))
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert declared == set(_lib.EXPORTS)
    assert lib.gdb_abi_version() == 7   # additions only
    # the comments that said so are corrected
    assert "gdb_sample, the\n * fused entries and the decoder have none" not in hdr
    assert "No gradient goes to d_rays_xyz" not in hdr
    assert "Columns 0 and 1 of d_g_uvd are written as zeros" in hdr


def test_encode_position_backward_refusals(lib):
    cfg, f, one = _cfg(), _frame(), C.c_void_p(256)
    n_max = f.B * f.H * f.W * cfg.max_num_samples
    call = lambda n, outs, pre=(one,) * 6, ups=(one, one), frame=f: lib.gdb_encode_position_backward(
        C.byref(cfg), C.byref(frame), *pre, n, *ups, *outs, None)
    assert call(1, (None, None, None)) == _lib.GDB_E_BADARG            # all three outputs NULL
    for bad in (0, -1, n_max + 1):                                      # gdb_encode's n_alloc refusals
        assert call(bad, (one, one, one)) == _lib.GDB_E_SHAPE
        assert call(bad, (None, one, None)) == _lib.GDB_E_SHAPE
    assert call(1, (one, one, one), pre=(None,) + (one,) * 5) == _lib.GDB_E_BADARG     # no workspace
    assert call(1, (one, one, one), ups=(None, one)) == _lib.GDB_E_BADARG              # no upstream
    assert call(1, (one, one, one), frame=_frame(ptrs=False)) == _lib.GDB_E_BADARG     # it reads the volume and the source images
    assert call(1, (one, one, one), frame=_frame(V=9)) == _lib.GDB_E_SHAPE


def test_sample_backward_refusals(lib):
    cfg, f, one = _cfg(), _frame(), C.c_void_p(256)
    n_max = f.B * f.H * f.W * cfg.max_num_samples
    call = lambda n, ups, outs, spb=one, scratch=one, frame=f: lib.gdb_sample_backward(
        C.byref(cfg), C.byref(frame), one, spb, one, n, *ups, *outs, scratch, None)
    all_up = (one,) * 4
    assert call(1, (None,) * 4, (one, one)) == _lib.GDB_E_BADARG        # all upstreams NULL
    assert call(1, all_up, (None, None)) == _lib.GDB_E_BADARG           # both outputs NULL
    for bad in (0, -1, n_max + 1):
        assert call(bad, all_up, (one, one)) == _lib.GDB_E_SHAPE
        assert call(bad, (None, one, None, None), (None, one)) == _lib.GDB_E_SHAPE
    assert call(1, all_up, (one, one), spb=None) == _lib.GDB_E_BADARG
    assert call(1, all_up, (one, one), scratch=None) == _lib.GDB_E_BADARG
    assert call(1, all_up, (one, one), frame=_frame(ptrs=False)) == _lib.GDB_E_BADARG   # it reads depth_range / vol_range


def test_the_new_file_is_built_with_contraction_off_and_uses_no_private_memory(lib):
    assert SRC in build.SOURCES and build.CONTRACT[SRC] == "off"
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json")))[SRC]
    names = " ".join(usage)
    for k in ("k_posbwd_vol", "k_posbwd_centre", "k_posbwd_colour", "k_smpbwd"):
        assert k in names, k
    assert len(usage) >= 4
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0, (name, u)


@pytest.mark.gpu
@pytest.mark.parametrize("Ho, Wo, scan_blocks", [(16, 24, 1), (64, 80, 2)])
def test_sample_backward_stays_inside_its_documented_scratch(lib, Ho, Wo, scan_blocks):
    """`gdb_sample_backward`'s scratch is documented as 4 * (B*H*W + ceil(B*H*W / 1024)) bytes: the offsets inside a scan block, then one
    offset per block - and no slot for the grand total `gdb_sample`'s own scan leaves behind its block offsets.  Called through ctypes
    with 8 sentinel words behind that size, it leaves them alone and returns the bits of `engine.sample_backward`; with two scan
    blocks the block offsets are read."""
    import numpy as np
    from conftest import FRAME_KEYS
    from gdb_nerf_amd import synthetic
    from gdb_nerf_amd.engine import HotPathEngine
    fr = synthetic.make_frame(Ho, Wo, V=2, B=1, bundle_size=2, scene="dtu", seed=11)
    eng = HotPathEngine(bundle_size=2)
    eng.prepare({k: torch.tensor(np.ascontiguousarray(fr[k]), dtype=torch.float32, device="cuda") for k in FRAME_KEYS})
    s = eng.sample()
    nb, n = eng.n_bundles, int(s["total"].item())
    assert nb == (Ho // 2) * (Wo // 2) and (nb + 1023) // 1024 == scan_blocks and n >= nb
    gen = torch.Generator().manual_seed(5)
    ups = [torch.randn(shape, generator=gen).cuda() for shape in ((n, 3, 4), (n, 3), (n,), (n,))]
    spb, total = s["samples_per_bundle"], s["total"]
    want = eng.sample_backward(spb, total, *ups)
    documented, sentinel = nb + (nb + 1023) // 1024, 0x5A5A5A5A
    scratch = torch.full((documented + 8,), sentinel, dtype=torch.int32, device="cuda")
    f = eng._need_frame()
    got = [torch.empty((f.B, 2, f.H, f.W), device="cuda") for _ in range(2)]
    _lib.check(eng.lib.gdb_sample_backward(C.byref(eng.cfg), C.byref(f), eng._ws.data_ptr(), spb.data_ptr(), total.data_ptr(), n,
                                           *(u.data_ptr() for u in ups), got[0].data_ptr(), got[1].data_ptr(), scratch.data_ptr(),
                                           eng._stream()))
    torch.cuda.synchronize()
    assert scratch[documented:].tolist() == [sentinel] * 8
    assert not (scratch[:documented] == sentinel).any()   # ... and the documented part was all written
    for g, w, name in zip(got, want, ("g_depth_range", "g_vol_range")):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), name
        assert g.abs().max() > 0, name


class _Entered(Exception):
    pass


def _raise(*a, **k):
    raise _Entered()


class _CudaLike:
    """Just enough of a tensor for `BundleSampler.sample` / `.encode` to reach their gates: claims to live on the GPU and to require
    grad (the pattern of test_encode_backward_surface.py)."""
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


class _CudaLikeFixed(_CudaLike):
    requires_grad = False


def _encode_args(make, make_pos):
    B, V, H, W = 1, 3, 4, 6
    return (make(B, V, 3, 2 * H, 2 * W), make(B, V, 19, H, W), make(B, 8, 4, H, W), make_pos(5, 3, 4), make_pos(5, 3), make_pos(5),
            make(B, V, 4, 4), make(B, V, 3, 3), make(B, 4, 4), torch.tensor([5]))


def test_encode_function_is_entered_for_positions_only_behind_all_three_conditions(lib, monkeypatch):
    from gdb_nerf_amd.networks.gdb_nerf import bundle_sampler as bs
    monkeypatch.setattr(bs.EncodeFunction, "apply", _raise)
    cpu = lambda *shape: torch.zeros(*shape, requires_grad=True)
    cases = [("switch off", False, True, _CudaLike), ("grad mode off", True, False, _CudaLike), ("CPU tensors", True, True, cpu),
             ("positions that do not require grad", True, True, _CudaLikeFixed)]
    for what, switch, grad, make in cases:
        s = bs.BundleSampler(64, 3, position_grad=switch)
        assert s.position_grad is switch and s.encode_grad is False
        with torch.set_grad_enabled(grad):
            with pytest.raises(Exception) as e:   # today's calls: the engine refuses what is not a CUDA tensor
                s.encode(*_encode_args(_CudaLike if make is _CudaLikeFixed else make, make))
        assert not isinstance(e.value, _Entered), what
    assert bs.BundleSampler(64, 3).position_grad is False   # the default
    # the gate opens when all three hold, on the positions alone: independent of encode_grad ...
    with torch.enable_grad(), pytest.raises(_Entered):
        bs.BundleSampler(64, 3, position_grad=True).encode(*_encode_args(_CudaLikeFixed, _CudaLike))
    # ... and encode_grad's own gate is what it was
    with torch.enable_grad(), pytest.raises(_Entered):
        bs.BundleSampler(64, 3, encode_grad=True).encode(*_encode_args(_CudaLike, _CudaLikeFixed))


def test_sample_function_is_entered_only_behind_all_three_conditions(lib, monkeypatch):
    from gdb_nerf_amd.networks.gdb_nerf import bundle_sampler as bs
    monkeypatch.setattr(bs.SampleFunction, "apply", _raise)
    cpu = lambda *shape: torch.zeros(*shape, requires_grad=True)

    def sampler(switch):
        s = bs.BundleSampler(64, 3, position_grad=switch)
        s.rays_o, s.H_orig, s.W_orig = object(), 8, 12   # as after build_rays()
        s._tar = {"tar_ext": torch.eye(4)[None], "tar_int": torch.eye(3)[None], "near_far": torch.ones(1, 2)}
        s._engine = lambda *a, **k: None
        return s

    cases = [("switch off", False, True, _CudaLike), ("grad mode off", True, False, _CudaLike), ("CPU tensors", True, True, cpu),
             ("ranges that do not require grad", True, True, _CudaLikeFixed)]
    for what, switch, grad, make in cases:
        with torch.set_grad_enabled(grad):
            with pytest.raises(Exception) as e:   # today's calls: there is no engine to prepare here
                sampler(switch).sample(make(1, 2, 4, 6), make(1, 2, 4, 6), 2, 3, False, True)
        assert not isinstance(e.value, _Entered), what
    for dr, vr in ((_CudaLike, _CudaLikeFixed), (_CudaLikeFixed, _CudaLike)):   # either range is enough
        with torch.enable_grad(), pytest.raises(_Entered):
            sampler(True).sample(dr(1, 2, 4, 6), vr(1, 2, 4, 6), 2, 3, False, True)


def test_accumulate_function_returns_the_z_vals_gradient():
    """g_z_vals = weights * g_depth_map[indices], formed in torch; the engine's call is stubbed."""
    from gdb_nerf_amd.networks.gdb_nerf import utils

    class Eng:
        def accumulate_backward(self, weights, feat, *a):
            return torch.zeros_like(weights), torch.zeros_like(feat)

    class Ctx:
        saved_tensors = (torch.tensor([0.5, 0.25, 1.0]), torch.zeros(3, 2), torch.ones(3), torch.tensor([0, 0, 2]))
        num_rays = 3

    old = dict(utils._ENGINES)
    utils._ENGINES[str(torch.device("cpu"))] = Eng()
    try:
        g_depth = torch.tensor([2.0, 3.0, 4.0])
        Ctx.needs_input_grad = (True, True, True, False, False)
        out = utils.AccumulateFunction.backward(Ctx, None, g_depth, None)
        assert torch.equal(out[2], torch.tensor([1.0, 0.5, 4.0])) and out[3] is None and out[4] is None
        Ctx.needs_input_grad = (True, True, False, False, False)
        assert utils.AccumulateFunction.backward(Ctx, None, g_depth, None)[2] is None
    finally:
        utils._ENGINES.clear()
        utils._ENGINES.update(old)


def test_position_grad_without_the_operator_mirrors_is_refused(lib):
    from gdb_nerf_amd.configs import make_cfg
    from gdb_nerf_amd.networks import make_network
    with pytest.raises(ValueError, match="position_grad"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.position_grad", "True"]))
    with pytest.raises(ValueError, match="position_grad"):
        make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.position_grad", "True", "nerf.hot_path", "fused"]))
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.position_grad", "True", "nerf.hot_path", "mirrors"]))
    assert net.position_grad is True and net.sampler.position_grad is True
    assert net.encode_grad is False and net.sampler.encode_grad is False   # independent switches
    net = make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors"]))
    assert net.position_grad is False and net.sampler.position_grad is False

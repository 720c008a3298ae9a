"""LPIPS-VGG from caller-supplied weights through the evaluator: `test.lpips_weights`, metrics.pack_lpips / eval_lpips /
lpips_weights_from and gdb_eval_lpips (include/gdb_nerf_hip.h).  The yardstick is the plain-torch restatement of
evaluators/gdb_nerf.py (`lpips_torch`, what the switch-off evaluator runs); tests/test_lpips_referee.py holds every layer to float64.
Weights are random and seeded here: agreement with the `lpips` package's published weights and values is unverified.

Bound of the evaluator comparison.  The device value and the restatement's are two fp32 realisations of one chain.  With E the
maximum, over 8 seeded frames of the shape and the frames of the test themselves, of |fp32 restatement - float64 restatement|, the
referee's rule holds the device value within K_RULE * E of float64 and the restatement is within E by construction:
|device - restatement| <= (K_RULE + 1) * E."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from gdb_nerf_amd import _lib, build, metrics
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.evaluators import make_evaluator
from gdb_nerf_amd.evaluators.gdb_nerf import lpips_torch
from test_hip_metrics import _batch, _images, _mask

K_RULE = 4.0
H, W = 40, 56


@functools.lru_cache(maxsize=None)
def _weights(seed=5):
    g = torch.Generator().manual_seed(seed)
    w = {}
    for i, (ci, co) in enumerate(metrics.LPIPS_CHANNELS):
        w[f"conv.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        w[f"conv.{i}.bias"] = torch.randn(co, generator=g) * 0.05
    for l, t in enumerate(metrics.LPIPS_TAPS):
        w[f"lin.{l}"] = torch.rand(metrics.LPIPS_CHANNELS[t][1], generator=g)
    return w


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lpips") / "lpips_vgg.pth")
    torch.save(_weights(), path)      # without shift / scale: the defaults
    return path


def _cfg(path, *opts):
    return make_cfg("configs/dtu_eval.yaml", ["eval_lpips", "True", "test.lpips_weights", path, *opts])


def _frames(center):
    """Two batches of B = 2 at 40 x 56: (gt, pred, mask, scenes); pred leaves [0, 1], the masks drop ~30 %."""
    out = []
    for i, scenes in enumerate((["scan1", "scan8"], ["scan8", "scan114"])):
        gt, pred = _images("noise" if i else "smooth", 2, H, W, 300 + i + 10 * center)
        out.append((gt, pred, _mask(2, H, W, True, 40 + i), scenes))
    return out


def _wired(gt, pred, mask, crop):
    """(a, b) (1,3,h,w) of one frame as the evaluator wires them: clamp, crop, zero outside the mask."""
    y0, x0, h, w = crop
    keep = torch.from_numpy(mask[y0:y0 + h, x0:x0 + w] >= 1)
    a = torch.from_numpy(pred).clamp(0.0, 1.0)[:, y0:y0 + h, x0:x0 + w] * keep
    b = torch.from_numpy(gt).permute(2, 0, 1)[:, y0:y0 + h, x0:x0 + w] * keep
    return a[None].contiguous(), b[None].contiguous()


def _e_ref(crop, frames):
    """max |fp32 restatement - float64 restatement| over 8 seeded frames of the cropped shape and the test's own frames."""
    w = metrics.lpips_weights_from(_weights())
    w64 = {k: v.double() for k, v in w.items()}
    pairs = []
    g = torch.Generator().manual_seed(77)
    for _ in range(8):
        pairs.append((torch.rand(1, 3, crop[2], crop[3], generator=g), torch.rand(1, 3, crop[2], crop[3], generator=g)))
    for gt, pred, mask, _ in frames:
        pairs += [_wired(gt[b], pred[b], mask[b], crop) for b in range(len(gt))]
    return max(float((lpips_torch(a, b, w).double() - lpips_torch(a.double(), b.double(), w64)).abs().max()) for a, b in pairs)


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_key_defaults_to_empty_and_the_constructor_loads_the_file_without_the_package(weights_file, tmp_path):
    assert make_cfg("configs/dtu_eval.yaml").test.lpips_weights == ""
    sys.modules.pop("lpips", None)
    ev = make_evaluator(_cfg(weights_file))
    assert "lpips" not in sys.modules and ev.loss_fn_vgg is None
    assert set(ev.lpips_weights) == set(metrics.lpips_weight_names())
    assert torch.equal(ev.lpips_weights["conv.7.weight"], _weights()["conv.7.weight"])
    assert ev.lpips_weights["shift"].tolist() == pytest.approx(metrics.LPIPS_SHIFT) and ev.lpips_weights["scale"].tolist() == pytest.approx(metrics.LPIPS_SCALE)
    # a path without the switch loads nothing
    off = make_evaluator(make_cfg("configs/dtu_eval.yaml", ["test.lpips_weights", weights_file]))
    assert off.lpips_weights is None and off.loss_fn_vgg is None
    # a missing or malformed file raises in the constructor
    with pytest.raises((FileNotFoundError, OSError)):
        make_evaluator(_cfg(str(tmp_path / "absent.pth")))
    bad = dict(_weights())
    del bad["lin.3"]
    torch.save(bad, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError, match="lin.3"):
        make_evaluator(_cfg(str(tmp_path / "bad.pth")))
    bad = dict(_weights(), **{"conv.4.weight": torch.zeros(256, 128, 1, 1)})
    torch.save(bad, str(tmp_path / "bad2.pth"))
    with pytest.raises(ValueError, match="conv.4.weight"):
        make_evaluator(_cfg(str(tmp_path / "bad2.pth")))


def test_without_the_path_the_switch_needs_the_package_as_before():
    try:
        import lpips  # noqa: F401
        pytest.skip("the lpips package is installed here")
    except ImportError:
        pass
    with pytest.raises(RuntimeError, match="lpips"):
        make_evaluator(make_cfg("configs/dtu_eval.yaml", ["eval_lpips", "True"]))


class _StandIn(torch.nn.Module):
    """LPIPS's structure under names of its own: a VGG-like feature stack (convolutions, ReLUs and pools in one Sequential, cut into
    slices), the tap convolutions registered twice - as attributes and in a ModuleList - behind dropout, and a scaling layer with
    `shift` / `scale` buffers."""

    def __init__(self, w):
        super().__init__()
        nn = torch.nn
        feats = []
        for i, (ci, co) in enumerate(metrics.LPIPS_CHANNELS):
            if i in (2, 4, 7, 10):
                feats.append(nn.MaxPool2d(2, 2))
            conv = nn.Conv2d(ci, co, 3, padding=1)
            conv.weight.data.copy_(w[f"conv.{i}.weight"]); conv.bias.data.copy_(w[f"conv.{i}.bias"])
            feats += [conv, nn.ReLU()]
        self.net = nn.Module()
        self.net.slice_all = nn.Sequential(*feats)
        self.scaling_layer = nn.Module()
        self.scaling_layer.register_buffer("shift", torch.tensor([-.03, -.09, -.19]).view(1, 3, 1, 1))
        self.scaling_layer.register_buffer("scale", torch.tensor([.46, .45, .44]).view(1, 3, 1, 1))
        lins = []
        for l, t in enumerate(metrics.LPIPS_TAPS):
            head = nn.Module()
            conv = nn.Conv2d(metrics.LPIPS_CHANNELS[t][1], 1, 1, bias=False)
            conv.weight.data.copy_(w[f"lin.{l}"].view(1, -1, 1, 1))
            head.model = nn.Sequential(nn.Dropout(), conv)
            setattr(self, f"head{l}", head)
            lins.append(head)
        self.heads = nn.ModuleList(lins)


def test_a_module_converts_by_structure_to_the_mapping_forms_tensors():
    w = _weights()
    shift, scale = torch.tensor([-.03, -.09, -.19]), torch.tensor([.46, .45, .44])
    from_map = metrics.lpips_weights_from(dict(w, shift=shift, scale=scale))
    from_mod = metrics.lpips_weights_from(_StandIn(w))
    assert list(from_map) == list(from_mod) == metrics.lpips_weight_names() and len(from_map) == _lib.LPIPS_TENSORS == 33
    for k in from_map:
        assert from_mod[k].dtype == torch.float32 and from_mod[k].is_contiguous() and torch.equal(from_map[k], from_mod[k]), k
    assert from_map["lin.2"].shape == (256,) and from_mod["shift"].shape == (3,)
    assert torch.equal(metrics.pack_lpips(from_map), metrics.pack_lpips(_StandIn(w)))
    broken = _StandIn(w)
    broken.net.slice_all = torch.nn.Sequential(*list(broken.net.slice_all)[2:])
    with pytest.raises(ValueError, match="13"):
        metrics.lpips_weights_from(broken)
    with pytest.raises(ValueError):
        metrics.lpips_weights_from([1, 2, 3])
    # the packer refuses a NULL tensor
    ts = [from_map[k] for k in metrics.lpips_weight_names()]
    ptrs = (C.c_void_p * 33)(*[t.data_ptr() for t in ts])
    ptrs[30] = None
    host = torch.empty(metrics.lpips_packed_floats())
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(_lib.load().gdb_pack_lpips_weights(ptrs, host.data_ptr()))


def test_cpu_tensors_take_the_torch_restatement_and_summarize_returns_lpips(weights_file, capsys):
    """CPU tensors take the numpy path whatever `test.hip_metrics` says; per frame the value is `lpips_torch` on the frame as wired."""
    w = metrics.lpips_weights_from(_weights())
    res = []
    for opts in ([], ["test.hip_metrics", "True"]):
        ev = make_evaluator(_cfg(weights_file, *opts))
        gt, pred = _images("noise", 2, 24, 32, 3)
        mask = _mask(2, 24, 32, True, 3)
        ev.evaluate({"rgb": torch.from_numpy(pred)}, _batch(gt, mask, ["scan1", "scan8"]))
        want = [float(lpips_torch(*_wired(gt[b], pred[b], mask[b], (0, 0, 24, 32)), w)[0]) for b in range(2)]
        assert ev.lpips == want and ev.scene["scan8"]["lpips"] == [want[1]]
        capsys.readouterr()
        r = ev.summarize()
        assert set(r) == {"psnr", "ssim", "lpips"} and r["lpips"] == np.mean(want) and "lpips:" in capsys.readouterr().out
        res.append(r)
    assert res[0] == res[1]


def test_the_source_is_built_with_contraction_off_and_its_kernels_use_no_private_memory():
    lib = build.build()
    so = C.CDLL(lib)
    names = ("gdb_lpips_packed_floats", "gdb_pack_lpips_weights", "gdb_lpips_workspace_bytes", "gdb_lpips_layout", "gdb_eval_lpips")
    for name in names:
        assert hasattr(so, name) and name in _lib.EXPORTS, name
    assert _lib.load().gdb_abi_version() == 7
    assert "gdb_lpips.hip" in build.SOURCES and build.CONTRACT["gdb_lpips.hip"] == "off"
    path = os.path.join(build.CSRC, "obj", "resource_usage.json")
    if not os.path.exists(path):
        build.build(force=True)
    usage = json.load(open(path))["gdb_lpips.hip"]
    assert sum("k_lpips_" in k for k in usage) >= 9, sorted(usage)      # scaled, conv0, conv, pool, four taps, finish
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0, (name, u)


def test_refusals_come_before_any_launch():
    """NULL pointers, unknown flags, a short workspace, a crop outside the image and a cropped extent below 16 are refused with a
    status and a message; the device pointers are never touched (they are not even device memory here)."""
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.gdb_lpips_packed_floats(None) == _lib.GDB_E_BADARG
    assert lib.gdb_lpips_workspace_bytes(1, 64, 96, 0, None) == _lib.GDB_E_BADARG
    for shape in ((0, 64, 96), (1, 15, 96), (1, 64, 15), (-1, 64, 96)):
        assert lib.gdb_lpips_workspace_bytes(*shape, 0, C.byref(n)) == _lib.GDB_E_SHAPE, shape
    assert lib.gdb_lpips_workspace_bytes(1, 64, 96, 2, C.byref(n)) == _lib.GDB_E_BADARG and b"flags" in lib.gdb_last_error()
    small, kept = metrics.lpips_workspace_bytes(2, 40, 56), metrics.lpips_workspace_bytes(2, 40, 56, metrics.LPIPS_KEEP)
    assert 2 * 4 * 4 * 40 * 56 * 64 <= small < kept           # two alternating buffers of the largest map, against every layer's own
    cnt = C.c_int32()
    assert lib.gdb_lpips_layout(2, 40, 56, 1, None, 0, C.byref(cnt)) == _lib.GDB_OK and cnt.value == 20 == _lib.LPIPS_REGIONS
    regs = (_lib.GdbDecRegion * 20)()
    assert lib.gdb_lpips_layout(2, 40, 56, 1, regs, 19, C.byref(cnt)) == _lib.GDB_E_BADARG
    assert list(metrics.lpips_layout(2, 40, 56)) == ["ping", "pong", "taps", "partials"]
    B, Hh, Ww = 2, 40, 56
    fake = 4096
    call = lambda pred=fake, gt=fake, mask=fake, B=B, H=Hh, W=Ww, crop=(0, 0, Hh, Ww), packed=fake, flags=0, wsp=fake, wsb=small, rec=fake, stride=16: \
        lib.gdb_eval_lpips(pred, gt, mask, B, H, W, *crop, packed, flags, wsp, wsb, rec, stride, None)
    for kw in ("pred", "gt", "mask", "packed", "wsp", "rec"):
        assert call(**{kw: None}) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error(), kw
    assert call(B=0) == _lib.GDB_E_SHAPE and call(H=0) == _lib.GDB_E_SHAPE and call(W=0) == _lib.GDB_E_SHAPE
    assert call(flags=4) == _lib.GDB_E_BADARG and call(stride=0) == _lib.GDB_E_BADARG
    assert call(crop=(1, 0, Hh, Ww)) == _lib.GDB_E_SHAPE and b"outside" in lib.gdb_last_error()
    assert call(crop=(0, -1, Hh, Ww)) == _lib.GDB_E_SHAPE and call(crop=(0, 10, Hh, Ww - 9)) == _lib.GDB_E_SHAPE
    assert call(crop=(0, 0, 15, Ww)) == _lib.GDB_E_SHAPE and b"fifth tap" in lib.gdb_last_error()
    assert call(crop=(4, 5, 32, 15)) == _lib.GDB_E_SHAPE and call(crop=(4, 5, 0, 0)) == _lib.GDB_E_SHAPE
    assert call(wsb=small - 8) == _lib.GDB_E_WORKSPACE and b"workspace" in lib.gdb_last_error()
    assert call(flags=1) == _lib.GDB_E_WORKSPACE and call(flags=1, wsb=kept - 8) == _lib.GDB_E_WORKSPACE
    assert call(crop=(4, 5, 32, 46), wsb=metrics.lpips_workspace_bytes(2, 32, 46) - 8) == _lib.GDB_E_WORKSPACE


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("center", [False, True])
def test_evaluator_lpips_matches_the_torch_restatement(center, weights_file, capsys):
    """`test.hip_metrics` with a weights file against the switch-off evaluator (CPU tensors: `lpips_torch`), B = 2 at 40 x 56, per frame
    and in summarize(), under the bound of the module docstring."""
    opts = ["test.eval_center", str(center)]
    off = make_evaluator(_cfg(weights_file, *opts))
    on = make_evaluator(_cfg(weights_file, *opts, "test.hip_metrics", "True"))
    frames = _frames(center)
    crop = (4, 5, 32, 46) if center else (0, 0, H, W)
    assert (int(H * 0.1), int(W * 0.1)) == (4, 5)
    bound = (K_RULE + 1.0) * _e_ref(crop, frames)
    for gt, pred, mask, scenes in frames:
        off.evaluate({"rgb": torch.from_numpy(pred)}, _batch(gt, mask, scenes))
        b = _batch(gt, mask, scenes, device="cuda")
        assert on.use_hip_metrics({"rgb": torch.from_numpy(pred).cuda()}, b)
        on.evaluate({"rgb": torch.from_numpy(pred).cuda()}, b)
    assert not on.lpips and len(off.lpips) == 4          # the device frames are still on the device
    want, scenes_off = list(off.lpips), {s: list(r["lpips"]) for s, r in off.scene.items()}
    capsys.readouterr()
    r_off = off.summarize()
    on.collect()
    got = list(on.lpips)
    for i, (g, w_) in enumerate(zip(got, want)):
        print(f"lpips frame {i} center {center}: device {g!r} restatement {w_!r} |d| {abs(g - w_):.3e} bound {bound:.3e}")
    assert len(got) == 4 and all(abs(g - w_) <= bound for g, w_ in zip(got, want)), (got, want, bound)
    assert all(0.0 < g < 5.0 for g in got)
    for s, vals in scenes_off.items():
        assert len(on.scene[s]["lpips"]) == len(vals) and all(abs(a - b) <= bound for a, b in zip(on.scene[s]["lpips"], vals)), s
    r_on = on.summarize()
    assert set(r_on) == set(r_off) == {"psnr", "ssim", "lpips"} and abs(r_on["lpips"] - r_off["lpips"]) <= bound
    assert abs(r_on["psnr"] - r_off["psnr"]) <= 1e-8 and abs(r_on["ssim"] - r_off["ssim"]) <= 1e-8      # the other two are untouched
    assert not on.lpips and not on.scene


@pytest.mark.gpu
def test_evaluate_with_lpips_makes_no_host_round_trip(weights_file):
    """Same form as test_hip_metrics.test_evaluate_makes_no_host_round_trip (a): under torch.cuda.set_sync_debug_mode("error") a warm
    `evaluate` with LPIPS on does not raise, while the switch-off evaluator's `.cpu()` does where this build honours the mode."""
    gt, pred = _images("noise", 2, H, W, 9)
    mask = _mask(2, H, W, True, 9)
    b = _batch(gt, mask, ["scan1", "scan8"], device="cuda")
    out = {"rgb": torch.from_numpy(pred).cuda()}
    on = make_evaluator(_cfg(weights_file, "test.hip_metrics", "True"))
    off = make_evaluator(_cfg(weights_file))
    on.evaluate(out, b)        # warm: library, the packed weights' upload, allocator blocks, the record table
    torch.cuda.synchronize()
    probe = torch.ones(4, device="cuda")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe[0].item()
            honoured = False
        except RuntimeError:
            honoured = True
        print("torch.cuda.set_sync_debug_mode('error') honoured on this build:", honoured)
        on.evaluate(out, b)    # must not raise either way
        if honoured:
            with pytest.raises(RuntimeError):
                off.evaluate(out, b)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    res = on.summarize()
    assert len(res) == 3 and np.isfinite(res["lpips"]) and res["lpips"] > 0


def _record(pred, gt, mask, packed, crop, flags, fill):
    B, Hh, Ww, _ = gt.shape
    nbytes = metrics.lpips_workspace_bytes(B, crop[2], crop[3], flags)
    ws = torch.full(((nbytes + 7) // 8,), fill, dtype=torch.float64, device="cuda")
    rec = torch.full((B, 3), fill, dtype=torch.float64, device="cuda")
    metrics.eval_lpips(pred, gt, mask, packed, rec[:, 1:], crop, flags=flags, workspace=ws)
    rec = rec.cpu().numpy()
    for col in (0, 2):       # the columns beside the record are not the call's to write
        assert np.array_equal(rec[:, col].view(np.int64), np.full(B, fill).view(np.int64))
    assert np.isfinite(rec[:, 1]).all()
    return rec[:, 1].copy().view(np.int64)


@pytest.mark.gpu
def test_records_are_bit_identical_across_runs_flags_and_batch_positions():
    packed = metrics.pack_lpips(_weights(), "cuda")
    gt, pred = _images("smooth", 2, H, W, 4)
    dg, dp, dm = (torch.from_numpy(a).cuda() for a in (gt, pred, _mask(2, H, W, True, 4)))
    crop = (3, 5, 33, 47)
    first = _record(dp, dg, dm, packed, crop, 0, 0.0)
    for flags, fill in ((0, float("nan")), (0, 1e300), (metrics.LPIPS_KEEP, 0.0), (metrics.LPIPS_KEEP, float("nan"))):
        assert np.array_equal(_record(dp, dg, dm, packed, crop, flags, fill), first), (flags, fill)
    assert first[0] != first[1]
    # one image at position 0 of B = 1 and at position 1 of B = 2
    alone = _record(dp[1:2].contiguous(), dg[1:2].contiguous(), dm[1:2].contiguous(), packed, crop, 0, float("nan"))
    assert alone[0] == first[1]
    with pytest.raises(ValueError, match="fifth tap"):
        metrics.eval_lpips(dp, dg, dm, packed, torch.zeros(2, 1, dtype=torch.float64, device="cuda"), (0, 0, 15, 40))

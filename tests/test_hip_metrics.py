"""The evaluator's metrics on the HIP library: gdb_eval_image / gdb_eval_depth (include/gdb_nerf_hip.h), metrics.py and the
`test.hip_metrics` switch of evaluators/gdb_nerf.py.  The yardstick everywhere is the numpy evaluator (`psnr`, `ssim`,
`_resize_bilinear`, `Evaluator` with the switch off).  CPU: the switch's plumbing, the refusals, the exports and the kernels'
resources.  GPU: records and summaries against numpy, no host round trip, determinism, the growing record table."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from gdb_nerf_amd import _lib, build
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.evaluators import make_evaluator
from gdb_nerf_amd.evaluators.gdb_nerf import _resize_bilinear, psnr, ssim

# |dPSNR| <= 1e-8 dB and |dSSIM| <= 1e-8: both sides compute in float64 from the same fp32 inputs and differ in summation order only
# (uniform_filter's running sums against direct window sums: <~ 3e-9 per window through the stabilisers c1 = 4e-4, c2 = 3.6e-3; a
# 5.8 M-term fp64 sum: <~ 3e-9 dB).
PSNR_TOL, SSIM_TOL = 1e-8, 1e-8
SHAPES = [(7, 7), (40, 48), (63, 95), (512, 640), (1200, 1600)]
KINDS = ("noise", "smooth", "same")


def _images(kind, B, H, W, seed):
    """gt (B,H,W,3) in [0, 1] and pred (B,3,H,W), fp32; pred leaves [0, 1] on both sides unless kind == 'same'."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        gt = rng.random((B, H, W, 3))
        pred = gt + rng.normal(0.0, 0.3, gt.shape)
    else:
        y, x = np.mgrid[0:H, 0:W]
        base = 0.5 + 0.5 * np.sin(0.9 * x + 0.3)[..., None] * np.cos(0.7 * y[..., None] + np.arange(3))
        gt = np.clip(base[None] + rng.normal(0.0, 0.02, (B, H, W, 3)), 0.0, 1.0)
        pred = gt if kind == "same" else 1.15 * (gt - 0.5) + 0.5 + rng.normal(0.0, 0.05, gt.shape)
    gt = gt.astype(np.float32)
    return gt, np.ascontiguousarray(pred.astype(np.float32).transpose(0, 3, 1, 2))


def _mask(B, H, W, random, seed):
    return (np.random.default_rng(seed).random((B, H, W)) >= 0.3).astype(np.float32) if random else np.ones((B, H, W), np.float32)


def _numpy_frame(gt, pred, mask, crop):
    """One frame as Evaluator.evaluate computes it: clamp (torch, fp32), crop, zero outside the mask, psnr over the mask, ssim."""
    p = torch.from_numpy(pred).permute(1, 2, 0).clamp(0.0, 1.0).numpy()
    y0, x0, h, w = crop
    g, p, m = gt[y0:y0 + h, x0:x0 + w].copy(), p[y0:y0 + h, x0:x0 + w].copy(), mask[y0:y0 + h, x0:x0 + w] >= 1
    g[~m], p[~m] = 0.0, 0.0
    return int(m.sum()), psnr(g[m], p[m], 1.0), ssim(g, p)


def _of_record(r, crop):
    mse = float(r[0] / (3.0 * r[1]))
    return int(r[1]), (float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse)), float(np.mean(r[2:5] / ((crop[2] - 6) * (crop[3] - 6))))


def _batch(gt, mask, scenes, src_hw=None, device="cpu", **extra):
    B, H, W, _ = gt.shape
    h, w = src_hw or (H, W)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {"src_views": {"rgb": torch.zeros(B, 3, 3, h, w)}, "tar_views": {"rgb": t(gt), "mask": t(mask), **extra.get("tar", {})},
            "tar_gt_ms": extra.get("ms", {}), "meta": {"scene": list(scenes), "tar_view": torch.zeros(B, dtype=torch.long),
                                                       "frame_id": torch.arange(B)}}


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_switch_is_read_from_the_config_and_cpu_tensors_take_the_numpy_path():
    """`test.hip_metrics` (default off) reaches the evaluator; CPU tensors take the numpy path whatever the switch says, and return
    what the switch-off evaluator returns, bit for bit."""
    assert make_cfg("configs/dtu_eval.yaml").test.hip_metrics is False
    off = make_evaluator(make_cfg("configs/dtu_eval.yaml"))
    assert off.hip_metrics is False
    cfg = make_cfg("configs/dtu_eval.yaml", ["test.hip_metrics", "True"])
    assert cfg.test.hip_metrics is True
    on = make_evaluator(cfg)
    assert on.hip_metrics is True and type(on) is type(off)
    res = []
    for ev in (off, on):
        for seed in range(3):
            gt, pred = _images("noise", 2, 24, 32, seed)
            b = _batch(gt, _mask(2, 24, 32, True, seed), ["scan1", "scan%d" % seed])
            assert not ev.use_hip_metrics({"rgb": torch.from_numpy(pred)}, b)
            ev.evaluate({"rgb": torch.from_numpy(pred)}, b)
        assert ev.capacity == 0 and len(ev.psnrs) == 6
        res.append((list(ev.psnrs), list(ev.ssims), ev.summarize()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][2] == res[1][2]


def test_library_exports_the_metric_entries_and_their_kernels_use_no_private_memory():
    lib = build.build()
    so = C.CDLL(lib)
    for name in ("gdb_eval_workspace_bytes", "gdb_eval_image", "gdb_eval_depth"):
        assert hasattr(so, name) and name in _lib.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    assert re.search(r"#define\s+GDB_ABI_VERSION\s+7\b", hdr) and _lib.load().gdb_abi_version() == 7
    for name in ("gdb_eval_workspace_bytes", "gdb_eval_image", "gdb_eval_depth"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert "gdb_metrics.hip" in build.SOURCES and build.CONTRACT["gdb_metrics.hip"] == "off"
    path = os.path.join(build.CSRC, "obj", "resource_usage.json")
    if not os.path.exists(path):
        build.build(force=True)
    usage = json.load(open(path))["gdb_metrics.hip"]
    assert sum("k_eval_" in k for k in usage) >= 4, sorted(usage)   # image, depth, and the finish launch for each record length
    for name, u in usage.items():
        assert u["scratch_bytes_per_lane"] == 0 and u["vgpr_spill"] == 0, (name, u)


def test_refusals_come_before_any_launch():
    """NULL pointers, sizes below 1, a crop outside the image or smaller than one window, a short record stride and a short workspace
    are refused with a status and a message; the device pointers are never touched (they are not even device memory here)."""
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.gdb_eval_workspace_bytes(1, 64, 96, None) == _lib.GDB_E_BADARG
    for shape in ((0, 64, 96), (1, 0, 96), (1, 64, 0), (-1, 64, 96)):
        assert lib.gdb_eval_workspace_bytes(*shape, C.byref(n)) == _lib.GDB_E_SHAPE, shape
    assert b"bad shape" in lib.gdb_last_error()

    def ws(B, H, W):
        _lib.check(lib.gdb_eval_workspace_bytes(B, H, W, C.byref(n)))
        return n.value
    assert ws(1, 7, 7) >= 40 and ws(2, 512, 640) == 2 * ws(1, 512, 640) and ws(1, 1200, 1600) > ws(1, 512, 640)
    B, H, W = 2, 63, 95
    need, fake = ws(B, H, W), 4096   # not device memory: a launch would fail, a refusal never gets there
    img = lambda pred=fake, gt=fake, mask=fake, B=B, H=H, W=W, crop=(0, 0, H, W), wsp=fake, wsb=need, rec=fake, stride=5: lib.gdb_eval_image(
        pred, gt, mask, B, H, W, *crop, wsp, wsb, rec, stride, None)
    for kw in ("pred", "gt", "mask", "wsp", "rec"):
        assert img(**{kw: None}) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error(), kw
    assert img(B=0) == _lib.GDB_E_SHAPE and img(H=0) == _lib.GDB_E_SHAPE and img(W=0) == _lib.GDB_E_SHAPE
    assert img(crop=(0, 0, 6, W)) == _lib.GDB_E_SHAPE and b"window" in lib.gdb_last_error()
    assert img(crop=(0, 0, H, 6)) == _lib.GDB_E_SHAPE and img(crop=(6, 9, 0, 0)) == _lib.GDB_E_SHAPE
    assert img(crop=(1, 0, H, W)) == _lib.GDB_E_SHAPE and b"outside" in lib.gdb_last_error()
    assert img(crop=(0, -1, H, W)) == _lib.GDB_E_SHAPE and img(crop=(0, 10, H, W - 9)) == _lib.GDB_E_SHAPE
    assert img(stride=4) == _lib.GDB_E_BADARG and b"stride" in lib.gdb_last_error()
    assert img(wsb=need - 8) == _lib.GDB_E_WORKSPACE and b"workspace" in lib.gdb_last_error()
    dep = lambda d=fake, Hd=32, Wd=48, gt=fake, B=B, H=H, W=W, resize=1, wsp=fake, wsb=need, rec=fake, stride=4: lib.gdb_eval_depth(
        d, Hd, Wd, gt, B, H, W, resize, wsp, wsb, rec, stride, None)
    for kw in ("d", "gt", "wsp", "rec"):
        assert dep(**{kw: None}) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error(), kw
    assert dep(B=0) == _lib.GDB_E_SHAPE and dep(H=0) == _lib.GDB_E_SHAPE and dep(Hd=0) == _lib.GDB_E_SHAPE and dep(Wd=-3) == _lib.GDB_E_SHAPE
    assert dep(resize=0) == _lib.GDB_E_SHAPE and b"resize" in lib.gdb_last_error()
    assert dep(stride=3) == _lib.GDB_E_BADARG
    assert dep(wsb=8) == _lib.GDB_E_WORKSPACE and b"workspace" in lib.gdb_last_error()


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _raw_eval_image(pred, gt, mask, crop, ws, rec):
    B, H, W, _ = gt.shape
    _lib.check(_lib.load().gdb_eval_image(pred.data_ptr(), gt.data_ptr(), mask.data_ptr(), B, H, W, *crop, ws.data_ptr(), ws.numel() * 8,
                                          rec.data_ptr(), rec.stride(0), torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_image_records_match_the_numpy_evaluator(H, W):
    """Every combination of B = 1 / 2, all-ones / random mask (~30 % off), eval_center off / on and the three image kinds at this
    shape: masked-pixel count equal, |dPSNR| <= 1e-8 dB, |dSSIM| <= 1e-8 per frame; gt == pred gives exactly inf and exactly 1.0.
    (At 7 x 7 the centre crop is int(0.7) = 0 pixels off each side: the numpy path slices [0:-0], an empty image; the device path
    refuses it.)  Prints the observed maxima (profiles/r09/metrics_parity_observed.txt holds a run's)."""
    from gdb_nerf_amd import metrics
    worst = {"psnr": 0.0, "ssim": 0.0}
    seed = 0
    for B in (1, 2):
        for random_mask in (False, True):
            for kind in KINDS:
                seed += 1
                gt, pred = _images(kind, B, H, W, 100 * H + seed)
                if kind != "same":
                    assert (pred < 0).any() and (pred > 1).any()
                mask = _mask(B, H, W, random_mask, seed)
                dg, dp, dm = (torch.from_numpy(a).cuda() for a in (gt, pred, mask))
                for center in (False, True):
                    ch, cw = int(H * 0.1), int(W * 0.1)
                    crop = (ch, cw, H - 2 * ch if ch else 0, W - 2 * cw if cw else 0) if center else (0, 0, H, W)
                    rec = torch.full((B, 5), float("nan"), dtype=torch.float64, device="cuda")
                    if crop[2] < 7 or crop[3] < 7:
                        with pytest.raises(ValueError, match="window"):
                            metrics.eval_image(dp, dg, dm, rec, crop)
                        continue
                    metrics.eval_image(dp, dg, dm, rec, crop)
                    rec = rec.cpu().numpy()
                    for b in range(B):
                        want = _numpy_frame(gt[b], pred[b], mask[b], crop)
                        got = _of_record(rec[b], crop)
                        case = (B, b, random_mask, kind, center)
                        assert got[0] == want[0], case
                        if kind == "same":
                            assert want[1] == float("inf") and want[2] == 1.0      # the numpy path's own property
                            assert got[1] == float("inf") and got[2] == 1.0, (case, got)
                            continue
                        dpsnr, dssim = abs(got[1] - want[1]), abs(got[2] - want[2])
                        worst["psnr"], worst["ssim"] = max(worst["psnr"], dpsnr), max(worst["ssim"], dssim)
                        print(f"parity {H}x{W} {case}: psnr {want[1]:.12f} d {dpsnr:.3e}  ssim {want[2]:.15f} d {dssim:.3e}")
                        assert dpsnr <= PSNR_TOL and dssim <= SSIM_TOL, (case, got, want)
    print(f"parity {H}x{W} observed maxima: |dPSNR| {worst['psnr']:.3e} dB, |dSSIM| {worst['ssim']:.3e}")


def _surface_batches():
    """Three scenes, several frames each, B = 2 among them, two image sizes; (gt, pred, mask, scenes)."""
    out = []
    plan = [("scan1", "scan1", 40, 48), ("scan8", None, 40, 48), ("scan1", "scan114", 63, 95), ("scan114", None, 40, 48),
            ("scan8", "scan8", 40, 48), ("scan114", None, 63, 95), ("scan8", None, 63, 95)]
    for i, (s0, s1, H, W) in enumerate(plan):
        scenes = [s0] if s1 is None else [s0, s1]
        gt, pred = _images("smooth" if i % 2 else "noise", len(scenes), H, W, 50 + i)
        out.append((gt, pred, _mask(len(scenes), H, W, i % 3 != 0, 70 + i), scenes))
    return out


def _away_from_rounding(v, decimals):
    f = (v * 10 ** decimals) % 1.0
    return abs(f - 0.5) > 1e-6 * 10 ** decimals


@pytest.mark.gpu
@pytest.mark.parametrize("center", [False, True])
def test_evaluator_summaries_match_with_the_switch_on(center, capsys):
    """The same batches through Evaluator.evaluate / summarize with the switch off (CPU tensors) and on (CUDA tensors): same keys,
    same per-scene grouping, psnr / ssim within the bounds, the same printed scene lines."""
    opts = ["test.eval_center", str(center)]
    off = make_evaluator(make_cfg("configs/dtu_eval.yaml", opts))
    on = make_evaluator(make_cfg("configs/dtu_eval.yaml", opts + ["test.hip_metrics", "True"]))
    for gt, pred, mask, scenes in _surface_batches():
        off.evaluate({"rgb": torch.from_numpy(pred)}, _batch(gt, mask, scenes))
        b = _batch(gt, mask, scenes, device="cuda")
        assert on.use_hip_metrics({"rgb": torch.from_numpy(pred).cuda()}, b)
        on.evaluate({"rgb": torch.from_numpy(pred).cuda()}, b)
    assert not on.psnrs and len(off.psnrs) == 10     # the device frames are still on the device
    for scene, rows in off.scene.items():   # the precondition for equal text, on the numpy side alone
        assert _away_from_rounding(np.mean(rows["psnr"]), 2) and _away_from_rounding(np.mean(rows["ssim"]), 3), scene
    capsys.readouterr()
    r_off = off.summarize()
    t_off = capsys.readouterr().out
    r_on = on.summarize()
    t_on = capsys.readouterr().out
    assert set(r_on) == set(r_off) == {"psnr", "ssim"}
    assert abs(r_on["psnr"] - r_off["psnr"]) <= PSNR_TOL and abs(r_on["ssim"] - r_off["ssim"]) <= SSIM_TOL
    lines = lambda t: [l for l in t.splitlines() if " psnr: " in l]
    assert lines(t_on) == lines(t_off) and [l.split()[0] for l in lines(t_on)] == ["scan1", "scan8", "scan114"]
    assert not on.psnrs and not on.scene


def _depth_case(seed=3, H=32, W=40):
    """The inputs of test_evaluator_depth_metrics: half-size rendered depth, holes in the ground truth."""
    rng = np.random.default_rng(seed)
    gt = rng.random((H, W, 3)).astype(np.float32)
    gtd = rng.uniform(430, 900, (H, W)).astype(np.float32)
    gtd[rng.random((H, W)) < 0.2] = 0.0
    mvs_gt = gtd[::2, ::2].copy()
    nerf_d = (gtd[::2, ::2] + rng.normal(0, 4, (H // 2, W // 2))).astype(np.float32)
    mvs_d = (mvs_gt + rng.normal(0, 6, mvs_gt.shape)).astype(np.float32)
    return gt, gtd, mvs_gt, nerf_d, mvs_d


@pytest.mark.gpu
def test_depth_metrics_match_the_numpy_evaluator():
    """`test.eval_depth`: valid-pixel counts equal, acc_2 / acc_10 equal, `abs` (the resized NeRF depth, float64 on both sides) within
    1e-9 relative, under the precondition - asserted on the numpy side alone - that no valid pixel's |err| lies within 1e-6 of 2 or
    10.  A scene outside the five is skipped.
    `mvs_abs`: the numpy path subtracts two float32 maps, so its errors and their mean are float32 (np.mean keeps the dtype: pairwise
    float32 sums); the device sums the same differences in float64 (the float32 subtraction of two depths within a factor 2 of each
    other is exact).  The reference's own rounding bounds the comparison: each float32 addition of the pairwise sum contributes at
    most 2^-24 relative, over at most 16 serial + 3 unrolled + log2(n / 128) pairwise levels (< 40 for any map), plus the division:
    40 * 2^-24 = 2.4e-6 relative."""
    from gdb_nerf_amd import metrics
    gt, gtd, mvs_gt, nerf_d, mvs_d = _depth_case()
    H, W = gtd.shape
    up = _resize_bilinear(nerf_d, (H, W))
    assert up.dtype == np.float64
    m, mm = gtd != 0, mvs_gt != 0
    err, merr = np.abs(up[m] - gtd[m]), np.abs(mvs_d[mm].astype(np.float64) - mvs_gt[mm].astype(np.float64))
    for e in (err, merr):
        assert np.abs(e - 2).min() > 1e-6 and np.abs(e - 10).min() > 1e-6
    # the records themselves
    rec = torch.full((2, 4), float("nan"), dtype=torch.float64, device="cuda")
    c = lambda a: torch.from_numpy(a)[None].cuda()
    metrics.eval_depth(c(nerf_d), c(gtd), rec[0:1], resize=True)
    metrics.eval_depth(c(mvs_d), c(mvs_gt), rec[1:2], resize=False)
    rec = rec.cpu().numpy()
    assert rec[0, 3] == m.sum() and rec[1, 3] == mm.sum()
    assert rec[0, 1] == (err < 2).sum() and rec[0, 2] == (err < 10).sum() and rec[1, 1] == (merr < 2).sum() and rec[1, 2] == (merr < 10).sum()
    assert abs(rec[0, 0] - err.sum()) <= 1e-9 * err.sum() and abs(rec[1, 0] - merr.sum()) <= 1e-9 * merr.sum()
    with pytest.raises(ValueError, match="resize"):
        metrics.eval_depth(c(nerf_d), c(gtd), torch.zeros((1, 4), dtype=torch.float64, device="cuda"), resize=False)
    # through the surface
    evs = {}
    for name, opts, dev in (("off", [], "cpu"), ("on", ["test.hip_metrics", "True"], "cuda")):
        ev = make_evaluator(make_cfg("configs/dtu_eval.yaml", ["test.eval_depth", "True"] + opts))
        t = lambda a: torch.from_numpy(a)[None].to(dev)
        for scene in ("scan114", "scan8", "scan21"):
            b = _batch(gt[None], np.ones((1, H, W), np.float32), [scene], device=dev, tar={"depth": t(gtd)},
                       ms={"depth": [torch.zeros(1, 4, 5), t(mvs_gt)]})
            ev.evaluate({"rgb": t(gt).permute(0, 3, 1, 2), "nerf_depth": t(nerf_d), "mvs_depth": t(mvs_d)}, b)
        ev.collect()
        evs[name] = ev
    off, on = evs["off"].depth, evs["on"].depth
    assert set(on) == set(off) and all(len(on[k]) == len(off[k]) == 2 for k in off)    # scan114 is not a depth-evaluation scene
    for i in range(2):
        for k in ("acc_2", "acc_10", "mvs_acc_2", "mvs_acc_10"):
            assert on[k][i] == off[k][i], (k, i)
        print(f"depth abs {off['abs'][i]!r} vs {on['abs'][i]!r}; mvs_abs {off['mvs_abs'][i]!r} vs {on['mvs_abs'][i]!r}")
        assert abs(on["abs"][i] - off["abs"][i]) <= 1e-9 * off["abs"][i]
        assert off["mvs_abs"][i].dtype == np.float32     # what the bound above rests on
        assert abs(on["mvs_abs"][i] - float(off["mvs_abs"][i])) <= 40 * 2.0 ** -24 * float(off["mvs_abs"][i])
    res = evs["on"].summarize()
    assert set(res) == {"psnr", "ssim"} and not evs["on"].depth


@pytest.mark.gpu
def test_evaluate_makes_no_host_round_trip():
    """With the switch on and a CUDA-resident batch, `evaluate` only enqueues.  Shown two ways: (a) under
    torch.cuda.set_sync_debug_mode("error") the call does not raise while the switch-off evaluator's `.cpu()` does - if this torch
    build honours the mode on ROCm, which the test probes with an `.item()` first (the outcome is printed; where it is not honoured
    (a) shows nothing and (b) carries the check); (b) `evaluate` returns while a long chain of matrix products enqueued ahead of it
    on the stream has not completed (an event recorded after the call is still pending)."""
    gt, pred = _images("noise", 2, 512, 640, 9)
    mask = _mask(2, 512, 640, True, 9).astype(np.uint8)       # a non-fp32 mask is converted on the device, not a reason to fall back
    b = _batch(gt, mask, ["scan1", "scan8"], device="cuda")
    out = {"rgb": torch.from_numpy(pred).cuda()}
    on = make_evaluator(make_cfg("configs/dtu_eval.yaml", ["test.hip_metrics", "True"]))
    off = make_evaluator(make_cfg("configs/dtu_eval.yaml"))
    assert on.use_hip_metrics(out, b) and not off.use_hip_metrics(out, b)
    on.evaluate(out, b)                                       # warm: library, allocator blocks, the record table
    torch.cuda.synchronize()
    # (b)
    a = torch.randn(8192, 8192, device="cuda")
    c = a @ a
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    for _ in range(40):                                       # ~ 44 TFLOP of fp32 ahead of the metrics on the stream
        c = a @ a
    on.evaluate(out, b)
    done.record()
    pending = not done.query()
    torch.cuda.synchronize()
    assert pending, "evaluate() returned only after the work enqueued ahead of it had completed"
    # (a)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            c[0, 0].item()
            honoured = False
        except RuntimeError:
            honoured = True
        print("torch.cuda.set_sync_debug_mode('error') honoured on this build:", honoured)
        on.evaluate(out, b)                                   # must not raise either way
        if honoured:
            with pytest.raises(RuntimeError):
                off.evaluate(out, b)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    res = on.summarize()
    want = [_numpy_frame(gt[i], pred[i], mask[i], (0, 0, 512, 640)) for i in range(2)]
    assert abs(res["psnr"] - np.mean([w[1] for w in want])) <= PSNR_TOL and abs(res["ssim"] - np.mean([w[2] for w in want])) <= SSIM_TOL


@pytest.mark.gpu
def test_records_are_deterministic_whatever_the_buffers_held():
    gt, pred = _images("smooth", 2, 63, 95, 4)
    dg, dp, dm = (torch.from_numpy(a).cuda() for a in (gt, pred, _mask(2, 63, 95, True, 4)))
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_eval_workspace_bytes(2, 63, 95, C.byref(n)))
    recs = []
    for fill in (0.0, 0.0, float("nan"), 1e300):
        ws = torch.full((n.value // 8,), fill, dtype=torch.float64, device="cuda")
        rec = torch.full((2, 7), fill, dtype=torch.float64, device="cuda")
        _raw_eval_image(dp, dg, dm, (3, 5, 50, 80), ws, rec)
        recs.append(rec[:, :5].cpu().numpy().view(np.int64))
        assert np.isfinite(rec[:, :5].cpu().numpy()).all()
        tail = rec[:, 5:].cpu().numpy()                       # the columns past the record are not the call's to write
        assert np.array_equal(tail.view(np.int64), np.full((2, 2), fill).view(np.int64))
    for r in recs[1:]:
        assert np.array_equal(r, recs[0])
    from gdb_nerf_amd import metrics
    gtd = np.random.default_rng(1).uniform(400, 900, (2, 64, 80)).astype(np.float32)
    d = (gtd[:, ::2, ::2] + 3).astype(np.float32)
    a, b = (torch.full((2, 4), f, dtype=torch.float64, device="cuda") for f in (0.0, float("nan")))
    metrics.eval_depth(torch.from_numpy(d).cuda(), torch.from_numpy(gtd).cuda(), a, resize=True)
    metrics.eval_depth(torch.from_numpy(d).cuda(), torch.from_numpy(gtd).cuda(), b, resize=True)
    assert np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64)) and a[0, 3].item() == 64 * 80


@pytest.mark.gpu
def test_three_hundred_frames_grow_the_table_and_summarize_resets():
    """300 frames through one evaluator: the record table grows at least twice, the summary equals the numpy path's on those
    frames, and summarize() resets so that a second epoch starts empty."""
    on = make_evaluator(make_cfg("configs/dtu_eval.yaml", ["test.hip_metrics", "True"]))
    off = make_evaluator(make_cfg("configs/dtu_eval.yaml"))
    caps = set()
    for i in range(300):
        gt, pred = _images("smooth" if i % 2 else "noise", 1, 24, 32, 1000 + i)
        mask = _mask(1, 24, 32, i % 3 == 0, i)
        scenes = ["scan%d" % (i % 4)]
        off.evaluate({"rgb": torch.from_numpy(pred)}, _batch(gt, mask, scenes))
        on.evaluate({"rgb": torch.from_numpy(pred).cuda()}, _batch(gt, mask, scenes, device="cuda"))
        caps.add(on.capacity)
    assert len(caps) >= 3 and max(caps) >= 300, caps
    per_scene = {s: (np.mean(r["psnr"]), np.mean(r["ssim"])) for s, r in off.scene.items()}
    r_off = off.summarize()
    on.collect()
    assert len(on.psnrs) == 300 and list(on.scene) == list(per_scene)
    for s, (p, q) in per_scene.items():
        assert abs(np.mean(on.scene[s]["psnr"]) - p) <= PSNR_TOL and abs(np.mean(on.scene[s]["ssim"]) - q) <= SSIM_TOL, s
    r_on = on.summarize()
    assert abs(r_on["psnr"] - r_off["psnr"]) <= PSNR_TOL and abs(r_on["ssim"] - r_off["ssim"]) <= SSIM_TOL
    # second epoch: one frame, and only that frame
    gt, pred = _images("noise", 1, 24, 32, 5)
    mask = _mask(1, 24, 32, False, 5)
    on.evaluate({"rgb": torch.from_numpy(pred).cuda()}, _batch(gt, mask, ["scan9"], device="cuda"))
    r2 = on.summarize()
    want = _numpy_frame(gt[0], pred[0], mask[0], (0, 0, 24, 32))
    assert abs(r2["psnr"] - want[1]) <= PSNR_TOL and abs(r2["ssim"] - want[2]) <= SSIM_TOL

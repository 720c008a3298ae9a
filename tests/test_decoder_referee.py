"""The default decoder (gdb_decoder.hip: gdb_decode / gdb_decode_rows at GDB_PREC_F32 and GDB_PREC_F32X), every layer against a float64
referee fed the kernel's OWN stored input.  tests/test_decoder.py compares the final image alone, with a second
fp32 implementation, at 3e-5 x scale: a 2^-17 slip of one layer's weights stays under it (test_a_slip_of_one_layer_is_seen prints it).

The driver runs gdb_decode_rows on a window equal to the frame one phase at a time and copies the workspace regions
(gdb_decoder_rows_regions, DecodeRows.activations) to the host after each, so every layer's input and output is a tensor the kernel wrote.

Rule, the same for every convolution, elementwise, no element excluded:
    |hip - ref64| <= 4 E32,    E32 = max |the same layer in fp32 on the CPU - ref64|, floored at 8 fp32 ulp of max |ref64|
(the project's 4x rule: the reference arithmetic's own error, kernel not involved).
  f32:   ref64 = the layer in float64 with the fp32 weights (the up stage: folded in float64 as the host packing does, rounded once).
  f32x:  the contract is refereed: input and weights split on the host, hi = f16(v), lo = f16(v - hi) (numpy: one rounding to nearest
         even, subnormals kept), ref64 = conv(x_hi, w_hi) + conv(x_hi, w_lo) + conv(x_lo, w_hi) in float64, E32 the same three terms in
         fp32: the bound follows the operands' magnitude by construction (below 2^-3 a pair keeps an absolute 2^-25, not 22 bits).
  part:  against float64 sums of the kernel's own T per (row, 32-pixel segment, real pixels only): d 2^-24 sum |T|, d = 5 - k_conv16
         <2, VEC, false, 2, true> adds a lane's two pixel halves (one rounding) and runs row16_sum's four steps, k_conv3x3x runs
         half_wave_sum's five steps; a wave holds a whole segment in both, there is no cross-wave step.
  part2: against float64 sums of the kernel's own part per group of DEC_SEG = 128 segments: k_se_gate's <= DEC_SEG / 4 = 32 sequential
         adds and a 4-way tree (2 levels): (min(32, ceil(n / 4)) + 2) 2^-24 sum |part|.
  gate:  against the float64 gate (mean -> fc0 -> ReLU -> fc2 -> sigmoid) of the kernel's own part: 4 x (the fp32-CPU gate of the same
         part against the float64 one), floored at 8 fp32 ulp, plus the two-stage sum's term pushed through |fc0|, |fc2| and the
         sigmoid's slope <= 1/4: (min(32, ceil(nseg / 4)) + 2 + ceil(ngrp / 4) + 2 + 2) 2^-24 sum |part| / (H W) (the last 2: the
         rounded 1 / (H W) and the product with it).
  trunk: x_b = x_{b-1} + T gate in float64 from the snapshots: two fp32 roundings, 2^-24 (|T gate| + |ref|); X of bundle_size 4 adds
         the global residual: three, 2^-24 (|T gate| + |x + T gate| + |ref|).
  up:    bundle_size 2 stages x_{L-1} + T gate + P0 without storing it: formed in float64, bound 4 E32 + conv(u, |w|),
         u = 2^-23 (|T gate| + |x|); bundle_size 4: the four sub-pixel convolutions from the stored X into the stored U, then the folded
         stage from the stored U.

Small-operand regime: the input and every convolution's weights (and biases) scaled on the CPU, layer by layer on the float64 module,
so that max |stored activation| of every layer is 1e-3 (achieved: exactly 1e-3 for in_conv, conv1, conv2, conv3 and the up stages by
construction, the image too; trunks 2.4e-3 and 2.6e-3 at most) - same rule, both precisions."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, synthetic
from gdb_nerf_amd.engine import HotPathEngine
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder

F64, F32 = torch.float64, torch.float32
DEC_SEG = 128                       # gdb_decoder.hip
PART_DEPTH = 5                      # see the module docstring
SMALL = 1e-3
# (bundle_size, B, H, W, blocks)
CASES_B2 = [(2, 1, 7, 33, 2), (2, 2, 19, 45, 3), (2, 1, 5, 32, 1), (2, 1, 24, 40, 5), (2, 1, 70, 70, 1), (2, 1, 103, 160, 1), "F7", (2, 1, 3, 5, 1)]
CASES_B4 = [(4, 1, 6, 9, 2), (4, 2, 13, 37, 2), (4, 1, 16, 24, 3)]
SMALL_CASES = [("small", (2, 2, 19, 45, 3)), ("small", "F7")]
CASES = CASES_B2 + CASES_B4 + SMALL_CASES
PRECS = pytest.mark.parametrize("prec", [1, 2], ids=["f32", "f32x"])


def _id(c):
    if isinstance(c, str):
        return c
    if c[0] == "small":
        return "small-" + _id(c[1])
    return f"b{c[0]}-" + "x".join(map(str, c[1:]))


ALL = pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])


# ---- the network in plain torch, functional, any dtype ------------------------------------------------------------------------
def _f7_state():
    f7 = load_golden("F7_network")
    return {k[len("sd.upsampler."):]: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in f7.items() if k.startswith("sd.upsampler.")}


def _fold64(wup, bup, wout, bout):
    """out_conv o PixelShuffle(2) o up as one 64 -> 12 convolution in float64 (gdb_pack_decoder_weights): channel 3 s + o, s = dy*2 + dx."""
    wup, bup, wout, bout = wup.to(F64), bup.to(F64), wout.to(F64)[:, :, 0, 0], bout.to(F64)
    w = torch.einsum("ok,ksctu->soctu", wout, wup.view(64, 4, 64, 3, 3)).reshape(12, 64, 3, 3)
    b = (torch.einsum("ok,ks->so", wout, bup.view(64, 4)) + bout[None]).reshape(12)
    return w, b


def _weights(sd, layers, bundle):
    """The kernel's fp32 weights by layer: the last up stage folded in float64 and rounded once; bundle_size 4: the first up stage as
    four 64 -> 64 convolutions, conv channel 4 k + sp -> feature k of sub-pixel sp."""
    last = "up.2" if bundle == 4 else "up.0"
    wf, bf = _fold64(sd[f"{last}.weight"], sd[f"{last}.bias"], sd["out_conv.weight"], sd["out_conv.bias"])
    w = {"in": sd["in_conv.weight"], "in_b": sd["in_conv.bias"], "up": wf.to(F32), "up_b": bf.to(F32)}
    for i in range(layers):
        for k in ("conv1", "conv2", "conv3"):
            w[f"{i}.{k}"] = sd[f"blocks.{i}.{k}.weight"]
        w[f"{i}.fc0"], w[f"{i}.fc2"] = sd[f"blocks.{i}.se.fc.0.weight"], sd[f"blocks.{i}.se.fc.2.weight"]
    if bundle == 4:
        for sp in range(4):
            w[f"u1.{sp}"], w[f"u1_b.{sp}"] = sd["up.0.weight"][sp::4].contiguous(), sd["up.0.bias"][sp::4].contiguous()
    return w


def _f16(t):
    """ONE rounding of a float64 / float32 tensor to f16, nearest even, subnormals kept (numpy casts directly), value back in t's dtype."""
    return torch.from_numpy(t.detach().numpy().astype(np.float16).astype(t.detach().numpy().dtype))


def _split(t):
    hi = _f16(t)
    return hi, _f16(t - hi)


def _conv(prec, x, w, bias=None, relu=False, dtype=F64):
    """One convolution of the contract in `dtype`: f32 - the plain one; f32x - x_hi w_hi + x_hi w_lo + x_lo w_hi as ONE convolution of
    [x_hi | x_hi | x_lo] with [w_hi | w_lo | w_hi] (x, w: float64 holding the stored fp32 / the fp32 weights)."""
    if prec == 2:
        (xh, xl), (wh, wl) = _split(x), _split(w)
        x, w = torch.cat((xh, xh, xl), 1), torch.cat((wh, wl, wh), 1)
    y = F.conv2d(x.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), padding=1)
    return F.relu(y) if relu else y


def _gate_of_mean(mean, w0, w2):
    return torch.sigmoid(F.linear(F.relu(F.linear(mean, w0)), w2))


def _unshuffle(y):
    """(B, 12, H, W), channel 3 s + o -> (B, 3, 2H, 2W)."""
    B, _, H, W = y.shape
    return y.view(B, 2, 2, 3, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, 3, 2 * H, 2 * W)


def _shuffle12(rgb):
    """The inverse: (B, 3, 2H, 2W) -> (B, 12, H, W)."""
    B, _, H2, W2 = rgb.shape
    return rgb.reshape(B, 3, H2 // 2, 2, W2 // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 12, H2 // 2, W2 // 2)


def _forward(w, layers, bundle, x, dtype, prec=1, keep=None):
    """The decoder as the kernels compute it, in `dtype` arithmetic (prec 2: every convolution on split operands); keep: a dict that
    receives the stored activations."""
    cv = lambda t, k, b=None, relu=False: _conv(prec, t.to(F64), w[k].to(F64), None if b is None else w[b], relu, dtype)
    keep = {} if keep is None else keep
    shallow = trunk = keep["in"] = cv(x.to(dtype), "in", "in_b")
    for i in range(layers):
        a1 = keep[f"{i}.conv1"] = cv(trunk, f"{i}.conv1", relu=True)
        a2 = keep[f"{i}.conv2"] = cv(torch.cat((trunk, a1), 1), f"{i}.conv2", relu=True)
        c = keep[f"{i}.conv3"] = cv(torch.cat((trunk, a1, a2), 1), f"{i}.conv3")
        g = keep[f"{i}.gate"] = _gate_of_mean(c.mean((2, 3)), w[f"{i}.fc0"].to(dtype), w[f"{i}.fc2"].to(dtype))
        trunk = keep[f"trunk.{i + 1}"] = trunk + c * g[:, :, None, None]
    xs = keep["X"] = trunk + shallow
    if bundle == 4:
        B, _, H, W = xs.shape
        U = torch.zeros((B, 64, 2 * H, 2 * W), dtype=dtype)
        for sp in range(4):
            U[:, :, sp >> 1::2, sp & 1::2] = cv(xs, f"u1.{sp}", f"u1_b.{sp}")
        xs = keep["U"] = U
    return _unshuffle(cv(xs, "up", "up_b"))


def _rescale_small(sd, layers, bundle, x):
    """Scale the input, then every convolution's weights (and bias) in turn so that the float64 module's output of that layer has
    max |.| = SMALL: (scaled state dict, scaled input, {layer: achieved max |activation|})."""
    sd = {k: v.clone() for k, v in sd.items()}
    x = x * (SMALL / float(x.abs().max()))
    order = ["in_conv"] + [f"blocks.{i}.{k}" for i in range(layers) for k in ("conv1", "conv2", "conv3")] + ["up.0"] + (["up.2"] if bundle == 4 else [])
    name = {"in_conv": "in", "up.0": "U" if bundle == 4 else None, "up.2": None}
    for key in order:
        keep = {}
        out = _forward(_weights(sd, layers, bundle), layers, bundle, x, F64, keep=keep)
        k = name.get(key, key[len("blocks."):] if key.startswith("blocks.") else None)
        cur = float((out if k is None else keep[k]).abs().max())
        sd[key + ".weight"] = (sd[key + ".weight"].to(F64) * (SMALL / cur)).to(F32)
        for extra in (key + ".bias",) + (("out_conv.bias",) if key == order[-1] else ()):   # (the image is linear in the last stage and out_conv's bias)
            if extra in sd:
                sd[extra] = (sd[extra].to(F64) * (SMALL / cur)).to(F32)
    keep = {}
    _forward(_weights(sd, layers, bundle), layers, bundle, x, F64, keep=keep)
    return sd, x, {k: float(v.abs().max()) for k, v in keep.items() if "gate" not in k}


@functools.lru_cache(maxsize=None)
def _case(case):
    """(state dict of fp32 CPU tensors, x (B, 27, H, W) fp32, blocks, bundle_size)."""
    if isinstance(case, tuple) and case[0] == "small":
        sd, x, layers, bundle = _case(case[1])
        sd, x, _ = _rescale_small(sd, layers, bundle, x)
        return sd, x.to(F32), layers, bundle
    if case == "F7":
        return _f7_state(), torch.from_numpy(load_golden("F7_network")["dec_in"].astype(np.float32)), 3, 2
    bundle, B, H, W, layers = case
    torch.manual_seed(3)
    dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=bundle).eval()
    with torch.no_grad():
        for p in dec.parameters():                                   # biases and gates that matter (tests/test_decoder.py)
            p.mul_(1.5)
    x = torch.randn(B, 27, H, W, generator=torch.Generator().manual_seed(7))
    return {k: v.detach().clone() for k, v in dec.state_dict().items()}, x, layers, bundle


def _ref64_module(case):
    sd, x, layers, bundle = _case(case)
    dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=bundle).to(F64).eval()
    dec.load_state_dict({k: v.to(F64) for k, v in sd.items()})
    with torch.no_grad():
        return dec(x.to(F64))


@functools.lru_cache(maxsize=None)
def _contract_sizes(case, prec):
    """(ref64 of the module, D = max |emulation in float64 - ref64|, E_acc = max |emulation in fp32 - in float64|), kernel not involved."""
    sd, x, layers, bundle = _case(case)
    w = _weights(sd, layers, bundle)
    with torch.no_grad():
        ref, e64, e32 = _ref64_module(case), _forward(w, layers, bundle, x, F64, prec), _forward(w, layers, bundle, x, F32, prec)
    return ref, float((e64 - ref).abs().max()), float((e32.to(F64) - e64).abs().max())


def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 2.0 ** -126))) - 23.0)


def _conv_referee(prec, src, w, bias=None, relu=False):
    """(ref64, E32) of one convolution on the float64 tensor `src`."""
    with torch.no_grad():
        r64, r32 = _conv(prec, src, w.to(F64), bias, relu, F64), _conv(prec, src, w.to(F64), bias, relu, F32)
    return r64, max(max_abs(r32.numpy(), r64.numpy()), 8 * _ulp32(r64.abs().max()))


def _seg_sums(t):
    """(B, 64, H, W) -> (B, H, ceil(W / 32), 64) sums over each row's 32-pixel segments (the last one: its real pixels only)."""
    B, Cn, H, W = t.shape
    nx = (W + 31) // 32
    return F.pad(t, (0, 32 * nx - W)).view(B, Cn, H, nx, 32).sum(-1).permute(0, 2, 3, 1)


def _gate_referee(part, w0, w2, hw):
    """(gate in float64, bound) from the kernel's own part (B, H, nx, 64) float64."""
    B = part.shape[0]
    seg = part.reshape(B, -1, 64)
    nseg = seg.shape[1]
    ngrp = (nseg + DEC_SEG - 1) // DEC_SEG
    g64 = _gate_of_mean(seg.sum(1) / hw, w0.to(F64), w2.to(F64))
    g32 = _gate_of_mean(seg.to(F32).sum(1) / hw, w0, w2).to(F64)
    roundings = min(DEC_SEG // 4, -(-nseg // 4)) + 2 + -(-ngrp // 4) + 2 + 2
    dmean = roundings * 2.0 ** -24 * seg.abs().sum(1) / hw
    dpre = F.linear(F.linear(dmean, w0.to(F64).abs()), w2.to(F64).abs())
    bound = max(4 * max_abs(g32.numpy(), g64.numpy()), 8 * _ulp32(g64.max())) + 0.25 * dpre
    return g64, bound


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def _lib_built():
    from gdb_nerf_amd import build
    build.build()
    return _lib.load()


def _cfg(b=2):
    return _lib.GdbConfig(b, 3, 1, 0, 64, 3, 16, 8, 64, 1)


def _regions(lib, b, B, H, W, r0, r1, L):
    f = _lib.GdbFrame()
    f.B, f.H, f.W = B, H, W
    n = C.c_int32()
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg(b)), C.byref(f), r0, r1, L, None, 0, C.byref(n), None) == 0
    regs, which = (_lib.GdbDecRegion * n.value)(), (C.c_int32 * L)()
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg(b)), C.byref(f), r0, r1, L, C.cast(regs, C.c_void_p), n.value, C.byref(n), which) == 0
    return f, regs, list(which)


def test_region_query_is_host_only_and_agrees_with_the_other_layout_entries():
    lib = _lib_built()
    for b, B, H, W, L in ((2, 2, 19, 45, 3), (4, 1, 16, 24, 5), (2, 1, 103, 160, 1)):
        f, regs, which = _regions(lib, b, B, H, W, 0, H, L)
        names = [r.name.decode() for r in regs]
        assert names == ["P0", "P1", "P2", "Y", "T", "part", "part2", "gate", "X", "U"] and len(regs) == 10
        assert which == [0] + [1 + (k - 1) % 2 for k in range(1, L)]
        by = {r.name.decode(): r for r in regs}
        need, off, pitch, w0, w1 = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int32(), C.c_int32()
        assert lib.gdb_decoder_rows_workspace_bytes(C.byref(_cfg(b)), C.byref(f), 0, H, L, C.byref(need)) == 0
        assert lib.gdb_decoder_rows_layout(C.byref(_cfg(b)), C.byref(f), 0, H, L, C.byref(off), C.byref(pitch), C.byref(w0), C.byref(w1)) == 0
        assert (w0.value, w1.value) == (0, H) and by["part"].offset == off.value and by["part"].bytes == B * H * pitch.value
        whole = C.c_size_t()
        assert lib.gdb_decoder_workspace_bytes(C.byref(_cfg(b)), C.byref(f), C.byref(whole)) == 0 and whole.value == need.value
        assert tuple(by["P1"].shape) == (B, H, W, 64) and tuple(by["gate"].shape) == (B, 64, 0, 0) and tuple(by["part"].shape) == (B, H, (W + 31) // 32, 64)
        assert tuple(by["part2"].shape) == (B, (H * ((W + 31) // 32) + DEC_SEG - 1) // DEC_SEG, 64, 0)
        for r in regs:
            assert r.bytes == 4 * int(np.prod([d for d in r.shape if d])) * (1 if r.shape[0] else 0)
        if b == 2:
            assert by["X"].bytes == 0 and by["U"].bytes == 0
        else:
            assert tuple(by["X"].shape) == (B, H, W, 64) and tuple(by["U"].shape) == (B, 2 * H, 2 * W, 64)
        spans = sorted((r.offset, r.offset + r.bytes) for r in regs if r.bytes)
        assert all(a[1] <= c[0] for a, c in zip(spans, spans[1:])) and spans[-1][1] <= need.value and all(s[0] % 256 == 0 for s in spans)
    # a window smaller than the frame: window-sized activations, frame-sized part
    f, regs, _ = _regions(lib, 2, 1, 64, 40, 40, 48, 1)
    by = {r.name.decode(): r for r in regs}
    w0, w1 = C.c_int32(), C.c_int32()
    assert lib.gdb_decoder_rows_layout(C.byref(_cfg()), C.byref(f), 40, 48, 1, None, None, C.byref(w0), C.byref(w1)) == 0
    assert tuple(by["T"].shape) == (1, w1.value - w0.value, 40, 64) and by["part"].shape[1] == 64
    # refusals (no device is touched by this entry at all)
    n = C.c_int32()
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg(1)), C.byref(f), 0, 8, 1, None, 0, C.byref(n), None) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg()), C.byref(f), 0, 8, 17, None, 0, C.byref(n), None) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg()), C.byref(f), 8, 8, 1, None, 0, C.byref(n), None) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg()), C.byref(f), 0, 65, 1, None, 0, C.byref(n), None) == _lib.GDB_E_SHAPE
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg()), C.byref(f), 0, 8, 1, None, 0, None, None) == _lib.GDB_E_BADARG
    regs = (_lib.GdbDecRegion * 10)()
    assert lib.gdb_decoder_rows_regions(C.byref(_cfg()), C.byref(f), 0, 8, 1, C.cast(regs, C.c_void_p), 9, C.byref(n), None) == _lib.GDB_E_BADARG


def test_the_functional_network_is_the_module():
    """The referee's own network (folded up stage, sub-pixel convolutions) against the PyTorch module in float64, and the split
    convolution against the plain one: a guard against a broken referee."""
    for case in ((2, 1, 7, 33, 2), (4, 1, 6, 9, 2)):
        sd, x, layers, bundle = _case(case)
        with torch.no_grad():
            got = _forward(_weights(sd, layers, bundle), layers, bundle, x, F64)
        ref = _ref64_module(case)
        assert got.shape == ref.shape and max_abs(got.numpy(), ref.numpy()) <= 2e-6 * float(ref.abs().max())
    # the split convolution against the plain one: each operand pair is within 2^-22 |v| + 2^-25 of v, lo x lo (<= 2^-22 |x w|) is dropped
    x, w = torch.randn(1, 8, 5, 6).to(F64), torch.randn(4, 8, 3, 3).to(F64)
    a, c = _conv(1, x, w), _conv(2, x, w)
    one = torch.ones_like
    slack = 3 * 2.0 ** -22 * _conv(1, x.abs(), w.abs()) + 2.0 ** -25 * (_conv(1, one(x), w.abs()) + _conv(1, x.abs(), one(w)))
    assert bool(((a - c).abs() <= slack).all()) and float((a - c).abs().max()) > 0
    hi, lo = _split(torch.tensor([1e-3, 3e-5, 0.3], dtype=F64))
    assert float(lo[0]) != 0 and abs(float(hi[0] + lo[0]) - 1e-3) <= 2.0 ** -25     # a subnormal low half is kept, to 2^-25 absolute


@pytest.mark.parametrize("case", SMALL_CASES, ids=[_id(c) for c in SMALL_CASES])
def test_the_small_operand_cases_are_small(case):
    sd, x, layers, bundle = _case(case[1])
    _, xs, got = _rescale_small(sd, layers, bundle, x)
    print(f"[decoder referee] {_id(case)}: max |activation| per layer {min(got.values()):.3e} .. {max(got.values()):.3e}, input {float(xs.abs().max()):.3e}")
    for k, v in got.items():
        assert (0.999 * SMALL <= v <= 1.001 * SMALL) if ("trunk" not in k and k != "X") else v <= (layers + 2) * SMALL, (k, v)


# the slip of one layer's weights, x (1 + 2^-k): per layer the SMALLEST slip (largest k) whose effect on the float64 layer - fed the
# float64 module's activations, kernel not involved - exceeds twice that layer's bound (_slip_sizes; pinned by the CPU test below)
SLIP_LAYERS = {2: ("in", "1.conv2", "up", "0.fc2"), 4: ("in", "1.conv2", "up", "u1.2", "0.fc2")}
SLIP_CASES = {2: (2, 2, 19, 45, 3), 4: (4, 1, 6, 9, 2)}
SLIP_K = {}   # filled in below: {(bundle_size, prec): {layer: k}}


@functools.lru_cache(maxsize=None)
def _slip_sizes(bundle, prec):
    case = SLIP_CASES[bundle]
    sd, x, layers, _ = _case(case)
    w = _weights(sd, layers, bundle)
    keep = {}
    with torch.no_grad():
        _forward(w, layers, bundle, x.to(F32), F32, prec, keep=keep)       # fp32 activations, as the kernel stores them
    keep = {k: v.to(F64) for k, v in keep.items()}
    trunk1 = keep["trunk.1"]
    src = {"in": (x.to(F64), "in_b"), "1.conv2": (torch.cat((trunk1, keep["1.conv1"]), 1), None),
           "up": (keep["U"] if bundle == 4 else keep["X"], "up_b"), "u1.2": (keep["X"], "u1_b.2")}
    last = layers - 1
    tg = keep[f"{last}.conv3"] * keep[f"{last}.gate"][:, :, None, None]
    up_extra = F.conv2d(2.0 ** -23 * (tg.abs() + keep["X"].abs()), w["up"].to(F64).abs(), padding=1) if bundle == 2 else 0.0
    out = {}
    for layer in SLIP_LAYERS[bundle]:
        if layer == "0.fc2":
            part = _seg_sums(keep["0.conv3"])
            hw = x.shape[2] * x.shape[3]
            g64, bound = _gate_referee(part, w["0.fc0"], w["0.fc2"], hw)
            mean = part.reshape(part.shape[0], -1, 64).sum(1) / hw
            diff = lambda k: float(((_gate_of_mean(mean, w["0.fc0"].to(F64), w["0.fc2"].to(F64) * (1 + 2.0 ** -k)) - g64).abs() / bound).max())
        else:
            s, b = src[layer]
            r64, e32 = _conv_referee(prec, s, w[layer], None if b is None else w[b], relu=layer == "1.conv2")
            lin = _conv_referee(prec, s, w[layer], None, relu=layer == "1.conv2")[0]      # the slip moves the product, not the bias
            extra = up_extra if layer == "up" else 0.0
            diff = lambda k: float((lin.abs() * 2.0 ** -k / (4 * e32 + extra)).max())
        out[layer] = max(k for k in range(1, 24) if diff(k) > 2.0)
    return out


_K2, _K4 = {"in": 17, "1.conv2": 17, "up": 17, "0.fc2": 13}, {"in": 17, "1.conv2": 17, "up": 17, "u1.2": 17, "0.fc2": 13}
SLIP_K.update({(2, 1): _K2, (2, 2): _K2, (4, 1): _K4, (4, 2): _K4})


@pytest.mark.parametrize("bundle,prec", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_slip_sizes_are_the_recorded_ones(bundle, prec):
    got = _slip_sizes(bundle, prec)
    print(f"[decoder referee] slip sizes k (weights x (1 + 2^-k)), bundle_size {bundle}, precision {prec}: {got}")
    assert got == SLIP_K[(bundle, prec)]


@pytest.mark.parametrize("case", [(2, 2, 19, 45, 3), (4, 1, 6, 9, 2), ("small", (2, 2, 19, 45, 3))], ids=["b2", "b4", "small"])
@PRECS
def test_contract_sizes(case, prec):
    """D and E_acc of the end-to-end bound, CPU only.  Asserted (a guard against a broken emulation): the emulation's fp32 and float64
    runs agree within D + 4 x the fp32 PyTorch module's own distance from the float64 module."""
    ref, D, E_acc = _contract_sizes(case, prec)
    sd, x, layers, bundle = _case(case)
    with torch.no_grad():
        dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=bundle).eval()
        dec.load_state_dict(sd)
        e_f32 = float((dec(x).to(F64) - ref).abs().max())
    print(f"[decoder referee] {_id(case)} precision {prec}: output scale {float(ref.abs().max()):.3e}  D {D:.3e}  E_acc {E_acc:.3e}  fp32 module {e_f32:.3e}")
    assert 0 < E_acc <= D + 4 * e_f32


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _dims(case):
    sd, x, layers, bundle = _case(case)
    return (bundle, layers) + tuple(x.shape[i] for i in (0, 2, 3))


@functools.lru_cache(maxsize=None)
def _engine(case):
    sd, x, layers, bundle = _case(case)
    B, _, H, W = x.shape
    frame = synthetic.make_frame(bundle * H, bundle * W, V=2, B=B, bundle_size=bundle, seed=1)
    eng = HotPathEngine(bundle_size=bundle)
    eng.prepare({k: torch.from_numpy(v).cuda() for k, v in frame.items()})
    eng.load_decoder_weights({k: v.numpy() for k, v in sd.items()}, layers)
    return eng, eng.decoder_rows(0, H)


@functools.lru_cache(maxsize=None)
def _rows(case, ld):
    """The bundle rows (N_b, ld): the decoder's 27 channels behind the 3 b^2 fine-RGB columns, everything else 7.0."""
    sd, x, layers, bundle = _case(case)
    B, _, H, W = x.shape
    bf = torch.full((B * H * W, ld), 7.0)
    bf[:, 3 * bundle * bundle:3 * bundle * bundle + 27] = x.permute(0, 2, 3, 1).reshape(B * H * W, 27)
    return bf.cuda().contiguous()


def _run(case, prec, ld, phases=None):
    """Phases 0 .. L one at a time: (rgb_c on the CPU or None, [per phase {region: float64 CPU tensor, activations channel-first}],
    block_input).  The workspace starts as all-ones bits (NaN): a region that a phase should have written and did not is not finite."""
    bundle, L, B, H, W = _dims(case)
    eng, dec = _engine(case)
    bf = _rows(case, ld)
    dec.ws.fill_(0xFF)
    snaps, rgb = [], None
    for p in range(L + 1 if phases is None else phases):
        rgb = dec.run_phase(bf, p, precision=prec)
        acts = dec.activations()
        want = ["P0"] + (["Y", "T", "part", dec.block_input[p]] if p < L else []) + (["gate", "part2"] if p else []) + (["X", "U"] if p == L and bundle == 4 else [])
        snap = {}
        for k in dict.fromkeys(want):
            v = acts[k].detach().cpu().to(F64)
            snap[k] = v.permute(0, 3, 1, 2).contiguous() if k in ("P0", "P1", "P2", "Y", "T", "X", "U") else v
        snaps.append(snap)
    return (None if rgb is None else rgb.cpu()), snaps, list(dec.block_input)


@functools.lru_cache(maxsize=None)
def _ran(case, prec):
    bundle = _dims(case)[0]
    return _run(case, prec, 41 if bundle == 2 else 77)


def _n_checks(bundle, L):
    """in_conv (bundle_size 2: at both row strides) + 6 per block + the folded up stage + the trunk updates (+ X and the four sub-pixel
    convolutions at bundle_size 4)."""
    return (2 if bundle == 2 else 1) + 6 * L + 1 + (L - 1) + (5 if bundle == 4 else 0)


def _check_layers(case, prec, rgb, snaps, which, only=None, in39=None):
    """{layer: (max over elements of |hip - ref64| / bound, max |hip - ref64|)}; `only`: the layers to compute."""
    sd, x, L, bundle = _case(case)
    B, _, H, W = x.shape
    w = _weights(sd, L, bundle)
    out = {}
    on = lambda name: only is None or name in only

    def put(name, got, ref, bound):
        err = (got - ref).abs()
        out[name] = (float((err / bound).max()), float(err.max()))

    def conv(name, key, src, hip, bias=None, relu=False, extra=0.0):
        if on(name):
            r64, e32 = _conv_referee(prec, src, w[key], None if bias is None else w[bias], relu)
            put(name, hip, r64, 4 * e32 + extra)

    conv("in_conv", "in", x.to(F64), snaps[0]["P0"], bias="in_b")
    if in39 is not None:
        conv("in_conv@39", "in", x.to(F64), in39, bias="in_b")
    for i in range(L):
        s, nxt = snaps[i], snaps[i + 1]
        t, y, c = s[which[i]], s["Y"], s["T"]
        conv(f"blocks.{i}.conv1", f"{i}.conv1", t, y[:, :32], relu=True)
        conv(f"blocks.{i}.conv2", f"{i}.conv2", torch.cat((t, y[:, :32]), 1), y[:, 32:], relu=True)
        conv(f"blocks.{i}.conv3", f"{i}.conv3", torch.cat((t, y), 1), c)
        part, g = s["part"], nxt["gate"]
        if on(f"blocks.{i}.part"):
            put(f"blocks.{i}.part", part, _seg_sums(c), PART_DEPTH * 2.0 ** -24 * _seg_sums(c.abs()))
        seg = part.reshape(B, -1, 64)
        nseg = seg.shape[1]
        ngrp = (nseg + DEC_SEG - 1) // DEC_SEG
        if on(f"blocks.{i}.part2"):
            pad = F.pad(seg, (0, 0, 0, ngrp * DEC_SEG - nseg)).view(B, ngrp, DEC_SEG, 64)
            assert tuple(nxt["part2"].shape) == (B, ngrp, 64)
            put(f"blocks.{i}.part2", nxt["part2"], pad.sum(2), (min(DEC_SEG // 4, -(-nseg // 4)) + 2) * 2.0 ** -24 * pad.abs().sum(2))
        if on(f"blocks.{i}.gate"):
            g64, bound = _gate_referee(part, w[f"{i}.fc0"], w[f"{i}.fc2"], H * W)
            put(f"blocks.{i}.gate", g, g64, bound)
        tg = c * g[:, :, None, None]
        if i + 1 < L:
            if on(f"trunk.{i + 1}"):
                put(f"trunk.{i + 1}", nxt[which[i + 1]], t + tg, 2.0 ** -24 * (tg.abs() + (t + tg).abs()))
        elif bundle == 2:
            xs = t + tg + nxt["P0"]
            u = 2.0 ** -23 * (tg.abs() + xs.abs())
            conv("up", "up", xs, _shuffle12(rgb.to(F64)), bias="up_b", extra=F.conv2d(u, w["up"].to(F64).abs(), padding=1))
        else:
            xs = t + tg + nxt["P0"]
            if on("X"):
                put("X", nxt["X"], xs, 2.0 ** -24 * (tg.abs() + (t + tg).abs() + xs.abs()))
            for sp in range(4):
                conv(f"up1.{sp}", f"u1.{sp}", nxt["X"], nxt["U"][:, :, sp >> 1::2, sp & 1::2], bias=f"u1_b.{sp}")
            conv("up", "up", nxt["U"], _shuffle12(rgb.to(F64)), bias="up_b")
    return out


@pytest.mark.gpu
@ALL
@PRECS
def test_every_layer_against_a_float64_referee_fed_the_kernels_own_inputs(case, prec):
    bundle, L, B, H, W = _dims(case)
    eng, dec = _engine(case)
    rgb, snaps, which = _ran(case, prec)
    assert all(torch.isfinite(v).all() for s in snaps for v in s.values()) and torch.isfinite(rgb).all()
    for ld in ((39, 41) if bundle == 2 else (77,)):                       # phase by phase = the one call, bit for bit
        assert torch.equal(rgb, eng.decode(_rows(case, ld), precision=prec).cpu()), ld
    in39 = _run(case, prec, 39, phases=1)[1][0]["P0"] if bundle == 2 else None
    res = _check_layers(case, prec, rgb, snaps, which, in39=in39)
    assert len(res) == _n_checks(bundle, L), sorted(res)
    for k, (ratio, err) in res.items():
        print(f"[decoder referee] {_id(case)} precision {prec} {k}: max |hip - ref64| {err:.3e}  observed / bound {ratio:.3f}")
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, bad


def _sections(layers, bundle):
    """Float offsets (start, count) of the packed buffer's sections by layer: ("w" fp32 form, "x" hi/lo form) (dec_layout)."""
    cf = lambda cin, nt: ((cin + 31) // 32) * 9 * 8 * 64 * 2 * nt
    off, o = {}, 0

    def take(name, n):
        nonlocal o
        off[name] = (o, n)
        o += n
    take("w.in", cf(27, 2)); take("in_b", 64)
    for i in range(layers):
        take(f"w.{i}.conv1", cf(64, 1)); take(f"w.{i}.conv2", cf(96, 1)); take(f"w.{i}.conv3", cf(128, 2)); take(f"w.{i}.fc0", 256); take(f"w.{i}.fc2", 256)
    take("w.up", cf(64, 1)); take("up_b", 32)
    take("x.in", cf(27, 2))
    for i in range(layers):
        take(f"x.{i}.conv1", cf(64, 1)); take(f"x.{i}.conv2", cf(96, 1)); take(f"x.{i}.conv3", cf(128, 2))
    take("x.up", cf(64, 1))
    if bundle == 4:
        for sp in range(4):
            take(f"w.u1.{sp}", cf(64, 2)); take(f"x.u1.{sp}", cf(64, 2)); take(f"u1_b.{sp}", 64)
    return off


@pytest.mark.gpu
@pytest.mark.parametrize("bundle", [2, 4], ids=["b2", "b4"])
@PRECS
def test_a_slip_of_one_layer_is_seen(bundle, prec):
    """One layer's packed weights x (1 + 2^-k) on the device (the fp32 section at f32; the hi / lo fragments at f32x, re-split from
    hi + lo; the gate: fc.2) must break that layer's bound, at the k of SLIP_K.  Printed, not asserted: the same slip against
    tests/test_decoder.py's end-to-end 3e-5 x scale - the gap this file closes."""
    case = SLIP_CASES[bundle]
    _, L, B, H, W = _dims(case)
    eng, dec = _engine(case)
    rgb0 = _ran(case, prec)[0]
    ld = 41 if bundle == 2 else 77
    off = _sections(L, bundle)
    good = eng.dec_weights.clone()
    name = {"in": "in_conv", "1.conv2": "blocks.1.conv2", "up": "up", "u1.2": "up1.2", "0.fc2": "blocks.0.gate"}
    try:
        for layer in SLIP_LAYERS[bundle]:
            k = SLIP_K[(bundle, prec)][layer]
            eng.dec_weights.copy_(good)
            o, n = off[("w." if prec == 1 or layer == "0.fc2" else "x.") + layer]
            sec = eng.dec_weights[o:o + n]
            if prec == 1 or layer == "0.fc2":
                sec.mul_(1 + 2.0 ** -k)
            else:                                                        # [..][hi, lo][64 lanes][8 halves]
                h = sec.view(torch.float16).view(-1, 2, 512)
                v = (h[:, 0].double() + h[:, 1].double()) * (1 + 2.0 ** -k)
                hi = v.to(torch.float32).to(torch.float16)
                h[:, 0], h[:, 1] = hi, (v - hi.double()).to(torch.float32).to(torch.float16)
            rgb, snaps, which = _run(case, prec, ld)
            ratio, err = _check_layers(case, prec, rgb, snaps, which, only=(name[layer],))[name[layer]]
            e2e, scale = float((rgb - rgb0).abs().max()), float(rgb0.abs().max())
            print(f"[decoder referee] b{bundle} precision {prec} slip 2^-{k} of {name[layer]}: observed / bound {ratio:.2f};  end to end it moves "
                  f"the image by {e2e:.3e} = {e2e / (3e-5 * max(1.0, scale)):.3f} of test_decoder.py's 3e-5 x scale")
            assert ratio > 1.0, layer
    finally:
        eng.dec_weights.copy_(good)
    assert torch.equal(_run(case, prec, ld)[0], rgb0)


@pytest.mark.gpu
@ALL
@PRECS
def test_end_to_end_against_float64(case, prec):
    ref, D, E_acc = _contract_sizes(case, prec)
    rgb = _ran(case, prec)[0]
    e = max_abs(rgb.numpy(), ref.numpy())
    print(f"[decoder referee] {_id(case)} precision {prec} end to end: max |hip - ref64| {e:.3e}  D {D:.3e}  E_acc {E_acc:.3e}  "
          f"observed / bound {e / (D + 4 * E_acc):.3f}  output scale {float(ref.abs().max()):.3e}")
    assert e <= D + 4 * E_acc

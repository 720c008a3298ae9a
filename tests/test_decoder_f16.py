"""The decoder on plain f16 MFMA with half-precision activations (gdb_decoder_f16.hip, gdb_decode_f16, HotPathEngine.decode_f16,
`nerf.decoder_precision: f16`) against the numerical contract of DESIGN.md section 4.10.

Rule: an end-to-end bound cannot referee this kernel (flipped f16 roundings propagate: D below is three times E_acc, and a 2^-8 slip
of one layer's weights stays under 4 E_acc), so every layer is compared with a float64 referee fed the kernel's OWN stored inputs:
    |hip - ref64| <= 1/2 ulp16(max(|hip|, |ref64|)) + 4 E32        (one correct f16 rounding of an fp32 accumulation)
with E32 = max |the same layer in fp32 on the CPU - ref64|, floored at 8 fp32 ulp of max |ref64| (the project's 4x rule: the
reference arithmetic's own error, kernel not involved).  The fp32 final layer gets 4 E32 alone; a gate 4 x (the fp32-CPU gate's own
distance from the float64 gate), floored at 8 fp32 ulp; a trunk update 1/2 ulp16 + 2^-22 |ref|.  No element is excluded."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gdb_oracle as oracle
from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.engine import HotPathEngine
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder

F64 = torch.float64
CFG = lambda b=2, fd=16, vd=8: _lib.GdbConfig(b, 3, 1, 0, 64, 3, fd, vd, 64, 1)
KEYS = lambda n: (["in_conv.weight", "in_conv.bias"] + [f"blocks.{i}.{k}" for i in range(n) for k in (
    "conv1.weight", "conv2.weight", "conv3.weight", "se.fc.0.weight", "se.fc.2.weight")] + ["up.0.weight", "up.0.bias", "out_conv.weight", "out_conv.bias"])
CONV_BYTES = lambda nct, nks: nct * nks * 9 * 64 * 16
# (B, H, W, blocks): edges inside a tile and a row group, batch 2, both buffer parities, more than one workgroup per axis
CASES = [(1, 7, 33, 2), (2, 19, 45, 3), (1, 32, 48, 3), (1, 70, 130, 1), (1, 24, 40, 5), "F7"]
CASE_IDS = [c if isinstance(c, str) else "x".join(map(str, c)) for c in CASES]


def _lib_built():
    from gdb_nerf_amd import build
    build.build()
    return _lib.load()


def _f7_state():
    f7 = load_golden("F7_network")
    return {k[len("sd.upsampler."):]: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in f7.items() if k.startswith("sd.upsampler.")}


@functools.lru_cache(maxsize=None)
def _case(case):
    """(state dict of fp32 CPU tensors, x (B, 27, H, W) fp32, blocks)."""
    if case == "F7":
        return _f7_state(), torch.from_numpy(load_golden("F7_network")["dec_in"].astype(np.float32)), 3
    B, H, W, layers = case
    torch.manual_seed(3)
    dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=2).eval()
    with torch.no_grad():
        for p in dec.parameters():                                   # biases and gates that matter (tests/test_decoder.py)
            p.mul_(1.5)
    x = torch.randn(B, 27, H, W, generator=torch.Generator().manual_seed(7))
    return {k: v.detach().clone() for k, v in dec.state_dict().items()}, x, layers


def _fold64(sd):
    """out_conv o PixelShuffle(2) o up as one 64 -> 12 convolution in float64: channel 3 s + o of sub-pixel s = dy*2 + dx."""
    wup, bup = sd["up.0.weight"].to(F64), sd["up.0.bias"].to(F64)
    wout, bout = sd["out_conv.weight"].to(F64)[:, :, 0, 0], sd["out_conv.bias"].to(F64)
    w = torch.einsum("ok,ksctu->soctu", wout, wup.view(64, 4, 64, 3, 3)).reshape(12, 64, 3, 3)
    b = (torch.einsum("ok,ks->so", wout, bup.view(64, 4)) + bout[None]).reshape(12)
    return w, b


def _f16(t):
    """ONE rounding to f16, nearest even (torch casts float64 through float32 - two roundings, 2^-13 of all values land on the other
    side of a tie - numpy casts it directly)."""
    return torch.from_numpy(t.detach().numpy().astype(np.float16)) if t.dtype == F64 else t.to(torch.float16)


def _h(t):
    """One rounding to f16 (nearest even), value kept in t's dtype."""
    return _f16(t).to(t.dtype)


def _unshuffle(y):
    """(B, 12, H, W), channel 3 s + o -> (B, 3, 2H, 2W)."""
    B, _, H, W = y.shape
    return y.view(B, 2, 2, 3, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, 3, 2 * H, 2 * W)


def _weights(sd, layers, dtype):
    """The contract's weights: f16(w) (the folded up stage rounded once from float64), fp32 biases, as `dtype`."""
    wf, bf = _fold64(sd)
    w = {"in": _h(sd["in_conv.weight"]).to(dtype), "in_b": sd["in_conv.bias"].to(dtype),
         "up": _f16(wf).to(dtype), "up_b": bf.to(torch.float32).to(dtype)}
    for i in range(layers):
        for k in ("conv1", "conv2", "conv3"):
            w[f"{i}.{k}"] = _h(sd[f"blocks.{i}.{k}.weight"]).to(dtype)
        w[f"{i}.fc0"], w[f"{i}.fc2"] = sd[f"blocks.{i}.se.fc.0.weight"].to(dtype), sd[f"blocks.{i}.se.fc.2.weight"].to(dtype)
    return w


def _gate(c, w0, w2):
    return torch.sigmoid(F.linear(F.relu(F.linear(c.mean((2, 3)), w0)), w2))


def _emulate(sd, layers, x, dtype):
    """The contract in `dtype` arithmetic: every stored activation rounded once to f16, gates from the unrounded conv3."""
    w = _weights(sd, layers, dtype)
    conv = lambda t, k, b=None: F.conv2d(t, w[k], b, padding=1)
    shallow = trunk = _h(conv(_h(x.to(dtype)), "in", w["in_b"]))
    for i in range(layers):
        a1 = _h(F.relu(conv(trunk, f"{i}.conv1")))
        a2 = _h(F.relu(conv(torch.cat((trunk, a1), 1), f"{i}.conv2")))
        c = conv(torch.cat((trunk, a1, a2), 1), f"{i}.conv3")
        g = _gate(c, w[f"{i}.fc0"], w[f"{i}.fc2"]).to(torch.float32).to(dtype)   # (the gate is stored in fp32)
        trunk = _h(trunk + _h(c) * g[:, :, None, None])
    return _unshuffle(conv(_h(shallow + trunk), "up", w["up_b"]))


def _ref64(sd, layers, x):
    dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=2).to(F64).eval()
    dec.load_state_dict({k: v.to(F64) for k, v in sd.items()})
    with torch.no_grad():
        return dec(x.to(F64))


@functools.lru_cache(maxsize=None)
def _contract_sizes(case):
    """(ref64, D = max |emul64 - ref64|, E_acc = max |emul32 - emul64|): the contract's own size, kernel not involved."""
    sd, x, layers = _case(case)
    with torch.no_grad():
        ref, e64, e32 = _ref64(sd, layers, x), _emulate(sd, layers, x, F64), _emulate(sd, layers, x, torch.float32)
    return ref, float((e64 - ref).abs().max()), float((e32.to(F64) - e64).abs().max())


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def _unpack(buf, cout, cin, nct, nks):
    """Inverse of the A-fragment lane map of v_mfma_f32_16x16x32_f16: [tile][K-step][tap][lane][8 halves], element j of lane l =
    W[16 tile + (l & 15)][32 kstep + 8 (l >> 4) + j][tap]; everything beyond the layer's channels must be zero."""
    a = buf[:CONV_BYTES(nct, nks)].view(np.float16).reshape(nct, nks, 9, 64, 8)
    w = np.zeros((cout, cin, 9), np.float16)
    for t in range(nct):
        for ks in range(nks):
            for l in range(64):
                for j in range(8):
                    co, ci = 16 * t + (l & 15), 32 * ks + 8 * (l >> 4) + j
                    if co < cout and ci < cin:
                        w[co, ci] = a[t, ks, :, l, j]
                    else:
                        assert np.all(a[t, ks, :, l, j] == 0)
    return w.reshape(cout, cin, 3, 3)


def _offsets(layers):
    """Byte offsets of the packed buffer's sections (include/gdb_nerf_hip.h)."""
    off, o = {}, 0
    off["in"] = o; o += CONV_BYTES(4, 1)
    off["in_b"] = o; o += 256
    for i in range(layers):
        off[f"{i}.conv1"] = o; o += CONV_BYTES(2, 2)
        off[f"{i}.conv2"] = o; o += CONV_BYTES(2, 3)
        off[f"{i}.conv3"] = o; o += CONV_BYTES(4, 4)
        off[f"{i}.fc0"] = o; o += 1024
        off[f"{i}.fc2"] = o; o += 1024
    off["up"] = o; o += CONV_BYTES(1, 2)
    off["up_b"] = o; o += 256
    off["total"] = o
    return off


def test_f16_packing_is_a_permutation_of_the_rounded_weights():
    lib = _lib_built()
    sd, layers = _f7_state(), 3
    n = C.c_size_t()
    assert lib.gdb_decoder_f16_packed_bytes(C.byref(CFG()), layers, C.byref(n)) == 0
    off = _offsets(layers)
    assert n.value == off["total"]
    arrs = [np.ascontiguousarray(sd[k].numpy(), dtype=np.float32) for k in KEYS(layers)]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    host = np.full(n.value, 0xAB, np.uint8)
    assert lib.gdb_pack_decoder_weights_f16(C.byref(CFG()), layers, ptrs, host.ctypes.data) == 0
    f16 = lambda k: sd[k].numpy().astype(np.float16)
    assert np.array_equal(_unpack(host[off["in"]:], 64, 27, 4, 1), f16("in_conv.weight"))
    assert np.array_equal(host[off["in_b"]:off["in_b"] + 256].view(np.float32), sd["in_conv.bias"].numpy())
    for i in range(layers):
        assert np.array_equal(_unpack(host[off[f"{i}.conv1"]:], 32, 64, 2, 2), f16(f"blocks.{i}.conv1.weight"))
        assert np.array_equal(_unpack(host[off[f"{i}.conv2"]:], 32, 96, 2, 3), f16(f"blocks.{i}.conv2.weight"))
        assert np.array_equal(_unpack(host[off[f"{i}.conv3"]:], 64, 128, 4, 4), f16(f"blocks.{i}.conv3.weight"))
        assert np.array_equal(host[off[f"{i}.fc0"]:off[f"{i}.fc0"] + 1024].view(np.float32).reshape(4, 64), sd[f"blocks.{i}.se.fc.0.weight"].numpy())
        assert np.array_equal(host[off[f"{i}.fc2"]:off[f"{i}.fc2"] + 1024].view(np.float32).reshape(64, 4), sd[f"blocks.{i}.se.fc.2.weight"].numpy())
    # the folded up stage: the float64 fold reproduces the three modules at the fp32 form's 2e-6 relative bound BEFORE the f16 rounding,
    # and the packed fragment is that fold rounded once
    wf, bf = _fold64(sd)
    x = torch.randn(2, 64, 9, 11, generator=torch.Generator().manual_seed(0))
    want = F.conv2d(F.pixel_shuffle(F.conv2d(x, sd["up.0.weight"], sd["up.0.bias"], padding=1), 2), sd["out_conv.weight"], sd["out_conv.bias"])
    got = _unshuffle(F.conv2d(x, wf.float(), bf.float(), padding=1))
    assert max_abs(got.numpy(), want.numpy()) <= 2e-6 * float(want.abs().max())
    assert np.array_equal(_unpack(host[off["up"]:], 12, 64, 1, 2), _f16(wf).numpy())
    ub = host[off["up_b"]:off["up_b"] + 256].view(np.float32)
    assert np.array_equal(ub[:12], bf.float().numpy()) and np.all(ub[12:] == 0)


def test_f16_refusals_come_before_any_launch():
    """Host integers stand in for device pointers: a launch on them would fail, a refusal never gets there."""
    lib = _lib_built()
    f = _lib.GdbFrame()
    f.B, f.H, f.W = 1, 8, 40
    n, cnt, fake = C.c_size_t(), C.c_int32(), 0x1000
    need = C.c_size_t()
    assert lib.gdb_decoder_f16_workspace_bytes(C.byref(CFG()), C.byref(f), 3, 0, C.byref(need)) == 0
    keep = C.c_size_t()
    assert lib.gdb_decoder_f16_workspace_bytes(C.byref(CFG()), C.byref(f), 3, _lib.DECF16_KEEP_LAYERS, C.byref(keep)) == 0
    assert keep.value > need.value > 0
    dec = lambda cfg=CFG(), layers=3, feat=fake, ld=41, pk=fake, flags=0, ws=fake, nws=None, rgb=fake: lib.gdb_decode_f16(
        C.byref(cfg), C.byref(f), feat, ld, pk, layers, flags, ws, need.value if nws is None else nws, rgb, None)
    for b in (1, 4):
        assert dec(cfg=CFG(b)) == _lib.GDB_E_BADARG
        assert lib.gdb_decoder_f16_packed_bytes(C.byref(CFG(b)), 3, C.byref(n)) == _lib.GDB_E_BADARG
        assert lib.gdb_decoder_f16_workspace_bytes(C.byref(CFG(b)), C.byref(f), 3, 0, C.byref(n)) == _lib.GDB_E_BADARG
        assert lib.gdb_decoder_f16_layout(C.byref(CFG(b)), C.byref(f), 3, 0, None, 0, C.byref(cnt)) == _lib.GDB_E_BADARG
    for layers in (0, 17):
        assert dec(layers=layers) == _lib.GDB_E_BADARG
        assert lib.gdb_decoder_f16_packed_bytes(C.byref(CFG()), layers, C.byref(n)) == _lib.GDB_E_BADARG
    assert dec(cfg=CFG(2, 32, 8)) == _lib.GDB_E_BADARG and dec(cfg=CFG(2, 16, 4)) == _lib.GDB_E_BADARG
    assert dec(nws=need.value - 1) == _lib.GDB_E_WORKSPACE
    assert dec(flags=_lib.DECF16_KEEP_LAYERS) == _lib.GDB_E_WORKSPACE       # the keep-layers workspace is the larger one
    for kw in ("feat", "pk", "ws", "rgb"):
        assert dec(**{kw: None}) == _lib.GDB_E_BADARG, kw
    assert dec(ld=38) == _lib.GDB_E_SHAPE and dec(flags=2) == _lib.GDB_E_BADARG
    arrs = (C.c_void_p * 21)()
    assert lib.gdb_pack_decoder_weights_f16(C.byref(CFG()), 3, arrs, fake) == _lib.GDB_E_BADARG   # NULL tensors
    assert lib.gdb_decoder_f16_layout(C.byref(CFG()), C.byref(f), 3, 0, None, 0, C.byref(cnt)) == 0 and cnt.value == 5 * 3 + 2
    regs = (_lib.GdbDecF16Region * cnt.value)()
    assert lib.gdb_decoder_f16_layout(C.byref(CFG()), C.byref(f), 3, 0, C.cast(regs, C.c_void_p), cnt.value - 1, C.byref(cnt)) == _lib.GDB_E_BADARG
    assert lib.gdb_decoder_f16_layout(C.byref(CFG()), C.byref(f), 3, _lib.DECF16_KEEP_LAYERS, C.cast(regs, C.c_void_p), cnt.value, C.byref(cnt)) == 0
    names = [r.name.decode() for r in regs]
    assert names[:4] == ["trunk.0", "trunk.1", "trunk.2", "trunk.3"] and names[-1] == "residual" and "blocks.2.gate" in names
    spans = sorted((r.offset, r.offset + (f.B * f.H * f.W if r.per_pixel else f.B) * r.channels * (2 if r.dtype == 0 else 4)) for r in regs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= keep.value   # keep-layers: no two regions overlap
    # the existing entries keep refusing precision 0
    assert lib.gdb_decode(C.byref(CFG()), C.byref(f), fake, 41, fake, 3, 0, fake, 1 << 40, fake, None) == _lib.GDB_E_BADARG


@pytest.mark.parametrize("case", [(2, 19, 45, 3), (1, 7, 33, 2), (1, 40, 72, 5)], ids=["2x19x45x3", "1x7x33x2", "1x40x72x5"])
def test_the_contract_emulation_agrees_with_itself(case):
    """D = max |emul64 - ref64| is the contract's own size, E_acc = max |emul32 - emul64| what fp32 accumulation order adds (a third
    of D: flipped f16 roundings propagate).  Only `emul32 and emul64 agree within D` is asserted: a guard against a broken emulation."""
    ref, D, E_acc = _contract_sizes(case)
    sd, x, layers = _case(case)
    with torch.no_grad():
        dec = Decoder(27, 3, num_feats=64, num_layers=layers, upscale_factor=2).eval()
        dec.load_state_dict(sd)
        e_f32 = float((dec(x).to(F64) - ref).abs().max())
    print(f"[f16 contract] {case}: output scale {float(ref.abs().max()):.2f}  D {D:.3e}  E_acc {E_acc:.3e}  fp32 module {e_f32:.3e}")
    assert 0 < E_acc <= D and e_f32 < D


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _ulp16(v):
    v = np.abs(np.asarray(v, np.float64))
    e = np.full(v.shape, -14.0)
    np.floor(np.log2(v, where=v > 0, out=np.full(v.shape, -14.0)), out=e)
    return 2.0 ** (np.maximum(e, -14.0) - 10.0)


def _ulp32(v):
    return 2.0 ** (np.floor(np.log2(max(float(v), 2.0 ** -126))) - 23.0)


@functools.lru_cache(maxsize=None)
def _engine(case):
    sd, x, layers = _case(case)
    B, _, H, W = x.shape
    frame = synthetic.make_frame(2 * H, 2 * W, V=2, B=B, seed=1)
    eng = HotPathEngine()
    eng.prepare({k: torch.from_numpy(v).cuda() for k, v in frame.items()})
    eng.load_decoder_weights(sd, layers)
    bf = torch.zeros((B * H * W, 41))
    bf[:, 12:39] = x.permute(0, 2, 3, 1).reshape(B * H * W, 27)
    bf[:, :12] = 7.0                                                     # the fine-RGB channels (and depth / opacity) are not the decoder's
    return eng, bf.cuda().contiguous()


def _run_kept(case):
    """One keep-layers decode: (rgb_c, {region: CPU tensor, channel-first float64 for the activations})."""
    eng, bf = _engine(case)
    rgb = eng.decode_f16(bf, keep_layers=True).cpu()
    acts = {}
    for k, v in eng.decoder_f16_activations().items():
        v = v.cpu()
        acts[k] = v.to(F64) if v.dim() == 2 else v.permute(0, 3, 1, 2).to(F64)
    return rgb, acts


@functools.lru_cache(maxsize=None)
def _kept(case):
    return _run_kept(case)


def _check_layers(case, rgb, acts, only=None):
    """Every layer of one keep-layers decode against its float64 referee fed the kernel's own stored inputs:
    {layer: (max over elements of |hip - ref64| / bound, max |hip - ref64|)}; `only`: the layers to compute."""
    sd, x, layers = _case(case)
    w64, w32 = _weights(sd, layers, F64), _weights(sd, layers, torch.float32)
    out = {}

    def conv(name, key, src, hip, bias=None, relu=False, stored_f16=True):
        if only is not None and name not in only:
            return None, None
        b = lambda w: None if bias is None else w[bias]
        with torch.no_grad():
            r64 = F.conv2d(src, w64[key], b(w64), padding=1)
            r32 = F.conv2d(src.float(), w32[key], b(w32), padding=1)
            if relu:
                r64, r32 = F.relu(r64), F.relu(r32)
        ref, got = r64.numpy(), hip.numpy()
        e32 = max(max_abs(r32.numpy(), ref), 8 * _ulp32(np.abs(ref).max()))
        bound = 4 * e32 + (0.5 * _ulp16(np.maximum(np.abs(got), np.abs(ref))) if stored_f16 else 0.0)
        err = np.abs(got - ref)
        out[name] = (float((err / bound).max()), float(err.max()))
        return r64, r32

    def rounded(name, ref, hip):
        if only is not None and name not in only:
            return
        ref, got = ref.numpy(), hip.numpy()
        err = np.abs(got - ref)
        out[name] = (float((err / (0.5 * _ulp16(np.maximum(np.abs(got), np.abs(ref))) + 2.0 ** -22 * np.abs(ref))).max()), float(err.max()))

    conv("in_conv", "in", x.to(torch.float16).to(F64), acts["trunk.0"], bias="in_b")
    for i in range(layers):
        t, a1, a2, c = acts[f"trunk.{i}"], acts[f"blocks.{i}.conv1"], acts[f"blocks.{i}.conv2"], acts[f"blocks.{i}.conv3"]
        conv(f"blocks.{i}.conv1", f"{i}.conv1", t, a1, relu=True)
        conv(f"blocks.{i}.conv2", f"{i}.conv2", torch.cat((t, a1), 1), a2, relu=True)
        c64, c32 = conv(f"blocks.{i}.conv3", f"{i}.conv3", torch.cat((t, a1, a2), 1), c)
        g = acts[f"blocks.{i}.gate"]
        if only is None or f"blocks.{i}.gate" in only:
            if c64 is None:
                with torch.no_grad():
                    c64 = F.conv2d(torch.cat((t, a1, a2), 1), w64[f"{i}.conv3"], padding=1)
                    c32 = F.conv2d(torch.cat((t, a1, a2), 1).float(), w32[f"{i}.conv3"], padding=1)
            g64, g32 = _gate(c64, w64[f"{i}.fc0"], w64[f"{i}.fc2"]), _gate(c32, w32[f"{i}.fc0"], w32[f"{i}.fc2"])
            bound = max(4 * max_abs(g32.numpy(), g64.numpy()), 8 * _ulp32(float(g64.max())))
            err = max_abs(g.numpy(), g64.numpy())
            out[f"blocks.{i}.gate"] = (err / bound, err)
        rounded(f"trunk.{i + 1}", t + c * g[:, :, None, None], acts[f"trunk.{i + 1}"])
    rounded("residual", acts["trunk.0"] + acts[f"trunk.{layers}"], acts["residual"])
    if only is None or "up" in only:
        B, _, H, W = x.shape
        hip12 = rgb.to(F64).view(B, 3, H, 2, W, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 12, H, W)   # the inverse of _unshuffle
        conv("up", "up", acts["residual"], hip12, bias="up_b", stored_f16=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_layer_against_a_float64_referee_fed_the_kernels_own_inputs(case):
    rgb, acts = _kept(case)
    assert all(torch.isfinite(v).all() for v in acts.values()) and torch.isfinite(rgb).all()
    res = _check_layers(case, rgb, acts)
    sd, x, layers = _case(case)
    assert len(res) == 1 + 5 * layers + 2
    for k, (ratio, err) in res.items():
        print(f"[f16 decoder] {case} {k}: max |hip - ref64| {err:.3e}  observed / bound {ratio:.3f}")
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 19, 45, 3), "F7"], ids=["2x19x45x3", "F7"])
def test_a_slip_of_one_layer_is_seen(case):
    """One layer's packed f16 weights x (1 + 2^-8) on the device - 4 f16 ulp, eight times the rounding term - must break that layer's
    bound of the test above; so must the gate's fc.2 weight x (1 + 2^-8)."""
    eng, bf = _engine(case)
    _kept(case)                                                          # (packs the weights)
    sd, x, layers = _case(case)
    off = _offsets(layers)
    good = eng.dec_weights_f16.clone()
    try:
        for layer, key, nbytes, dt in (("blocks.1.conv2", "1.conv2", CONV_BYTES(2, 3), torch.float16), ("in_conv", "in", CONV_BYTES(4, 1), torch.float16),
                                      ("up", "up", CONV_BYTES(1, 2), torch.float16), ("blocks.0.gate", "0.fc2", 1024, torch.float32)):
            eng.dec_weights_f16.copy_(good)
            sec = eng.dec_weights_f16[off[key]:off[key] + nbytes].view(dt)
            sec.copy_((sec.float() * (1 + 2.0 ** -8)).to(dt))
            rgb, acts = _run_kept(case)
            ratio, err = _check_layers(case, rgb, acts, only=(layer,))[layer]
            print(f"[f16 decoder] {case} slip of {layer}: observed / bound {ratio:.2f}")
            assert ratio > 1.0, layer
    finally:
        eng.dec_weights_f16.copy_(good)
    rgb, acts = _run_kept(case)
    assert torch.equal(rgb, _kept(case)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_end_to_end_within_the_contracts_own_size(case):
    ref, D, E_acc = _contract_sizes(case)
    rgb, _ = _kept(case)
    e = max_abs(rgb.numpy(), ref.numpy())
    msg = f"[f16 decoder] {case} end to end: max |hip - ref64| {e:.3e}  D {D:.3e}  E_acc {E_acc:.3e}  bound {D + 4 * E_acc:.3e}"
    if case == "F7":
        msg += f"  max |hip - the fixture's dec_out| {max_abs(rgb.numpy(), load_golden('F7_network')['dec_out']):.3e}"
    print(msg)
    assert e <= D + 4 * E_acc


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 19, 45, 3), (1, 24, 40, 5), (1, 70, 130, 1)], ids=["2x19x45x3", "1x24x40x5", "1x70x130x1"])
def test_keep_layers_determinism_and_workspace_contents(case):
    eng, bf = _engine(case)
    want = _kept(case)[0]
    for keep in (False, True):
        a = eng.decode_f16(bf, keep_layers=keep).clone()
        assert torch.equal(a.cpu(), want) and torch.equal(eng.decode_f16(bf, keep_layers=keep), a)
        eng._dec_ws_f16.view(torch.float16).fill_(float("nan"))
        assert torch.equal(eng.decode_f16(bf, keep_layers=keep), a)
        eng._dec_ws_f16.fill_(0xFF)
        assert torch.equal(eng.decode_f16(bf, keep_layers=keep), a)
    with pytest.raises(ValueError, match="bundle_feat"):
        eng.decode_f16(bf[:-1])
    with pytest.raises(ValueError, match="precision"):                   # the existing entry keeps refusing precision 0
        eng.decode(bf, precision=0)


def _f7_net(opts):
    f7 = load_golden("F7_network")
    net = make_network(make_cfg(str(f7["yaml"]) if "yaml" in f7 else "configs/dtu_eval.yaml", opts)).eval()
    net.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v, dtype=np.float32) if v.dtype == np.float16 else v) for k, v in f7.items() if k.startswith("sd.")},
                        strict=True)
    return net


def test_network_refuses_the_f16_decoder_where_it_does_not_run():
    for opts, match in ((["nerf.bundle_size", "4"], "bundle_size 2"), (["nerf.hip_decoder", "False"], "hip_decoder"),
                        (["nerf.shard", "tiles"], "row windows"), (["nerf.decoder_precision", "f32"], "'auto' or 'f16'")):
        opts = (["nerf.decoder_precision", "f16"] if "nerf.decoder_precision" not in opts else []) + opts
        with pytest.raises(ValueError, match=match):
            make_network(make_cfg("configs/dtu_eval.yaml", opts))
    assert make_network(make_cfg("configs/dtu_eval.yaml", [])).decoder_precision == "auto"


@pytest.mark.gpu
def test_network_forward_with_the_f16_decoder():
    fx = load_golden("F7_network")
    tt = lambda k: torch.from_numpy(fx[k].astype(np.float32) if k == "src_images" else fx[k]).cuda()
    batch = {"src_views": {"rgb": tt("src_images"), "extrinsics": tt("src_exts"), "intrinsics": tt("src_ints")},
             "tar_views": {"extrinsics": tt("tar_ext"), "intrinsics": tt("tar_int")}, "near_far": tt("near_far")}
    imgs = {}
    for name, opts in (("absent", []), ("auto", ["nerf.decoder_precision", "auto"]), ("f16", ["nerf.decoder_precision", "f16"])):
        net = _f7_net(opts).cuda()
        with torch.no_grad():
            imgs[name] = net(batch)[0]["rgb"].cpu()
    assert torch.equal(imgs["absent"], imgs["auto"])                    # without the key: today's choice, bit for bit
    assert max_abs(imgs["absent"].numpy(), fx["rgb"]) <= 5e-4
    H, W = fx["rgb"].shape[2:]
    hwc = lambda t: np.transpose(np.asarray(t[0]), (1, 2, 0))
    gt = np.clip(hwc(fx["rgb"]) + np.random.default_rng(1).normal(0, 0.03, (H, W, 3)), 0, 1)
    d_psnr = abs(oracle.psnr(gt, hwc(imgs["f16"].numpy())) - oracle.psnr(gt, hwc(imgs["absent"].numpy())))
    print(f"[f16 decoder] Network.forward (F7): max |f16 - fp32 path| {max_abs(imgs['f16'].numpy(), imgs['absent'].numpy()):.3e}  |dPSNR| {d_psnr:.4f} dB")
    assert d_psnr <= 0.05

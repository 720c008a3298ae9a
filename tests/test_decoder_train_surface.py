"""The surface of the decoder's training mode: the host-only entries (queries, refusals), the fold's backward
restated in numpy against float64 autograd, and - on the GPU - `nerf.hip_decoder_train` in `Network`.

Tolerances of the Network comparison (switch on against switch off, same weights, same batch) are derived, not chosen.  Both arms hand
the decoder the same bundle rows and the same upstream (the loss is rgb.sum()), so the decoder's float64 CPU referee on those rows
(tests/test_decoder_train_referee.py) bounds either arm's distance from the truth by the rule 4 * max(E32, 8 ulp32(max |ref64|)); two
results inside one bound differ by at most twice it.  The `nerf.*` gradients are a linear map J of the row gradient: the arms' row
gradients differ by some D (bounded as above), so their `nerf.*` gradients must differ by J D, which autograd evaluates on the
switch-off arm's own graph; what is left is the fp32 rounding of two sums of the gradient's size, allowed the rule's floor,
4 * 8 ulp32(max |any nerf.* gradient|): the summands' size, see the helper."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gdb_nerf_amd import _lib, synthetic
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder

ENTRIES = ("gdb_decoder_train_packed_floats", "gdb_decoder_train_pack", "gdb_decoder_train_saved_bytes", "gdb_decoder_train_layout",
           "gdb_decoder_train_forward", "gdb_decoder_train_backward_bytes", "gdb_decoder_train_backward")


def _cfg(bundle=2):
    return _lib.GdbConfig(bundle, 3, 1, 0, 64, 3, 16, 8, 64, 1)


def _frame(B, H, W):
    f = _lib.GdbFrame()
    f.B, f.H, f.W = B, H, W
    return f


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 0.0


# ---- host only -----------------------------------------------------------------------------------------------------------------------
def test_entries_are_exported_and_declared():
    lib = _lib.load()
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib.HERE), "include", "gdb_nerf_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None and f"int {name}(" in header, name
    assert lib.gdb_abi_version() == 7


def test_size_and_layout_queries():
    lib, cfg = _lib.load(), _cfg()
    n1, n3 = C.c_size_t(), C.c_size_t()
    _lib.check(lib.gdb_decoder_train_packed_floats(C.byref(cfg), 1, C.byref(n1)))
    _lib.check(lib.gdb_decoder_train_packed_floats(C.byref(cfg), 3, C.byref(n3)))
    fwd = lambda L: 2 * 9216 + 64 + L * (13 * 9216 + 512) + 2 * 9216 + 32        # the fp32 sections of the eval-mode buffer
    bwd = lambda L: 2 * 9216 + L * (4 * 9216 + 4 * 9216 + 2 * 9216 + 9216 + 2 * 9216) + 2 * 9216   # the data-gradient forms
    for L, n in ((1, n1), (3, n3)):
        assert n.value % 64 == 0 and n.value >= fwd(L) + 1024 + bwd(L) + 1024
    B, H, W, L = 2, 5, 36, 3
    f, sb, wb, cnt = _frame(B, H, W), C.c_size_t(), C.c_size_t(), C.c_int32()
    _lib.check(lib.gdb_decoder_train_saved_bytes(C.byref(cfg), C.byref(f), L, C.byref(sb)))
    _lib.check(lib.gdb_decoder_train_backward_bytes(C.byref(cfg), C.byref(f), L, C.byref(wb)))
    _lib.check(lib.gdb_decoder_train_layout(C.byref(cfg), C.byref(f), L, None, 0, C.byref(cnt)))
    assert cnt.value == 4 * L + 3
    regs = (_lib.GdbDecRegion * cnt.value)()
    _lib.check(lib.gdb_decoder_train_layout(C.byref(cfg), C.byref(f), L, C.cast(regs, C.c_void_p), cnt.value, C.byref(cnt)))
    names = [r.name.decode() for r in regs]
    assert names == [f"{k}.{b}" for b in range(L) for k in ("x", "ab", "T", "gate")] + ["xu", "part", "part2"]
    end = 0
    for r in regs:   # in order, 256-byte aligned, not overlapping, inside the buffer
        assert r.offset % 256 == 0 and r.offset >= end and r.offset + r.bytes <= sb.value
        end = r.offset + r.bytes
        shape = tuple(d for d in r.shape if d)
        assert shape == ((B, 64) if r.name.startswith(b"gate") else (B, H, 2, 64) if r.name == b"part" else (B, 1, 64) if r.name == b"part2"
                         else (B, H, W, 64)), (r.name, shape)
        assert r.bytes == 4 * int(np.prod(shape))
    assert wb.value >= 8 * 4 * B * H * W * 64
    with pytest.raises(ValueError, match="capacity"):
        _lib.check(lib.gdb_decoder_train_layout(C.byref(cfg), C.byref(f), L, C.cast(regs, C.c_void_p), 3, C.byref(cnt)))


def test_refusals():
    lib, n, f = _lib.load(), C.c_size_t(), _frame(1, 4, 4)
    one = (C.c_void_p * 11)(*([1] * 11))
    with pytest.raises(ValueError, match="bundle_size 2.*got 4"):
        _lib.check(lib.gdb_decoder_train_packed_floats(C.byref(_cfg(4)), 3, C.byref(n)))
    for L in (0, 17):
        with pytest.raises(ValueError, match=f"layers {L} outside 1..16"):
            _lib.check(lib.gdb_decoder_train_saved_bytes(C.byref(_cfg()), C.byref(f), L, C.byref(n)))
    for prec in (_lib.PREC_F16, _lib.PREC_F32X):
        with pytest.raises(ValueError, match=f"fp32 only.*got {prec}"):
            _lib.check(lib.gdb_decoder_train_pack(C.byref(_cfg()), 1, prec, one, 1, 1 << 30, None))
        with pytest.raises(ValueError, match="fp32 only"):
            _lib.check(lib.gdb_decoder_train_forward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, prec, 1, 1 << 40, 1, None))
        with pytest.raises(ValueError, match="fp32 only"):
            _lib.check(lib.gdb_decoder_train_backward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, prec, one, 1, 1 << 40, 1, 1, 1 << 40, None, None, 0, None))
    with pytest.raises(ValueError, match="batch 257 > 256"):
        _lib.check(lib.gdb_decoder_train_saved_bytes(C.byref(_cfg()), C.byref(_frame(257, 4, 4)), 1, C.byref(n)))
    with pytest.raises(ValueError, match="batch 257 > 256"):
        _lib.check(lib.gdb_decoder_train_backward_bytes(C.byref(_cfg()), C.byref(_frame(257, 4, 4)), 1, C.byref(n)))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(lib.gdb_decoder_train_packed_floats(C.byref(_cfg()), 1, None))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(lib.gdb_decoder_train_pack(C.byref(_cfg()), 1, _lib.PREC_F32, None, 1, 1 << 30, None))
    with pytest.raises(ValueError, match="tensor 3 is NULL"):
        _lib.check(lib.gdb_decoder_train_pack(C.byref(_cfg()), 1, _lib.PREC_F32, (C.c_void_p * 11)(1, 1, 1, None, 1, 1, 1, 1, 1, 1, 1), 1, 1 << 30, None))
    with pytest.raises(_lib.GdbError, match="packed buffer"):
        _lib.check(lib.gdb_decoder_train_pack(C.byref(_cfg()), 1, _lib.PREC_F32, one, 1, 16, None))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(lib.gdb_decoder_train_forward(C.byref(_cfg()), C.byref(f), None, 39, 1, 1, _lib.PREC_F32, 1, 1 << 40, 1, None))
    with pytest.raises(ValueError, match="row stride 38 < 39"):
        _lib.check(lib.gdb_decoder_train_forward(C.byref(_cfg()), C.byref(f), 1, 38, 1, 1, _lib.PREC_F32, 1, 1 << 40, 1, None))
    with pytest.raises(_lib.GdbError, match="saved buffer"):
        _lib.check(lib.gdb_decoder_train_forward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, _lib.PREC_F32, 1, 16, 1, None))
    with pytest.raises(ValueError, match="NULL"):
        _lib.check(lib.gdb_decoder_train_backward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, _lib.PREC_F32, one, 1, 1 << 40, None, 1, 1 << 40, None, None, 0, None))
    with pytest.raises(ValueError, match="row-gradient stride 38 < 39"):
        _lib.check(lib.gdb_decoder_train_backward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, _lib.PREC_F32, one, 1, 1 << 40, 1, 1, 1 << 40, None, 1, 38, None))
    with pytest.raises(_lib.GdbError, match="backward workspace"):
        _lib.check(lib.gdb_decoder_train_backward(C.byref(_cfg()), C.byref(f), 1, 39, 1, 1, _lib.PREC_F32, one, 1, 1 << 40, 1, 1, 16, None, None, 0, None))


def fold_backward(dWf, dbf, up_w, up_b, out_w):
    """The fold's backward of DESIGN.md 4.23 (k_dect_fold_back) in numpy float64: dWf (12, 64, 9), dbf (12), up_w (256, 64, 9), up_b (256),
    out_w (3, 64) -> d up_w, d up_b, d out_w, d out_b.  Folded channel 3 s + o, up channel 4 m + s."""
    dW4, up4 = dWf.reshape(4, 3, 64, 9), up_w.reshape(64, 4, 64, 9)           # [s][o][ci][tap], [m][s][ci][tap]
    db4, ub4 = dbf.reshape(4, 3), up_b.reshape(64, 4)
    d_up_w = np.einsum("om,sock->msck", out_w, dW4).reshape(256, 64, 9)
    d_up_b = np.einsum("om,so->ms", out_w, db4).reshape(256)
    d_out_w = np.einsum("sock,msck->om", dW4, up4) + np.einsum("so,ms->om", db4, ub4)
    return d_up_w, d_up_b, d_out_w, db4.sum(0)


def fold_backward_swapped(dWf, dbf, up_w, up_b, out_w):
    """The slip tests/test_decoder_train_slips.py keeps as a control: the folded channel read as 4 o + s instead of 3 s + o."""
    dW4, up4 = dWf.reshape(3, 4, 64, 9).transpose(1, 0, 2, 3), up_w.reshape(64, 4, 64, 9)
    db4, ub4 = dbf.reshape(3, 4).T, up_b.reshape(64, 4)
    d_up_w = np.einsum("om,sock->msck", out_w, dW4).reshape(256, 64, 9)
    d_up_b = np.einsum("om,so->ms", out_w, db4).reshape(256)
    d_out_w = np.einsum("sock,msck->om", dW4, up4) + np.einsum("so,ms->om", db4, ub4)
    return d_up_w, d_up_b, d_out_w, db4.sum(0)


def fold_case(seed=0, H=3, W=5):
    """float64: the unfused up -> PixelShuffle -> out_conv under autograd, and dWf / dbf of the folded 64 -> 12 convolution."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, up_w, up_b, out_w, out_b, gy = r(2, 64, H, W), r(256, 64, 3, 3) * 0.05, r(256), r(3, 64, 1, 1) * 0.2, r(3), r(2, 3, 2 * H, 2 * W)
    ps = [t.requires_grad_(True) for t in (up_w, up_b, out_w, out_b)]
    y = F.conv2d(F.pixel_shuffle(F.conv2d(x, ps[0], ps[1], padding=1), 2), ps[2], ps[3])
    want = torch.autograd.grad((y * gy).sum(), ps)
    # the folded layer's own gradients: g12[b][3 s + o][y][x] = gy[b][o][2y + (s >> 1)][2x + (s & 1)], dWf = conv weight gradient, dbf = column sums
    g12 = gy.reshape(2, 3, H, 2, W, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 12, H, W)
    wf = torch.zeros(12, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    dWf = torch.autograd.grad((F.conv2d(x, wf, padding=1) * g12).sum(), wf)[0]
    return ([t.detach().numpy() for t in want], dWf.numpy().reshape(12, 64, 9), g12.sum((0, 2, 3)).numpy(),
            up_w.detach().numpy().reshape(256, 64, 9), up_b.detach().numpy(), out_w.detach().numpy().reshape(3, 64))


def test_fold_backward_formulas_against_float64_autograd():
    want, dWf, dbf, up_w, up_b, out_w = fold_case()
    got = fold_backward(dWf, dbf, up_w, up_b, out_w)
    for w, g, name in zip(want, got, ("up.0.weight", "up.0.bias", "out_conv.weight", "out_conv.bias")):
        w = w.reshape(g.shape)
        assert np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), name   # float64 against float64: rounding of a few thousand terms


def test_switch_is_refused_where_it_cannot_work():
    base = ["nerf.hip_decoder_train", "True"]
    with pytest.raises(ValueError, match="hip_decoder_train needs nerf.hot_path 'mirrors'.*'fused'"):
        make_network(make_cfg("configs/dtu_eval.yaml", base + ["nerf.hot_path", "fused"]))
    with pytest.raises(ValueError, match="hip_decoder_train needs nerf.hot_path 'mirrors'"):
        make_network(make_cfg("configs/dtu_eval.yaml", base))
    with pytest.raises(ValueError, match=r"bundle_size 2 \(got 4\)"):
        make_network(make_cfg("configs/dtu_eval.yaml", base + ["nerf.hot_path", "mirrors", "nerf.bundle_size", "4"]))
    with pytest.raises(ValueError, match=r"dec_layers 1..16 \(got 17\)"):
        make_network(make_cfg("configs/dtu_eval.yaml", base + ["nerf.hot_path", "mirrors", "nerf.dec_layers", "17"]))
    for y in ("dtu_eval.yaml", "dtu_pretrain.yaml", "llff_eval.yaml", "nerf_eval.yaml"):
        assert not getattr(make_cfg("configs/" + y).nerf, "hip_decoder_train", False)
    assert make_network(make_cfg("configs/dtu_eval.yaml", ["nerf.hot_path", "mirrors"])).hip_decoder_train is False


# ---- Network, on the GPU -------------------------------------------------------------------------------------------------------------
MIRRORS = ["nerf.hot_path", "mirrors", "nerf.hip_decoder", "False"]


def _batch():
    fr = synthetic.make_frame(32, 64, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
            "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}


def _net(*opts, seed=109):
    torch.manual_seed(seed)
    return make_network(make_cfg("configs/dtu_eval.yaml", MIRRORS + list(opts))).cuda()


def _step(net, batch, retain=False):
    """One forward + backward of rgb.sum(): (rgb, bundle rows, their gradient, {name: grad})."""
    seen = {}
    inner = net.render_bundles

    def render_bundles(*a):
        f, d, o = inner(*a)
        seen["rows"] = f
        f.register_hook(lambda g: seen.__setitem__("g_rows", g.detach().clone()))
        return f, d, o

    net.render_bundles = render_bundles
    net.zero_grad()
    rgb = net(batch)[0]["rgb"]
    rgb.sum().backward(retain_graph=retain)
    net.render_bundles = inner
    return rgb.detach(), seen["rows"], seen["g_rows"], {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _rule_bounds(net, rows, rgb_shape):
    """The decoder's float64 CPU referee on the rows a forward handed it, upstream = ones (the loss is rgb.sum()):
    ({tensor: ref64}, {tensor: 4 * max(E32, 8 ulp32(max |ref64|))}) for every parameter gradient, "rows" and "rgb_c"."""
    from test_decoder_train_referee import _autograd, _observe
    B, _, Ho, Wo = rgb_shape
    H, W = Ho // 2, Wo // 2
    x = rows.detach().cpu()[:, 12:39].reshape(B, H, W, 27).permute(0, 3, 1, 2).contiguous()
    m = copy.deepcopy(net.upsampler).cpu()
    ones = torch.ones(B, 3, Ho, Wo)
    r32, r64 = _autograd(copy.deepcopy(m), x, ones), _autograd(copy.deepcopy(m).double(), x.double(), ones.double())
    with torch.no_grad():
        r32["rgb_c"], r64["rgb_c"] = _observe(m, x)["rgb_c"], _observe(copy.deepcopy(m).double(), x.double())["rgb_c"]
    return r64, {k: 4 * max(float((r32[k].double() - r64[k]).abs().max()), 8 * _ulp32(float(r64[k].abs().max()))) for k in r64}


def _arms_within_the_rule(net0, res0, res1, r64, bound, hip_arm):
    """Two arms on the same rows (res = _step's tuple; res0 from net0 with its graph retained): `upsampler.*`, the row gradient and
    rgb within twice the rule's bound of each other (both obey it; the HIP arm is also held to the bound itself), and the `nerf.*`
    gradients apart by J D, the linear map of the row-gradient difference, up to the rule's floor."""
    from test_decoder_train_referee import PARAM_NAMES
    (rgb0, rows0, grow0, g0), (rgb1, rows1, grow1, g1) = res0, res1
    assert torch.equal(rows0, rows1)                                          # the decoder's input is the same in both arms
    assert set(g0) == set(g1) and all(k.startswith(("nerf.", "upsampler.")) for k in g1)
    assert {k for k in g1 if k.startswith("upsampler.")} == {"upsampler." + k for k in PARAM_NAMES(net0.dec_layers)}
    for k in PARAM_NAMES(net0.dec_layers):
        d = float((g1["upsampler." + k] - g0["upsampler." + k]).abs().max())
        print(f"upsampler.{k}: arm 1 - arm 0 {d:.3e}, 2 x rule bound {2 * bound[k]:.3e}")
        if hip_arm:
            assert float((g1["upsampler." + k].cpu().double() - r64[k]).abs().max()) <= bound[k], k     # the rule itself, for the HIP arm
        assert d <= 2 * bound[k], k
    # the decoder's part of the row gradient (columns 12 .. 38; rgb_f's columns are autograd's in both arms)
    D = grow1 - grow0
    assert not D[:, :12].any()
    if hip_arm:
        assert float((grow1[:, 12:].cpu().double() - r64["rows"]).abs().max()) <= bound["rows"]
    assert float(D.abs().max()) <= 2 * bound["rows"]
    # nerf.*: linear in the row gradient
    names = [k for k in g0 if k.startswith("nerf.")]
    JD = torch.autograd.grad(rows0, [dict(net0.named_parameters())[k] for k in names], grad_outputs=D, allow_unused=True, retain_graph=True)
    scale = max(float(g0[k].abs().max()) for k in names)
    for k, jd in zip(names, JD):
        jd = torch.zeros_like(g0[k]) if jd is None else jd
        left = float((g1[k] - g0[k] - jd).abs().max())
        # the floor follows the size of the SUMMANDS, not of the result: every nerf.* gradient adds, over the same samples, products of
        # the same upstream row gradients with O(1) activations and weights, and several cancel almost entirely (agg_w_fc.0.bias: the
        # view softmax's score gradients sum to zero; sigma.0.*, weight.2.bias: the normalised composite's weights sum to one -
        # DESIGN.md 4.14), so their rounding noise is that of the summands.  The largest nerf.* gradient measures the summands' size.
        size = scale
        floor = 4 * 8 * _ulp32(size)
        print(f"{k}: |arm 1 - arm 0 - J D| {left:.3e}, floor {floor:.3e}, |J D| {float(jd.abs().max()):.3e}")
        assert left <= floor, k
    assert float((rgb1 - rgb0).abs().max()) <= 2 * bound["rgb_c"]


@pytest.mark.gpu
def test_network_switch_on_against_switch_off():
    batch = _batch()
    off, on = _net().train(), _net("nerf.hip_decoder_train", "True").train()
    on.load_state_dict(off.state_dict())
    res0, res1 = _step(off, batch, retain=True), _step(on, batch)
    assert on._decoder_train is not None and on._decoder_train.forwards == 1 and off._decoder_train is None
    r64, bound = _rule_bounds(off, res0[1], res0[0].shape)
    _arms_within_the_rule(off, res0, res1, r64, bound, hip_arm=True)


REPRODUCIBILITY = __import__("os").path.join(__import__("os").path.dirname(_lib.HERE), "profiles", "decoder_train", "module_path_reproducibility.txt")


@pytest.mark.gpu
def test_switch_off_and_eval_mode_are_the_parents_path(monkeypatch):
    """Switch absent, switch False, and switch True in eval mode or under no_grad: the PyTorch module decodes and the HIP training
    path is never built or called; the decoder's input is bit-identical everywhere.  Outputs and gradients are compared at the
    strength the module path itself has: each configuration first runs the SAME switch-absent network twice; where those two runs
    are bit-identical, the other arm must be bit-identical too (decoder output, rgb, row gradient, every gradient); where they are
    not - the convolution library under the PyTorch decoder does not promise run-to-run bits - the figures are recorded
    (profiles/decoder_train/module_path_reproducibility.txt) and the arms are held to the bound derived from the referee rule, as in
    test_network_switch_on_against_switch_off: nothing is left uncompared."""
    from gdb_nerf_amd import decoder_train

    def never(*a, **k):
        raise AssertionError("DecodeTrainFunction ran")

    monkeypatch.setattr(decoder_train.DecodeTrainFunction, "apply", never)
    batch = _batch()
    absent, false, on = _net(), _net("nerf.hip_decoder_train", "False"), _net("nerf.hip_decoder_train", "True")
    false.load_state_dict(absent.state_dict())
    on.load_state_dict(absent.state_dict())
    seen = {}
    for name, net in (("absent", absent), ("false", false), ("on", on)):
        net.upsampler.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, (inp[0].detach().clone(), out.detach().clone())))
    record = ["# configuration: two runs of the SAME switch-absent network in one process - max |difference| of the decoder's output, of rgb"
              " (and, with a backward, of the row gradient and of any gradient); 0 everywhere = bit-identical"]

    def run(net, name, mode, grad):
        getattr(net, mode)()
        if grad:
            res = _step(net, batch, retain=True)
        else:
            with torch.no_grad():
                res = (net(batch)[0]["rgb"].detach(), None, None, {})
        return seen[name] + (res,)   # (decoder input, decoder output, (rgb, rows, row gradient, gradients))

    def apart(a, b):
        (xa, ya, (rgba, _, growa, ga)), (xb, yb, (rgbb, _, growb, gb)) = a, b
        assert torch.equal(xa, xb) and set(ga) == set(gb)                     # the decoder's input: bit-identical, always
        d = {"decoder out": float((ya - yb).abs().max()), "rgb": float((rgba - rgbb).abs().max())}
        if growa is not None:
            d["row gradient"] = float((growa - growb).abs().max())
            d["gradients"] = max(float((ga[k] - gb[k]).abs().max()) for k in ga)
        return d

    # the switch on, where it does not apply (eval mode with grad mode on, eval mode under no_grad, train mode under no_grad), and
    # the switch False in train mode with a backward; train mode last: it moves the running statistics, which only eval mode reads
    for other, oname, mode, grad in ((on, "on", "eval", True), (on, "on", "eval", False), (on, "on", "train", False), (false, "false", "train", True)):
        a0, a1, o = run(absent, "absent", mode, grad), run(absent, "absent", mode, grad), run(other, oname, mode, grad)
        own, cross = apart(a0, a1), apart(a1, o)
        record.append(f"{mode} mode, {'grad mode on, backward' if grad else 'no_grad'}: same network twice {own}; switch {oname} against absent {cross}")
        print(record[-1])
        __import__("os").makedirs(__import__("os").path.dirname(REPRODUCIBILITY), exist_ok=True)
        with open(REPRODUCIBILITY, "w") as f:   # (after every configuration: the figures are evidence whether or not the comparison below holds)
            f.write("\n".join(record) + "\n")
        if not any(own.values()):
            assert not any(cross.values()), (mode, grad, cross)
            continue
        r64, bound = _rule_bounds(absent, a1[2][1], a1[2][0].shape) if grad else (None, None)
        if grad:
            _arms_within_the_rule(absent, a1[2], o[2], r64, bound, hip_arm=False)
        else:   # no rows captured under no_grad: the decoder's own input gives the same referee
            from test_decoder_train_referee import _observe
            m, x = copy.deepcopy(absent.upsampler).cpu(), a1[0].cpu()
            with torch.no_grad():
                c32, c64 = _observe(m, x)["rgb_c"], _observe(copy.deepcopy(m).double(), x.double())["rgb_c"]
            bound = {"rgb_c": 4 * max(float((c32.double() - c64).abs().max()), 8 * _ulp32(float(c64.abs().max())))}
        assert cross["decoder out"] <= 2 * bound["rgb_c"] and cross["rgb"] <= 2 * bound["rgb_c"], (mode, grad, cross, bound["rgb_c"])
    assert on._decoder_train is None and absent._decoder_train is None and false._decoder_train is None


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["HipAdam", "torch.optim.Adam"])
def test_an_optimiser_step_reaches_the_next_forwards_pack(which):
    from gdb_nerf_amd.optim import HipAdam
    batch = _batch()
    net = _net("nerf.hip_decoder_train", "True").train()
    _step(net, batch)
    params = [p for p in net.parameters() if p.grad is not None]
    opt = HipAdam(params, lr=1e-3) if which == "HipAdam" else torch.optim.Adam(params, lr=1e-3)
    before = [p.detach().clone() for p in net.upsampler.parameters()]
    opt.step()
    assert all(not torch.equal(a, b) for a, b in zip(before, net.upsampler.parameters()))
    rgb = net(batch)[0]["rgb"].detach()
    assert net._decoder_train.packs == 2 and net._decoder_train.forwards == 2
    fresh = _net("nerf.hip_decoder_train", "True").train()
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(rgb, fresh(batch)[0]["rgb"].detach()) and fresh._decoder_train.packs == 1

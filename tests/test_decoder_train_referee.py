"""The decoder in TRAINING mode on the HIP library (gdb_decoder_train.hip, decoder_train.DecoderTrain): the
device-side weight pack, the saved-activation forward and the backward.

Bit identities (no referee needed):
  * the device pack's fp32 sections equal gdb_pack_decoder_weights' output byte for byte (the fold of the last up stage included);
  * the training forward's rgb_c equals gdb_decode at fp32 on every case, and on the F7 shape;
  * forward + backward run twice give bit-identical outputs and gradients (run at the multi-slab case).

Referee: `copy.deepcopy(Decoder(27, 3, 64, L, 2)).double()` on the CPU under autograd, on the float64 copies of the fp32 input and of a
fixed upstream g, loss = sum(rgb_c * g).  E32 = the error of the fp32 CPU module against it, per observation point and per gradient
tensor: what the reference ARITHMETIC loses; the kernel is never involved in a bound.
Rule, everywhere: max |hip - ref64| <= 4 * max(E32, 8 ulp32(max |ref64|)) - the rule of tests/test_cost_reg_train_referee.py.
Observation points.  Forward, read by name from the saved buffer (gdb_decoder_train_layout): shallow (x.0), every block's a and b
(ab.<b>), T (T.<b>), gate (gate.<b>) and x_{b+1} (x.<b+1>; the last block's through xu = x_L + shallow), and rgb_c.  Backward: every
parameter gradient and the bundle-row gradient (columns 12 .. 38; 0 .. 11 must be zero, sentinels behind column 38 must survive).

Cases (B, H, W, L): one pixel; one partial tile; one pixel past the 32-pixel tile with an odd row count; the exact tile at batch 2; two
full tiles; batch 3; more blocks than the eval path's rotating buffers; the recipe's three blocks at the W = 36 tile tail; a row stride
above Q with sentinels behind column 38; an all-zero upstream; only the rows requiring grad; only the parameters requiring grad; and
(1, 34, 3, 1), the multi-slab case: the weight gradient's plan (dect_dw_plan, gdb_decoder_train_index.h: slabs = min(rows, 256,
ceil(8192 / (tiles * tap groups))); nine taps per wave for conv3's 32 tiles, three for every other layer) gives every layer 34 slabs
of one row - more than one slab per tile and more partials than the first reduction level's fan-in of 16; its 102 pixels are two
groups of the squeeze-excitation and bias sums (DECT_PG = 64 pixels each; every case above one pixel row has several).  (2, 129, 2, 1) has 258 image rows, more than the plan's 256 slabs: a wave walks two rows, and slab
64 holds the last row of item 0 and the first of item 1; its 258 pixels per item are five groups of the pixel sums, two of their
second level (DECT_R2 = 4).  The multi-slab case is not
(1, 70, 70, 1): 313,600 pre-activations never all clear the kink margin below, and slabs are rows, so a narrow tall map reaches the
same paths.  (1, 70, 70, 1) stays as a forward-only case: 210 segments are two groups (DEC_SEG = 128) of the forward's gate sums.

ReLU kinks: a conv1 / conv2 output, or a hidden unit of a squeeze-excitation (k_dect_se takes its ReLU' from h = fc.0 mean(T) formed
again in double, the forward's gate from fp32), within rounding of zero has two valid fp32 gradients, so no element may sit there and
nothing is excluded.  Per case, on the CPU before any kernel runs (test_cases_are_clear_of_relu_kinks): the float64 run's smallest
|conv1 / conv2 output| and smallest |hidden unit| per block exceed twice that tensor's forward bound (the rule applied to the
pre-activation), and the fp32 CPU masks equal the float64 ones.  The seeds in CASES were searched on the CPU for it.

Observed error / bound per (case, tensor): profiles/decoder_train/referee_observed.txt, rewritten by a GPU run of this file."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from gdb_nerf_amd import _lib
from gdb_nerf_amd.decoder_train import DecoderTrain, decoder_params
from gdb_nerf_amd.engine import HotPathEngine
from gdb_nerf_amd.networks.gdb_nerf.decoder_rdn import Decoder

K_RULE = 4.0
Q = 39
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "decoder_train", "referee_observed.txt")

def _case(B, H, W, L, seed, ld=Q, zero_g=False, rows_grad=True, param_grad=True, backward=True):
    return dict(B=B, H=H, W=W, L=L, seed=seed, ld=ld, zero_g=zero_g, rows_grad=rows_grad, param_grad=param_grad, backward=backward)


CASES = {
    "1x1x1-L1": _case(1, 1, 1, 1, 0),
    "1x3x5-L1": _case(1, 3, 5, 1, 0),
    "1x7x33-L2": _case(1, 7, 33, 2, 1),
    "2x4x32-L1": _case(2, 4, 32, 1, 0),
    "1x2x64-L1": _case(1, 2, 64, 1, 0),
    "3x3x17-L2": _case(3, 3, 17, 2, 2),
    "1x4x8-L4": _case(1, 4, 8, 4, 0),
    "1x5x36-L3": _case(1, 5, 36, 3, 1),
    "1x5x36-L3-ld44": _case(1, 5, 36, 3, 1, ld=44),
    "1x3x5-L1-zero-upstream": _case(1, 3, 5, 1, 0, zero_g=True),
    "3x3x17-L2-rows-only": _case(3, 3, 17, 2, 2, param_grad=False),
    "1x7x33-L2-params-only": _case(1, 7, 33, 2, 1, rows_grad=False),
    "1x34x3-L1-multi-slab": _case(1, 34, 3, 1, 0),
    "2x129x2-L1-slab-across-items": _case(2, 129, 2, 1, 0),
    "1x70x70-L1-two-groups": _case(1, 70, 70, 1, 0, backward=False),   # forward only: 313,600 pre-activations cannot all clear a kink margin
}
BACKWARD_IDS = [k for k, c in CASES.items() if c["backward"]]
CASE_IDS = list(CASES)
SENTINEL = 12345.0


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 0.0


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(module fp32 on the CPU, rows (N, ld) fp32 with sentinels behind column Q - 1)."""
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    torch.manual_seed(seed)
    m = Decoder(27, 3, 64, L, 2)
    rows = torch.full((B * H * W, ld), SENTINEL)
    rows[:, :Q] = torch.randn(B * H * W, Q, generator=torch.Generator().manual_seed(100 + seed))
    return m, rows


def _observe(m, x):
    """The module's forward in x's dtype with every observation point kept."""
    keep = {}
    shallow = trunk = keep["x.0"] = m.in_conv(x)
    L = len(m.blocks)
    for i, blk in enumerate(m.blocks):
        a = F.relu(keep.setdefault(f"pre1.{i}", blk.conv1(trunk)))
        b = F.relu(keep.setdefault(f"pre2.{i}", blk.conv2(torch.cat((trunk, a), 1))))
        keep[f"ab.{i}"] = torch.cat((a, b), 1)
        t = keep[f"T.{i}"] = blk.conv3(torch.cat((trunk, a, b), 1))
        keep[f"preh.{i}"] = blk.se.fc[0](t.mean((2, 3)))          # the squeeze-excitation's hidden units before their ReLU
        g = keep[f"gate.{i}"] = blk.se.fc(t.mean((2, 3)))
        trunk = trunk + t * g[:, :, None, None]
        if i + 1 < L:
            keep[f"x.{i + 1}"] = trunk
    keep["xu"] = shallow + trunk
    keep["rgb_c"] = m.out_conv(m.up(keep["xu"]))
    return keep


@functools.lru_cache(maxsize=None)
def _referee(name):
    """{point: (ref64 numpy, bound)}: float64 module against the fp32 CPU module, kernel not involved."""
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    m, rows = _setup(name)
    x = rows[:, 12:Q].reshape(B, H, W, 27).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        k32, k64 = _observe(m, x), _observe(copy.deepcopy(m).double(), x.double())
    out = {}
    for key, r in k64.items():
        e32 = float((k32[key].double() - r).abs().max())
        out[key] = (r.numpy(), K_RULE * max(e32, 8 * _ulp32(float(r.abs().max()))))
    return out


_observed = {}


def _record(case, tensor, err, bound):
    _observed[(case, tensor)] = (err, bound)
    os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
    with open(OBSERVED, "w") as f:
        f.write("# case tensor max|hip-ref64| bound ratio   (rule: 4 * max(E32, 8 ulp32(max|ref64|)); tests/test_decoder_train_referee.py)\n")
        for (c, t), (e, b) in _observed.items():
            f.write(f"{c} {t} {e:.3e} {b:.3e} {e / b if b else 0.0:.3f}\n")


def _host_pack(m):
    """gdb_pack_decoder_weights of the module's values: (numpy buffer, engine with it loaded)."""
    L = len(m.blocks)
    eng = HotPathEngine(device="cuda:0")
    eng.load_decoder_weights({k: v.detach() for k, v in m.state_dict().items()}, L)
    return eng


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("layers", [1, 3, 16])
def test_device_pack_equals_host_pack_bytes(layers):
    torch.manual_seed(layers)
    m = Decoder(27, 3, 64, layers, 2)
    eng = _host_pack(m)
    dt = DecoderTrain(copy.deepcopy(m).cuda())
    dev = dt.pack().cpu().numpy()
    host = eng.dec_weights.cpu().numpy()
    # the fp32 sections (dec_layout, gdb_decoder_layout.h): in_conv, its bias, five tensors per block, the folded stage and its bias
    fp32_floats = 2 * 9216 + 64 + layers * (2 * 9216 + 3 * 9216 + 4 * 2 * 9216 + 512) + 2 * 9216 + 32
    assert dev.size - fp32_floats >= 8 * 128                      # the tap block the weight prefetch runs into
    assert dev[:fp32_floats].tobytes() == host[:fp32_floats].tobytes()
    assert not dev[fp32_floats:fp32_floats + 8 * 128].any()
    assert np.abs(dev[:fp32_floats]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_forward_bits_and_layers(name):
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    m, rows = _setup(name)
    dt = DecoderTrain(copy.deepcopy(m).cuda())
    d_rows = rows.cuda()
    rgb = dt.forward(d_rows, B, H, W)
    # bit identity with the eval-mode decode on the host-packed weights
    eng = _host_pack(m)
    ref_bits = _eval_decode(eng, d_rows, B, H, W, L)
    assert torch.equal(rgb, ref_bits)
    assert torch.equal(d_rows.cpu(), rows)                       # the rows, sentinels included, are read only
    acts = {k: v.cpu() for k, v in dt.activations().items()}
    acts["rgb_c"] = rgb.cpu()
    for key, (ref, bound) in _referee(name).items():
        if key.startswith("pre"):   # the pre-activations are the kink check's, the kernels store what follows the ReLU
            continue
        got = acts[key].double().numpy()
        got = got if key.startswith("gate") or key == "rgb_c" else np.transpose(got, (0, 3, 1, 2))
        err = float(np.abs(got - ref).max())
        print(f"{name} {key}: {err:.3e} / {bound:.3e}")
        _record(name, key, err, bound)
        assert err <= bound, (name, key, err, bound)


def _eval_decode(eng, d_rows, B, H, W, L):
    """gdb_decode at fp32 on the engine's host-packed weights, for a bare (B, H, W) bundle map."""
    lib, f, need = _lib.load(), _lib.GdbFrame(), C.c_size_t()
    f.B, f.H, f.W = B, H, W
    _lib.check(lib.gdb_decoder_workspace_bytes(C.byref(eng.cfg), C.byref(f), C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda:0")
    out = torch.empty((B, 3, 2 * H, 2 * W), device="cuda:0")
    _lib.check(lib.gdb_decode(C.byref(eng.cfg), C.byref(f), d_rows.data_ptr(), int(d_rows.stride(0)), eng.dec_weights.data_ptr(), L, _lib.PREC_F32,
                              ws.data_ptr(), need.value, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.gpu
def test_forward_bits_at_the_f7_shape():
    f7 = load_golden("F7_network")
    sd = {k[len("sd.upsampler."):]: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in f7.items() if k.startswith("sd.upsampler.")}
    x = torch.from_numpy(f7["dec_in"].astype(np.float32))
    B, _, H, W = x.shape
    m = Decoder(27, 3, 64, 3, 2)
    m.load_state_dict(sd)
    rows = torch.zeros(B * H * W, Q)
    rows[:, 12:] = x.permute(0, 2, 3, 1).reshape(-1, 27)
    d_rows = rows.cuda()
    rgb = DecoderTrain(copy.deepcopy(m).cuda()).forward(d_rows, B, H, W)
    assert torch.equal(rgb, _eval_decode(_host_pack(m), d_rows, B, H, W, 3))
    assert rgb.abs().max() > 0


# ---- the backward -------------------------------------------------------------------------------------------------------------------
def _upstream(name):
    c = CASES[name]
    shape = (c["B"], 3, 2 * c["H"], 2 * c["W"])
    return torch.zeros(shape) if c["zero_g"] else torch.randn(shape, generator=torch.Generator().manual_seed(200 + c["seed"]))


PARAM_NAMES = lambda L: (["in_conv.weight", "in_conv.bias"] + [f"blocks.{b}.{k}" for b in range(L) for k in
                         ("conv1.weight", "conv2.weight", "conv3.weight", "se.fc.0.weight", "se.fc.2.weight")]
                         + ["up.0.weight", "up.0.bias", "out_conv.weight", "out_conv.bias"])


def _autograd(m, x, g):
    """{tensor name: gradient} of loss = sum(m(x) * g) in x's dtype: every parameter (state-dict order) and "rows" (N_b, 27)."""
    x = x.clone().requires_grad_(True)
    m.zero_grad()
    (m(x) * g).sum().backward()
    out = {k: p.grad.detach().clone() for k, p in zip(PARAM_NAMES(len(m.blocks)), decoder_params(m))}
    out["rows"] = x.grad.permute(0, 2, 3, 1).reshape(-1, 27)
    return out


@functools.lru_cache(maxsize=None)
def _grad_referee(name):
    """{tensor: (ref64 numpy, bound)} for the backward, kernel not involved."""
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    m, rows = _setup(name)
    x = rows[:, 12:Q].reshape(B, H, W, 27).permute(0, 3, 1, 2).contiguous()
    g = _upstream(name)
    g32, g64 = _autograd(copy.deepcopy(m), x, g), _autograd(copy.deepcopy(m).double(), x.double(), g.double())
    out = {}
    for key, r in g64.items():
        e32 = float((g32[key].double() - r).abs().max())
        out[key] = (r.numpy(), K_RULE * max(e32, 8 * _ulp32(float(r.abs().max()))))
    return out


def kink_margins(name):
    """Per conv1 / conv2 layer of the case: (smallest |pre-activation| of the float64 run, that layer's forward bound, masks equal)."""
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    m, rows = _setup(name)
    x = rows[:, 12:Q].reshape(B, H, W, 27).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        k32, k64 = _observe(m, x), _observe(copy.deepcopy(m).double(), x.double())
    ref = _referee(name)
    return {key: (float(k64[key].abs().min()), ref[key][1], bool(torch.equal(k32[key] > 0, k64[key] > 0))) for key in k64 if key.startswith("pre")}


@pytest.mark.parametrize("name", BACKWARD_IDS)
def test_cases_are_clear_of_relu_kinks(name):
    for key, (smallest, bound, same) in kink_margins(name).items():
        assert smallest > 2 * bound, (name, key, smallest, bound)
        assert same, (name, key)


def _run_backward(name, dt=None):
    """(rgb_c, g_rows or None, [parameter gradients or None]) of one forward + backward on the GPU; sentinels behind column 38 of g_rows."""
    c = CASES[name]
    B, H, W, L, ld = c["B"], c["H"], c["W"], c["L"], c["ld"]
    m, rows = _setup(name)
    dt = DecoderTrain(copy.deepcopy(m).cuda()) if dt is None else dt
    d_rows = rows.cuda()
    rgb = dt.forward(d_rows, B, H, W)
    n = 2 + 5 * L + 4
    g_rows = torch.full((B * H * W, ld), SENTINEL, device="cuda:0") if c["rows_grad"] else None
    g_rows, grads = dt.backward(d_rows, _upstream(name).cuda(), want_params=[c["param_grad"]] * n, want_rows=c["rows_grad"], g_rows=g_rows)
    return rgb, g_rows, grads


@pytest.mark.gpu
@pytest.mark.parametrize("name", BACKWARD_IDS)
def test_backward_against_float64(name):
    c = CASES[name]
    rgb, g_rows, grads = _run_backward(name)
    ref = _grad_referee(name)
    got = {}
    if c["rows_grad"]:
        gr = g_rows.cpu()
        assert not gr[:, :12].any()                                 # rgb_f's columns: zero, autograd adds its own
        assert c["ld"] == Q or bool((gr[:, Q:] == SENTINEL).all())   # columns from 39 on are left alone
        got["rows"] = gr[:, 12:Q]
    else:
        assert g_rows is None
    for k, g in zip(PARAM_NAMES(c["L"]), grads):
        assert (g is not None) == c["param_grad"]
        if g is not None:
            got[k] = g.cpu()
    assert got
    for key, t in got.items():
        r, bound = ref[key]
        assert tuple(t.shape) == r.shape, (key, t.shape, r.shape)
        err = float(np.abs(t.double().numpy() - r).max())
        print(f"{name} grad {key}: {err:.3e} / {bound:.3e}")
        _record(name, "grad." + key, err, bound)
    for key, t in got.items():
        r, bound = ref[key]
        assert float(np.abs(t.double().numpy() - r).max()) <= bound, (name, key)


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    name = "1x34x3-L1-multi-slab"
    runs = []
    for _ in range(2):
        m, _rows = _setup(name)
        dt = DecoderTrain(copy.deepcopy(m).cuda())
        rgb, g_rows, grads = _run_backward(name, dt)
        runs.append((dt.packed.clone(), rgb.clone(), g_rows.clone(), [g.clone() for g in grads], {k: v.clone() for k, v in dt.activations().items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    for a, b in zip(runs[0][3], runs[1][3]):
        assert torch.equal(a, b)
    for k in runs[0][4]:
        assert torch.equal(runs[0][4][k], runs[1][4][k]), k


@pytest.mark.gpu
def test_repack_follows_the_parameters_version():
    """An in-place update (what an optimiser step is) bumps `_version`: the next forward packs again, and equals a fresh pack."""
    name = "1x3x5-L1"
    B, H, W, L, seed, ld = (CASES[name][k] for k in ("B", "H", "W", "L", "seed", "ld"))
    m, rows = _setup(name)
    mod = copy.deepcopy(m).cuda()
    dt = DecoderTrain(mod)
    d_rows = rows.cuda()
    a = dt.forward(d_rows, B, H, W).clone()
    dt.forward(d_rows, B, H, W)
    assert dt.packs == 1
    opt = torch.optim.Adam(decoder_params(mod), lr=1e-2)
    for p in decoder_params(mod):
        p.grad = torch.ones_like(p)
    opt.step()
    b = dt.forward(d_rows, B, H, W)
    assert dt.packs == 2 and not torch.equal(a, b)
    assert torch.equal(b, DecoderTrain(copy.deepcopy(mod)).forward(d_rows, B, H, W))

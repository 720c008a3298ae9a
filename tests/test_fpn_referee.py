"""Every layer of the feature pyramid network (gdb_fpn.hip, fpn.FeaturePyramid) against a float64 referee, on every kind of channel
plan gdb_fpn accepts.

Observation points: the caller owns the workspace, and after gdb_fpn returns it still holds the channel-last intermediates (layout:
include/gdb_nerf_hip.h, restated in _regions): A (conv0.0), F0 (conv0), T1 / H1 (conv1.0 / conv1), T2 / Q (conv2.0 / conv2),
I1 = interpolate(Q) + inner1(H1), I2 = interpolate(I1) + inner2(F0), and the levels L0 / L1 / L2.  With level 2 in the mask A lives
in I2's space and is overwritten, so one run at mask 3 and one at mask 7 on the same input show every layer's input and output;
what the two runs have in common is asserted bit-identical, so they are one computation.

Referee: every layer is checked on the kernel's OWN stored fp32 input (the decoder referee's form), so no
layer hides behind the rounding of the layers before it.  ref64_k is the repo's own FeatureNet sub-module, copy.deepcopy(m).double(),
on the float64 copy of that stored input (a conv_block2d in eval mode, a 1 x 1 lateral + F.interpolate(top, size, "nearest"), or a
head).  E_ref_k = max |the fp32 CPU sub-module on that same stored input - ref64_k|: what the reference ARITHMETIC loses there; the
kernel takes no part in it.  The fp32 module is pinned to fixture F7's feat_l1 first, and the float64 upsample's source index to
the index the kernel restates, so the referee is tied to the reference and not only to itself.
Rule at every point: max |hip_k - ref64_k| <= max(K_RULE * E_ref_k, 8 ulp32(max |ref64_k|)), K_RULE = 4 as for the cost volume and
the U-Nets (tests/test_cost_reg_referee.py): kernel and module are two realisations (another order of the tap products, another
BatchNorm formula) of one fp32 computation, whose maximum error over 1e1 .. 1e5 elements moves by a small factor between
realisations, while a wrong tap, statistic, border or source index errs by the activations themselves.  No element is excluded
(cap 0, asserted).  End to end the existing form of tests/test_fpn.py is kept: every level within 5e-6 of max(1, max |ref|) of the
float64 module on the image (the alternative, summed per-layer bounds times the layers' gains, was not chosen: the per-layer
points are the sharp check, and the old form stays comparable with the old suite).

Every GPU case has a CPU half (inputs, referee, E_ref, what the case claims) under -m "not gpu", where the fp32 CPU chain stands in
for the kernel's stored activations; the slips at the end show on the CPU alone that the rule catches a subtly wrong layer at that
layer's own point."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, fpn
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from test_fpn import _fpn, _layers, _pack, _state_dict

K_RULE = 4.0
EXCLUDED_CAP = 0          # every element of every point is compared
EPS = 1e-5
N = 2
SMALL = 1e-3

# ---- the plans, the shapes and what each is there for ------------------------------------------------------------------------
PLANS = {
    "P1": (8, (32, 16, 8)),     # the configured plan
    "P2": (8, (8, 8, 16)),      # 8-row out0 (half a tile at ks = 1), two-row out1 at half resolution, one-row out2
    "P3": (16, (64, 24, 40)),   # 27-k conv0.0, E = 4 everywhere, inner2 at E = 4, four-tile out0, partial tiles 24 and 40
    "P4": (24, (16, 8, 24)),    # E = 2 with K = 3, cout 24 / 48 / 96: partial and six-tile layers
    "P5": (32, (32, 16, 8)),    # K up to 8, cout 128
}
# the layers whose last 16-row tile is partial (GEMM rows = zs x cout)
PARTIAL = {"P1": set(), "P2": {"out0"}, "P3": {"out1", "out2"}, "P4": {"conv0.0", "conv0.1", "out2"}, "P5": set()}
# (H, W): the fp_nearest branch of (Q -> H1, I1 -> F0) along y and along x, and the number of 32-column tiles at full resolution
SHAPES = {
    (1, 1): dict(y=("equal", "equal"), x=("equal", "equal"), nct=1),
    (1, 40): dict(y=("equal", "equal"), x=("double", "double"), nct=2),
    (2, 3): dict(y=("equal", "double"), x=("double", "general"), nct=1),
    (8, 64): dict(y=("double", "double"), x=("double", "double"), nct=2),
    (9, 17): dict(y=("general", "general"), x=("general", "general"), nct=1),
    (6, 34): dict(y=("general", "double"), x=("general", "double"), nct=2),
    (5, 33): dict(y=("general", "general"), x=("general", "general"), nct=2),
    (37, 70): dict(y=("general", "general"), x=("general", "double"), nct=3),
}
FAMILY_SHAPES = ((9, 17), (8, 64))      # the exact and the small-operand families
CASES = [(p, "random", s) for p in PLANS for s in SHAPES] + [(p, f, s) for p in PLANS for f in ("exact", "small") for s in FAMILY_SHAPES]
CASE_IDS = [f"{p}-{f}-{s[0]}x{s[1]}" for p, f, s in CASES]
ALL = pytest.mark.parametrize("case", CASES, ids=CASE_IDS)

# observation point: (layer, the points it reads); a lateral reads (top, skip)
POINTS = {"A": ("conv0.0", ("img",)), "F0": ("conv0.1", ("A",)), "T1": ("conv1.0", ("F0",)), "H1": ("conv1.1", ("T1",)),
          "T2": ("conv2.0", ("H1",)), "Q": ("conv2.1", ("T2",)), "L0": ("out0", ("Q",)), "I1": ("inner1", ("Q", "H1")),
          "L1": ("out1", ("I1",)), "I2": ("inner2", ("I1", "F0")), "L2": ("out2", ("I2",))}
LEVELS = ("L0", "L1", "L2")


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 0.0


def _sub(m, layer):
    mod = m
    for part in layer.split("."):
        mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
    return mod


def _conv_of(m, layer):
    mod = _sub(m, layer)
    return mod[0] if isinstance(mod, torch.nn.Sequential) else mod


def _apply(m, point, src):
    """Layer `point` of FeatureNet `m` (any dtype) on its stored inputs: FeatureNet.forward's own expressions, one at a time."""
    layer, reads = POINTS[point]
    with torch.no_grad():
        if len(reads) == 2:
            top, skip = src[reads[0]], src[reads[1]]
            return F.interpolate(top, size=skip.shape[-2:], mode="nearest") + _sub(m, layer)(skip)
        return _sub(m, layer)(src[reads[0]])


def _chain(m, x, replace=None):
    """All observation points of one forward, layer by layer; `replace` = {point: function of the stored inputs} for the slips."""
    st = {"img": x}
    for p in POINTS:
        st[p] = replace[p](st) if replace and p in replace else _apply(m, p, st)
    return st


# ---- the geometry restated --------------------------------------------------------------------------------------------------
def _dims(H, W):
    h, w = (H + 1) // 2, (W + 1) // 2
    return [(H, W), (h, w), ((h + 1) // 2, (w + 1) // 2)]


def _nearest(dst, n_in, n_out):
    """fp_nearest restated: (source index, branch)."""
    if n_in == n_out:
        return dst, "equal"
    if n_out == 2 * n_in:
        return dst >> 1, "double"
    scale = np.float32(n_in) / np.float32(n_out)
    return min(int(np.floor(np.float32(dst) * scale)), n_in - 1), "general"


def _regions(c, H, W, mask):
    """The workspace after gdb_fpn(level_mask = mask), restated: {region: (offset in floats, (N, h, w, channels))} and the total.
    Order A, F0, T1, H1, T2, Q, I1, I2, each rounded up to 64 floats; I1 only with level 1 or 2, I2 only with level 2, and with
    level 2 A has no region of its own (it is written into I2's space and overwritten by inner2)."""
    d = _dims(H, W)
    spec = [("A", 0, c, not mask & 4), ("F0", 0, c, True), ("T1", 1, 2 * c, True), ("H1", 1, 2 * c, True), ("T2", 2, 4 * c, True),
            ("Q", 2, 4 * c, True), ("I1", 1, 4 * c, bool(mask & 6)), ("I2", 0, 4 * c, bool(mask & 4))]
    out, o = {}, 0
    for name, lvl, ch, present in spec:
        if present:
            shape = (N, d[lvl][0], d[lvl][1], ch)
            out[name] = (o, shape)
            o += (int(np.prod(shape)) + 63) // 64 * 64
    return out, o


def _dispatch_keys(c, outs):
    """fp_layer's dispatch key (IMG, ZS, E, EPI) of every launch of a plan, extended with what changes the work inside one
    instantiation: more than one row tile, a partial last tile, more than one k-chunk, three or more row tiles."""
    keys = {}
    for L in _layers(c, outs)[0]:
        epi = "BN" if L["kind"] == "bn" else "LAT" if L["name"].startswith("inner") else "OUT"
        nmt = (L["rows"] + 15) // 16
        keys[L["name"]] = (L["name"] == "conv0.0", L["zs"], L["E"], epi, nmt > 1, L["rows"] % 16 != 0, L["K"] > 1, nmt >= 3)
    return keys


# ---- modules and inputs -----------------------------------------------------------------------------------------------------
def _bns(m):
    return [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]


LAYERS = [POINTS[p][0] for p in POINTS]
DYADIC = (0.25, 0.5, -0.25, 0.125, 0.0, 0.375, -0.125)


def _exact_module(m, which):
    """Identity BatchNorm (mean 0, var 1 - eps, weight 1) with dyadic biases, dyadic lateral / out0 biases, and sparse +-1 weights:
    output channel co of layer li takes tap (co + which * cout + li) mod ks^2 with +1 - two cases of >= 8 channels walk through
    all 9, two of >= 16 through all 25 - then a second +1 and a -1 at random taps.  With inputs that are multiples of 2^-3 every
    partial sum is a small multiple of 2^-3: nothing rounds in fp32, whatever the order."""
    rng = np.random.default_rng(40 + which)
    taps = {}
    with torch.no_grad():
        for k, bn in enumerate(_bns(m)):
            bn.running_mean.zero_(); bn.running_var.fill_(1.0 - EPS); bn.weight.fill_(1.0)
            bn.bias.copy_(torch.tensor([DYADIC[(3 * i + k) % len(DYADIC)] for i in range(bn.bias.numel())]))
        for li, layer in enumerate(LAYERS):
            conv = _conv_of(m, layer)
            w = conv.weight
            w.zero_()
            cout, cin, ks, _ = w.shape
            used = set()
            for co in range(cout):
                for k in range(3):
                    tap = (co + which * cout + li) % (ks * ks) if k == 0 else int(rng.integers(0, ks * ks))
                    w[co, (3 * co + 5 * k + li) % cin].view(-1)[tap] = -1.0 if k == 2 else 1.0
                    used.add(tap)
            taps[layer] = used
            if conv.bias is not None:
                conv.bias.copy_(torch.tensor([DYADIC[(2 * i + li) % len(DYADIC)] for i in range(cout)]))
    return taps


def _layer_outputs(m, x):
    rec, hooks = {}, []
    for layer in LAYERS:
        hooks.append(_sub(m, layer).register_forward_hook(lambda _m, _i, out, layer=layer: rec.__setitem__(layer, out.detach())))
    try:
        with torch.no_grad():
            m(x)
    finally:
        for h in hooks:
            h.remove()
    return rec


def _small_module(m, x):
    """Activations of order 1e-3: the BatchNorm means and biases and the convolutions' biases times 2^-10, then every convolution's
    weights times a power of two of its own (exact in fp32) so that each layer's float64 output on `x` has max| | about 1e-3."""
    with torch.no_grad():
        for bn in _bns(m):
            bn.running_mean.mul_(2.0 ** -10); bn.bias.mul_(2.0 ** -10)
        for layer in LAYERS:
            if _conv_of(m, layer).bias is not None:
                _conv_of(m, layer).bias.mul_(2.0 ** -10)
    m64 = copy.deepcopy(m).double()
    for layer in LAYERS:
        for _ in range(3):                     # BatchNorm's mean and bias make the output affine, not linear, in the factor
            top = float(_layer_outputs(m64, x.double())[layer].abs().max())
            if top == 0:
                break
            with torch.no_grad():
                _conv_of(m64, layer).weight.mul_(2.0 ** round(math.log2(SMALL / top)))
    with torch.no_grad():
        for layer in LAYERS:
            _conv_of(m, layer).weight.copy_(_conv_of(m64, layer).weight.float())
            assert torch.equal(_conv_of(m, layer).weight.double(), _conv_of(m64, layer).weight)
    return m


@functools.lru_cache(maxsize=None)
def _case(case):
    """The fp32 module, its float64 copy, the image and the float64 module's levels on the image (the end-to-end reference)."""
    plan, family, (H, W) = case
    c, outs = PLANS[plan]
    seed = 1000 * list(PLANS).index(plan) + 10 * H + W
    m = _fpn(c, outs, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.rand(N, 3, H, W, generator=g) * 2.0 - 0.5
    taps = None
    if family == "exact":
        x = torch.randint(-4, 13, (N, 3, H, W), generator=g).float() / 8.0
        taps = _exact_module(m, FAMILY_SHAPES.index((H, W)))
    elif family == "small":
        x = x * 2.0 ** -10
        _small_module(m, x)
    m64 = copy.deepcopy(m).double()
    if family == "exact":      # the identity BatchNorm that fp32 realises exactly (test_bn_identity_is_exact), written down exactly
        for bn in _bns(m64):
            bn.running_var.fill_(1.0)
            bn.eps = 2.0 ** -60      # (1 + 2^-60 is 1 in float64; PyTorch refuses an eps of 0)
    with torch.no_grad():
        e2e = [t.numpy() for t in m64(x.double())]
    return dict(case=case, c=c, outs=outs, H=H, W=W, family=family, m=m, m64=m64, x=x, e2e=e2e, taps=taps)


def _judge(r, stored, got=None):
    """Every layer on the stored fp32 activations `stored` ({point: (N, C, h, w) tensor}, the image included): per point ref64,
    E_ref, the floor, the bound, and the error of got[point] (default: the stored output itself)."""
    got = stored if got is None else got
    st64 = {k: v.double() for k, v in stored.items()}
    out = {}
    for p in POINTS:
        ref64 = _apply(r["m64"], p, st64)
        cpu32 = _apply(r["m"], p, stored)
        assert ref64.dtype == torch.float64 and cpu32.dtype == torch.float32 and ref64.shape == got[p].shape, p
        e_ref = float((cpu32.double() - ref64).abs().max())
        top = float(ref64.abs().max())
        floor = 8 * _ulp32(top)
        bound = floor if r["family"] == "exact" else max(K_RULE * e_ref, floor)     # exact cases are held to bit equality besides
        err = float((got[p].double() - ref64).abs().max())          # every element: nothing is excluded
        out[p] = dict(ref64=ref64, e_ref=e_ref, top=top, floor=floor, bound=bound, err=err, excluded=0)
    return out


def _e2e(levels, r):
    """The end-to-end form of tests/test_fpn.py: max |level - float64 module| / max(1, max |ref|) per level."""
    return [float(np.abs(np.asarray(g, np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max())) for g, ref in zip(levels, r["e2e"])]


@functools.lru_cache(maxsize=None)
def _cpu_half(case):
    r = _case(case)
    stored = _chain(r["m"], r["x"])
    return r, stored, _judge(r, stored)


# ---- CPU: the referee is tied to the reference ------------------------------------------------------------------------------
def test_fp32_module_is_pinned_to_f7():
    """The fp32 CPU FeatureNet reproduces F7's feat_l1 under the bound of test_network_surface.py, its float64 copy is a refinement
    of the same thing, and the layer-by-layer chain of this file IS the module's forward (bit for bit, in both types)."""
    f7 = load_golden("F7_network")
    net = make_network(make_cfg("configs/dtu_eval.yaml")).eval()
    net.load_state_dict(_state_dict(f7), strict=True)
    m = net.feature_net
    src = torch.from_numpy(f7["src_images"]).float().flatten(0, 1)
    with torch.no_grad():
        out = m(src)
    assert max_abs(out[1].numpy(), f7["feat_l1"]) <= 1e-5
    st = _chain(m, src)
    assert all(torch.equal(st[k], o) for k, o in zip(LEVELS, out))
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        out64 = m64(src.double())
    assert out64[1].dtype == torch.float64 and max_abs(out64[1].numpy(), f7["feat_l1"]) <= 1e-5
    st64 = _chain(m64, src.double())
    assert all(torch.equal(st64[k], o) for k, o in zip(LEVELS, out64))


def test_float64_upsample_takes_the_restated_source_index():
    """F.interpolate(size=, mode="nearest") on a float64 tensor reads source index min(floor(float32(dst) * float32(in / out)), in - 1)
    - the index itself at equal sizes, dst >> 1 at twice the size - along both axes: every out in 1 .. 200 with in = ceil(out / 2)
    (each top-down step) and in == out."""
    seen = set()
    for n_out in range(1, 201):
        for n_in in {(n_out + 1) // 2, n_out}:
            want = [_nearest(d, n_in, n_out) for d in range(n_out)]
            seen |= {b for _, b in want}
            idx = torch.tensor([i for i, _ in want], dtype=torch.float64)
            ramp = torch.arange(n_in, dtype=torch.float64)
            rows = F.interpolate(ramp.view(1, 1, n_in, 1).expand(1, 1, n_in, 3).contiguous(), size=(n_out, 5), mode="nearest")
            cols = F.interpolate(ramp.view(1, 1, 1, n_in).expand(1, 1, 3, n_in).contiguous(), size=(5, n_out), mode="nearest")
            assert torch.equal(rows[0, 0, :, 0], idx) and torch.equal(rows[0, 0, :, 4], idx), (n_in, n_out)
            assert torch.equal(cols[0, 0, 0, :], idx) and torch.equal(cols[0, 0, 4, :], idx), (n_in, n_out)
            rows32 = F.interpolate(ramp.float().view(1, 1, n_in, 1).contiguous(), size=(n_out, 1), mode="nearest")
            assert torch.equal(rows32[0, 0, :, 0].double(), idx), (n_in, n_out)     # and the fp32 module's, which E_ref uses
    assert seen == {"equal", "double", "general"}


def test_bn_identity_is_exact():
    """var = 1 - eps makes the packer's and the module's 1 / sqrt(var + eps) exactly 1 in fp32."""
    v = np.float32(np.float32(1.0 - EPS) + np.float32(EPS))
    assert v == np.float32(1.0) and np.float32(1.0) / np.sqrt(v) == np.float32(1.0)
    r = _case(("P1", "exact", (9, 17)))
    assert float(r["m"].conv0[0][1].running_var[0]) + np.float32(EPS) == np.float32(1.0)
    x = torch.randn(2, 8, 3, 3)
    bn = copy.deepcopy(r["m"].conv0[0][1])
    with torch.no_grad():
        bn.bias.zero_()
    assert torch.equal(bn(x), x)
    host, _ = _pack(r["m"], *PLANS["P1"])
    for L in _layers(*PLANS["P1"])[0]:
        if L["kind"] == "bn":
            assert np.array_equal(host[L["ep_off"]:L["ep_off"] + L["cout"]], np.ones(L["cout"], np.float32)), L["name"]


# the instantiations of k_fpn_conv that fp_layer names and no accepted plan reaches: (IMG, ZS, E, EPI)
UNREACHED = {(False, 2, 4, "BN"), (False, 1, 2, "OUT"), (False, 2, 2, "OUT")}
NAMED = {(True, 2, 1, "BN"), (True, 1, 1, "BN")} | {(False, zs, e, epi) for zs in (1, 2) for e in (2, 4) for epi in ("BN", "OUT")} | {
    (False, 1, 2, "LAT"), (False, 1, 4, "LAT")}


def test_plans_cover_every_dispatch_key():
    """P1 .. P5 launch every (IMG, ZS, E, EPI, more than one row tile, partial last tile, more than one k-chunk, three or more row
    tiles) that any of the 4 x 8^3 accepted plans can; the instantiations fp_layer names and no plan reaches are listed, so a plan
    change that makes one reachable fails here."""
    lib = _lib.load()
    n = C.c_size_t()
    reachable, count = set(), 0
    for c in range(8, 33, 8):
        for o0 in range(8, 65, 8):
            for o1 in range(8, 65, 8):
                for o2 in range(8, 65, 8):
                    reachable |= set(_dispatch_keys(c, (o0, o1, o2)).values())
                    count += 1
        assert lib.gdb_fpn_packed_floats(c, 64, 8, 40, C.byref(n)) == _lib.GDB_OK and n.value == _layers(c, (64, 8, 40))[1]
    assert count == 4 * 8 ** 3
    for c, outs in ((40, (8, 8, 8)), (4, (8, 8, 8)), (8, (72, 8, 8)), (8, (8, 8, 0))):      # and nothing beyond them is accepted
        assert lib.gdb_fpn_packed_floats(c, *outs, C.byref(n)) == _lib.GDB_E_BADARG
    covered = {}
    for p, (c, outs) in PLANS.items():
        keys = _dispatch_keys(c, outs)
        for layer, key in keys.items():
            covered.setdefault(key, []).append(f"{p}:{layer}")
        assert {layer for layer, key in keys.items() if key[5]} == PARTIAL[p], p
    missing = sorted(reachable - set(covered))
    assert not missing, missing
    assert set(covered) == reachable
    inst = {k[:4] for k in reachable}
    assert inst == NAMED - UNREACHED and UNREACHED <= NAMED and len(inst) == 9
    # what the table of plans says about each of them
    k = {p: _dispatch_keys(*PLANS[p]) for p in PLANS}
    assert k["P1"]["conv0.0"][:4] == (True, 2, 1, "BN") and all(k[p]["conv0.0"][:4] == (True, 1, 1, "BN") for p in ("P3", "P4", "P5"))
    assert k["P2"]["out0"] == (False, 1, 4, "OUT", False, True, True, False) and k["P2"]["out1"][:4] == (False, 2, 4, "OUT") and k["P2"]["out2"][1] == 1
    assert k["P3"]["inner2"][:4] == (False, 1, 4, "LAT") and k["P5"]["inner2"][:4] == (False, 1, 4, "LAT") and k["P1"]["inner2"][2] == 2
    assert {key[2] for key in k["P3"].values()} == {1, 4} and k["P3"]["out0"][7] and k["P3"]["out1"][5] and k["P3"]["out2"][5]
    layers = {L["name"]: L for L in _layers(*PLANS["P4"])[0]}
    assert layers["conv0.1"]["E"] == 2 and layers["conv0.1"]["K"] == 3 and layers["conv2.1"]["rows"] == 96 and k["P4"]["conv2.1"][7]
    assert max(L["K"] for L in _layers(*PLANS["P5"])[0]) == 8 and max(L["cout"] for L in _layers(*PLANS["P5"])[0]) == 128
    for key, where in sorted(covered.items()):
        print(f"[fpn referee] key {key}: {' '.join(where)}")


def test_shapes_are_what_they_claim():
    branches = {"y": [set(), set()], "x": [set(), set()]}
    for (H, W), claim in SHAPES.items():
        d = _dims(H, W)
        for axis, ax in (("y", 0), ("x", 1)):
            got = tuple(_nearest(0, d[lvl + 1][ax], d[lvl][ax])[1] for lvl in (1, 0))       # Q -> H1, then I1 -> F0
            assert got == claim[axis], ((H, W), axis, got)
            for step in (0, 1):
                branches[axis][step].add(got[step])
        assert (W + 31) // 32 == claim["nct"]
    for axis in ("y", "x"):
        for step in (0, 1):
            assert branches[axis][step] == {"equal", "double", "general"}, (axis, step)
    assert {s["nct"] for s in SHAPES.values()} == {1, 2, 3} and (5, 33) in SHAPES and 33 % 32 == 1 and 33 % 16 == 1
    odd = [(H, W) for H, W in SHAPES if H % 2 and H > 1]
    assert (9, 17) in odd and _dims(9, 17)[1][0] % 2 == 1        # an odd height under the two-row layers, full and half resolution
    assert all(s in SHAPES for s in FAMILY_SHAPES) and len(CASES) == 5 * (8 + 2 + 2)
    # the exact family: between its cases, every tap of every layer
    for p in PLANS:
        union = {}
        for s in FAMILY_SHAPES:
            for layer, used in _case((p, "exact", s))["taps"].items():
                union.setdefault(layer, set()).update(used)
        for layer, used in union.items():
            ks = _conv_of(_case((p, "exact", FAMILY_SHAPES[0]))["m"], layer).kernel_size[0]
            assert used == set(range(ks * ks)), (p, layer, sorted(set(range(ks * ks)) - used))
        assert sorted(len(u) for u in union.values()) == [1, 1, 1, 9, 9, 9, 9, 9, 9, 25, 25]


@ALL
def test_fpn_case_referee(case):
    """CPU half of every case: the inputs, the float64 referee of every layer on the fp32 CPU chain's stored activations, E_ref and
    the floor per point, and what the case claims about itself - proven sane before a GPU is involved."""
    r, stored, j = _cpu_half(case)
    name = CASE_IDS[CASES.index(case)]
    regions, total = _regions(r["c"], r["H"], r["W"], 7)
    n = C.c_size_t()
    _lib.check(_lib.load().gdb_fpn_workspace_bytes(r["c"], *r["outs"], N, r["H"], r["W"], 7, C.byref(n)))
    assert n.value == 4 * total and "A" not in regions
    regions3, total3 = _regions(r["c"], r["H"], r["W"], 3)
    _lib.check(_lib.load().gdb_fpn_workspace_bytes(r["c"], *r["outs"], N, r["H"], r["W"], 3, C.byref(n)))
    assert n.value == 4 * total3 and set(regions3) | set(regions) == {"A", "F0", "T1", "H1", "T2", "Q", "I1", "I2"}
    for p in POINTS:
        v = j[p]
        print(f"[fpn referee cpu] {name} {p}: E_ref {v['e_ref']:.3e}  floor {v['floor']:.3e}  bound {v['bound']:.3e}  max|ref64| {v['top']:.3e}")
        assert torch.isfinite(v["ref64"]).all() and torch.isfinite(stored[p]).all() and v["excluded"] == EXCLUDED_CAP == 0
        if p in regions or p in regions3:
            assert tuple(stored[p].permute(0, 2, 3, 1).shape) == (regions.get(p) or regions3[p])[1]
    e = _e2e([stored[k].numpy() for k in LEVELS], r)
    print(f"[fpn referee cpu] {name}: fp32 chain end to end {e}")
    assert max(e) <= 5e-6
    if r["family"] == "random":
        assert all(j[p]["e_ref"] > 0 and j[p]["top"] > 0 for p in POINTS), {p: j[p]["e_ref"] for p in POINTS}
        assert -0.5 <= float(r["x"].min()) < float(r["x"].max()) <= 1.5 and (r["H"] * r["W"] < 16 or float(r["x"].min()) < 0)
    elif r["family"] == "exact":        # a closed form: fp32 arithmetic in any order lands on the float64 values
        assert torch.equal(r["x"] * 8, (r["x"] * 8).round())
        for p in POINTS:
            q = j[p]["ref64"] * 8
            assert j[p]["e_ref"] == 0.0 and torch.equal(q, q.round()) and j[p]["top"] < 2 ** 20, p
            assert int(torch.count_nonzero(j[p]["ref64"])) > 0 and len(torch.unique(j[p]["ref64"])) > 2, p
        assert max(e) == 0.0
    else:                               # small operands: every layer's own output of order 1e-3, the two sums at most twice that
        outs = _layer_outputs(r["m64"], r["x"].double())
        for layer in LAYERS:
            top = float(outs[layer].abs().max())
            assert 0.5 * SMALL <= top <= 2.0 * SMALL, (layer, top)
        assert all(0.25 * SMALL <= j[p]["top"] <= 4.0 * SMALL and j[p]["e_ref"] > 0 for p in POINTS)
        assert float(r["x"].abs().max()) <= 1.5 * 2.0 ** -10


# ---- CPU: slips the rule must catch -----------------------------------------------------------------------------------------
SLIP_SHAPE = (37, 70)
# slip: the smallest size 2^-k (largest k) at which the rule is broken at the slipped layer's own point, for every layer the slip
# applies to, in every plan (random family, 37 x 70); size 1 (k = 0) is the slip as named.  Beside it: does the end-to-end 5e-6 form
# see the slip at that size anywhere / at size 1 everywhere.
#   weights  one layer's weights x (1 + 2^-k)                                     (all 11 layers)
#   eps      eps x (1 - 2^-k) in one BatchNorm's invstd; k = 0: eps dropped       (the 6 conv blocks)
#   border   the centre tap x (1 - 2^-k) in the last output column; k = 0: zeroed (all 11 layers)
#   bias     a lateral's bias x (1 + 2^-k) on one channel; k = 0: added twice     (inner1, inner2)
#   uprow    the upsample's last source row taken as in - 2 (no size)             (I1, I2)
SLIP_K = {"weights": None, "eps": None, "border": None, "bias": None, "uprow": 0}


def _slip_fn(r, slip, point, k):
    """The fp32 CPU layer `point` with one subtle mistake of size 2^-k, as a function of the stored inputs; None if not applicable."""
    layer, reads = POINTS[point]
    m = copy.deepcopy(r["m"])
    conv = _conv_of(m, layer)
    s = 2.0 ** -k
    with torch.no_grad():
        if slip == "weights":
            conv.weight.mul_(1.0 + s)
        elif slip == "eps":
            if not isinstance(_sub(m, layer), torch.nn.Sequential):
                return None
            _sub(m, layer)[1].eps = EPS * (1.0 - s) if k else 1e-30
        elif slip == "bias":
            if len(reads) != 2:
                return None
            ch = int(conv.bias.abs().argmax())
            conv.bias[ch] *= 1.0 + s
        elif slip == "border":
            ctr = conv.kernel_size[0] // 2
            conv.weight[:, :, ctr, ctr] *= 1.0 - s

            def fn(st, m=m):
                y = _apply(r["m"], point, st).clone()
                y[..., -1] = _apply(m, point, st)[..., -1]
                return y
            return fn
        elif slip == "uprow":
            if len(reads) != 2:
                return None

            def fn(st):
                top, skip = st[reads[0]], st[reads[1]]
                n_in, n_out = top.shape[2], skip.shape[2]
                iy = [min(_nearest(d, n_in, n_out)[0], max(n_in - 2, 0)) for d in range(n_out)]
                ix = [_nearest(d, top.shape[3], skip.shape[3])[0] for d in range(skip.shape[3])]
                with torch.no_grad():
                    return top[:, :, iy][:, :, :, ix] + _sub(r["m"], layer)(skip)
            return fn
    return lambda st, m=m: _apply(m, point, st)


@functools.lru_cache(maxsize=None)
def _slip_ratio(plan, slip, point, k):
    """(error / bound at the slipped layer's own point, the end-to-end form's worst level / 5e-6) of one slip."""
    r, stored, j = _cpu_half((plan, "random", SLIP_SHAPE))
    fn = _slip_fn(r, slip, point, k)
    if fn is None:
        return None
    own = float((fn(stored).double() - j[point]["ref64"]).abs().max()) / j[point]["bound"]
    st = _chain(r["m"], r["x"], replace={point: fn})
    return own, max(_e2e([st[lv].numpy() for lv in LEVELS], r)) / 5e-6


def _slip_points(slip):
    r = _case(("P1", "random", SLIP_SHAPE))
    return [p for p in POINTS if _slip_fn(r, slip, p, 1) is not None]


def _smallest(slip, around=None):
    """The largest k at which the slip breaks the rule everywhere: over 0 .. 23, or (the test) the pinned k and two steps either way."""
    ks = [0] if slip == "uprow" else range(0, 24) if around is None else range(max(around - 2, 0), around + 3)
    good = [k for k in ks if all(_slip_ratio(plan, slip, p, k)[0] > 1.0 for plan in PLANS for p in _slip_points(slip))]
    return max(good) if good else None


SLIP_K.update({"weights": 18, "eps": 0, "border": 15, "bias": 18})
SLIP_SEEN_END_TO_END = {"weights": 0, "eps": 0, "border": None, "bias": 0, "uprow": 10}
# end to end (the 5e-6 form of tests/test_fpn.py on the three levels) at those sizes, of plans x layers: weights 2^-18 seen in 0 of
# 55 (first seen at 2^-16, in 3; everywhere only from 2^-2), eps dropped altogether seen in 0 of 30 (at most 0.30 of 5e-6), border
# 2^-15 in a few of 55 (none at 2^-16), bias 2^-18 in 0 of 10 (first at 2^-14), the upsample's row in 10 of 10: that one alone
# the old form catches


@pytest.mark.parametrize("slip", list(SLIP_K))
def test_rule_catches_a_slip_at_its_own_point(slip):
    """No kernel here: one subtly wrong fp32 CPU layer per slip, layer and plan, fed the fp32 chain's stored activations.  At the
    pinned size its error against the float64 referee exceeds the rule's bound at that layer's own point, everywhere; the pinned size
    is the smallest such power of two (give or take one step: E_ref depends on the CPU library's summation order)."""
    k = SLIP_K[slip]
    pts = _slip_points(slip)
    assert len(pts) == {"weights": 11, "eps": 6, "border": 11, "bias": 2, "uprow": 2}[slip]
    bad, seen_e2e, seen_named = [], 0, 0
    for plan in PLANS:
        for p in pts:
            own, e2e = _slip_ratio(plan, slip, p, k)
            own0, e2e0 = _slip_ratio(plan, slip, p, 0)
            print(f"[fpn slip] {slip} 2^-{k} {plan} {p}: err / bound {own:.2f}; end to end / 5e-6 {e2e:.3f}"
                  f"{'' if e2e > 1 else '  (missed end to end)'}; as named: {own0:.1f}, end to end {e2e0:.3f}")
            seen_e2e += e2e > 1
            seen_named += e2e0 > 1
            if not (own > 1.0 and own0 > 1.0):
                bad.append((plan, p, own, own0))
    print(f"[fpn slip] {slip}: end to end sees {seen_e2e} of {len(PLANS) * len(pts)} at 2^-{k}, {seen_named} as named")
    assert not bad, bad
    if SLIP_SEEN_END_TO_END[slip] is not None:       # what the old form makes of the same slip, as recorded above
        assert seen_e2e == SLIP_SEEN_END_TO_END[slip]
    found = _smallest(slip, around=k)
    print(f"[fpn slip] {slip}: smallest size that breaks the rule everywhere 2^-{found}, pinned 2^-{k}")
    assert found is not None and abs(found - k) <= 1


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _run_hip(r, mask):
    """gdb_fpn through the C ABI on a workspace of the test's own (NaN beforehand): {point: (N, C, h, w) fp32 CPU tensor} of every
    region and level that mask leaves behind."""
    c, outs, H, W = r["c"], r["outs"], r["H"], r["W"]
    lib = _lib.load()
    packed = fpn.FeaturePyramid(r["m"]).pack(torch.device("cuda"))
    x = r["x"].cuda().contiguous()
    n = C.c_size_t()
    _lib.check(lib.gdb_fpn_workspace_bytes(c, *outs, N, H, W, mask, C.byref(n)))
    regions, total = _regions(c, H, W, mask)
    assert n.value == 4 * total
    ws = torch.full((total,), float("nan"), device="cuda")
    d = _dims(H, W)
    lv = [torch.full((N, outs[l], *d[2 - l]), float("nan"), device="cuda") if mask >> l & 1 else None for l in range(3)]
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.gdb_fpn(c, *outs, x.data_ptr(), N, H, W, packed.data_ptr(), mask, ws.data_ptr(), n.value, ptr(lv[0]), ptr(lv[1]),
                           ptr(lv[2]), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ws = ws.cpu()
    got = {f"L{l}": t.cpu() for l, t in enumerate(lv) if t is not None}
    written = torch.zeros(total, dtype=torch.bool)
    for name, (o, shape) in regions.items():
        size = int(np.prod(shape))
        got[name] = ws[o:o + size].view(shape).permute(0, 3, 1, 2).contiguous()
        written[o:o + size] = True
    assert bool(torch.isnan(ws[~written]).all())          # the padding is never written
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), (mask, k)   # and every element of every region is
    return got


@pytest.mark.gpu
@ALL
def test_hip_fpn_every_layer_vs_float64(case):
    """Every layer of every case on the GPU against the float64 referee on the kernel's own stored input, under the rule of the module
    docstring: A, F0, T1, H1, T2, Q, I1, I2 and the three levels, all elements; the exact family bit for bit.  Measured ratios:
    DESIGN.md section 4.12 and profiles/r13/fpn_referee_observed.txt."""
    r = _case(case)
    name = CASE_IDS[CASES.index(case)]
    lo, hi = _run_hip(r, 3), _run_hip(r, 7)
    assert set(lo) == {"A", "F0", "T1", "H1", "T2", "Q", "I1", "L0", "L1"} and set(hi) == set(lo) - {"A"} | {"I2", "L2"}
    for k in set(lo) & set(hi):
        assert torch.equal(lo[k], hi[k]), k               # the two runs are one computation
    stored = {"img": r["x"], **hi, "A": lo["A"]}
    j = _judge(r, stored)
    failed = []
    for p in POINTS:
        v = j[p]
        ratio = v["err"] / v["bound"] if v["bound"] else (0.0 if v["err"] == 0 else float("inf"))
        print(f"[fpn referee] {name} {p}: E_ref {v['e_ref']:.3e}  hip err {v['err']:.3e}  bound {v['bound']:.3e}  err/bound {ratio:.3f}  "
              f"max|ref64| {v['top']:.3e}  excluded {v['excluded']}")
        assert v["excluded"] == EXCLUDED_CAP == 0
        if not v["err"] <= v["bound"]:
            failed.append((p, v["err"], v["bound"]))
        if r["family"] == "exact" and not torch.equal(stored[p].double(), v["ref64"]):
            failed.append((p, "not bit for bit", v["err"]))
    e = _e2e([stored[k].numpy() for k in LEVELS], r)
    print(f"[fpn referee] {name}: end to end vs the float64 module {e[0]:.2e} {e[1]:.2e} {e[2]:.2e} of max(1, max |ref|)")
    assert not failed, failed
    assert max(e) <= (0.0 if r["family"] == "exact" else 5e-6)

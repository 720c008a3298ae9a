"""Every layer of the cost-regularisation 3-D U-Nets (gdb_costreg.hip, costvol.CostReg) against a float64 referee.

Referee: the repo's own `_UNet3d`, `copy.deepcopy(m).double()`, on the float64 copy of the fp32 input; forward hooks record every
layer's float64 output.  The fp32 module is pinned to fixture F7's feat_volume first (test_fp32_module_is_pinned_to_f7), so the
referee is tied to the reference and not only to itself.
E_ref_k = max |fp32 module on the CPU - ref64_k| at observation point k: what the reference ARITHMETIC loses there; the kernel is
never involved.
Rule at every observation point: max |hip - ref64_k| <= max(K_RULE * E_ref_k, 8 ulp32(max |ref64_k|)), K_RULE = 4 as for the cost
volume (tests/test_costvol.py): kernel and module are two realisations (another order of the tap products, another BatchNorm
formula) of one fp32 computation, whose maximum error over 1e3 .. 1e7 voxels moves by a small factor between realisations, while
a wrong tap, a wrong statistic or a wrong border errs by the activations themselves.  No element is excluded (cap 0, asserted).

Observation points: the caller owns the workspace, and after gdb_cost_reg returns it still holds the channel-last intermediates
(layout: include/gdb_nerf_hip.h).  T_l = the stride-2 conv(2l - 1); S_depth = the deepest stride-1 layer; S_l (l < depth) = skip_l +
the transposed convolution's result; then the volume and the prob.  Each layer's output is visible at its own magnitude, directly
or as one of two summands of equal scale - end to end a deep layer drowns in the heads' own rounding.

Every GPU case has a CPU half (inputs, referee, E_ref, what the case claims) under -m "not gpu"; the slips of section 4 show on
the CPU alone that the rule catches a subtly wrong layer at that layer's observation point."""
import copy
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, max_abs
from gdb_nerf_amd import _lib, costvol
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks import make_network
from gdb_nerf_amd.networks.gdb_nerf.cost_reg_net import _UNet3d
from test_cost_reg import _layers, _state_dict, _unet

K_RULE = 4.0
EXCLUDED_CAP = 0          # nothing in this operator is ill-conditioned the way a perspective divide is: every element is compared
EPS = 1e-5


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 0.0


# ---- the plan restated: layers, observation points, dispatch keys -----------------------------------------------------------
def _conv_names(depth):
    return [f"conv{i}" for i in range(3 * depth + 1)]


def _up_name(depth, lvl):
    """The transposed convolution that writes level `lvl` (conv(2 depth + 1) writes level depth - 1, the last one level 0)."""
    return f"conv{2 * depth + 1 + (depth - 1 - lvl)}"


def _skip_name(lvl):
    return "conv0" if lvl == 0 else f"conv{2 * lvl}"


def _points(depth):
    return [f"T{l}" for l in range(1, depth + 1)] + [f"S{depth}"] + [f"S{l}" for l in reversed(range(depth))] + ["volume", "prob"]


def _point_of_layer(depth, name):
    """Where a layer's own output is observed."""
    if name == "feat_head":
        return "volume"
    if name == "prob_head":
        return "prob"
    i = int(name[4:])
    if i == 0:
        return "S0"
    if i <= 2 * depth:
        return f"T{(i + 1) // 2}" if i % 2 else f"S{i // 2}"
    return f"S{depth - 1 - (i - 2 * depth - 1)}"


def _dispatch_keys(depth, cin, c, cout):
    """cr_layer's dispatch key (mode, E, NC, ZS, EPI) of every launch of a plan, from the layout restated in test_cost_reg._layers."""
    keys = set()
    for L in _layers(depth, cin, c, cout)[0]:
        heads = L["kind"] == "heads"
        keys.add(("s1" if heads else L["kind"], L["E"], bool(L["nc"]), L["zs"], "heads" if heads else "bn"))
    return keys


def _all_plans():
    for depth in (2, 3):
        for c in range(8, (128 >> depth) + 1, 8):
            for cin in range(8, 257, 8):
                yield depth, cin, c


# ---- modules ----------------------------------------------------------------------------------------------------------------
def _bns(m):
    return [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]


def _identity_bn(m, bias=None):
    """mean 0, var 1 - eps, weight 1, bias 0 (or dyadic per-channel biases): (x - 0) * 1 * 1 + b, provided fl(fl(1 - eps) + fl(eps))
    is 1, which the CPU half asserts."""
    with torch.no_grad():
        for k, bn in enumerate(_bns(m)):
            bn.running_mean.zero_(); bn.running_var.fill_(1.0 - EPS); bn.weight.fill_(1.0); bn.bias.zero_()
            if bias is not None:
                n = bn.bias.numel()
                bn.bias.copy_(torch.tensor([bias[(3 * i + k) % len(bias)] for i in range(n)]))


def _sparse_weights(m, depth, nnz, seed):
    """Every output channel of every (transposed) convolution takes `nnz` (input channel, tap) pairs: +1, +1, -1, ... .  With
    identity BatchNorm and dyadic inputs every partial sum is a small multiple of 2^-3: nothing rounds in fp32, whatever the order."""
    rng = np.random.default_rng(seed)
    taps = {}
    with torch.no_grad():
        for li, name in enumerate(_conv_names(depth) + ["feat_head", "prob_head"]):
            mod = getattr(m, name)
            conv = mod[0] if isinstance(mod, torch.nn.Sequential) else mod
            w = conv.weight
            w.zero_()
            transposed = isinstance(conv, torch.nn.ConvTranspose3d)
            n_out, n_in = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
            used = set()
            for co in range(n_out):
                for k in range(nnz):
                    if k:
                        tap = int(rng.integers(0, 27))
                    elif name.endswith("_head"):      # 9 rows a case: three cases of 8 + 1 rows walk through the 27 taps
                        tap = ((co if name == "feat_head" else m.feat_head.out_channels) + 9 * seed) % 27
                    else:
                        tap = (co * 7 + li * 5 + seed * 11) % 27
                    ci = (co + k) % n_in
                    v = -1.0 if k == 2 else 1.0
                    if transposed:
                        w[ci, co].view(-1)[tap] = v
                    else:
                        w[co, ci].view(-1)[tap] = v
                    used.add(tap)
            taps[name] = used
    return taps


def _blocks(m, depth):
    return [(n, getattr(m, n)) for n in _conv_names(depth)] + [("feat_head", m.feat_head), ("prob_head", m.prob_head)]


def _observe(m, x):
    """One forward of a `_UNet3d` of any dtype: {observation point: tensor in the module's layouts}, plus every layer's own output
    under its name (the prob head's logits included)."""
    depth = m._depth
    rec, hooks = {}, []
    for name, mod in _blocks(m, depth):
        hooks.append(mod.register_forward_hook(lambda _m, _i, out, name=name: rec.__setitem__(name, out.detach().clone())))
    try:
        with torch.no_grad():
            vol, prob = m(x)
    finally:
        for h in hooks:
            h.remove()
    obs = dict(rec)
    for l in range(1, depth + 1):
        obs[f"T{l}"] = rec[f"conv{2 * l - 1}"]
    obs[f"S{depth}"] = rec[f"conv{2 * depth}"]
    y = rec[f"conv{2 * depth}"]
    for l in reversed(range(depth)):       # S_l = skip_l + up(y), the module's own `skips.pop() + conv(y)` (cost_reg_net.py:52)
        y = rec[_skip_name(l)] + rec[_up_name(depth, l)]
        obs[f"S{l}"] = y
    obs["volume"], obs["prob"] = vol, prob
    return obs


def _rescale(m, depth, cin, signed, seed):
    """Rescale every convolution's weights (one factor per layer, a power of two) so that each layer's float64 output has max| | of
    order 1 on an input drawn like the case's: calibrated on a small volume, measured on the case itself in the CPU half."""
    g = torch.Generator().manual_seed(900 + seed)
    x = torch.rand(1, cin, 8, 8, 16, generator=g, dtype=torch.float64) * 2.0 - (0.5 if signed else 0.0)
    m64 = copy.deepcopy(m).double()
    for name, mod in _blocks(m64, depth):
        conv = mod[0] if isinstance(mod, torch.nn.Sequential) else mod
        for _ in range(3):                     # BatchNorm's mean and bias make the output affine, not linear, in the factor
            top = float(_observe(m64, x)[name].abs().max())
            if top == 0:
                break
            with torch.no_grad():
                conv.weight.mul_(2.0 ** round(-np.log2(top)))
    with torch.no_grad():
        for (_, a), (_, b) in zip(_blocks(m, depth), _blocks(m64, depth)):
            ca, cb = (a[0], b[0]) if isinstance(a, torch.nn.Sequential) else (a, b)
            ca.weight.copy_(cb.weight.float())     # power-of-two factors: exact in fp32
    return m


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _case(depth, cin, c, cout, B, D, H, W, inp="pos", weights="default", seed=0, **kw):
    return dict(depth=depth, cin=cin, c=c, cout=cout, B=B, D=D, H=H, W=W, inp=inp, weights=weights, seed=seed, **kw)


CASES = {
    # the F7 and the c2 (512 x 640) stage shapes
    "f7-stage0-d2-cin32-c8-B2-64x8x12": _case(2, 32, 8, 8, 2, 64, 8, 12, seed=1),
    "f7-stage1-d3-cin16-c8-B2-8x32x48": _case(3, 16, 8, 8, 2, 8, 32, 48, seed=2),
    "c2-stage0-d2-cin32-c8-B1-64x64x80-signed": _case(2, 32, 8, 8, 1, 64, 64, 80, inp="signed", seed=3),
    "c2-stage1-d3-cin16-c8-B1-8x256x320": _case(3, 16, 8, 8, 1, 8, 256, 320, seed=4),
    # instantiations and channel edges; the minimum volumes (level `depth` is a single voxel); W = one tile + a remainder
    "d3-cin16-c16-cout4-B1-8x8x8-min": _case(3, 16, 16, 4, 1, 8, 8, 8, inp="signed", seed=5),
    "d2-cin8-c16-cout1-B3-4x4x4-min-rescaled": _case(2, 8, 16, 1, 3, 4, 4, 4, inp="signed", weights="rescaled", seed=6),
    "d2-cin24-c24-cout15-B1-4x4x36": _case(2, 24, 24, 15, 1, 4, 4, 36, inp="signed", seed=7),
    "d2-cin40-c32-cout4-B2-8x8x68-rescaled": _case(2, 40, 32, 4, 2, 8, 8, 68, weights="rescaled", seed=8),
    "d2-cin8-c8-cout15-B3-4x4x68": _case(2, 8, 8, 15, 3, 4, 4, 68, seed=9),
    "d2-cin16-c8-cout8-B1-192x4x8-signed": _case(2, 16, 8, 8, 1, 192, 4, 8, inp="signed", seed=10),
    # inputs
    "d2-cin32-c8-B2-8x8x12-signed-x1000": _case(2, 32, 8, 8, 2, 8, 8, 12, inp="big", seed=11),
    "d3-cin16-c8-B2-8x16x24-signed-rescaled": _case(3, 16, 8, 8, 2, 8, 16, 24, inp="signed", weights="rescaled", seed=12),
    "d2-cin32-c8-B1-16x8x36-signed-rescaled": _case(2, 32, 8, 8, 1, 16, 8, 36, inp="signed", weights="rescaled", seed=13),
    "d3-cin24-c16-cout4-B1-8x8x40-rescaled": _case(3, 24, 16, 4, 1, 8, 8, 40, weights="rescaled", seed=14),
    # all-zero input: the BatchNorm-bias chain; sparse +-1 weights and dyadic biases, so every layer has an exact closed form
    "zero-d2-cin16-c8-B1-8x8x12": _case(2, 16, 8, 8, 1, 8, 8, 12, inp="zero", weights="sparse3", seed=15, exact=True),
    "zero-d3-cin16-c16-cout4-B2-8x8x40": _case(3, 16, 16, 4, 2, 8, 8, 40, inp="zero", weights="sparse3", seed=16, exact=True),
    # impulses: identity BatchNorm, one-hot weights, a one-hot voxel at each of the 8 corners and one interior point (odd z): batch
    # item b holds impulse b.  Every activation is 0, 1 or 2 exactly.
    "impulse-d2-cin8-c8-B9-8x8x8-a": _case(2, 8, 8, 8, 9, 8, 8, 8, inp="impulse", weights="onehot", seed=17, exact=True),
    "impulse-d2-cin8-c8-B9-8x8x8-b": _case(2, 8, 8, 8, 9, 8, 8, 8, inp="impulse", weights="onehot", seed=18, exact=True),
    "impulse-d2-cin16-c16-cout15-B9-4x8x36": _case(2, 16, 16, 15, 9, 4, 8, 36, inp="impulse", weights="onehot", seed=19, exact=True),
    "impulse-d3-cin16-c16-cout4-B9-8x8x16": _case(3, 16, 16, 4, 9, 8, 8, 16, inp="impulse", weights="onehot", seed=20, exact=True),
    # the same impulses on the sparse +-1 nets with dyadic biases.  With one-hot weights and no bias an impulse seldom survives two
    # stride-2 layers (each needs the right parity in all three dimensions); here the bias chain keeps every layer alive and the
    # impulse rides on it down to the deepest level, still exactly
    "impulse-biased-d2-cin8-c8-B9-8x8x8": _case(2, 8, 8, 8, 9, 8, 8, 8, inp="impulse", weights="sparse3", seed=26, exact=True),
    "impulse-biased-d3-cin16-c16-cout4-B9-8x8x16": _case(3, 16, 16, 4, 9, 8, 8, 16, inp="impulse", weights="sparse3", seed=27, exact=True),
    # softmax
    "softmax-pm60-d2-cin32-c8-B2-64x8x12": _case(2, 32, 8, 8, 2, 64, 8, 12, inp="signed", seed=21, logits=60.0),
    "softmax-pm60-d3-cin16-c16-B1-8x8x40": _case(3, 16, 16, 8, 1, 8, 8, 40, inp="signed", seed=22, logits=60.0),
    "softmax-constant-d2-cin16-c8-B1-192x4x8": _case(2, 16, 8, 8, 1, 192, 4, 8, seed=23, logits=0.0),
    "softmax-constant-d3-cin16-c8-B2-8x8x16": _case(3, 16, 8, 8, 2, 8, 8, 16, seed=24, logits=0.0),
    "softmax-dominant-d2-cin32-c8-B1-64x8x12": _case(2, 32, 8, 8, 1, 64, 8, 12, inp="plane", seed=25, logits=60.0, dominant=True),
}
CASE_IDS = list(CASES)


def _impulse_positions(D, H, W):
    corners = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    return corners + [(D // 2 + 1 - (D // 2) % 2, H // 2, W // 2 + 1)]     # the interior point sits on an odd plane


def _input(c):
    g = torch.Generator().manual_seed(100 + c["seed"])
    shape = (c["B"], c["cin"], c["D"], c["H"], c["W"])
    kind = c["inp"]
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "impulse":
        x = torch.zeros(shape)
        pos = _impulse_positions(c["D"], c["H"], c["W"])
        assert len(pos) == c["B"] == 9
        for b, (z, y, xx) in enumerate(pos):
            x[b, :, z, y, xx] = 1.0
        return x
    x = torch.rand(shape, generator=g) * 2.0
    if kind in ("signed", "big", "plane"):
        x = x - 0.5
    if kind == "big":
        x = x * 1e3
    if kind == "plane":                       # one plane carries 32 times the signal of the others
        x[:, :, c["D"] // 3] *= 32.0
    return x


def _module(c):
    depth, cin, cc, cout = c["depth"], c["cin"], c["c"], c["cout"]
    m = _unet(cin, cc, cout, depth, seed=c["seed"])
    if c["weights"] == "rescaled":
        _rescale(m, depth, cin, c["inp"] != "pos", c["seed"])
    elif c["weights"] == "onehot":
        _identity_bn(m)
        m.taps = _sparse_weights(m, depth, 1, c["seed"])
    elif c["weights"] == "sparse3":
        _identity_bn(m, bias=(0.25, 0.5, -0.25, 0.125, 0.0, 0.375, -0.125))
        m.taps = _sparse_weights(m, depth, 3, c["seed"])
    return m


@functools.lru_cache(maxsize=None)
def _referee(name):
    c = CASES[name]
    t0 = time.perf_counter()
    m, x = _module(c), _input(c)
    m64 = copy.deepcopy(m).double()
    if c.get("exact"):     # the identity BatchNorm that fp32 realises exactly (test_bn_identity_is_exact), written down exactly
        for bn in _bns(m64):
            bn.running_var.fill_(1.0)
            bn.eps = 2.0 ** -60      # (1 + 2^-60 is 1 in float64; PyTorch refuses an eps of 0)
    if "logits" in c:      # scale the prob head (a power of two, exact in fp32) so that the float64 logits reach about +-c["logits"]
        top = float(_observe(m64, x.double())["prob_head"].abs().max())
        s = 0.0 if c["logits"] == 0 else 2.0 ** round(np.log2(c["logits"] / top))
        with torch.no_grad():
            m.prob_head.weight.mul_(s); m64.prob_head.weight.mul_(s)
    ref64 = {k: v.numpy() for k, v in _observe(m64, x.double()).items()}
    cpu32 = {k: v.numpy() for k, v in _observe(m, x).items()}
    pts = _points(c["depth"])
    r = dict(case=c, m=m, x=x, ref64=ref64, cpu32=cpu32, points=pts, e_ref={}, top={}, floor={}, excluded=0)
    for k in pts:
        assert ref64[k].dtype == np.float64 and cpu32[k].dtype == np.float32 and ref64[k].shape == cpu32[k].shape, k
        r["e_ref"][k] = float(np.abs(cpu32[k].astype(np.float64) - ref64[k]).max())
        r["top"][k] = float(np.abs(ref64[k]).max())
        r["floor"][k] = 8 * _ulp32(r["top"][k])
    r["seconds"] = time.perf_counter() - t0
    return r


def _bound(r, k, floor_only=False):
    return r["floor"][k] if floor_only else max(K_RULE * r["e_ref"][k], r["floor"][k])


def _err(got, r, k):
    got = np.asarray(got, np.float64)
    assert got.shape == r["ref64"][k].shape, (k, got.shape, r["ref64"][k].shape)
    return float(np.abs(got - r["ref64"][k]).max())     # every element: nothing is excluded


def _floor_only(c, k):
    """Exact cases are held to the floor alone; their prob goes through exp(), which has no exact value: the full rule there."""
    return bool(c.get("exact")) and k != "prob"


# ---- CPU: the referee is tied to the reference ------------------------------------------------------------------------------
def test_fp32_module_is_pinned_to_f7():
    """The fp32 CPU modules inside DepthNet reproduce F7's feat_volume under the bound of test_cnns_match_reference_on_cpu; the
    float64 copy of the last stage's U-Net on the very cost volume DepthNet fed it is a refinement of the same thing."""
    f7 = load_golden("F7_network")
    net = make_network(make_cfg("configs/dtu_eval.yaml")).eval()
    net.load_state_dict(_state_dict(f7), strict=True)
    t = lambda k: torch.from_numpy(f7[k])
    seen = []
    hooks = [reg.register_forward_hook(lambda m, i, o: seen.append((m, i[0].detach().clone(), o[0].detach().clone()))) for reg in net.depth_net.cost_regs]
    with torch.no_grad():
        src = t("src_images")
        ms = [f.unflatten(0, (1, 3)) for f in net.feature_net(src.flatten(0, 1))]
        d, rng, vrng, vol, _ = net.depth_net(src, ms, t("src_exts"), t("src_ints"), t("tar_ext"), t("tar_int"), t("near_far"))
    for h in hooks:
        h.remove()
    assert max_abs(vol[-1].numpy(), f7["feat_volume"]) <= 1e-4
    assert len(seen) == 2 and [m._depth for m, _, _ in seen] == [2, 3]
    m, cost, out = seen[-1]
    assert torch.equal(out, vol[-1])
    obs64 = _observe(copy.deepcopy(m).double(), cost.double())
    assert obs64["volume"].dtype == torch.float64 and max_abs(obs64["volume"].numpy(), f7["feat_volume"]) <= 1e-4
    obs32 = _observe(m, cost)
    assert torch.equal(obs32["volume"], out)       # the hooks observe, they do not disturb


def test_bn_identity_is_exact():
    """var = 1 - eps makes the packer's and the module's 1 / sqrt(var + eps) exactly 1 in fp32."""
    v = np.float32(1.0 - EPS) + np.float32(EPS)
    assert v == np.float32(1.0) and np.float32(1.0) / np.sqrt(v) == np.float32(1.0)
    m = _module(CASES["impulse-d2-cin8-c8-B9-8x8x8-a"])
    x = torch.randn(2, 8, 1, 1, 1)
    assert torch.equal(m.conv0[1](x), x)


def test_case_table_covers_what_it_claims():
    cs = list(CASES.values())
    reachable = set()
    for depth, cin, c in _all_plans():
        reachable |= _dispatch_keys(depth, cin, c, 8)
    covered = set()
    for c in cs:
        covered |= _dispatch_keys(c["depth"], c["cin"], c["c"], c["cout"])
    assert covered == reachable and len(reachable) == 8     # every kernel cr_layer can launch is launched by some case
    # the four forms no plan reaches (removed from cr_layer)
    for dead in (("s1", 4, False, 2, "bn"), ("s1", 2, False, 2, "bn"), ("s1", 2, False, 1, "bn"), ("up", 2, False, 1, "bn")):
        assert dead not in reachable
    assert {(c["depth"], c["c"]) for c in cs} >= {(2, 8), (2, 16), (2, 24), (2, 32), (3, 8), (3, 16)}
    assert {c["cin"] for c in cs} >= {8, 16, 24, 32, 40} and {c["cout"] for c in cs} >= {1, 4, 8, 15}
    assert {c["B"] for c in cs} >= {1, 2, 3} and {c["D"] for c in cs} >= {4, 8, 64, 192} and 4 in {c["H"] for c in cs}
    assert {(c["D"], c["H"], c["W"]) for c in cs if c["depth"] == 2} >= {(4, 4, 4), (64, 8, 12), (64, 64, 80)}
    assert {(c["D"], c["H"], c["W"]) for c in cs if c["depth"] == 3} >= {(8, 8, 8), (8, 32, 48), (8, 256, 320)}
    assert {c["W"] for c in cs} >= {36, 68} and 68 // 2 == 34          # 64 + 4 (conv0), 32 + 4 (channel-last), 32 + 2 (transposed)
    assert {c["inp"] for c in cs} >= {"pos", "signed", "big", "zero", "impulse", "plane"}
    assert {c["weights"] for c in cs} >= {"default", "rescaled", "onehot", "sparse3"}
    # c = 24: a second row tile with 8 of 16 rows; c = 32 at depth 2: 8 row tiles at level 2; partly filled first-layer k-chunks
    assert any(c["c"] == 24 for c in cs) and any((c["c"] << c["depth"]) == 128 for c in cs) and any(c["cin"] % 16 for c in cs)
    # the exact cases (one-hot and sparse +-1 weights): between them, every one of the 27 taps of every kind of layer
    by_kind = {}
    for n, c in CASES.items():
        if c["weights"] not in ("onehot", "sparse3"):
            continue
        m = _module(c)
        kinds = {L["name"]: ("conv0" if L["nc"] else L["kind"]) for L in _layers(c["depth"], c["cin"], c["c"], c["cout"])[0]}
        for name, used in m.taps.items():
            by_kind.setdefault(kinds.get(name, "heads"), set()).update(used)
        if c["inp"] != "impulse":
            continue
        pos = _impulse_positions(c["D"], c["H"], c["W"])
        assert len(set(pos)) == 9 and pos[-1][0] % 2 == 1 and (c["D"] - 1, c["H"] - 1, c["W"] - 1) in pos
    assert set(by_kind) == {"conv0", "s1", "s2", "up", "heads"}
    for kind, used in by_kind.items():
        assert used == set(range(27)), (kind, sorted(set(range(27)) - used))


@pytest.mark.parametrize("name", CASE_IDS)
def test_cost_reg_case_referee(name):
    """CPU half of every case: the inputs, the float64 referee with every layer's output, E_ref and the floor per observation
    point, and what the case claims about itself - proven sane before a GPU is involved."""
    r = _referee(name)
    c = r["case"]
    print(f"[costreg cpu] {name}: referee + fp32 module {r['seconds']:.1f} s")
    for k in r["points"]:
        print(f"[costreg cpu] {name} {k}: E_ref {r['e_ref'][k]:.3e}  floor {r['floor'][k]:.3e}  bound {_bound(r, k, _floor_only(c, k)):.3e}  max|ref64| {r['top'][k]:.3e}")
        assert np.isfinite(r["ref64"][k]).all() and np.isfinite(r["cpu32"][k]).all()
    assert r["excluded"] == EXCLUDED_CAP == 0
    lay = [n for n in _conv_names(c["depth"])] + ["feat_head", "prob_head"]
    if c["weights"] == "rescaled":      # weights that do not attenuate: every layer's output of order 1
        for n in lay:
            top = float(np.abs(r["ref64"][n]).max())
            print(f"[costreg cpu] {name} {n}: max|ref64| {top:.3f}")
            assert 0.25 <= top <= 4.0, (n, top)
    if c.get("exact"):                  # a closed form: fp32 arithmetic in any order lands on the float64 values
        for k in r["points"]:
            if k != "prob":
                assert r["e_ref"][k] == 0.0, k
                q = r["ref64"][k] * 8
                assert np.array_equal(q, np.round(q)) and r["top"][k] < 2 ** 20
        alive = {k: int(np.count_nonzero(r["ref64"][k])) for k in r["points"]}
        print(f"[costreg cpu] {name}: non-zero elements {alive}")
        deep = f"S{c['depth']}"
        if c["weights"] == "onehot":    # conv0 in both forms, the first stride-2 layer, the last transposed layer and the heads see it
            assert set(np.unique(r["ref64"]["volume"])) <= {0.0, 1.0} and r["top"]["S0"] <= 2.0
            assert all(alive[k] > 0 for k in ("T1", "S0", "volume")), alive
            assert all(r["ref64"]["S0"][b].any() for b in range(c["B"]))
        else:                           # the bias chain keeps every layer alive
            assert all(alive[k] > 0 for k in r["points"]), alive
            assert len(np.unique(r["ref64"]["T1"])) > 1 and len(np.unique(r["ref64"][deep])) > 1
            if c["inp"] == "impulse":   # and the impulses reach the deepest level: the items differ there
                assert np.ptp(r["ref64"][deep], axis=0).any()
            else:
                assert not r["x"].any()
    elif "logits" not in c:
        assert all(r["e_ref"][k] > 0 and r["top"][k] > 0 for k in r["points"])
    if c["inp"] == "big":
        assert float(r["x"].abs().max()) > 1e3
    if c["inp"] in ("signed", "big", "plane"):
        assert float(r["x"].min()) < -0.4 * float(r["x"].abs().max()) / 1.5
    lg = r["ref64"]["prob_head"]
    if c.get("logits") == 60.0:
        print(f"[costreg cpu] {name}: logits {lg.min():.1f} .. {lg.max():.1f}")
        assert 60.0 / 2 ** 0.5 <= np.abs(lg).max() <= 60.0 * 2 ** 0.5 and lg.max() - lg.min() >= 60.0 / 2 ** 0.5   # (a power-of-two factor)
    if c.get("logits") == 0.0:
        assert not lg.any() and np.array_equal(r["cpu32"]["prob"], np.full_like(r["cpu32"]["prob"], np.float32(1.0) / np.float32(c["D"])))
    if c.get("dominant"):
        frac = float((r["ref64"]["prob"].max(axis=1) > 0.99).mean())
        print(f"[costreg cpu] {name}: pixels with one plane above 0.99: {frac:.3f}")
        assert frac >= 0.5
    s = np.abs(r["ref64"]["prob"].sum(axis=1) - 1.0).max()
    assert s <= 1e-12


# ---- CPU: slips the rule must catch -----------------------------------------------------------------------------------------
class _Wrapped(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)


def _conv_of(m, layer):
    mod = getattr(m, layer)
    return (mod, 0) if isinstance(mod, torch.nn.Sequential) else (m, layer)


def _set_conv(m, layer, new):
    holder, key = _conv_of(m, layer)
    if isinstance(key, int):
        holder[key] = new
    else:
        setattr(m, key, new)


def _get_conv(m, layer):
    holder, key = _conv_of(m, layer)
    return holder[key] if isinstance(key, int) else getattr(m, key)


def _layer_input(r, layer):
    depth = r["case"]["depth"]
    if layer.endswith("_head"):
        return r["cpu32"]["S0"]
    i = int(layer[4:])
    if i == 0:
        return r["x"].numpy()
    if i <= 2 * depth + 1:
        return r["cpu32"][f"conv{i - 1}"]
    return r["cpu32"][f"S{depth - (i - 2 * depth - 1)}"]


def _pick(r, layer, kx, last_column):
    """The (output channel, input channel) whose tap (1, 1, kx) matters most: a tap into a channel that the ReLU silences, or from a
    silent one, cannot be seen by anything.  The 32 pairs with the largest |w| max|x| are tried on this layer alone."""
    block = copy.deepcopy(getattr(r["m"], layer))
    conv = block[0] if isinstance(block, torch.nn.Sequential) else block
    transposed = isinstance(conv, torch.nn.ConvTranspose3d)
    x = torch.from_numpy(np.ascontiguousarray(_layer_input(r, layer)))
    ax = x.abs()[..., -2:] if last_column else x.abs()
    w = conv.weight.detach()
    wc = (w[:, :, 1, 1, kx].t() if transposed else w[:, :, 1, 1, kx]).abs()                  # (cout, cin)
    score = (wc * ax.amax(dim=(0, 2, 3, 4))[None, :]).flatten()
    best, best_effect = None, -1.0
    with torch.no_grad():
        y0 = block(x)
        for flat in score.topk(min(32, score.numel())).indices.tolist():
            co, ci = divmod(flat, wc.shape[1])
            conv.weight.copy_(w)
            conv.weight[(ci, co) if transposed else (co, ci)][1, 1, kx] *= 1.0 + 2.0 ** -10
            d = (block(x) - y0).abs()
            effect = float((d[..., -1] if last_column else d).max())
            if effect > best_effect:
                best, best_effect = (co, ci), effect
    return best


def _slipped(r, layer, slip):
    """A copy of the fp32 module with one subtle mistake in `layer`; None where the slip does not apply to that layer."""
    s = copy.deepcopy(r["m"])
    conv = _get_conv(s, layer)
    transposed = isinstance(conv, torch.nn.ConvTranspose3d)
    head = layer.endswith("_head")
    w = conv.weight
    with torch.no_grad():
        if slip == "tap":                  # (a) one tap x (1 + 2^-10): a centre tap
            co, ci = _pick(r, layer, 1, False)
            w[(ci, co) if transposed else (co, ci)][1, 1, 1] *= 1.0 + 2.0 ** -10
        elif slip == "border-tap":         # (a) a tap that only the border sees: the slipped weight acts on the last column only
            w2 = w.detach().clone()
            kx = 2 if transposed else 1    # (a transposed layer's last column is odd: tap 2 from i = Wi - 1; tap 0 falls outside)
            co, ci = _pick(r, layer, kx, True)
            w2[(ci, co) if transposed else (co, ci)][1, 1, kx] *= 1.0 + 2.0 ** -10
            orig = copy.deepcopy(conv)
            bad = copy.deepcopy(conv)
            bad.weight.copy_(w2)

            def fn(x, orig=orig, bad=bad):
                y = orig(x).clone()
                y[..., -1] = bad(x)[..., -1]
                return y
            _set_conv(s, layer, _Wrapped(fn))
        elif slip == "var":                # (b) running_var x (1 + 2^-12)
            if head:
                return None
            getattr(s, layer)[1].running_var.mul_(1.0 + 2.0 ** -12)
        elif slip == "replicate":          # (c) zero padding replaced by replicate padding
            if transposed:                 # input voxels beyond the border (i = Di feeds o = 2 Di - 1 through tap 0) replicate the edge
                def fn(x, w=w.detach().clone()):
                    y = F.conv_transpose3d(F.pad(x, (1,) * 6, mode="replicate"), w, stride=2, padding=1, output_padding=1)
                    return y[:, :, 2:-2, 2:-2, 2:-2]
            else:
                def fn(x, w=w.detach().clone(), st=conv.stride):
                    return F.conv3d(F.pad(x, (1,) * 6, mode="replicate"), w, stride=st)
            _set_conv(s, layer, _Wrapped(fn))
        elif slip == "swap-x":             # (d) a transposed layer with taps 0 and 2 swapped along x
            if not transposed:
                return None
            w.copy_(w.flip(-1))
    return s


SLIPS = ("tap", "border-tap", "var", "replicate", "swap-x")
SLIP_CASES = ["f7-stage1-d3-cin16-c8-B2-8x32x48", "d2-cin24-c24-cout15-B1-4x4x36", "d3-cin16-c8-B2-8x16x24-signed-rescaled",
              "d2-cin32-c8-B1-16x8x36-signed-rescaled"]


def _slip_table(name):
    r = _referee(name)
    c = r["case"]
    rows = []
    for layer in _conv_names(c["depth"]) + ["feat_head", "prob_head"]:
        k = _point_of_layer(c["depth"], layer)
        for slip in SLIPS:
            s = _slipped(r, layer, slip)
            if s is None:
                continue
            obs = {p: v.numpy() for p, v in _observe(s, r["x"]).items()}
            own = _err(obs[k], r, k) / _bound(r, k)
            e2e = max(_err(obs["volume"], r, "volume") / _bound(r, "volume"), _err(obs["prob"], r, "prob") / _bound(r, "prob"))
            rows.append((layer, slip, k, own, e2e))
    return rows


@pytest.mark.parametrize("name", SLIP_CASES)
def test_rule_catches_a_slip_in_every_layer(name):
    """No kernel here: one subtly wrong fp32 CPU module per layer and slip.  At the layer's own observation point its error against
    the float64 referee exceeds the rule's bound; printed beside it, whether the end-to-end outputs alone (volume and prob under
    the same rule) would have seen it."""
    rows = _slip_table(name)
    missed_e2e = 0
    for layer, slip, k, own, e2e in rows:
        print(f"[costreg slip] {name} {layer} {slip}: at {k} err / bound {own:.2f}; end to end {e2e:.2f}{'  (missed end to end)' if e2e <= 1 else ''}")
        missed_e2e += e2e <= 1
    print(f"[costreg slip] {name}: {len(rows)} slips, {missed_e2e} of them invisible in the volume and the prob")
    c = CASES[name]
    assert len(rows) == (3 * c["depth"] + 1) * 4 + c["depth"] + 2 * 3
    bad = [(layer, slip, k, round(own, 3)) for layer, slip, k, own, _ in rows if not own > 1.0]
    assert not bad, bad


# ---- GPU --------------------------------------------------------------------------------------------------------------------
def _channel_first(flat, B, D, H, W, ch):
    return flat.view(B, D, H, W, ch).permute(0, 4, 1, 2, 3).contiguous().cpu().numpy()


def _run_hip(r):
    """gdb_cost_reg through the C ABI on a workspace of the test's own (NaN beforehand): {observation point: array}."""
    c = r["case"]
    depth, cin, cc, cout, B, D, H, W = (c[k] for k in ("depth", "cin", "c", "cout", "B", "D", "H", "W"))
    lib = _lib.load()
    reg = costvol.CostReg(r["m"])
    packed = reg.pack(torch.device("cuda"))
    cost = r["x"].cuda()
    n = C.c_size_t()
    _lib.check(lib.gdb_cost_reg_workspace_bytes(depth, cin, cc, cout, B, D, H, W, C.byref(n)))
    level = lambda l: (B * (D >> l) * (H >> l) * (W >> l) * (cc << l) + 63) // 64 * 64
    assert n.value == 4 * sum((2 if l else 1) * level(l) for l in range(depth + 1))
    ws = torch.full((n.value // 4,), float("nan"), device="cuda")
    vol = torch.full((B, cout, D, H, W), float("nan"), device="cuda")
    prob = torch.full((B, D, H, W), float("nan"), device="cuda")
    _lib.check(lib.gdb_cost_reg(depth, cin, cc, cout, cost.data_ptr(), B, D, H, W, packed.data_ptr(), ws.data_ptr(), n.value,
                                vol.data_ptr(), prob.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got, o = {"volume": vol.cpu().numpy(), "prob": prob.cpu().numpy()}, 0
    for l in range(depth + 1):           # S_0 | S_1 T_1 | ... | S_depth T_depth, each padded to 64 floats
        dims = (B, D >> l, H >> l, W >> l, cc << l)
        size = int(np.prod(dims))
        got[f"S{l}"] = _channel_first(ws[o:o + size], *dims)
        pad = ws[o + size:o + level(l)]
        assert bool(torch.isnan(pad).all())          # the padding is never written
        o += level(l)
        if l:
            got[f"T{l}"] = _channel_first(ws[o:o + size], *dims)
            o += level(l)
    assert o == ws.numel()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_hip_cost_reg_every_layer_vs_float64(name):
    """Every layer of every case on the GPU against the float64 referee under the rule of the module docstring: every T_l, S_depth,
    every S_l = skip + up, the volume and the prob; all elements.  Measured ratios: DESIGN.md section 4.6."""
    r = _referee(name)
    c = r["case"]
    got = _run_hip(r)
    failed = []
    for k in r["points"]:
        err, bound = _err(got[k], r, k), _bound(r, k, _floor_only(c, k))
        ratio = err / r["e_ref"][k] if r["e_ref"][k] else float("nan")
        print(f"[costreg] {name} {k}: E_ref {r['e_ref'][k]:.3e}  hip err {err:.3e}  ratio {ratio:.2f}  bound {bound:.3e}  max|ref64| {r['top'][k]:.3e}  excluded 0")
        assert np.isfinite(got[k]).all(), k
        if not err <= bound:
            failed.append((k, err, bound))
    assert not failed, failed
    s = float(np.abs(got["prob"].astype(np.float64).sum(axis=1) - 1.0).max())
    print(f"[costreg] {name}: max |sum over D of prob - 1| = {s:.3e} (D 2^-24 = {c['D'] * 2.0 ** -24:.3e})")
    assert s <= c["D"] * 2.0 ** -24
    if c.get("logits") == 0.0:           # constant logits: exactly 1 / D
        assert np.array_equal(got["prob"], np.full_like(got["prob"], np.float32(1.0) / np.float32(c["D"])))
    if c.get("exact"):                   # the closed forms: bit for bit
        for k in r["points"]:
            if k != "prob":
                assert np.array_equal(got[k].astype(np.float64), r["ref64"][k]), k

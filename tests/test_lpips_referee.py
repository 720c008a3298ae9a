"""Every stored point of LPIPS-VGG on the HIP library (gdb_lpips.hip, metrics.eval_lpips) against a float64 referee, in the form of
tests/test_fpn_referee.py.  Weights are random and seeded here (He-scaled convolutions keep the activations O(1) through thirteen
layers, tap weights non-negative): no published weights exist on the test machines, so what is pinned is the written definition
(include/gdb_nerf_hip.h), not agreement with the `lpips` package's values - that stays unverified.

Observation points: with GDB_LPIPS_KEEP the caller's workspace holds the scaled input, the 13 convolution outputs, the 4 pooled maps
and the 5 t_l after the call; the record holds the total.  Every point is checked on the kernel's OWN stored fp32 input: ref64 is
the torch restatement (evaluators/gdb_nerf.py: lpips_scale / lpips_conv / lpips_pool / lpips_tap) of that one layer in float64,
E_ref = max |the fp32 CPU restatement - ref64| on the same input.
Rule at every point: max |hip - ref64| <= max(K_RULE * E_ref, 8 ulp32(max |ref64|)), K_RULE = 4 as everywhere in this repository; no
element is excluded (cap 0, asserted); pooled maps must be bit-exact.  For the scalars (t_l and the total) a single E_ref can vanish
by cancellation, so E_ref is the maximum over 8 seeds of the fp32 chain's error at that shape.  End to end the total is compared with
the float64 chain on the image under 4 x the 8-seed maximum of the fp32 chain's end-to-end error.

Every GPU case has a CPU half under -m "not gpu": the fp32 CPU chain stands in for the kernel's stored activations, and a SECOND
fp32 realisation (F.unfold + matmul with the k order reversed, reversed channel and pixel sums) must pass the rule at every point -
the reference arithmetic alone stays inside the bound on these inputs.  The slips at the end each break the rule at their own point."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gdb_nerf_amd import metrics
from gdb_nerf_amd.evaluators.gdb_nerf import LPIPS_TAPS, lpips_conv, lpips_pool, lpips_scale, lpips_tap, lpips_torch

K_RULE = 4.0
EXCLUDED_CAP = 0
SEEDS = 8
CH = metrics.LPIPS_CHANNELS
GROUP_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)

# name: (B, H, W, crop (y0, x0, h, w) or None, masked, family)
CASES = {
    "16x16": (1, 16, 16, None, False, "random"),              # every map down to 1 x 1
    "17x35": (1, 17, 35, None, True, "random"),               # odd extents at every pool: 35 -> 17 -> 8 -> 4 -> 2
    "32x96": (2, 32, 96, None, False, "random"),              # several column tiles, two batch items
    "33x47-crop": (2, 40, 56, (3, 5, 33, 47), True, "random"),   # an unaligned crop
    "exact-17x35": (1, 17, 35, None, True, "exact"),
    "exact-32x96": (2, 32, 96, None, False, "exact"),
    "small-17x35": (1, 17, 35, None, True, "small"),          # the second tap's feature norms of the order of 1e-5: the eps counts
}
SMALL = 2.0 ** -17
ALL = pytest.mark.parametrize("name", list(CASES))

CONVS = [f"conv.{i}" for i in range(13)]
POOLS = [f"pool.{g}" for g in range(4)]
TAPS = [f"t.{l}" for l in range(5)]
POINTS = ["scaled"]
for _i in range(13):
    if _i and GROUP_OF[_i] != GROUP_OF[_i - 1]:
        POINTS.append(f"pool.{GROUP_OF[_i] - 1}")
    POINTS.append(f"conv.{_i}")
POINTS += TAPS + ["total"]
SCALARS = set(TAPS) | {"total"}


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else 0.0


def _input_of(i):
    if i == 0:
        return "scaled"
    return f"pool.{GROUP_OF[i] - 1}" if GROUP_OF[i] != GROUP_OF[i - 1] else f"conv.{i - 1}"


# ---- weights and inputs ----------------------------------------------------------------------------------------------------
DYADIC = (0.25, 0.5, -0.25, 0.125, 0.0, 0.375, -0.125)


def _weights(seed, family):
    g = torch.Generator().manual_seed(seed)
    w = {}
    for i, (ci, co) in enumerate(CH):
        if family == "exact":
            # three entries per output channel, +s, +s, -s with s = 1 (even layers) or 2^-1 (odd): with inputs and biases that are
            # multiples of 2^-3 every partial sum is a small multiple of a power of two and nothing rounds in fp32, whatever the order
            t = torch.zeros(co, ci, 9)
            s = 1.0 if i % 2 == 0 else 0.5
            rnd = torch.randint(0, 9 * ci, (co,), generator=g)
            for c in range(co):
                t[c, (3 * c + i) % ci, (c + i) % 9] = s
                t[c, (5 * c + 7 + i) % ci, (c + 4 + 2 * i) % 9] = -s
                t[c].view(-1)[int(rnd[c])] = s
            w[f"conv.{i}.weight"] = t.view(co, ci, 3, 3)
            w[f"conv.{i}.bias"] = torch.tensor([DYADIC[(2 * c + i) % len(DYADIC)] for c in range(co)])
        else:
            w[f"conv.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
            w[f"conv.{i}.bias"] = torch.randn(co, generator=g) * 0.05
    for l, t in enumerate(LPIPS_TAPS):
        w[f"lin.{l}"] = torch.rand(CH[t][1], generator=g)          # non-negative
    if family == "exact":
        w["shift"], w["scale"] = torch.zeros(3), torch.ones(3)
    if family == "small":        # the second tapped convolution's output times 2^-17 (an exact scaling of its weights and bias)
        i = LPIPS_TAPS[1]
        w[f"conv.{i}.weight"], w[f"conv.{i}.bias"] = w[f"conv.{i}.weight"] * SMALL, w[f"conv.{i}.bias"] * SMALL
    return metrics.lpips_weights_from(w)


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """Weights, pred (B,3,H,W) with values outside [0, 1], gt (B,H,W,3), mask (B,H,W) and the crop; `seed` > 0: the same kind of case
    from other random numbers (the 8 seeds of the scalars' E_ref)."""
    B, H, W, crop, masked, family = CASES[name]
    base = 1000 * list(CASES).index(name) + 17 * seed
    g = torch.Generator().manual_seed(base + 1)
    if family == "exact":
        pred = torch.randint(-3, 12, (B, 3, H, W), generator=g).float() / 8.0
        gt = torch.randint(0, 9, (B, H, W, 3), generator=g).float() / 8.0
    else:
        pred = torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2
        gt = torch.rand(B, H, W, 3, generator=g)
    y0, x0, h, w = crop or (0, 0, H, W)
    mask = torch.ones(B, H, W)
    if masked:     # about a third of the pixels off, whole border rows of the cropped image among them
        mask = (torch.rand(B, H, W, generator=g) >= 0.3).float()
        mask[:, y0] = 0.0
        mask[:, y0 + h - 1] = 0.0
        mask[:, y0 + h - 2, x0:x0 + w // 2] = 0.5        # below 1: off
    return dict(name=name, B=B, H=H, W=W, crop=(y0, x0, h, w), h=h, w=w, family=family, pred=pred, gt=gt, mask=mask,
                weights=_weights(base, family))


def _wire(c):
    """The evaluator's wiring: clamp pred, crop both, zero both except where mask >= 1: a, b (B,3,h,w)."""
    y0, x0, h, w = c["crop"]
    keep = (c["mask"] >= 1)[:, y0:y0 + h, x0:x0 + w]
    a = c["pred"].clamp(0.0, 1.0)[:, :, y0:y0 + h, x0:x0 + w].clone()
    b = c["gt"].permute(0, 3, 1, 2)[:, :, y0:y0 + h, x0:x0 + w].clone()
    a[~keep[:, None].expand_as(a)] = 0.0
    b[~keep[:, None].expand_as(b)] = 0.0
    return a, b


def _w64(w):
    return {k: v.double() for k, v in w.items()}


def _apply(w, point, st, B):
    """Point `point` from its stored inputs `st`, in the dtype of the weights `w`: the restatement's own functions, one at a time."""
    dt = w["shift"].dtype
    with torch.no_grad():
        if point == "scaled":
            return lpips_scale(st["img"].to(dt), w["shift"], w["scale"])
        kind, _, k = point.partition(".")
        if kind == "conv":
            return lpips_conv(st[_input_of(int(k))].to(dt), w[f"conv.{k}.weight"], w[f"conv.{k}.bias"])
        if kind == "pool":
            return lpips_pool(st[f"conv.{LPIPS_TAPS[int(k)]}"].to(dt))
        if kind == "t":
            x = st[f"conv.{LPIPS_TAPS[int(k)]}"].to(dt)
            return lpips_tap(x[:B], x[B:], w[f"lin.{k}"])
        total = st["t.0"].to(dt)
        for l in range(1, 5):
            total = total + st[f"t.{l}"].to(dt)
        return total


def _chain(w, img, B, replace=None):
    st = {"img": img}
    for p in POINTS:
        st[p] = replace[p](st) if replace and p in replace else _apply(w, p, st, B)
    return st


# ---- the second fp32 realisation ---------------------------------------------------------------------------------------------
def _apply2(w, point, st, B):
    with torch.no_grad():
        if point == "scaled":
            return ((st["img"] * 2.0 - 1.0) - w["shift"].view(1, 3, 1, 1)) * (1.0 / w["scale"]).view(1, 3, 1, 1)
        kind, _, k = point.partition(".")
        if kind == "conv":
            x = st[_input_of(int(k))]
            n, _, h, wd = x.shape
            cols = F.unfold(x, 3, padding=1).flip(1)                            # (n, cin 9, h w), k reversed
            wm = w[f"conv.{k}.weight"].reshape(w[f"conv.{k}.weight"].shape[0], -1).flip(1)
            y = torch.matmul(wm, cols) + w[f"conv.{k}.bias"].view(1, -1, 1)
            return torch.relu(y).view(n, -1, h, wd)
        if kind == "pool":
            x = st[f"conv.{LPIPS_TAPS[int(k)]}"]
            h2, w2 = x.shape[2] // 2 * 2, x.shape[3] // 2 * 2
            return torch.maximum(torch.maximum(x[:, :, 0:h2:2, 0:w2:2], x[:, :, 0:h2:2, 1:w2:2]),
                                 torch.maximum(x[:, :, 1:h2:2, 0:w2:2], x[:, :, 1:h2:2, 1:w2:2]))
        if kind == "t":
            x = st[f"conv.{LPIPS_TAPS[int(k)]}"]
            fa, fb, lin = x[:B].flip(1), x[B:].flip(1), w[f"lin.{k}"].flip(0)
            na = torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10
            nb = torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10
            d = (((fa / na - fb / nb) ** 2) * lin.view(1, -1, 1, 1)).sum(1)
            return d.flatten(1).flip(1).sum(1) / d[0].numel()
        total = st["t.4"]
        for l in (3, 2, 1, 0):
            total = total + st[f"t.{l}"]
        return total


# ---- the referee -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_chain(name, seed=0):
    c = _case(name, seed)
    a, b = _wire(c)
    img = torch.cat([a, b])
    return c, img, _chain(c["weights"], img, c["B"])


@functools.lru_cache(maxsize=None)
def _scalar_eref(name):
    """Per scalar point the maximum over SEEDS seeds of the fp32 chain's error at this case's shape: for t_l and "total" against
    float64 on the chain's own stored input, for "e2e" the chain's total against the float64 chain on the image."""
    out = {p: 0.0 for p in SCALARS | {"e2e"}}
    for s in range(SEEDS):
        c, img, st = _cpu_chain(name, s)
        w64 = _w64(c["weights"])
        for p in SCALARS:
            out[p] = max(out[p], float((st[p].double() - _apply(w64, p, st, c["B"])).abs().max()))
        out["e2e"] = max(out["e2e"], float((st["total"].double() - _chain(w64, img.double(), c["B"])["total"]).abs().max()))
    return out


def _judge(c, stored, got, e8):
    """Every point on the stored activations `stored` (the image included): ref64, E_ref, the floor, the bound, and the error of
    got[point]."""
    w, w64, B = c["weights"], _w64(c["weights"]), c["B"]
    out = {}
    for p in POINTS:
        ref64 = _apply(w64, p, stored, B)
        cpu32 = _apply(w, p, stored, B)
        assert ref64.dtype == torch.float64 and cpu32.dtype == torch.float32
        same_shape = tuple(ref64.shape) == tuple(got[p].shape)
        e_ref = e8[p] if p in SCALARS else float((cpu32.double() - ref64).abs().max())
        top = float(ref64.abs().max())
        floor = 8 * _ulp32(top)
        bound = 0.0 if p.startswith("pool") else max(K_RULE * e_ref, floor)       # pooled maps: bit-exact
        err = float((got[p].double() - ref64).abs().max()) if same_shape else float("inf")      # every element: nothing is excluded
        out[p] = dict(ref64=ref64, e_ref=e_ref, top=top, floor=floor, bound=bound, err=err, excluded=0)
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    assert [(_case(n)["h"], _case(n)["w"], _case(n)["B"]) for n in list(CASES)[:4]] == [(16, 16, 1), (17, 35, 1), (32, 96, 2), (33, 47, 2)]
    assert _case("33x47-crop")["crop"][:2] == (3, 5) and (_case("33x47-crop")["H"], _case("33x47-crop")["W"]) == (40, 56)
    for n in ("17x35", "33x47-crop"):
        c = _case(n)
        y0, x0, h, w = c["crop"]
        m = c["mask"][:, y0:y0 + h, x0:x0 + w]
        off = float((m < 1).float().mean())
        assert 0.25 <= off <= 0.45, off                                       # about a third
        assert bool((m[:, 0] < 1).all()) and bool((m[:, -1] < 1).all())       # whole border rows
        assert bool(((m > 0) & (m < 1)).any())                                # and values below 1 that are not 0
    for n in CASES:
        c = _case(n)
        assert float(c["pred"].min()) < 0 and float(c["pred"].max()) > 1, n   # the clamp has work to do
    dims = [(17 >> g, 35 >> g) for g in range(5)]
    assert dims == [(17, 35), (8, 17), (4, 8), (2, 4), (1, 2)] and (16 >> 4) == 1
    assert len(POINTS) == 1 + 13 + 4 + 5 + 1
    # the restatement's chain of points IS lpips_torch
    c, img, st = _cpu_chain("17x35")
    a, b = _wire(c)
    assert torch.equal(st["total"], lpips_torch(a, b, c["weights"]))


@ALL
def test_lpips_case_referee(name):
    """CPU half: the fp32 CPU chain stands in for the kernel's stored activations; the second fp32 realisation must pass the rule at
    every point on those stored inputs; the layout the library reports matches the restated shapes; the exact family is exact."""
    c, img, stored = _cpu_chain(name)
    e8 = _scalar_eref(name)
    second = {p: _apply2(c["weights"], p, stored, c["B"]) for p in POINTS}
    j1, j2 = _judge(c, stored, stored, e8), _judge(c, stored, second, e8)
    lay = metrics.lpips_layout(c["B"], c["h"], c["w"], metrics.LPIPS_KEEP)
    assert list(lay)[:18] == ["scaled"] + [p for p in POINTS if p.startswith(("conv", "pool"))] and list(lay)[18:] == ["taps", "partials"]
    end = 0
    for p in POINTS:
        v, v2 = j1[p], j2[p]
        print(f"[lpips referee cpu] {name} {p}: E_ref {v['e_ref']:.3e}  floor {v['floor']:.3e}  bound {v['bound']:.3e}  "
              f"max|ref64| {v['top']:.3e}  second realisation err/bound {v2['err'] / v2['bound'] if v2['bound'] else v2['err']:.3f}")
        assert torch.isfinite(v["ref64"]).all() and v["excluded"] == EXCLUDED_CAP == 0
        assert v["err"] <= v["bound"] and v2["err"] <= v2["bound"], (p, v["err"], v2["err"], v["bound"])
        if p in lay:
            off, nbytes, shape = lay[p]
            n, ch, hh, ww = stored[p].shape
            assert shape == (n, hh, ww, ch) and nbytes == 4 * n * ch * hh * ww and off >= end and off % 256 == 0, p
            end = off + nbytes
    assert lay["taps"][0] >= end and lay["taps"][1] == 8 * c["B"] * 5
    assert metrics.lpips_workspace_bytes(c["B"], c["h"], c["w"], metrics.LPIPS_KEEP) >= lay["partials"][0] + lay["partials"][1]
    e2e = float((stored["total"].double() - _chain(_w64(c["weights"]), img.double(), c["B"])["total"]).abs().max())
    print(f"[lpips referee cpu] {name}: fp32 chain end to end {e2e:.3e}, 8-seed maximum {e8['e2e']:.3e}; total {stored['total'].tolist()}")
    assert e2e <= e8["e2e"] and float(stored["total"].min()) > 0
    if c["family"] == "exact":       # fp32 arithmetic in any order lands on the float64 values at every convolution point
        assert float(c["weights"]["shift"].abs().max()) == 0 and bool((c["weights"]["scale"] == 1).all())
        assert torch.equal(img * 8, (img * 8).round())
        for p in ["scaled"] + CONVS:
            assert j1[p]["e_ref"] == 0.0 and torch.equal(stored[p].double(), j1[p]["ref64"]), p
            assert torch.equal(second[p].double(), j1[p]["ref64"]), p
            assert int(torch.count_nonzero(j1[p]["ref64"])) > 0 and len(torch.unique(j1[p]["ref64"])) > 2 and j1[p]["top"] < 2 ** 20, p
    else:
        assert all(j1[p]["e_ref"] > 0 for p in POINTS if not p.startswith("pool")), {p: j1[p]["e_ref"] for p in POINTS}
        for p in CONVS:
            if c["family"] == "small" and p == f"conv.{LPIPS_TAPS[1]}":
                x = stored[p]
                norms = torch.sqrt((x.double() ** 2).sum(1))
                assert 0.05 * SMALL < j1[p]["top"] < 50.0 * SMALL and 1e-6 < float(norms.min()) and float(norms.max()) < 1e-3, p
                # here eps inside the root is another number: sqrt(n^2 + 1e-10) against n + 1e-10 differs by more than 1e-4 of n
                assert float(((torch.sqrt(norms ** 2 + 1e-10) - (norms + 1e-10)) / norms).min()) > 1e-4
            elif c["family"] == "small" and int(p.split(".")[1]) > LPIPS_TAPS[1]:
                assert 0.01 < j1[p]["top"] < 50.0, (p, j1[p]["top"])   # behind it the biases carry the activations
            else:
                assert 0.05 < j1[p]["top"] < 50.0, (p, j1[p]["top"])   # He scaling keeps the activations O(1)


# ---- CPU: slips the rule must catch ------------------------------------------------------------------------------------------
SLIP_CASE = "17x35"
EPS_SLIP_CASE = "small-17x35"      # where a pixel's feature norm at the second tap is of the order of 1e-5


def _slips(c):
    """{slip: (point, function of the stored inputs)}: one mistake each, in the fp32 CPU restatement."""
    w, B = c["weights"], c["B"]
    y0, x0, h, wd = c["crop"]
    sh, sc = w["shift"].view(1, 3, 1, 1), w["scale"].view(1, 3, 1, 1)

    def tap_of(l, feats, lin=None):
        return lambda st: (lambda x: lpips_tap(x[:B], x[B:], w[f"lin.{l}"] if lin is None else lin))(feats(st))

    def pre_relu(st):
        i = LPIPS_TAPS[2]
        return F.conv2d(st[_input_of(i)], w[f"conv.{i}.weight"], w[f"conv.{i}.bias"], padding=1)

    def eps_inside(st):
        x = st[f"conv.{LPIPS_TAPS[1]}"]
        fa, fb = x[:B], x[B:]
        na = torch.sqrt(torch.sum(fa ** 2, dim=1, keepdim=True) + 1e-10)
        nb = torch.sqrt(torch.sum(fb ** 2, dim=1, keepdim=True) + 1e-10)
        return F.conv2d((fa / na - fb / nb) ** 2, w["lin.1"].view(1, -1, 1, 1)).mean(dim=(2, 3))[:, 0]

    lin = w["lin.3"].clone()
    i0, i1 = int(lin.argmax()), int(lin.argmin())
    lin[i0], lin[i1] = w["lin.3"][i1], w["lin.3"][i0]

    def mask_after_map(st):
        keep = (c["mask"] >= 1)[:, y0:y0 + h, x0:x0 + wd]
        a = c["pred"].clamp(0.0, 1.0)[:, :, y0:y0 + h, x0:x0 + wd] * 2.0 - 1.0
        b = c["gt"].permute(0, 3, 1, 2)[:, :, y0:y0 + h, x0:x0 + wd] * 2.0 - 1.0
        x = torch.cat([a * keep[:, None], b * keep[:, None]])
        return (x - sh) / sc

    def pad_before_scaling(st):
        x = F.pad(st["img"] * 2.0 - 1.0, (1, 1, 1, 1))       # the zero border goes through the scaling layer: (0 - shift) / scale
        return F.relu(F.conv2d((x - sh) / sc, w["conv.0.weight"], w["conv.0.bias"], padding=0))

    return {
        "pool with ceil": ("pool.0", lambda st: F.max_pool2d(st[f"conv.{LPIPS_TAPS[0]}"], 2, 2, ceil_mode=True)),
        "eps inside the root": ("t.1", eps_inside),
        "tap taken after the pool": ("t.0", tap_of(0, lambda st: st["pool.0"])),
        "tap before the ReLU": ("t.2", tap_of(2, pre_relu)),
        "two tap-weight channels swapped": ("t.3", tap_of(3, lambda st: st[f"conv.{LPIPS_TAPS[3]}"], lin)),
        "shift and scale exchanged": ("scaled", lambda st: ((st["img"] * 2.0 - 1.0) - sc) / sh),
        "masked pixels set to 0 after the 2x - 1 map": ("scaled", mask_after_map),
        "zero padding applied before the scaling layer": ("conv.0", pad_before_scaling),
    }


SLIPS = ["pool with ceil", "eps inside the root", "tap taken after the pool", "tap before the ReLU", "two tap-weight channels swapped",
         "shift and scale exchanged", "masked pixels set to 0 after the 2x - 1 map", "zero padding applied before the scaling layer"]


@pytest.mark.parametrize("slip", SLIPS)
def test_rule_catches_a_slip_at_its_own_point(slip):
    """No kernel here: one wrong fp32 CPU layer per slip, fed the fp32 chain's stored activations; its error against the float64 referee
    exceeds the rule's bound at that layer's own point.  `eps inside the root` changes a value only where a pixel's feature norm is of
    the order of 1e-5, so that slip is judged on the case whose second tapped convolution is scaled by 2^-17 - a case the GPU runs
    too, so the kernel's own eps is held to the same point."""
    case = EPS_SLIP_CASE if slip == "eps inside the root" else SLIP_CASE
    c, img, stored = _cpu_chain(case)
    assert set(_slips(c)) == set(SLIPS)
    point, fn = _slips(c)[slip]
    e8 = dict(_scalar_eref(case))
    with torch.no_grad():
        wrong = fn(stored)
    got = dict(stored, **{point: wrong})
    right = dict(stored, **{point: _apply(c["weights"], point, stored, c["B"])})
    v, ok = _judge(c, stored, got, e8)[point], _judge(c, stored, right, e8)[point]
    print(f"[lpips slip] {slip} at {point}: err {v['err']:.3e}  bound {v['bound']:.3e}; without the slip err {ok['err']:.3e}")
    assert ok["err"] <= ok["bound"]          # the point itself passes ...
    assert v["err"] > v["bound"]             # ... and the slip does not


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _run_hip(c, flags=metrics.LPIPS_KEEP, fill=float("nan")):
    """gdb_eval_lpips on a workspace of the test's own (`fill` beforehand): ({point: CPU tensor}, the record (B,) float64)."""
    B, h, w = c["B"], c["h"], c["w"]
    packed = metrics.pack_lpips(c["weights"], "cuda")
    nbytes = metrics.lpips_workspace_bytes(B, h, w, flags)
    ws = torch.full(((nbytes + 7) // 8,), fill, dtype=torch.float64, device="cuda")
    rec = torch.full((B, 3), fill, dtype=torch.float64, device="cuda")
    metrics.eval_lpips(c["pred"].cuda(), c["gt"].cuda(), c["mask"].cuda(), packed, rec[:, 1:], c["crop"], flags=flags, workspace=ws)
    torch.cuda.synchronize()
    raw = ws.cpu()
    got = {}
    if flags & metrics.LPIPS_KEEP:
        f32 = raw.view(torch.float32)
        for name, (off, nb, shape) in metrics.lpips_layout(B, h, w, flags).items():
            if name == "taps":
                t = raw[off // 8:off // 8 + B * 5].view(B, 5)
                got.update({f"t.{l}": t[:, l].clone() for l in range(5)})
            elif name != "partials":
                got[name] = f32[off // 4:(off + nb) // 4].view(shape).permute(0, 3, 1, 2).contiguous()
    rec = rec.cpu()
    assert bool(torch.isnan(rec[:, 0]).all()) and bool(torch.isnan(rec[:, 2]).all()) if fill != fill else True    # only its own column
    got["total"] = rec[:, 1].clone()
    return got


@pytest.mark.gpu
@ALL
def test_hip_lpips_every_point_vs_float64(name):
    """Every stored point of every case on the GPU against the float64 referee on the kernel's own stored input, under the rule of the
    module docstring; pooled maps and the exact family's convolution points bit for bit; the total end to end against the float64 chain
    on the image.  Prints one line per point with the observed err / bound (records under profiles/lpips/)."""
    c, img, _ = _cpu_chain(name)
    e8 = _scalar_eref(name)
    got = _run_hip(c)
    assert set(got) == set(POINTS)
    for p in POINTS:
        assert bool(torch.isfinite(got[p]).all()), p
    stored = dict(got, img=img)
    j = _judge(c, stored, got, e8)
    failed = []
    for p in POINTS:
        v = j[p]
        ratio = v["err"] / v["bound"] if v["bound"] else (0.0 if v["err"] == 0 else float("inf"))
        print(f"[lpips referee] {name} {p}: E_ref {v['e_ref']:.3e}  hip err {v['err']:.3e}  bound {v['bound']:.3e}  err/bound {ratio:.3f}  "
              f"max|ref64| {v['top']:.3e}  excluded {v['excluded']}")
        assert v["excluded"] == EXCLUDED_CAP == 0
        if not v["err"] <= v["bound"]:
            failed.append((p, v["err"], v["bound"]))
        if c["family"] == "exact" and (p == "scaled" or p.startswith("conv")) and not torch.equal(got[p].double(), v["ref64"]):
            failed.append((p, "not bit for bit", v["err"]))
    ref = _chain(_w64(c["weights"]), img.double(), c["B"])["total"]
    e2e, bound = float((got["total"] - ref).abs().max()), max(K_RULE * e8["e2e"], 8 * _ulp32(float(ref.abs().max())))
    print(f"[lpips referee] {name}: total {got['total'].tolist()} end to end err {e2e:.3e}  bound {bound:.3e}  err/bound {e2e / bound:.3f}")
    assert not failed, failed
    assert e2e <= bound

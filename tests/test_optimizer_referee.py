"""gdb_adam_step (through optim.HipAdam) against its definition in float64.

Rule, that of tests/test_loss_referee.py, per tensor for param, exp_avg, exp_avg_sq and the written-back grad:
    |hip - ref64| <= 4 * max(E32, 8 fp32 ulp of max |ref64|)
ref64 = the header's formula in float64 numpy from the shared fp32 state; E32 = |torch.optim.Adam / AdamW on the CPU in float32
(foreach=False, after clip_grad_value_) - ref64|.  Non-finite values are compared as a pattern first: NaN and +-inf must sit where
torch's float32 result has them, in all four arrays; the rule then runs over the finite elements.

Every case runs one step from the same state at t = 1 and at t = 1000; three cases also run five consecutive steps with fresh
gradients.  Every array sits between sentinel words inside a larger buffer, and those must be unchanged after the call.  The sizes
come from the kernel's own constants (chunk, table, vector width), read from csrc/gdb_optim.hip.

Observed |hip - ref64| / bound: profiles/optimizer/referee_observed.txt (rewritten by a run of this file)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gdb_nerf_amd.optim import HipAdam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = os.path.join(ROOT, "profiles", "optimizer", "referee_observed.txt")
_SRC = open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "gdb_optim.hip")).read()
CHUNK = int(re.search(r"#define OPT_CHUNK (\d+)", _SRC).group(1))
TABLE = int(re.search(r"#define OPT_TABLE (\d+)", _SRC).group(1))
VEC = 4            # floats per 16-byte access
GUARD = 8          # sentinel words before and after every array (a multiple of VEC: offset 0 keeps the array 16-byte aligned)
SENTINEL = np.float32(-12345.678)
CLIP = 40.0
BASE = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
_observed = {}


def T(numel, offset=0, grad="normal", no_grad=False, **hyper):
    """One tensor of a case: `offset` elements into its buffer (1: 4-byte aligned only), the kind of gradient, its group's hyper-parameters."""
    return dict(numel=numel, offset=offset, grad=grad, no_grad=no_grad, hyper={**BASE, **hyper})


def _special(n):
    """Gradients at exactly +-40, beyond, +-inf and one NaN, the rest ordinary; every one at least once when n allows."""
    vals = [40.0, -40.0, 40.000004, -40.000004, 1e30, -1e30, np.inf, -np.inf, np.nan, 39.999996, -39.999996, 0.0, -0.0]
    g = np.random.default_rng(n).standard_normal(n).astype(np.float32) * 30
    idx = np.random.default_rng(n + 1).permutation(n)[:len(vals)]
    g[idx] = np.array(vals[:len(idx)], np.float32)
    return g


MIXED = [1, 3, CHUNK + 1, 5, 64, 2 * CHUNK + 3, 7, 1, 130, CHUNK - 1, 2, 17]
CASES = {
    "numel_1_and_3": dict(tensors=[T(1), T(3)]),
    "chunk_and_chunk_pm_1": dict(tensors=[T(CHUNK), T(CHUNK - 1), T(CHUNK + 1)]),
    "vector_width_pm_1": dict(tensors=[T(VEC - 1), T(VEC), T(VEC + 1)]),
    "views_at_element_offset_1": dict(tensors=[T(CHUNK + 5, offset=1), T(3, offset=1), T(VEC, offset=1), T(2 * CHUNK, offset=1)], steps5=True),
    "table_exactly_full": dict(tensors=[T(MIXED[i % len(MIXED)]) for i in range(TABLE)]),
    "table_plus_one_two_launches": dict(tensors=[T(MIXED[i % len(MIXED)]) for i in range(TABLE + 1)], steps5=True),
    "grad_none_in_the_middle": dict(tensors=[T(CHUNK + 2), T(33, no_grad=True), T(6)]),
    "numel_0": dict(tensors=[T(9), T(0), T(5)]),
    "clip_edges_inf_nan": dict(tensors=[T(CHUNK + 13, grad="special"), T(13, grad="special", offset=1)]),
    "tiny_gradients_eps_dominates": dict(tensors=[T(VEC * 3 + 1, grad="tiny"), T(CHUNK + 1, grad="tiny")]),
    "weight_decay_adam": dict(tensors=[T(CHUNK + 7, weight_decay=0.01), T(10, weight_decay=0.01)], steps5=True),
    "weight_decay_adamw": dict(tensors=[T(CHUNK + 7, weight_decay=0.01), T(10, weight_decay=0.01)], decoupled=True),
    "lr_and_eps_per_group": dict(tensors=[T(50, lr=1e-2, eps=1e-6), T(CHUNK + 50, lr=3e-4, eps=1e-10, betas=(0.8, 0.99)), T(5, lr=0.0), T(7, betas=(0.0, 0.0))]),
    "no_clip": dict(tensors=[T(CHUNK + 9, grad="wide"), T(11, grad="wide", offset=1)], clip=None),
}


def _state(case, seed, steps):
    """Shared fp32 state: per tensor p, m, v and `steps` gradients."""
    out = []
    for i, t in enumerate(CASES[case]["tensors"]):
        rng = np.random.default_rng([seed, i])
        n = t["numel"]
        p = rng.standard_normal(n).astype(np.float32)
        m = (0.1 * rng.standard_normal(n)).astype(np.float32)
        v = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
        if t["grad"] == "tiny":
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
            gs = [np.full(n, 1e-20, np.float32) * (1 if k % 2 == 0 else -1) for k in range(steps)]
        elif t["grad"] == "special":
            gs = [_special(n) for _ in range(steps)]
        elif t["grad"] == "wide":
            gs = [(rng.standard_normal(n) * 100).astype(np.float32) for _ in range(steps)]
        else:
            gs = [(rng.standard_normal(n) * 25).astype(np.float32) for _ in range(steps)]   # a few percent lie beyond the clip
        out.append(dict(p=p, m=m, v=v, grads=gs))
    return out


def ref64(case, state, t0, steps):
    """The header's formula, float64 numpy -> per tensor {param, exp_avg, exp_avg_sq, grad} (grad: as the last step left it)."""
    c = CASES[case]
    clip, decoupled = c.get("clip", CLIP), c.get("decoupled", False)
    out = []
    with np.errstate(all="ignore"):
        for t, s in zip(c["tensors"], state):
            p, m, v = (s[k].astype(np.float64) for k in ("p", "m", "v"))
            h = t["hyper"]
            (b1, b2), lr, eps, wd = h["betas"], h["lr"], h["eps"], h["weight_decay"]
            g = None
            if not t["no_grad"]:
                for k in range(steps):
                    step = t0 + k + 1
                    g = s["grads"][k].astype(np.float64)
                    if clip:
                        g = np.where(g < -clip, -clip, np.where(g > clip, clip, g))     # NaN stays NaN
                    gg = g
                    if wd:
                        if decoupled:
                            p = p * (1 - lr * wd)
                        else:
                            gg = g + wd * p
                    m = m + (gg - m) * (1 - b1)
                    v = v * b2
                    v = v + (1 - b2) * gg * gg
                    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
                    p = p - (lr / (1 - b1 ** step)) * (m / denom)
            out.append({"param": p, "exp_avg": m, "exp_avg_sq": v, "grad": g})
    return out


def torch32(case, state, t0, steps):
    """torch.optim.Adam / AdamW on the CPU, float32, foreach=False, after clip_grad_value_."""
    c = CASES[case]
    clip, decoupled = c.get("clip", CLIP), c.get("decoupled", False)
    params = [nn.Parameter(torch.from_numpy(s["p"].copy())) for s in state]
    Opt = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = Opt([{"params": [p], **t["hyper"]} for p, t in zip(params, c["tensors"])], foreach=False)
    for p, s in zip(params, state):
        opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(s["m"].copy()), "exp_avg_sq": torch.from_numpy(s["v"].copy())}
    for k in range(steps):
        for p, s, t in zip(params, state, c["tensors"]):
            p.grad = None if t["no_grad"] else torch.from_numpy(s["grads"][k].copy())
        if clip:
            torch.nn.utils.clip_grad_value_(params, clip)
        opt.step()
    f = lambda x: x.detach().double().numpy()
    return [{"param": f(p), "exp_avg": f(opt.state[p]["exp_avg"]), "exp_avg_sq": f(opt.state[p]["exp_avg_sq"]), "grad": None if p.grad is None else f(p.grad)}
            for p in params]


class Guarded:
    """`numel` floats at `offset` elements past GUARD sentinel words of a CUDA buffer, GUARD + (VEC - offset) sentinel words behind."""

    def __init__(self, values, offset):
        n = values.size
        self.lo, self.n = GUARD + offset, n
        host = np.full(self.lo + n + GUARD + VEC, SENTINEL, np.float32)
        host[self.lo:self.lo + n] = values
        self.buf = torch.from_numpy(host).cuda()
        self.view = self.buf[self.lo:self.lo + n]
        assert self.buf.data_ptr() % 16 == 0 and (self.view.data_ptr() % 16 == 0) == (offset % VEC == 0 or n == 0)

    def values(self):
        return self.view.detach().cpu().numpy().copy()

    def guards_intact(self):
        host = self.buf.cpu().numpy().view(np.uint32)
        want = np.float32(SENTINEL).view(np.uint32)
        return bool((host[:self.lo] == want).all() and (host[self.lo + self.n:] == want).all())


def hip(case, state, t0, steps):
    """-> per tensor {param, exp_avg, exp_avg_sq, grad} as float32 numpy, after asserting guards, steps and untouched tensors."""
    c = CASES[case]
    clip, decoupled = c.get("clip", CLIP), c.get("decoupled", False)
    arrays, params = [], []
    for t, s in zip(c["tensors"], state):
        a = {k: Guarded(s[k], t["offset"]) for k in ("p", "m", "v")}
        arrays.append(a)
        params.append(nn.Parameter(a["p"].view))
        assert params[-1].data_ptr() == a["p"].view.data_ptr()
    opt = HipAdam([{"params": [p], **t["hyper"]} for p, t in zip(params, c["tensors"])], decoupled=decoupled, clip_value=clip)
    for p, a, t in zip(params, arrays, c["tensors"]):
        if t0 or not t["no_grad"]:       # at t = 1 the gradient-less tensor has no state at all: none may be created
            opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": a["m"].view, "exp_avg_sq": a["v"].view}
    grads = [None] * len(params)
    for k in range(steps):
        for i, (p, s, t) in enumerate(zip(params, state, c["tensors"])):
            grads[i] = None if t["no_grad"] else Guarded(s["grads"][k], t["offset"])     # a fresh allocation per step, as under zero_grad
            p.grad = None if t["no_grad"] else grads[i].view
        opt.step()
        for i, (p, a, t) in enumerate(zip(params, arrays, c["tensors"])):
            assert all(x.guards_intact() for x in a.values()) and (grads[i] is None or grads[i].guards_intact()), (case, i, "sentinel words changed")
    torch.cuda.synchronize()
    out = []
    for p, a, g, t, s in zip(params, arrays, grads, c["tensors"], state):
        if t["no_grad"]:                 # bytes unchanged, step neither created nor advanced
            assert all(np.array_equal(a[k].values().view(np.uint32), s[k].view(np.uint32)) for k in ("p", "m", "v")), case
            assert (p not in opt.state or len(opt.state[p]) == 0) if t0 == 0 else float(opt.state[p]["step"]) == float(t0), case
        else:
            st = opt.state[p]["step"]
            assert st.dtype == torch.float32 and st.device.type == "cpu" and st.dim() == 0 and float(st) == float(t0 + steps), case
        out.append({"param": a["p"].values(), "exp_avg": a["m"].values(), "exp_avg_sq": a["v"].values(), "grad": None if g is None else g.values()})
    return out


def check_rule(tag, got, r64, r32):
    """Prints each figure, records it, then asserts the pattern and the rule for every tensor and array."""
    fails = []
    for i, (h, a, b) in enumerate(zip(got, r64, r32)):
        for name in ("param", "exp_avg", "exp_avg_sq", "grad"):
            if a[name] is None:
                assert h[name] is None and b[name] is None
                continue
            hv, av, bv = np.asarray(h[name], np.float64), a[name], b[name]
            assert hv.shape == av.shape == bv.shape, (tag, i, name)
            if hv.size == 0:
                continue
            same_pattern = (np.array_equal(np.isnan(hv), np.isnan(bv)) and np.array_equal(np.isposinf(hv), np.isposinf(bv))
                            and np.array_equal(np.isneginf(hv), np.isneginf(bv)))
            fin = np.isfinite(bv) & np.isfinite(av)
            top = float(np.abs(av[fin]).max()) if fin.any() else 0.0
            e32 = float(np.abs(bv[fin] - av[fin]).max()) if fin.any() else 0.0
            bound = 4.0 * max(e32, 8.0 * float(np.spacing(np.float32(top))))
            err = float(np.abs(hv[fin] - av[fin]).max()) if fin.any() and same_pattern else (0.0 if same_pattern else float("inf"))
            line = (f"{tag:44s} t{i:<3d} {name:10s} n {hv.size:<6d} err {err:.3e}  bound {bound:.3e}  err/bound {err / bound:.3f}  "
                    f"max|ref64| {top:.3e}  nonfinite {int((~np.isfinite(bv)).sum())}")
            if i < 4 or not err <= bound:
                print(line)
            key = (tag, name)
            if key not in _observed or err / bound > _observed[key][0]:
                _observed[key] = (err / bound, line)
            if not (same_pattern and err <= bound):
                fails.append(line + ("" if same_pattern else "  NaN / inf pattern differs from torch's"))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        old = {}
        if os.path.exists(OBSERVED):
            for l in open(OBSERVED):
                if l.strip() and not l.startswith("#"):
                    parts = l.split()
                    old[(parts[0], parts[2])] = l.rstrip("\n")
        old.update({k: v[1] for k, v in _observed.items()})
        with open(OBSERVED, "w") as f:
            f.write("# worst tensor per case and array: |hip - ref64| against the bound 4 * max(E32, 8 ulp of max |ref64|); tests/test_optimizer_referee.py\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError:
        pass
    assert not fails, "\n".join(fails)


_refs = {}


def _references(case, t0, steps):
    """ref64 and torch32 of a (case, t0, steps), computed once and shared."""
    key = (case, t0, steps)
    if key not in _refs:
        state = _state(case, 7, steps)
        _refs[key] = (state, ref64(case, state, t0, steps), torch32(case, state, t0, steps))
    return _refs[key]


@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("case", list(CASES))
def test_one_step_vs_float64(case, t):
    state, r64, r32 = _references(case, t - 1, 1)
    check_rule(f"{case}/t={t}", hip(case, state, t - 1, 1), r64, r32)


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c].get("steps5")])
def test_five_steps_vs_float64(case):
    state, r64, r32 = _references(case, 0, 5)
    check_rule(f"{case}/5_steps", hip(case, state, 0, 5), r64, r32)


def test_nan_pattern_equals_torchs():
    """The one NaN gradient: NaN in grad, exp_avg, exp_avg_sq and param at that element and nowhere else; +-inf clamp to +-40."""
    state, r64, r32 = _references("clip_edges_inf_nan", 0, 1)
    got = hip("clip_edges_inf_nan", state, 0, 1)
    for h, b, s in zip(got, r32, state):
        at = np.isnan(s["grads"][0])
        assert at.sum() == 1
        for name in ("param", "exp_avg", "exp_avg_sq", "grad"):
            assert np.array_equal(np.isnan(h[name]), at), name
            assert np.array_equal(np.isnan(b[name]), at), name
            assert np.isfinite(h[name][~at]).all(), name
        assert np.array_equal(h["grad"][~at].view(np.uint32), b["grad"][~at].astype(np.float32).view(np.uint32))   # the clamp is exact
        assert float(np.abs(h["grad"][~at]).max()) == CLIP


def test_two_calls_from_identical_state_give_identical_bits():
    for case in ("table_plus_one_two_launches", "views_at_element_offset_1", "clip_edges_inf_nan"):
        state = _references(case, 0, 1)[0]
        a, b = hip(case, state, 0, 1), hip(case, state, 0, 1)
        for x, y in zip(a, b):
            for name in x:
                assert (x[name] is None and y[name] is None) or np.array_equal(x[name].view(np.uint32), y[name].view(np.uint32)), (case, name)

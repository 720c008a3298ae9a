"""The surface of the one-call optimiser step: the exported entry, its refusals, the compiler's resource report, the
`train.hip_optimizer` switch, `make_optimizer`'s recipe and `HipAdam`'s constructor - no GPU - and, on the GPU, `HipAdam`'s refusals,
the version bump that makes the next forward see the new weights, and the interchange of optimiser state with torch.optim.Adam / AdamW."""
import copy
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gdb_nerf_amd import _lib, build
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.optim import HipAdam
from gdb_nerf_amd.train import make_optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "gdb_optim.hip"


def test_entry_is_declared_bound_and_built():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    assert "int gdb_adam_step(" in header and "gdb_adam_step" in _lib.EXPORTS and lib.gdb_adam_step is not None
    assert lib.gdb_abi_version() == 7 and "#define GDB_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    assert SRC in build.SOURCES and build.CONTRACT[SRC] == "off"
    assert len(_lib._SIGNATURES["gdb_adam_step"][1]) == 15


def test_kernel_uses_no_private_memory_and_its_table_fits():
    usage = json.load(open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json")))
    kernels = {k: v for k, v in usage[SRC].items() if "k_adam_step" in k}
    assert len(kernels) == 1, sorted(usage[SRC])
    for k, v in kernels.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds_bytes"] == 0, (k, v)
    src = open(os.path.join(ROOT, "gdb-nerf_amd", "csrc", SRC)).read()
    table = int(re.search(r"#define OPT_TABLE (\d+)", src).group(1))
    # pointers 4 x 8, numel 8, eight floats of hyper-parameters, one prefix entry: the launch's arguments stay inside 4 KB
    assert table * (32 + 8 + 32 + 4) + 4 + 4 + 8 <= 4096 and "static_assert(sizeof(OptTable)" in src


def _call(lib, n=1, null=None, numel=(8,), step=(1,), beta1=(0.9,), beta2=(0.999,), arrays=True):
    fake = 4096   # a host integer: a launch on it would fail, a refusal never gets there
    cols = [(C.c_void_p * max(n, 1))(*[None if null == (k, i) else fake for i in range(max(n, 1))]) for k in range(4)]
    d = lambda vals: (C.c_double * max(n, 1))(*vals)
    i64 = lambda vals: (C.c_int64 * max(n, 1))(*vals)
    if not arrays:
        return lib.gdb_adam_step(n, None, None, None, None, None, None, None, None, None, None, None, 0.0, 0, None)
    return lib.gdb_adam_step(n, *cols, i64(numel), d((1e-3,) * max(n, 1)), d(beta1), d(beta2), d((1e-8,) * max(n, 1)), d((0.0,) * max(n, 1)),
                             i64(step), 40.0, 0, None)


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    assert _call(lib, n=-1) == _lib.GDB_E_BADARG and b"-1 tensors" in lib.gdb_last_error()
    assert _call(lib, n=1, arrays=False) == _lib.GDB_E_BADARG and b"NULL" in lib.gdb_last_error()
    for k in range(4):
        assert _call(lib, null=(k, 0)) == _lib.GDB_E_BADARG and b"NULL pointer" in lib.gdb_last_error(), k
    assert _call(lib, numel=(-1,)) == _lib.GDB_E_SHAPE and b"numel" in lib.gdb_last_error()
    assert _call(lib, step=(0,)) == _lib.GDB_E_BADARG and b"step" in lib.gdb_last_error()
    for kw in (dict(beta1=(1.0,)), dict(beta1=(-0.1,)), dict(beta2=(1.0,)), dict(beta2=(float("nan"),))):
        assert _call(lib, **kw) == _lib.GDB_E_BADARG and b"betas" in lib.gdb_last_error(), kw
    # the second tensor is the bad one: nothing of the first has been launched (its pointers are not device pointers)
    assert _call(lib, n=2, numel=(8, 8), step=(1, 0), beta1=(0.9, 0.9), beta2=(0.999, 0.999)) == _lib.GDB_E_BADARG
    with pytest.raises(ValueError, match="step"):
        _lib.check(_call(lib, step=(-3,)))
    # nothing to do is not an error, and launches nothing
    assert _call(lib, n=0, arrays=False) == _lib.GDB_OK
    assert _call(lib, n=1, numel=(0,)) == _lib.GDB_OK
    assert _call(lib, n=2, numel=(0, 0), step=(1, 5), beta1=(0.9, 0.0), beta2=(0.999, 0.0)) == _lib.GDB_OK


class Four(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(3, 2)
        self.w = nn.Parameter(torch.ones(5))
        self.frozen = nn.Parameter(torch.ones(2), requires_grad=False)
        self.s = nn.Parameter(torch.tensor(1.0))


def test_switch_default_and_make_optimizer_recipe():
    for y in ("dtu_pretrain.yaml", "dtu_eval.yaml", "llff_eval.yaml", "nerf_eval.yaml"):
        assert make_cfg("configs/" + y).train.hip_optimizer is False
    assert "hip_optimizer" in open(os.path.join(ROOT, "gdb-nerf_amd", "configs", "dtu_pretrain.yaml")).read()
    net = Four()
    cfg = lambda *o: make_cfg("configs/dtu_pretrain.yaml", ["train.weight_decay", "0.01", "train.eps", "1e-6", *o])
    for opts, cls, decoupled in (((), torch.optim.Adam, False), (("train.optim", "adamw"), torch.optim.AdamW, True),
                                 (("train.hip_optimizer", "True"), HipAdam, False),
                                 (("train.hip_optimizer", "True", "train.optim", "adamw"), HipAdam, True)):
        opt = make_optimizer(cfg(*opts), net)
        assert type(opt) is cls
        assert len(opt.param_groups) == 4                       # one group per TRAINABLE parameter, in named_parameters order
        want = [p for _, p in net.named_parameters() if p.requires_grad]
        for g, p in zip(opt.param_groups, want):
            assert len(g["params"]) == 1 and g["params"][0] is p
            assert g["lr"] == 5e-4 and g["weight_decay"] == 0.01 and g["eps"] == 1e-6 and tuple(g["betas"]) == (0.9, 0.999)
            assert bool(g["decoupled_weight_decay"]) is decoupled
    sgd = make_optimizer(cfg("train.optim", "sgd"), net)
    assert type(sgd) is torch.optim.SGD and len(sgd.param_groups) == 4 and sgd.param_groups[0]["momentum"] == 0.9
    with pytest.raises(NotImplementedError, match="radam"):
        make_optimizer(cfg("train.optim", "radam"), net)
    with pytest.raises(NotImplementedError, match="radam"):
        make_optimizer(cfg("train.optim", "radam", "train.hip_optimizer", "True"), net)
    with pytest.raises(ValueError, match="sgd"):
        make_optimizer(cfg("train.optim", "sgd", "train.hip_optimizer", "True"), net)


def test_hip_adam_constructor():
    p = [nn.Parameter(torch.zeros(3))]
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=name):
            HipAdam(p, **{name: True})
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1), dict(clip_value=0.0)):
        with pytest.raises(ValueError):
            HipAdam(p, **kw)
    opt = HipAdam([{"params": p, "lr": 0.5}], lr=1e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.1, decoupled=True, clip_value=40)
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["decoupled_weight_decay"]) == (0.5, (0.8, 0.9), 1e-6, 0.1, True)
    assert opt.clip_value == 40.0 and isinstance(opt, torch.optim.Optimizer)
    assert opt.state_dict()["state"] == {}
    opt.step()                                                     # no gradient anywhere: nothing to do, no state, no library call
    assert len(opt.state) == 0
    p[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="parameter 0"):           # a CPU tensor: refused by name, never another path
        opt.step()
    assert len(opt.state) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_adam_refuses_what_the_kernel_cannot_take():
    ok = nn.Parameter(torch.zeros(4, device="cuda"))
    ok.grad = torch.ones(4, device="cuda")
    cpu = nn.Parameter(torch.zeros(4))
    cpu.grad = torch.ones(4)
    half = nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float16))
    half.grad = torch.ones(4, device="cuda", dtype=torch.float16)
    strided = nn.Parameter(torch.zeros(4, 6, device="cuda").t())
    strided.grad = torch.ones(6, 4, device="cuda")
    gstrided = nn.Parameter(torch.zeros(6, 4, device="cuda"))
    gstrided.grad = torch.ones(4, 6, device="cuda").t()
    for bad, what in ((cpu, "the data"), (half, "the data"), (strided, "the data"), (gstrided, "the gradient")):
        opt = HipAdam([ok, bad], lr=1e-3)
        with pytest.raises(ValueError, match=f"{what} of parameter 1"):
            opt.step()
        assert len(opt.state) == 0 and ok._version == 0 and torch.equal(ok.detach(), torch.zeros(4, device="cuda"))   # refused before anything ran


def _frame():
    from gdb_nerf_amd import synthetic
    fr = synthetic.make_frame(64, 96, V=3, scene="dtu", seed=11)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return {"src_views": {"rgb": t(fr["src_images"]), "extrinsics": t(fr["src_exts"]), "intrinsics": t(fr["src_ints"])},
            "tar_views": {"extrinsics": t(fr["tar_ext"]), "intrinsics": t(fr["tar_int"])}, "near_far": t(fr["near_far"])}


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [("nerf.hot_path", "mirrors"), ("fpn.hip_feature_net", "True", "mvs.hip_cost_reg", "True")],
                         ids=["mirrors", "fused_hip_fpn_cost_reg_decoder"])
def test_step_reaches_the_next_forward_through_the_weight_caches(opts, monkeypatch):
    """The kernel writes through raw pointers; every packed-weight cache is keyed on (data_ptr, _version).  `mirrors` is the
    configuration that trains; the second one puts the FPN, the U-Nets, the render and the decoder on the library, i.e. every cache
    there is.  PyTorch's convolutions are asked for their deterministic algorithms: without that the `mirrors` render (PyTorch FPN,
    U-Nets and decoder) differs from itself by one ulp from run to run, whatever the optimiser."""
    from gdb_nerf_amd.networks import make_network
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    cfg = make_cfg("configs/dtu_eval.yaml", list(opts))
    torch.manual_seed(5)
    net = make_network(cfg).cuda().eval()
    batch = _frame()
    with torch.no_grad():
        first = net(batch)[0]["rgb"].clone()                 # fills the caches with the old weights
    params = [p for p in net.parameters() if p.requires_grad]
    g = torch.Generator(device="cuda").manual_seed(6)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    versions = [p._version for p in params]
    gversions = [p.grad._version for p in params]
    HipAdam([{"params": [p]} for p in params], lr=1e-3, clip_value=0.5).step()
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(p.grad._version > v for p, v in zip(params, gversions))         # the clip rewrote every gradient
    assert all(float(p.grad.abs().max()) <= 0.5 for p in params)
    with torch.no_grad():
        second = net(batch)[0]["rgb"].clone()
    fresh = make_network(cfg).cuda().eval()
    fresh.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad():
        want = fresh(batch)[0]["rgb"]
    assert torch.isfinite(second).all() and not torch.equal(second, first)
    assert torch.equal(second, want), float((second - want).abs().max())
    # without the clip the gradients are only read: their versions stay
    gversions = [p.grad._version for p in params]
    HipAdam(params, lr=1e-3).step()
    assert all(p.grad._version == v for p, v in zip(params, gversions))


def _ref64_steps(p, m, v, grads, t0, lr, b1, b2, eps, wd, decoupled):
    """The header's formula in float64 numpy over a list of gradients (no clip)."""
    p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for i, g in enumerate(grads):
        t = t0 + i + 1
        g = g.astype(np.float64)
        if wd:
            if decoupled:
                p = p * (1 - lr * wd)
            else:
                g = g + wd * p
        m = m + (g - m) * (1 - b1)
        v = v * b2 + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return {"param": p, "exp_avg": m, "exp_avg_sq": v}


def _drive(opt, p, grads, device):
    for g in grads:
        p.grad = torch.from_numpy(g).to(device)
        opt.step()
    st = opt.state[p]
    return {"param": p.detach().double().cpu().numpy(), "exp_avg": st["exp_avg"].double().cpu().numpy(), "exp_avg_sq": st["exp_avg_sq"].double().cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("hip_first", [True, False], ids=["hip_to_torch", "torch_to_hip"])
def test_state_interchange_with_torch_adam(hip_first, decoupled):
    """Three steps with one class, its state_dict loaded into the other class over a clone of the parameter, two more steps: still
    within the referee rule of the float64 formula over all five gradients (E32: torch's CPU float32 optimiser over the same five)."""
    rng = np.random.default_rng(3)
    n, hyper = 2048 + 37, dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(5)]
    Torch = torch.optim.AdamW if decoupled else torch.optim.Adam
    make = {True: lambda q: HipAdam([q], decoupled=decoupled, **hyper), False: lambda q: Torch([q], foreach=False, **hyper)}
    a = nn.Parameter(torch.from_numpy(p0).cuda())
    first = make[hip_first](a)
    _drive(first, a, grads[:3], "cuda")
    sd = copy.deepcopy(first.state_dict())      # as a checkpoint would hold it: load_state_dict itself keeps the tensors it is given
    assert sd["state"][0]["step"].dtype == torch.float32 and sd["state"][0]["step"].device.type == "cpu" and float(sd["state"][0]["step"]) == 3.0
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    b = nn.Parameter(a.detach().clone())
    second = make[not hip_first](b)
    second.load_state_dict(sd)
    assert bool(second.param_groups[0]["decoupled_weight_decay"]) is decoupled
    got_b = _drive(second, b, grads[3:], "cuda")
    got_a = _drive(first, a, grads[3:], "cuda")                    # the first class goes on as well
    assert float(second.state[b]["step"]) == 5.0 and float(first.state[a]["step"]) == 5.0
    c = nn.Parameter(torch.from_numpy(p0.copy()))
    e32 = _drive(Torch([c], foreach=False, **hyper), c, grads, "cpu")
    z = np.zeros(n, np.float32)
    ref = _ref64_steps(p0, z, z, grads, 0, hyper["lr"], *hyper["betas"], hyper["eps"], hyper["weight_decay"], decoupled)
    fails = []
    for who, got in (("loaded", got_b), ("original", got_a)):
        for k in ref:
            top, e = float(np.abs(ref[k]).max()), float(np.abs(e32[k] - ref[k]).max())
            bound = 4.0 * max(e, 8.0 * float(np.spacing(np.float32(top))))
            err = float(np.abs(got[k] - ref[k]).max())
            print(f"[interchange {'hip->torch' if hip_first else 'torch->hip'} {'adamw' if decoupled else 'adam'}] {who:8s} {k:10s} err {err:.3e}  bound {bound:.3e}")
            if not err <= bound:
                fails.append((who, k, err, bound))
    assert not fails, fails

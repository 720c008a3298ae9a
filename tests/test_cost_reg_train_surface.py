"""The host surface of the train-mode cost-regularisation U-Nets (include/gdb_nerf_hip.h, "ABI v7, added"): exported
symbols, the layout query on the CPU for every plan cr_plan accepts, its refusals, the compiler's resource report for the new file,
and the `mvs.hip_cost_reg_train` switch on CPU tensors.  No GPU."""
import ctypes as C
import json
import os

import pytest
import torch

from gdb_nerf_amd import _lib, costvol
from gdb_nerf_amd.configs import make_cfg
from gdb_nerf_amd.networks.gdb_nerf import depth_net as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gdb_cost_reg_train_layout", "gdb_cost_reg_train", "gdb_cost_reg_train_backward")


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gdb_nerf_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
        assert f"int {name}(" in header
    assert "GdbCostRegTrainRegion" in header and lib.gdb_abi_version() == 7
    assert C.sizeof(_lib.GdbCostRegTrainRegion) == 64


def _plans():
    for depth in (2, 3):
        for c in range(8, (128 >> depth) + 1, 8):
            for cin in range(8, 257, 8):
                yield depth, cin, c


def _check_layout(depth, cin, c, cout, B, D, H, W):
    regions, saved, ws = costvol.cost_reg_train_layout(depth, cin, c, cout, B, D, H, W)
    names = [n for _, n in regions]
    assert len(names) == len(set(names)), "region names are unique across both buffers"
    for buf, total in ((0, saved), (1, ws)):
        spans = sorted((off, off + nb) for (b, _), (off, nb, _, _) in regions.items() if b == buf)
        assert spans[0][0] == 0 and spans[-1][1] <= total
        for (_, e0), (b1, _) in zip(spans, spans[1:]):
            assert e0 <= b1, "no two regions overlap"
    chans = [c] + [c << (l + 1) for l in range(depth) for _ in (0, 1)] + [c << l for l in reversed(range(depth))]
    levels = [0] + [l + 1 for l in range(depth) for _ in (0, 1)] + list(reversed(range(depth)))
    for i, (ch, lvl) in enumerate(zip(chans, levels)):
        nvox = B * (D >> lvl) * (H >> lvl) * (W >> lvl)
        for k in ("z", "out"):
            assert regions[(0, f"conv{i}.{k}")][1:] == (4 * nvox * ch, ch, lvl)
        for k in ("mean", "invstd"):
            assert regions[(0, f"conv{i}.{k}")][1:3] == (4 * ch, ch)
    assert regions[(0, "prob")][1] == 4 * B * D * H * W
    return saved, ws, regions[(1, "dw_partials")][1] + regions[(1, "dw_partials2")][1]   # (the weight gradient's partials are reported)


def test_layout_answers_for_every_accepted_plan():
    n = 0
    for depth, cin, c in _plans():
        for cout in (1, 8, 15):
            m = 1 << depth
            _check_layout(depth, cin, c, cout, 1, 2 * m, m, 3 * m)
            n += 1
    assert n == (4 + 2) * 32 * 3
    _check_layout(2, 8, 8, 1, 1, 4, 4, 8)        # the minimum: two values per channel at the deepest level
    _check_layout(3, 16, 8, 8, 2, 8, 8, 8)


def test_layout_at_the_c2_stage_shapes():
    """The byte counts DESIGN.md 4.19 quotes."""
    s0 = _check_layout(2, 32, 8, 8, 1, 64, 64, 80)
    s1 = _check_layout(3, 16, 8, 8, 1, 8, 256, 320)
    print(f"[crt layout] c2 stage 0: saved {s0[0]} B, workspace {s0[1]} B; stage 1: saved {s1[0]} B, workspace {s1[1]} B")
    assert s0[:2] == (62519808, 71823872) and s1[:2] == (128907776, 84705792)
    assert 0 < s0[2] < s0[0] and 0 < s1[2] < s1[0]   # the weight gradient's partials stay below the saved buffer at both


@pytest.mark.parametrize("args", [(4, 16, 8, 8), (1, 16, 8, 8), (2, 12, 8, 8), (2, 264, 8, 8), (2, 0, 8, 8), (2, 16, 4, 8), (2, 16, 40, 8),
                                  (3, 16, 24, 8), (2, 16, 8, 0), (2, 16, 8, 16)])
def test_layout_refuses_bad_plans(args):
    with pytest.raises(ValueError):
        costvol.cost_reg_train_layout(*args, 1, 8, 8, 8)


@pytest.mark.parametrize("shape", [(1, 6, 8, 8), (1, 8, 8, 10), (0, 8, 8, 8), (1, 8, 0, 8), (1, 4, 4, 4)])
def test_layout_refuses_bad_shapes(shape):
    """Not divisible by 2^depth, empty, and the single-value level (B * D*H*W >> 3 depth == 1), which PyTorch refuses too."""
    lib = _lib.load()
    n = C.c_int32()
    assert lib.gdb_cost_reg_train_layout(2, 16, 8, 8, *shape, None, 0, C.byref(n), None, None) == _lib.GDB_E_SHAPE
    with pytest.raises(ValueError):
        costvol.cost_reg_train_layout(2, 16, 8, 8, *shape)
    assert lib.gdb_cost_reg_train_layout(2, 16, 8, 8, 2, 4, 4, 4, None, 0, C.byref(n), None, None) == _lib.GDB_OK   # two values: accepted
    assert lib.gdb_cost_reg_train_layout(3, 16, 8, 8, 1, 8, 8, 8, None, 0, C.byref(n), None, None) == _lib.GDB_E_SHAPE
    regs = (_lib.GdbCostRegTrainRegion * 2)()
    assert lib.gdb_cost_reg_train_layout(2, 16, 8, 8, 1, 8, 8, 8, C.cast(regs, C.c_void_p), 2, C.byref(n), None, None) == _lib.GDB_E_BADARG


def test_new_kernels_use_no_private_memory():
    path = os.path.join(ROOT, "gdb-nerf_amd", "csrc", "obj", "resource_usage.json")
    usage = json.load(open(path))["gdb_costreg_train.hip"]
    kernels = {k: v for k, v in usage.items() if "k_crt_" in k}
    assert len(kernels) >= 19, sorted(kernels)
    for k, v in kernels.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0, (k, v)


def test_switch_default_and_cpu_tensors_are_untouched():
    """The switch defaults to off; with it on, CPU tensors take the PyTorch module exactly as with it off (bit-identical outputs and
    gradients), in training and in eval mode."""
    assert make_cfg("configs/dtu_pretrain.yaml").mvs.hip_cost_reg_train is False
    assert dn.DepthNet(make_cfg("configs/dtu_pretrain.yaml")).hip_cost_reg_train is False
    outs = []
    for on in (False, True):
        torch.manual_seed(3)
        net = dn.DepthNet(make_cfg("configs/dtu_pretrain.yaml", ["mvs.hip_cost_reg_train", str(on), "mvs.stage_render", "False"])).train()
        assert net.hip_cost_reg_train is on
        g = torch.Generator().manual_seed(4)
        cost = torch.randn(1, net.cost_regs[0].conv0[0].in_channels, 8, 8, 12, generator=g)
        feats = torch.zeros(1)
        assert not net.use_hip_cost_reg_train(feats)
        vol, prob = net._cost_reg(0, cost, feats)
        (vol.sum() + (prob * prob).sum()).backward()
        grads = [p.grad.clone() for p in net.cost_regs[0].parameters()]
        net.eval()
        with torch.no_grad():
            ev = net._cost_reg(0, cost, feats)
        outs.append((vol.detach(), prob.detach(), *grads, *ev))
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))

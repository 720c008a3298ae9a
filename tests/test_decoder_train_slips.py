"""No kernel here: the rule of test_decoder_train_referee.py must reject a subtly wrong decoder backward.  On every backward case with a
non-zero upstream an fp32 CPU restatement of the decoder, written the way the kernels run it (the up stage folded with out_conv and its
gradient mapped back by the formulas of DESIGN.md 4.23; ReLU masks from the post-ReLU values; the gate's own path through the mean of
T), carries one of three slips:
  (a) "fold-swapped"  the fold's backward with the folded channel read as 4 o + s instead of 3 s + o;
  (b) "no-se-term"    the squeeze-excitation's path through the mean dropped: dT = dx * gate alone;
  (c) "relu-at-zero"  ReLU'(0) = 1: the mask taken as (saved value >= 0), which holds for every saved post-ReLU value.
Each must exceed the bound at some gradient; the restatement without a slip must pass everywhere (the control: without it a rejection
could be the restatement's own doing).  Without this the bound could pass a wrong backward."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_decoder_train_referee import BACKWARD_IDS, CASES, PARAM_NAMES, Q, _grad_referee, _setup, _upstream
from test_decoder_train_surface import fold_backward, fold_backward_swapped

SLIPS = ("fold-swapped", "no-se-term", "relu-at-zero")
IDS = [k for k in BACKWARD_IDS if not CASES[k]["zero_g"]]   # with an all-zero upstream every gradient is zero, right or wrong


class _Fold(torch.autograd.Function):
    """(up_w, up_b, out_w, out_b) -> the folded 64 -> 12 layer, summed in float64 and rounded once; backward by the written-out map."""

    @staticmethod
    def forward(ctx, up_w, up_b, out_w, out_b, swapped):
        ctx.save_for_backward(up_w, up_b, out_w)
        ctx.swapped = swapped
        ow, uw = out_w.double()[:, :, 0, 0], up_w.double().view(64, 4, 64, 3, 3)
        wf = torch.einsum("ok,ksctu->soctu", ow, uw).reshape(12, 64, 3, 3)
        bf = (torch.einsum("ok,ks->so", ow, up_b.double().view(64, 4)) + out_b.double()[None]).reshape(12)
        return wf.to(up_w.dtype), bf.to(up_w.dtype)

    @staticmethod
    def backward(ctx, dwf, dbf):
        up_w, up_b, out_w = ctx.saved_tensors
        fn = fold_backward_swapped if ctx.swapped else fold_backward
        a, b, c, d = fn(dwf.double().numpy().reshape(12, 64, 9), dbf.double().numpy(), up_w.double().numpy().reshape(256, 64, 9),
                        up_b.double().numpy(), out_w.double().numpy().reshape(3, 64))
        t = lambda x, like: torch.from_numpy(np.ascontiguousarray(x)).reshape(like.shape).to(like.dtype)
        return t(a, up_w), t(b, up_b), t(c, out_w), t(d, up_b[:3]), None


class _ReluAtZero(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = F.relu(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * (y >= 0).to(g.dtype)


def _restated(m, x, slip):
    relu = _ReluAtZero.apply if slip == "relu-at-zero" else F.relu
    shallow = trunk = m.in_conv(x)
    for blk in m.blocks:
        a = relu(blk.conv1(trunk))
        b = relu(blk.conv2(torch.cat((trunk, a), 1)))
        t = blk.conv3(torch.cat((trunk, a, b), 1))
        g = blk.se.fc((t.detach() if slip == "no-se-term" else t).mean((2, 3)))
        trunk = trunk + t * g[:, :, None, None]
    wf, bf = _Fold.apply(m.up[0].weight, m.up[0].bias, m.out_conv.weight, m.out_conv.bias, slip == "fold-swapped")
    y = F.conv2d(shallow + trunk, wf, bf, padding=1)
    B, _, H, W = y.shape
    return y.view(B, 2, 2, 3, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, 3, 2 * H, 2 * W)   # channel 3 s + o -> (o, 2y + (s >> 1), 2x + (s & 1))


@pytest.fixture(scope="module", params=IDS)
def case(request):
    return request.param


def _ratios(name, slip):
    """{tensor: error / bound} of the fp32 CPU restatement against the float64 referee of the case."""
    c = CASES[name]
    m, rows = _setup(name)
    m = copy.deepcopy(m)
    x = rows[:, 12:Q].reshape(c["B"], c["H"], c["W"], 27).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (_restated(m, x, slip) * _upstream(name)).sum().backward()
    from gdb_nerf_amd.decoder_train import decoder_params
    got = {k: p.grad for k, p in zip(PARAM_NAMES(c["L"]), decoder_params(m))}
    got["rows"] = x.grad.permute(0, 2, 3, 1).reshape(-1, 27)
    out = {}
    for k, (ref, bound) in _grad_referee(name).items():
        out[k] = float(np.abs(got[k].double().numpy().reshape(ref.shape) - ref).max()) / bound
    return out


def test_the_restatement_without_a_slip_passes(case):
    r = _ratios(case, None)
    assert max(r.values()) <= 1.0, {k: v for k, v in r.items() if v > 1.0}


@pytest.mark.parametrize("slip", SLIPS)
def test_a_slip_misses_the_rule(case, slip):
    r = _ratios(case, slip)
    worst = max(r, key=r.get)
    print(f"{case} {slip}: worst {worst} at {r[worst]:.3g} x the bound")
    assert r[worst] > 1.0, (case, slip, r)

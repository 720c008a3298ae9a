"""No kernel here: the rule of test_cost_reg_train_referee.py must reject a subtly wrong train-mode U-Net.  On every backward case an
fp32 CPU restatement of `_UNet3d.forward` in .train() carries one of three slips in one layer:
  (a) "const-stats"  the eval-mode BN backward: the batch statistics treated as constants;
  (b) "unbiased"     the unbiased instead of the biased variance in the normalisation;
  (c) "unflipped"    the layer's data gradient with its taps the other way round (the weight gradient stays right).
Each must exceed the bound at some observation point or gradient; the restatement without a slip must pass everywhere (the control:
without it a rejection could be the restatement's own doing).  Without this the bound could pass a wrong backward."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_cost_reg_train_referee import BACKWARD_IDS, _nbn, observe, referee

SLIPS = ("const-stats", "unbiased", "unflipped")


def _conv(x, conv, w):
    if isinstance(conv, torch.nn.ConvTranspose3d):
        return F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    return F.conv3d(x, w, stride=conv.stride, padding=1)


class _UnflippedDx(torch.autograd.Function):
    """The layer as it is, its weight gradient as it is, its data gradient from the spatially flipped kernel."""

    @staticmethod
    def forward(ctx, x, w, conv):
        ctx.save_for_backward(x, w)
        ctx.conv = conv
        return _conv(x, conv, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        with torch.enable_grad():
            wd = w.detach().requires_grad_()
            gw, = torch.autograd.grad(_conv(x.detach(), ctx.conv, wd), wd, g)
            xd = x.detach().requires_grad_()
            gx, = torch.autograd.grad(_conv(xd, ctx.conv, w.detach().flip(2, 3, 4)), xd, g)
        return gx, gw, None


def restated(slip, layer):
    """`forward(m, x, zs, hs)` for `observe`: _UNet3d.forward in .train() written out, with `slip` in BN layer `layer` (layer == number
    of BN layers: the two heads, for "unflipped")."""
    def conv_of(i, conv, y):
        if slip == "unflipped" and i == layer:
            return _UnflippedDx.apply(y, conv.weight, conv)
        return _conv(y, conv, conv.weight)

    def forward(m, x, zs, hs):
        depth, dims = m._depth, (0, 2, 3, 4)

        def block(i, y):
            conv, bn = getattr(m, f"conv{i}")[0], getattr(m, f"conv{i}")[1]
            z = conv_of(i, conv, y)
            mean, var = z.mean(dims, keepdim=True), z.var(dims, unbiased=False, keepdim=True)
            with torch.no_grad():
                n = z.numel() // z.shape[1]
                bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean.flatten())
                bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var.flatten() * n / (n - 1))
                bn.num_batches_tracked += 1
            if i == layer and slip == "unbiased":
                var = z.var(dims, unbiased=True, keepdim=True)
            if i == layer and slip == "const-stats":
                mean, var = mean.detach(), var.detach()
            h = (z - mean) / torch.sqrt(var + bn.eps) * bn.weight.view(1, -1, 1, 1, 1) + bn.bias.view(1, -1, 1, 1, 1)
            zs[i], hs[i] = z.detach(), h.detach()
            return torch.relu(h)

        skips, n = [block(0, x)], 1
        for _ in range(depth):
            skips.append(block(n + 1, block(n, skips[-1])))
            n += 2
        y = skips.pop()
        while skips:
            y = skips.pop() + block(n, y)
            n += 1
        return conv_of(n, m.feat_head, y), F.softmax(conv_of(n, m.prob_head, y).squeeze(1), dim=1)
    return forward


def _flip_shows(case, layer):
    """A flipped kernel differs only where more than the centre tap meets data: not for a stride-1 layer on a 1 x 1 x 1 grid."""
    depth = case["depth"]
    if layer == _nbn(depth) or layer > 2 * depth or layer % 2 == 1:   # the heads, transposed and stride-2 layers: two grids, one > 1
        return True
    lvl = layer // 2
    return max(case["D"] >> lvl, case["H"] >> lvl, case["W"] >> lvl) > 1


def _ratios(r, forward):
    got = observe(copy.deepcopy(r["m"]).train(), r["x"], r["gv"], r["gp"], True, forward=forward)
    return {k: float(np.abs(got[k] - r["ref"][k]).max()) / r["bound"][k] for k in r["points"] if r["bound"][k] > 0}


@pytest.mark.parametrize("name", BACKWARD_IDS)
def test_rule_rejects_each_slip_and_passes_the_restatement(name):
    r = referee(name)
    idx, nbn = BACKWARD_IDS.index(name), _nbn(r["case"]["depth"])
    clean = _ratios(r, restated(None, -1))
    worst = max(clean, key=clean.get)
    print(f"[crt slip] {name} restatement without a slip: worst err / bound {clean[worst]:.3f} at {worst}")
    assert clean[worst] <= 1.0, (worst, clean[worst])
    for s, slip in enumerate(SLIPS):
        # the layer moves with the case: over the cases every layer kind meets every slip; conv0 has no data gradient, the heads no BN
        layer = 1 + (idx + s) % nbn if slip == "unflipped" else (idx + s) % nbn
        while slip == "unflipped" and not _flip_shows(r["case"], layer):
            layer = 1 + layer % nbn
        ratios = _ratios(r, restated(slip, layer))
        worst = max(ratios, key=ratios.get)
        where = "heads" if layer == nbn else f"conv{layer}"
        print(f"[crt slip] {name} {slip} in {where}: worst err / bound {ratios[worst]:.2f} at {worst}; {sum(v > 1 for v in ratios.values())} of {len(ratios)} points over")
        assert ratios[worst] > 1.0, (slip, where, worst, ratios[worst])

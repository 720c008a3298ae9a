"""Volume-integration operators of the hot path with the reference's signatures
(networks/gdb_nerf/utils.py:19-43, 88-121), backed by `gdb_render_weights` / `gdb_accumulate`.  When grad mode is on and an
input requires grad, the calls go through the autograd Functions below (`gdb_render_weights_backward`,
`gdb_accumulate_backward`); `z_vals` gets weights * g_depth_map[indices], formed in torch, when it requires grad; the indices get
no gradient."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ...engine import HotPathEngine

_ENGINES = {}


def _engine(device) -> HotPathEngine:
    key = str(device)
    if key not in _ENGINES:
        _ENGINES[key] = HotPathEngine(device=device)
    return _ENGINES[key]


class RenderWeightsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigma, ray_indices, num_rays):
        ctx.save_for_backward(sigma, ray_indices)
        ctx.num_rays = num_rays
        return _engine(sigma.device).render_weights(sigma, ray_indices, num_rays)

    @staticmethod
    def backward(ctx, g_weights):
        sigma, ray_indices = ctx.saved_tensors
        return _engine(sigma.device).render_weights_backward(sigma, ray_indices, ctx.num_rays, g_weights.contiguous()), None, None


class AccumulateFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, feat, z_vals, ray_indices, num_rays):
        ctx.save_for_backward(weights, feat, z_vals, ray_indices)
        ctx.num_rays = num_rays
        return _engine(feat.device).accumulate(weights, feat, z_vals, ray_indices, num_rays)

    @staticmethod
    def backward(ctx, g_feat_map, g_depth_map, g_opacity_map):
        weights, feat, z_vals, ray_indices = ctx.saved_tensors
        nb, dev = ctx.num_rays, feat.device
        g_feat_map = torch.zeros((nb, feat.shape[1]), device=dev) if g_feat_map is None else g_feat_map.contiguous()
        g_depth_map = torch.zeros((nb,), device=dev) if g_depth_map is None else g_depth_map.contiguous()
        g_opacity_map = torch.zeros((nb,), device=dev) if g_opacity_map is None else g_opacity_map.contiguous()
        g_w, g_f = _engine(dev).accumulate_backward(weights, feat, z_vals, ray_indices, nb, g_feat_map, g_depth_map, g_opacity_map)
        # depth_map = segmented sum of weights * z: the path of `nerf_depth` to the depth net once z_vals carries a graph
        g_z = weights * g_depth_map[ray_indices] if ctx.needs_input_grad[2] else None
        return g_w, g_f, g_z, None, None


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t.is_cuda and t.requires_grad for t in tensors)


def weights_init(m):  # reference utils.py:8-16 (training helper, kept for API parity)
    if isinstance(m, (nn.Linear, nn.Conv2d)):
        nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        if m.bias is not None:
            nn.init.zeros_(m.bias)


def render_weight_from_density(sigma: torch.Tensor, ray_indices: torch.Tensor, num_rays: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Normalised transmittance weights per bundle (`gdb_render_weights`).  The second value is the
    reference's `inverse_indices` (dense rank of each sample's bundle among the non-empty bundles)."""
    if _wants_grad(sigma):
        w = RenderWeightsFunction.apply(sigma.contiguous(), ray_indices.contiguous(), int(num_rays))
    else:
        w = _engine(sigma.device).render_weights(sigma.contiguous(), ray_indices.contiguous(), int(num_rays))
    return w, torch.unique_consecutive(ray_indices, return_inverse=True)[1]


def accumulate_value_along_rays(feat: torch.Tensor, z_vals: torch.Tensor, weights: torch.Tensor, ray_indices: torch.Tensor,
                                num_rays: int, inverse_indices: Optional[torch.Tensor] = None):
    """Segmented sum of weights · [feat | z | 1] per bundle -> (feat_map, depth_map, opacity_map) (`gdb_accumulate`)."""
    if _wants_grad(weights, feat, z_vals):
        return AccumulateFunction.apply(weights.contiguous(), feat.contiguous(), z_vals.contiguous(), ray_indices.contiguous(), int(num_rays))
    return _engine(feat.device).accumulate(weights.contiguous(), feat.contiguous(), z_vals.contiguous(), ray_indices.contiguous(), int(num_rays))

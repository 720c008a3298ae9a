"""Radiance / density MLP of the hot path (reference networks/gdb_nerf/nerf.py).  The module owns the
parameters under the reference's key names; `forward` runs `gdb_mlp` (exact fp32 HIP kernel).  When grad mode is on and
an input or a parameter requires grad, the call goes through `MLPFunction`, whose backward is `gdb_mlp_backward`."""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from ...engine import HotPathEngine, NERF_KEYS


class MLPFunction(torch.autograd.Function):
    """`gdb_mlp` with `gdb_mlp_backward` as its derivative.  Inputs: vox_feat, rgbs_feat_rgb_dir and the module's parameters (in
    `engine.packed_grad_slices` order, view_fc first when the module has it), so that autograd fills their `.grad`.  Nothing but
    the inputs and the packed weights of this forward is kept: the backward recomputes the activations."""

    @staticmethod
    def forward(ctx, engine, has_view_fc, vox_feat, rfd, *params):
        sigma, feat = engine.mlp(vox_feat, rfd)
        ctx.engine, ctx.has_view_fc = engine, has_view_fc
        ctx.packed = engine.weights   # load_weights makes a new tensor per pack: this one stays what the forward read
        ctx.save_for_backward(vox_feat, rfd)
        return sigma, feat

    @staticmethod
    def backward(ctx, g_sigma, g_feat):
        vox_feat, rfd = ctx.saved_tensors
        eng = ctx.engine
        n = vox_feat.shape[0]
        g_sigma = torch.zeros((n,), device=vox_feat.device) if g_sigma is None else g_sigma.contiguous()
        g_feat = torch.zeros((n, eng.Q), device=vox_feat.device) if g_feat is None else g_feat.contiguous()
        need = ctx.needs_input_grad
        g_packed, g_vox, g_rfd = eng.mlp_backward(vox_feat, rfd, g_sigma, g_feat, weights=ctx.packed, need_vox=need[2], need_rfd=need[3])
        slices, _ = eng.packed_grad_slices()
        if not ctx.has_view_fc:
            slices = slices[2:]
        g_params = tuple(g_packed[o:o + int(torch.Size(shp).numel())].view(shp) if nd else None
                         for (o, shp), nd in zip(slices, need[4:]))
        return (None, None, g_vox, g_rfd) + g_params


class NeRF(nn.Module):
    def __init__(self, hid_dim: int = 64, feat_dim: int = 16, voxel_dim: int = 8, viewdir_agg: bool = True) -> None:
        super().__init__()
        self.feat_dim, self.viewdir_agg = feat_dim, viewdir_agg
        act = lambda i, o: nn.Sequential(nn.Linear(i, o), nn.ReLU(inplace=True))
        if viewdir_agg:
            self.view_fc = act(4, feat_dim + 3)
        self.global_fc = act(3 * (feat_dim + 3), 32)
        self.agg_w_fc = act(32, 1)
        self.fc = act(32, 16)
        self.lr0 = act(voxel_dim + 16, hid_dim)
        self.sigma = nn.Sequential(nn.Linear(hid_dim, 1), nn.Softplus())
        self.weight = nn.Sequential(nn.Linear(hid_dim + voxel_dim + 16 + feat_dim + 3 + 4, hid_dim), nn.ReLU(inplace=True),
                                    nn.Linear(hid_dim, 1), nn.ReLU(inplace=True))
        self.feat_head = act(hid_dim, voxel_dim)
        self._hid, self._vox = hid_dim, voxel_dim
        self._engine: Optional[HotPathEngine] = None
        self._packed_versions = None

    def param_versions(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def sync_engine(self, engine: HotPathEngine) -> None:
        """(Re)pack the weights into `engine` when they changed since the last pack."""
        v = self.param_versions()
        if engine.weights is None or getattr(engine, "_nerf_versions", None) != v:
            engine.load_weights({k: t.detach() for k, t in self.state_dict().items()})
            engine._nerf_versions = v

    def forward(self, vox_feat: torch.Tensor, rgbs_feat_rgb_dir: torch.Tensor, only_geo: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """vox_feat (N,C_v), rgbs_feat_rgb_dir (V,N,3b²+C_f+3+4) -> sigma (N,), feat (N,3b²+C_f+3+C_v)
        (None when only_geo, as nerf.py:104-115)."""
        P = rgbs_feat_rgb_dir.shape[-1]
        b2 = (P - self.feat_dim - 7) // 3
        b = int(round(b2 ** 0.5))
        if self._engine is None or self._engine.b != b:
            self._engine = HotPathEngine(bundle_size=b, feat_dim=self.feat_dim, voxel_dim=self._vox, hid_dim=self._hid,
                                         viewdir_agg=self.viewdir_agg, device=vox_feat.device)
        self.sync_engine(self._engine)
        params = self._mlp_params()
        if vox_feat.is_cuda and torch.is_grad_enabled() and (vox_feat.requires_grad or rgbs_feat_rgb_dir.requires_grad
                                                           or any(p.requires_grad for p in params)):
            sigma, feat = MLPFunction.apply(self._engine, self.viewdir_agg, vox_feat.contiguous(), rgbs_feat_rgb_dir.contiguous(), *params)
        else:
            sigma, feat = self._engine.mlp(vox_feat.contiguous(), rgbs_feat_rgb_dir.contiguous())
        return sigma, (None if only_geo else feat)

    def _mlp_params(self):
        """The 18 (16 without view_fc) parameters in the order of the packed section."""
        mods = ([self.view_fc[0]] if self.viewdir_agg else []) + [self.global_fc[0], self.agg_w_fc[0], self.fc[0], self.lr0[0],
                                                                   self.sigma[0], self.weight[0], self.weight[2], self.feat_head[0]]
        return [p for m in mods for p in (m.weight, m.bias)]


assert NERF_KEYS[0] == "view_fc.0"

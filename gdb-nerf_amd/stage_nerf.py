"""The depth net's train-time stage render on the HIP library (gdb_stage_nerf.hip): the auxiliary per-stage NeRF
and the un-normalised composite of the reference's `DepthNet._render_rays`, forward (`gdb_stage_nerf`, one launch) and backward
(`gdb_stage_nerf_backward`).  fp32 CUDA tensors only; the plain-torch restatement in networks/gdb_nerf/depth_net.py is the CPU path,
the path with `mvs.hip_stage_render` off, and the tests' reference.  A shape the kernels are not built for raises: nothing falls
back."""
import ctypes as C

import numpy as np
import torch

from . import _lib

LAYERS = ("view_fc", "global_fc", "agg_w_fc", "fc", "lr0", "sigma", "color.0", "color.2")


def stage_params(nerf):
    """The 16 tensors in the packed order (weight then bias per layer); view_fc's two are None without viewdir_agg."""
    mods = [nerf.view_fc[0] if hasattr(nerf, "view_fc") else None, nerf.global_fc[0], nerf.agg_w_fc[0], nerf.fc[0], nerf.lr0[0],
            nerf.sigma[0], nerf.color[0], nerf.color[2]]
    return [p for m in mods for p in ((m.weight, m.bias) if m is not None else (None, None))]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class StageNerf:
    """Holds the packed weights of one `_AuxStageNerf` on the device; re-packs when a tensor's (storage, version) changes."""

    def __init__(self, nerf):
        self.lib = _lib.load()
        self.nerf = nerf
        self.viewdir = int(hasattr(nerf, "view_fc"))
        self.feat_dim = nerf.global_fc[0].in_features // 3 - 3
        self.voxel_dim = nerf.lr0[0].in_features - 16
        self.hid_dim = nerf.lr0[0].out_features
        self.net = (self.feat_dim, self.voxel_dim, self.hid_dim, self.viewdir)
        n = C.c_size_t()
        _lib.check(self.lib.gdb_stage_nerf_packed_floats(*self.net, C.byref(n)))
        self.floats = int(n.value)
        self.packed, self._versions = None, None
        # where each of the 16 tensors sits in the packed layout: unpack a ramp once, on the host
        ramp = np.arange(self.floats, dtype=np.float32)
        outs = [None if p is None else np.empty(tuple(p.shape), dtype=np.float32) for p in stage_params(nerf)]
        arr = (C.c_void_p * 16)(*[None if o is None else o.ctypes.data for o in outs])
        _lib.check(self.lib.gdb_unpack_stage_nerf_grads(*self.net, C.c_void_p(ramp.ctypes.data), arr))
        self.offsets = [None if o is None else int(o.reshape(-1)[0]) for o in outs]

    def invalidate(self):
        self._versions = None

    def sync(self, device):
        params = stage_params(self.nerf)
        v = tuple((p.data_ptr(), p._version) for p in params if p is not None) + (str(device),)
        if self.packed is None or self._versions != v:
            host = [None if p is None else np.ascontiguousarray(p.detach().cpu().numpy(), dtype=np.float32) for p in params]
            arr = (C.c_void_p * 16)(*[None if h is None else h.ctypes.data for h in host])
            out = np.empty(self.floats, dtype=np.float32)
            _lib.check(self.lib.gdb_pack_stage_nerf_weights(*self.net, arr, C.c_void_p(out.ctypes.data)))
            self.packed = torch.from_numpy(out).to(device)   # a new tensor per pack: a pending backward keeps the one it read
            self._versions = v
        return self.packed

    def layout(self, V, S, n_rays):
        out = (C.c_size_t * 3)()
        _lib.check(self.lib.gdb_stage_nerf_layout(*self.net, int(V), int(S), int(n_rays), out))
        return int(out[0]), int(out[1]), int(out[2])

    def _check(self, vox, img, S):
        if not (vox.is_cuda and img.is_cuda and vox.dtype == img.dtype == torch.float32):
            raise ValueError("the stage NeRF kernels take fp32 CUDA tensors")
        N, V, P = img.shape
        if vox.shape != (N, self.voxel_dim) or P != self.feat_dim + 7 or N % S:
            raise ValueError(f"stage NeRF: vox_feat {tuple(vox.shape)} / img_feat_rgb_dir {tuple(img.shape)} do not fit feat_dim {self.feat_dim}, "
                             f"voxel_dim {self.voxel_dim}, S {S}")
        return N // S, V

    def forward(self, packed, vox, img, S, want_samples=False):
        """vox (N, C_v), img (N, V, C_f+7), N = rays * S -> rgb_map (rays, 3) [, sigma (N), rgb (N, 3)]."""
        n_rays, V = self._check(vox, img, S)
        self.layout(V, S, n_rays)   # an unsupported shape raises here, before any allocation
        rgb_map = torch.empty((n_rays, 3), device=vox.device)
        sigma = torch.empty((n_rays * S,), device=vox.device) if want_samples else None
        rgb = torch.empty((n_rays * S, 3), device=vox.device) if want_samples else None
        _lib.check(self.lib.gdb_stage_nerf(*self.net, _ptr(packed), V, int(S), _ptr(vox), _ptr(img), n_rays, _ptr(rgb_map), _ptr(sigma), _ptr(rgb),
                                           _stream(vox.device)))
        return (rgb_map, sigma, rgb) if want_samples else rgb_map

    def backward(self, packed, vox, img, S, g_map, need_vox=True, need_img=True, workspace=None, g_packed=None):
        n_rays, V = self._check(vox, img, S)
        nbytes = self.layout(V, S, n_rays)[0]
        if workspace is None:
            workspace = torch.empty((nbytes // 4,), device=vox.device)
        if g_packed is None:
            g_packed = torch.empty((self.floats,), device=vox.device)
        g_vox = torch.empty_like(vox) if need_vox else None
        g_img = torch.empty_like(img) if need_img else None
        _lib.check(self.lib.gdb_stage_nerf_backward(*self.net, _ptr(packed), V, int(S), _ptr(vox), _ptr(img), n_rays, _ptr(g_map), _ptr(g_packed),
                                                    _ptr(g_vox), _ptr(g_img), _ptr(workspace), workspace.numel() * 4, _stream(vox.device)))
        return g_packed, g_vox, g_img

    def grads_of(self, g_packed):
        """The packed gradient as 16 views shaped like the parameters (None where the module has no view_fc)."""
        return [None if p is None else g_packed[o:o + p.numel()].view(p.shape) for p, o in zip(stage_params(self.nerf), self.offsets)]

    def render(self, vox, img, S):
        """rgb_map (rays, 3), differentiable when grad mode is on and something requires grad."""
        vox, img = vox.contiguous(), img.contiguous()
        packed = self.sync(vox.device)
        params = [p for p in stage_params(self.nerf) if p is not None]
        if torch.is_grad_enabled() and (vox.requires_grad or img.requires_grad or any(p.requires_grad for p in params)):
            return StageNerfFunction.apply(self, packed, int(S), vox, img, *params)
        return self.forward(packed, vox, img, S)


class StageNerfFunction(torch.autograd.Function):
    """`gdb_stage_nerf` with `gdb_stage_nerf_backward` as its derivative.  Inputs: vox_feat, img_feat_rgb_dir and the module's
    parameters in packed order.  Only the inputs and the packed weights this forward read are kept: the backward recomputes."""

    @staticmethod
    def forward(ctx, holder, packed, S, vox, img, *params):
        ctx.holder, ctx.packed, ctx.S = holder, packed, S
        ctx.save_for_backward(vox, img)
        return holder.forward(packed, vox, img, S)

    @staticmethod
    def backward(ctx, g_map):
        vox, img = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_packed, g_vox, g_img = ctx.holder.backward(ctx.packed, vox, img, ctx.S, g_map.contiguous(), need_vox=need[3], need_img=need[4])
        grads = [g for g in ctx.holder.grads_of(g_packed) if g is not None]
        return (None, None, None, g_vox, g_img) + tuple(g if nd else None for g, nd in zip(grads, need[5:]))

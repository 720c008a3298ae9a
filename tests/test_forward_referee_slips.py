"""No kernel here: the rule of test_forward_referee.py must see what the hand-set tolerances of test_hip_parity.py do not.  The float32
CPU restatement carrying ONE slip is put to the same rule against the same float64 referee, with the bound from the restatement without
the slip, and must miss it by at least 2x at some tensor.  The inputs of each operator are the float32 restatement's own outputs of the
operator before it (no GPU is involved).

Slips, stated exactly:
  view_fc_bias     every element of view_fc.0.bias times (1 + 2^-12);
  biased_variance  the variance over views as sum (g - m)^2 / V instead of / (V - 1), where the mean m - the one fed to global_fc too - is
                   rounded another way: (sum g) * fl(1 / V) instead of (sum g) / V;
  rgb_half_pixel   the source-pixel coordinate of encode's RGB fetch as ((g + 1) W - 1) / 2 - 2^-10, i.e. the half-pixel offset 1/2 taken
                   as 1/2 + 2^-10, on both axes;
  mip_level_bias   the mip level of the feature fetch plus 2^-8;
  vox_depth_extent the trilinear depth coordinate formed as (d + 1) D' / 2 - 1/2 with D' = D (1 + 2^-10);
  den_clamp        the composite's normalising denominator clamped at 1e-5 instead of 1e-6, on the drawn segments, whose sigma ~ 1e-6
                   bundles sit under the clamp.
Each prints its worst error over the new bound, and over the tolerance test_hip_parity.py applies to that output (recorded, not
asserted).  Every slip clears 2x as stated: none had to be enlarged to a higher power of two."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gdb_oracle_torch as oracle_t
from gdb_nerf_amd import synthetic
from test_forward_referee import (ENC_IN, NUM_DEPTH, both, composite_ref, default_dtype, drawn_segments, encode_ref, encode_tensors, mlp_ref,
                                  mlp_tensors, render_tensors, rule, weights)

B_SIZE, S_MAX = 2, 3
# what test_hip_parity.py allows on each output (test_encode_vs_golden, test_mlp_vs_golden, test_composite_vs_golden); depth: times max |depth|
PARITY_TOL = {"rgb": 2e-5, "mip_feature": 2e-4, "dir_code": 2e-5, "vox_01": 2e-5, "vox_23": 2e-5, "vox_45": 2e-5, "vox_67": 2e-5,
              "sigma": 1e-5, "feat_blend": 1e-5, "feat_head": 1e-5, "weights": 1e-6, "bundle_feat": 2e-6, "depth": 2e-6, "opacity": 1e-6}


class _Proxy:
    """A module with some attributes replaced (the restatement looks its torch functions up through `oracle_t.torch` / `oracle_t.F`)."""

    def __init__(self, module, **replaced):
        self._module, self._replaced = module, replaced

    def __getattr__(self, name):
        return self._replaced[name] if name in self._replaced else getattr(self._module, name)


@contextlib.contextmanager
def slipped(**attrs):
    """`oracle_t.<name>` replaced for the duration."""
    saved = {k: getattr(oracle_t, k) for k in attrs}
    for k, v in attrs.items():
        setattr(oracle_t, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(oracle_t, k, v)


def _grid_sample(slip):
    def grid_sample(inp, grid, **kw):
        if slip == "rgb_half_pixel" and inp.dim() == 4 and inp.shape[1] == 3:     # the source images (the mip levels hold 19 channels)
            grid = grid - torch.tensor([2.0 / inp.shape[-1], 2.0 / inp.shape[-2]]) * 2.0 ** -10
        if slip == "vox_depth_extent" and inp.dim() == 5:
            grid = torch.cat((grid[..., :2], (grid[..., 2:] + 1.0) * (1.0 + 2.0 ** -10) - 1.0), dim=-1)
        return F.grid_sample(inp, grid, **kw)
    return grid_sample


def _var_mean(g, dim, keepdim):
    V = g.shape[dim]
    m = g.sum(dim, keepdim=keepdim) * (torch.ones(()) / V)
    return ((g - m) ** 2).sum(dim, keepdim=keepdim) / V, m


def _mip_bias(texture_mip):
    return lambda pyramid, uv, level: texture_mip(pyramid, uv, level + 2.0 ** -8)


def run32(fn):
    with default_dtype(torch.float32), torch.no_grad():
        return {k: v.double().numpy() for k, v in fn(lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)).items()}


_shared = {}


def inputs():
    """One frame, and the float32 restatement's sample arrays and encode outputs on it: computed once, read-only."""
    if not _shared:
        fr = synthetic.make_frame(32, 64, V=3, seed=11, src_focal_scale=(1.0, 2.5, 6.0))
        Ho, Wo = fr["src_images"].shape[-2:]
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
        with torch.no_grad():
            s = oracle_t.sample_bundles(oracle_t.build_rays(t(fr["tar_ext"]), t(fr["tar_int"]), Ho, Wo), t(fr["depth_range"]), t(fr["vol_range"]),
                                        t(fr["near_far"][:, 0]), t(fr["near_far"][:, 1]), B_SIZE, S_MAX, NUM_DEPTH, False, True)
            rfd, vox = oracle_t.encode(t(fr["src_images"]), t(fr["img_feat"]), t(fr["feat_volume"]), s, t(fr["src_exts"]), t(fr["src_ints"]),
                                       t(fr["tar_ext"]), B_SIZE, Ho, Wo, 3)
        _shared.update(fr=fr, smp={k: s[k].numpy() for k in ENC_IN}, spb=s["samples_per_batch"].numpy(), rfd=rfd.numpy(), vox=vox.numpy())
    return _shared


def report(slip, tensors):
    """tensors: {name: (slipped float32, ref64, ref32[, groups])} -> the worst error / bound; prints it beside error / parity tolerance."""
    worst, worst_old = (0.0, ""), (0.0, "")
    for name, t in tensors.items():
        tol = PARITY_TOL[name] * (float(np.abs(t[1]).max()) if name == "depth" else 1.0)
        worst_old = max(worst_old, (float(np.abs(t[0] - t[1]).max()) / tol, name))
        for label, e32, err, bound in rule(*t):
            worst = max(worst, (err / bound, name + (":" + label if label else "")))
    print(f"[forward referee slip] {slip}: err / bound {worst[0]:.1f} at {worst[1]}; err / test_hip_parity tolerance {worst_old[0]:.2f} at {worst_old[1]}")
    return worst[0]


def encode_slipped(slip):
    i = inputs()
    r64, r32 = encode_ref(i["fr"], i["smp"], i["spb"], B_SIZE)
    ctx = slipped(texture_mip=_mip_bias(oracle_t.texture_mip)) if slip == "mip_level_bias" else slipped(F=_Proxy(F, grid_sample=_grid_sample(slip)))
    with ctx:
        bad = encode_ref(i["fr"], i["smp"], i["spb"], B_SIZE)[1]
    return encode_tensors(bad["rfd"], bad["vox"], r64, r32, B_SIZE)


def mlp_slipped(slip):
    i, w = inputs(), weights()
    r64, r32 = mlp_ref(w, i["vox"], i["rfd"])
    if slip == "view_fc_bias":
        w = dict(w, **{"view_fc.0.bias": w["view_fc.0.bias"] * np.float32(1.0 + 2.0 ** -12)})
        bad = mlp_ref(w, i["vox"], i["rfd"])[1]
    else:
        with slipped(torch=_Proxy(torch, var_mean=_var_mean)):
            bad = mlp_ref(w, i["vox"], i["rfd"])[1]
    return mlp_tensors(bad["sigma"], bad["feat"], r64, r32)


def composite_slipped(slip):
    fx = drawn_segments(False)
    idx, nb = fx["indices"], fx["n_bundles"]
    it = torch.as_tensor(idx)
    run = lambda floor: (lambda c: composite_ref(c(fx["sigma"]), c(fx["feat"]), c(fx["z_vals"]), it, nb, False, floor))
    r64, r32 = both(run(1e-6))
    return render_tensors(run32(run(1e-5)), r64, r32, idx, nb)


SLIPS = {"view_fc_bias": mlp_slipped, "biased_variance": mlp_slipped, "rgb_half_pixel": encode_slipped, "mip_level_bias": encode_slipped,
         "vox_depth_extent": encode_slipped, "den_clamp": composite_slipped}


@pytest.mark.parametrize("slip", list(SLIPS))
def test_rule_rejects_the_slip(slip):
    assert report(slip, SLIPS[slip](slip)) >= 2.0


def test_rule_passes_the_restatement_and_the_slips_leave_no_trace():
    """The control: the patched-in functions are gone after each slip - the restatement reruns bit for bit - and without a slip it sits at
    E32 / bound <= 1/4 by construction."""
    i = inputs()
    for slip in ("rgb_half_pixel", "mip_level_bias"):
        encode_slipped(slip)
    mlp_slipped("biased_variance")
    assert oracle_t.F is F and oracle_t.torch is torch
    r64, r32 = encode_ref(i["fr"], i["smp"], i["spb"], B_SIZE)
    assert np.array_equal(r32["rfd"], i["rfd"].astype(np.float64)) and np.array_equal(r32["vox"], i["vox"].astype(np.float64))
    assert report("none (encode)", encode_tensors(r32["rfd"], r32["vox"], r64, r32, B_SIZE)) <= 0.25
    r64, r32 = mlp_ref(weights(), i["vox"], i["rfd"])
    assert report("none (mlp)", mlp_tensors(r32["sigma"], r32["feat"], r64, r32)) <= 0.25

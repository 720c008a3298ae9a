"""The rule of tests/test_costvol_backward_referee.py must see a slip.  No kernel, CPU only: the float32 restatement of the backward
(`restated_backward`) passes the rule on every referee case, and turned wrong in one of four ways it fails it:
  "divisor"   the unbiased divisor V - 1 in place of V;
  "factor2"   a dropped factor 2 of d var / d val;
  "invdepth"  a missing -1 / h^2 under inv_depth;
  "border"    border taps that are not zeroed (an out-of-range tap reads the clamped texel, as padding_mode="border" would).
A slip is asserted on every case where it changes anything at all, decided from the case and not from the result:
  * none on the single-view cases (the variance of one view: every gradient is exactly zero whatever the factor) nor on `behind-V3`
    (every voxel excluded: the upstream is zero);
  * "invdepth" on the inv_depth cases that compare g_depth_values;
  * "border" where, in float64, some kept voxel has a view with a tap outside the source map and a tap inside it.
"""
import numpy as np
import pytest
import torch

from test_costvol_backward_referee import IDS, _coords64, referee, restated_backward, rule

SLIPS = ("divisor", "factor2", "invdepth", "border")


def _applies(r, slip):
    c = r["c"]
    V, Hs, Ws = c["feat"].shape[1], c["feat"].shape[3], c["feat"].shape[4]
    if V == 1 or r["excl"].all():
        return False
    if slip == "invdepth":
        return bool(c["inv"]) and r["which"] == "both"
    if slip == "border":
        with np.errstate(all="ignore"):
            ix, iy = _coords64(c, np.asarray(c["dv"], np.float64))
            x0, y0 = np.floor(ix), np.floor(iy)
            some_in = (x0 + 1 >= 0) & (x0 <= Ws - 1) & (y0 + 1 >= 0) & (y0 <= Hs - 1)
            some_out = (x0 < 0) | (x0 + 1 > Ws - 1) | (y0 < 0) | (y0 + 1 > Hs - 1)
            straddles = (some_in & some_out & np.isfinite(ix) & np.isfinite(iy)).any(1)
        return bool((straddles & ~r["excl"]).any())
    return True


@pytest.mark.parametrize("name", IDS)
def test_the_rule_rejects_every_slip(name):
    r = referee(name)
    with np.errstate(all="ignore"):
        good = restated_backward(r["c"], r["up"], torch.float32)
    for nm, err, bound in rule(r, good, f"slip none {name}"):
        assert err <= bound, nm
    for slip in SLIPS:
        if not _applies(r, slip):
            print(f"[costvol bwd slip] {name} {slip}: does not apply")
            continue
        with np.errstate(all="ignore"):
            bad = restated_backward(r["c"], r["up"], torch.float32, slip=slip)
        res = rule(r, bad, f"slip {slip} {name}")
        assert any(err > bound for _, err, bound in res), slip
        if slip in ("divisor", "factor2"):   # a wrong factor scales both gradients: each tensor compared sees it
            assert all(err > bound for _, err, bound in res), slip


def test_every_slip_is_exercised():
    seen = {s: [n for n in IDS if _applies(referee(n), s)] for s in SLIPS}
    for s, names in seen.items():
        print(f"[costvol bwd slip] {s}: {len(names)} cases")
        assert len(names) >= 3, s

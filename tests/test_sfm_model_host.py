"""The triangulation bars bite (host, no GPU): deliberately wrong variants of the header's rules
go through the comparisons that the kernel goes through (sfm_tri.npz: reason, n_kept and obs_keep
equal; xyz and err within the recorded tolerance; xyz and err bit-equal, the bar that the fixed
summation order earns) and must miss them; the unbroken oracle must meet them.  Each variant
names the input that separates it.  The figures are printed (pytest -s)."""
import numpy as np
import pytest

import sfm_cases as C
import sfm_oracle as O
from conftest import golden

TRI = golden("sfm_tri")
MARGIN = 10.0

# variant -> (the case that separates it, what it gets wrong there)
VARIANTS = {
    "no drop-worst loop": ("several_outliers", "kept set: one pass on the polluted point drops "
                                               "inliers with the outliers"),
    "no duplicate rule": ("two_in_one_image", "kept set: both observations of one image stay"),
    "no refinement": ("len17", "xyz: the DLT point is not the pixel-error minimum"),
    "angle between image rays": ("angle_rays", "reason: the rays through the pixels open past "
                                               "1.5 degrees, the angle at X does not"),
    "sums in reverse order": ("len130", "bits: xyz and err differ in the last places"),
}


def _run(variant):
    p = C.tri_problem()
    return O.triangulate_all(p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"],
                             C.MAX_REPROJ, C.MIN_ANGLE, variant=variant)


def _bars(out, t):
    """(decisions equal, deviation / tolerance, bits equal) of track t."""
    p = C.tri_problem()
    a, b = p["track_start"][t], p["track_start"][t + 1]
    same = (out["reason"][t] == TRI["reason"][t] and out["n_kept"][t] == TRI["n_kept"][t]
            and np.array_equal(out["obs_keep"][a:b], TRI["obs_keep"][a:b]))
    if not same or TRI["reason"][t] != 0:
        return same, np.nan, same
    dev = max(np.abs(out["xyz"][t] - TRI["xyz"][t]).max(), abs(out["err"][t] - TRI["err"][t]))
    bits = (out["xyz"][t].tobytes() == TRI["xyz"][t].tobytes()
            and out["err"][t].tobytes() == TRI["err"][t].tobytes())
    return same, dev / TRI["tol"][t], bits


def test_the_oracle_meets_every_bar():
    out = _run(None)
    for t, name in enumerate(C.TRI_NAMES):
        same, ratio, bits = _bars(out, t)
        assert same and bits and not ratio > 0, name


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_wrong_rule_misses_a_bar(variant):
    case, what = VARIANTS[variant]
    t = C.TRI_NAMES.index(case)
    same, ratio, bits = _bars(_run(variant), t)
    print(f"{variant} on {case}: decisions equal {same}, deviation {ratio:.3g} x the tolerance, "
          f"bits equal {bits} ({what})")
    if what.startswith(("kept set", "reason")):
        assert not same
    elif what.startswith("xyz"):
        assert same and ratio >= MARGIN
    else:
        assert same and not bits

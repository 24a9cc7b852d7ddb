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


# ---- the edge fixture's bars (tests/golden/make_golden_sfm_edges.py) ------------------------------
EDGES = golden("sfm_tri_edges")

# variant -> (the track of edge_problem() that separates it, what it gets wrong there)
EDGE_VARIANTS = {
    "duplicate ties to the highest position": ("dup_exact_tie", "kept set: the byte copies at 6, "
                                               "67 and 70 stay instead of 2, 3 and 10"),
    "no final check": ("final_check_drop", "kept set: the observation that fails at the refined "
                                           "point stays"),
    "depth not tested": ("behind_two", "kept set: the two observations behind their cameras "
                                       "have small residuals and stay"),
    "worst among the first 64 positions": ("drop_past_64", "xyz: the gross errors at 64, 67, 130 "
                                           "and 199 are never the worst, stay through the solves "
                                           "and the refinement and leave only at the final check"),
}


def _edge_bars(variant, t):
    p = C.edge_problem()
    a, b = p["track_start"][t], p["track_start"][t + 1]
    why, X, err, keep = O.triangulate(p["Rt"], p["K4"], p["obs_image"][a:b], p["obs_xy"][a:b],
                                      C.MAX_REPROJ, C.MIN_ANGLE, variant=variant)
    want = EDGES["edge_obs_keep"][a:b]
    same = (why == EDGES["edge_reason"][t] and (keep.sum() if why == 0 else 0) == EDGES["edge_n_kept"][t]
            and np.array_equal(keep if why == 0 else np.zeros(b - a, bool), want))
    if not same or why != 0:
        return same, same, np.nan, keep, want
    bits = (np.asarray(X).tobytes() == EDGES["edge_xyz"][t].tobytes()
            and np.float64(err).tobytes() == EDGES["edge_err"][t].tobytes())
    dev = max(np.abs(X - EDGES["edge_xyz"][t]).max(), abs(err - EDGES["edge_err"][t]))
    return same, bits, dev / EDGES["edge_tol"][t], keep, want


def test_the_oracle_meets_every_edge_bar():
    for t, name in enumerate(C.EDGE_NAMES):
        same, bits, ratio, _, _ = _edge_bars(None, t)
        assert same and bits and not ratio > 0, name


@pytest.mark.parametrize("variant", list(EDGE_VARIANTS))
def test_a_wrong_rule_misses_an_edge_bar(variant):
    case, what = EDGE_VARIANTS[variant]
    same, bits, ratio, keep, want = _edge_bars(variant, C.EDGE_NAMES.index(case))
    differ = np.nonzero(keep != want)[0].tolist()
    print(f"{variant} on {case}: decisions equal {same}, obs_keep differs at positions {differ}, "
          f"deviation {ratio:.3g} x the tolerance, bits equal {bits} ({what})")
    if what.startswith("kept set"):
        assert not same and differ
    else:
        assert same and not bits and ratio >= MARGIN


# variant of check_csr -> (the malformed CSR that separates it, what it reports there)
CSR_VARIANTS = {"first offender found": ("starts_1500_2600", (1, 2600)),
                "image ids before starts": ("start_2000_image_5", (2, 5))}


def test_the_csr_check_meets_its_bars_and_its_wrong_variants_miss_them():
    p = C.big_csr()
    cases = C.malformed_csrs(p)
    for name, (ts, img, want) in cases.items():
        assert O.check_csr(ts, img, len(p["Rt"])) == want, name
    for variant, (name, wrong) in CSR_VARIANTS.items():
        ts, img, want = cases[name]
        got = O.check_csr(ts, img, len(p["Rt"]), variant=variant)
        print(f"{variant} on {name}: {got}, the header's sentence gives {want}")
        assert got == wrong != want

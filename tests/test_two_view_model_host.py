"""The two-view bars bite (host, no GPU): deliberately wrong variants of the header's rules go
through the comparisons that the kernel goes through (two_view.npz: status, mask, inlier count and
iterations equal; F within the recorded tolerance; F bit-equal, the bar that the fixed summation
order earns and that the package's host path is held to) and must miss them; the unbroken oracle
must meet them.  Each variant names the pair that separates it.  Figures are printed (pytest -s)."""
import numpy as np
import pytest

import two_view_cases as C
import two_view_oracle as O
from conftest import golden

GOLD = golden("two_view")
MARGIN = 10.0

# variant -> (the pair of the "main" batch that separates it, what it gets wrong there)
VARIANTS = {
    "no_hartley": ("n64_out30", "decisions: raw pixel coordinates give another best hypothesis, "
                                "another mask and another iteration count"),
    "no_rank2": ("n257_out30", "F: without the rank-2 step the epipolar lines do not meet"),
    "algebraic": ("n257_out30", "decisions: (x1^T F x0)^2 is not in pixels, every match passes"),
    "no_refit": ("n257_out30", "F: the minimal sample's model, not the inliers' least squares"),
    "reverse_sums": ("n1000_out0", "bits: F differs in the last places only"),
}


@pytest.fixture(scope="module")
def main_batch():
    return C.gpu_batches(int(GOLD["max_points"]))["main"]


def _bars(batch, name, variant):
    """(decisions equal, F deviation / tolerance, F bits equal) on one pair."""
    b = batch["names"].index(name)
    n = int(batch["n"][b])
    r = O.verify(batch["pts0"][b, :n], batch["pts1"][b, :n], variant=variant, **batch["options"])
    same = (r["status"] == GOLD["main_status"][b] and r["iters"] == GOLD["main_iters"][b]
            and r["n_inliers"] == GOLD["main_n_inliers"][b]
            and np.array_equal(r["mask"], GOLD["main_mask"][b, :n].astype(bool)))
    dev = np.abs(O.normalised(r["F"]) - O.normalised(GOLD["main_F"][b])).max()
    return same, dev / float(GOLD["f_tol"]), r["F"].tobytes() == GOLD["main_F"][b].tobytes()


def test_the_oracle_meets_every_bar(main_batch):
    for name in sorted({case for case, _ in VARIANTS.values()}):
        same, ratio, bits = _bars(main_batch, name, None)
        assert same and bits and ratio == 0, name


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_wrong_rule_misses_a_bar(variant, main_batch):
    assert set(VARIANTS) == set(O.VARIANTS)
    case, what = VARIANTS[variant]
    same, ratio, bits = _bars(main_batch, case, variant)
    print(f"{variant} on {case}: decisions equal {same}, F deviation {ratio:.3g} x the tolerance, "
          f"bits equal {bits} ({what})")
    if what.startswith("decisions"):
        assert not same
    elif what.startswith("F"):
        assert same and ratio >= MARGIN
    else:
        assert same and ratio <= 1.0 and not bits


# ---- the option fixtures' bar (tests/golden/make_golden_two_view_options.py) ----------------------
OPT = golden("two_view_options")


def _refit_bars(variant):
    """(decisions equal, F bits equal, inlier count) on the pair of tight_refine5 that the
    generator recorded: its refit after the RANSAC model is not kept, which ends the refits."""
    call = C.option_calls()["tight_refine5"]
    b = int(OPT["refine_pairs"][2])
    n = int(call["n"][b])
    r = O.verify(call["pts0"][b, :n], call["pts1"][b, :n], variant=variant, **call["options"])
    same = (r["status"] == OPT["tight_refine5_status"][b] and r["iters"] == OPT["tight_refine5_iters"][b]
            and r["n_inliers"] == OPT["tight_refine5_n_inliers"][b]
            and np.array_equal(r["mask"], OPT["tight_refine5_mask"][b, :n].astype(bool)))
    return call["names"][b], same, r["F"].tobytes() == OPT["tight_refine5_F"][b].tobytes(), r["n_inliers"]


def test_refits_that_never_stop_miss_the_option_bar():
    """At refine_iters = 5 with max_error = 0.7 px the recorded pair keeps its RANSAC model: the
    first refit has fewer inliers and ends the refits.  Going on from the inliers of the refit that
    was not kept reaches another model, another mask and another F."""
    assert O.OPTION_VARIANTS == ("refits_never_stop",)
    name, same, bits, nin = _refit_bars(None)
    assert same and bits
    name, same, bits, other = _refit_bars("refits_never_stop")
    print(f"refits_never_stop on tight_refine5/{name}: decisions equal {same}, F bits equal {bits}, "
          f"{other} inliers where the contract keeps {nin}")
    assert not same and not bits

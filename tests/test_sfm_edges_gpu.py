"""The paths of the sparse-reconstruction kernels that tests/test_sfm_gpu.py never enters, against
the plain-loop oracle's recorded results (tests/golden/make_golden_sfm_edges.py): drops, duplicates
and +inf errors past position 63, exact duplicate ties, the final check removing an observation,
a rejected first Gauss-Newton step, a drop loop of 62 turns, a non-finite X, empty tracks; a CSR
of more tracks and observations than one stride of its check, clean and malformed; the thresholds
at +inf and 0; and the status words of onepose_track_components."""
import numpy as np
import pytest

import sfm_cases as C
import sfm_oracle as O
from conftest import golden
from onepose_amd import _lib
from test_sfm_gpu import GRAPHS, components, triangulate

pytestmark = pytest.mark.gpu

EDGES = golden("sfm_tri_edges")
EDGE_BITS = [n for t, n in enumerate(C.EDGE_NAMES)
             if EDGES["edge_reason"][t] == 0 and n not in C.EDGE_DEGENERATE]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def keep_of(p, out, name):
    t = C.EDGE_NAMES.index(name)
    return out["obs_keep"][p["track_start"][t]:p["track_start"][t + 1]]


def assert_decisions(p, out, want, prefix):
    """reason, n_kept and obs_keep equal the fixture; a rejected track has NaN, NaN, 0, zeros."""
    assert out["status"][0] == 0
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(out[k], want[f"{prefix}_{k}"]), (k, out[k], want[f"{prefix}_{k}"])
    lost = want[f"{prefix}_reason"] != 0
    assert np.isnan(out["xyz"][lost]).all() and np.isnan(out["err"][lost]).all()
    assert not out["n_kept"][lost].any()
    kept_obs = np.repeat(~lost, np.diff(p["track_start"]))
    assert not out["obs_keep"][~kept_obs].any()


def bits_equal(out, want, prefix, t):
    return (out["xyz"][t].tobytes() == want[f"{prefix}_xyz"][t].tobytes()
            and out["err"][t].tobytes() == want[f"{prefix}_err"][t].tobytes())


# ---- the edge fixture ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_out(lib, device):
    p = C.edge_problem()
    assert C.tri_sha(p) == str(EDGES["edge_sha"])
    return p, triangulate(lib, device, p)


def test_edge_decisions_equal_the_oracle(edge_out):
    p, out = edge_out
    assert float(EDGES["edge_margin"]) >= 1e-6
    assert_decisions(p, out, EDGES, "edge")
    got = {n: int(out["reason"][t]) for t, n in enumerate(C.EDGE_NAMES)}
    print("reasons:", got)
    for name in C.EDGE_KEPT:
        assert got[name] == 0, name
    assert got["empty_mid"] == got["empty_last"] == 3 and got["parallel_rays"] == 4
    # what each case is for, so that a fixture recorded again cannot change it silently
    for name, dropped in C.EDGE_DROPS.items():
        assert np.array_equal(np.nonzero(~keep_of(p, out, name))[0], dropped), name
    k = keep_of(p, out, "dup_exact_tie")
    assert all(k[s] and not k[d] for s, d in C.EDGE_TIES) and k.sum() == len(k) - 3
    k = keep_of(p, out, "dup_past_64")
    assert all(k[list(g)].sum() == 1 for g in C.EDGE_DUPS) and k.sum() == len(k) - 3
    assert keep_of(p, out, "final_check_drop").sum() == 3   # all four pass at the DLT point
    assert keep_of(p, out, "noise_free").all()
    assert len(keep_of(p, out, "mostly_unrelated")) == 64


@pytest.mark.parametrize("name", EDGE_BITS)
def test_edge_track_within_the_recorded_tolerance_and_bit_equal(name, edge_out):
    p, out = edge_out
    t = C.EDGE_NAMES.index(name)
    tol = float(EDGES["edge_tol"][t])
    dev = max(np.abs(out["xyz"][t] - EDGES["edge_xyz"][t]).max(),
              abs(out["err"][t] - EDGES["edge_err"][t]))
    ls = np.abs(out["xyz"][t] - EDGES["edge_ls_xyz"][t]).max()
    bits = bits_equal(out, EDGES, "edge", t)
    print(f"{name}: deviation {dev:.2e} (tol {tol:.1e}), {ls:.2e} from the least_squares minimum "
          f"(the oracle: {float(EDGES['edge_ls_dist'][t]):.2e}), bits equal: {bits}")
    assert out["reason"][t] == 0
    assert dev <= tol
    assert ls <= float(EDGES["edge_ls_dist"][t]) + tol
    assert bits


def test_edge_two_calls_are_bit_equal(lib, device, edge_out):
    p, out = edge_out
    again = triangulate(lib, device, p)
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k


def test_edge_thresholds_are_arguments(lib, device, edge_out):
    """max_reproj = +inf: no error exceeds it, so nothing is dropped by the loop or the final
    check (a point behind a camera scores +inf, and +inf <= +inf), the duplicate rule and the
    reasons 3 and 4 stay; max_reproj = 0: every track of two or more observations is lost to
    reason 1, 3 or 4, the degenerate ones aside (same_ray's errors are exactly 0 and pass e <= 0)."""
    p, _ = edge_out
    loose = triangulate(lib, device, p, max_reproj=float("inf"))
    assert_decisions(p, loose, EDGES, "inf")
    kept = np.nonzero(EDGES["inf_reason"] == 0)[0]
    bits = [bits_equal(loose, EDGES, "inf", t) for t in kept]
    print(f"max_reproj = +inf: kept {loose['n_kept'].tolist()}, bit-equal on {sum(bits)} of "
          f"{len(kept)} kept tracks")
    assert all(bits)
    lens = np.diff(p["track_start"])
    assert np.array_equal(loose["n_kept"][kept], lens[kept] - np.array(
        [3 if C.EDGE_NAMES[t] in ("dup_past_64", "dup_exact_tie") else 0 for t in kept]))
    none = triangulate(lib, device, p, max_reproj=0.0)
    assert np.array_equal(none["reason"], EDGES["zero_reason"])
    plain = np.array([lens[t] >= 2 and n not in C.EDGE_DEGENERATE
                      for t, n in enumerate(C.EDGE_NAMES)])
    assert set(none["reason"][plain].tolist()) <= {1, 3, 4}
    assert not none["obs_keep"].any() and not none["n_kept"].any()


# ---- a CSR larger than one stride of the check ---------------------------------------------------
@pytest.fixture(scope="module")
def big():
    p = C.big_csr()
    assert C.tri_sha(p) == str(EDGES["big_sha"])
    assert len(p["track_start"]) - 1 > 2048 and len(p["obs_image"]) > 4096
    return p


def test_big_csr_equals_the_oracle(lib, device, big):
    out = triangulate(lib, device, big)
    assert float(EDGES["big_margin"]) >= 1e-6
    assert tuple(out["status"]) == (0, 0)
    assert_decisions(big, out, EDGES, "big")
    kept = EDGES["big_reason"] == 0
    dev = np.maximum(np.abs(out["xyz"] - EDGES["big_xyz"]).max(1), np.abs(out["err"] - EDGES["big_err"]))
    bits = sum(bits_equal(out, EDGES, "big", t) for t in np.nonzero(kept)[0])
    print(f"big CSR: {kept.sum()} of {len(kept)} tracks kept, largest deviation / tolerance "
          f"{(dev[kept] / EDGES['big_tol'][kept]).max():.3g}, bit-equal on {bits}")
    assert (dev[kept] <= EDGES["big_tol"][kept]).all()
    assert bits == kept.sum()
    assert (EDGES["big_reason"][np.diff(big["track_start"]) == 0] == 3).all()


BIG_WANT = {"start_1023": (1, 1023), "start_1024": (1, 1024),
            "start_last_track": (1, C.BIG_TRACKS - 1), "starts_1500_2600": (1, 1500),
            "image_4095": (2, 4095), "images_4500_1030": (2, 1030), "start_2000_image_5": (1, 2000),
            "end_entry": (1, C.BIG_TRACKS)}


@pytest.mark.parametrize("what", list(BIG_WANT))
def test_a_malformed_big_csr_sets_status_and_writes_nothing(what, lib, device, big):
    ts, img, want = C.malformed_csrs(big)[what]
    assert want == BIG_WANT[what] == O.check_csr(ts, img, len(big["Rt"]))
    out = triangulate(lib, device, dict(big, track_start=ts, obs_image=img))
    assert tuple(out["status"]) == want
    # Guarded fills with 0xA5: every output byte is still that
    assert (out["reason"].view(np.uint8) == 0xA5).all() and (out["n_kept"].view(np.uint8) == 0xA5).all()
    assert (out["xyz"].view(np.uint8) == 0xA5).all() and (out["err"].view(np.uint8) == 0xA5).all()
    assert (out["obs_keep"].view(np.uint8) != 0).all()


# ---- the status words of the components ---------------------------------------------------------
@pytest.mark.parametrize("name", ["out_of_range", "duplicates", "self_loops", "sparse65537"])
def test_no_round_leaves_the_identity_and_counts_the_open_edges(name, lib, device):
    edges, n = GRAPHS[name]
    par, status = components(lib, device, edges, n, 0)
    inside = ((edges >= 0) & (edges < n)).all(1)
    assert np.array_equal(par.numpy(), np.arange(n))
    assert status[1] == 0
    assert status[0] == int((inside & (edges[:, 0] != edges[:, 1])).sum())   # duplicates count
    assert status[2] == int((~inside).sum())
    assert status[2] == (C.OUT_OF_RANGE_COUNT if name == "out_of_range" else 0)


def test_one_round_reports_the_edges_still_open(lib, device):
    edges, n = GRAPHS["path1025_random"]
    par, status = components(lib, device, edges, n, 1)
    label = par.numpy()
    still = int((label[edges[:, 0]] != label[edges[:, 1]]).sum())
    print(f"path1025_random after one round: {still} of {len(edges)} edges open")
    assert 0 < still < len(edges) and status[0] == still and status[1] == 1

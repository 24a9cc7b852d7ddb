"""onepose_triangulate on the GPU against the numpy.linalg.svd oracle's recorded results.  The
tolerance of each size is 16 x the deviation, on the same inputs, between svd(A) and an
eigh(A^T A) evaluation in float64 (floor 1e-12), recorded by tests/golden/make_golden_ba.py; the
keep masks must be equal (the generator keeps every decision >= 1e-6 from its threshold)."""
import os

import numpy as np
import pytest
import torch

import ba_cases
import ba_oracle as O
from ba_cases import Guarded
from onepose_amd import _lib, tracker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def tri():
    return np.load(os.path.join(ba_cases.GOLDEN, "triangulate.npz"))


def run(lib, device, P1, P2, p1, p2, rep_thr=20.0, z_max=0.15):
    n = len(p1)
    g = [Guarded(device, data=a) for a in (P1, P2, p1, p2)]
    X, e1, e2, z = (Guarded(device, nbytes=8 * n * k) for k in (3, 1, 1, 1))
    keep = Guarded(device, nbytes=n, dtype=torch.uint8)
    rc = lib.onepose_triangulate(g[0].ptr, g[1].ptr, g[2].ptr, g[3].ptr, n, rep_thr, z_max,
                                 X.ptr, e1.ptr, e2.ptr, z.ptr, keep.ptr, _lib.stream_ptr(device))
    _lib.check(rc, "onepose_triangulate")
    torch.cuda.synchronize(device)
    for x in (*g, X, e1, e2, z, keep):
        assert x.intact(), "guard words overwritten"
    return X.numpy((n, 3)), e1.numpy(), e2.numpy(), z.numpy(), keep.numpy().astype(bool)


@pytest.mark.parametrize("n", ba_cases.TRI_SIZES)
def test_triangulate_matches_the_svd_oracle(n, lib, tri, device):
    d, P1, P2 = ba_cases.tri_inputs(n)
    assert ba_cases.sha(*[d[k] for k in sorted(d)]) == str(tri[f"n{n}_sha"])
    X, e1, e2, z, keep = run(lib, device, P1, P2, d["kpt2d_1"], d["kpt2d_2"])
    tol = float(tri[f"n{n}_tol"])
    dev = max(np.abs(X - tri[f"n{n}_points"]).max(), np.abs(e1 - tri[f"n{n}_err1"]).max(),
              np.abs(e2 - tri[f"n{n}_err2"]).max())
    print(f"n={n}: deviation {dev:.2e} (tol {tol:.1e}), kept {int(keep.sum())}")
    assert np.array_equal(keep, tri[f"n{n}_keep"])
    assert dev <= tol
    assert np.array_equal(z, X[:, 2])
    if n >= 63:   # each of the three filters removes something, and something stays
        assert (e1 > 20).any() and (e2 > 20).any() and (z > 0.15).any() and keep.any()
        again = run(lib, device, P1, P2, d["kpt2d_1"], d["kpt2d_2"])
        assert all(np.array_equal(a, b) for a, b in zip((X, e1, e2, z, keep), again))


def test_thresholds_are_arguments(lib, device):
    d, P1, P2 = ba_cases.tri_inputs(65)
    X, e1, e2, z, keep = run(lib, device, P1, P2, d["kpt2d_1"], d["kpt2d_2"], 1e9, 1e9)
    assert keep.all()
    _, _, _, _, none = run(lib, device, P1, P2, d["kpt2d_1"], d["kpt2d_2"], -1.0, 1e9)
    assert not none.any()
    _, _, _, _, byz = run(lib, device, P1, P2, d["kpt2d_1"], d["kpt2d_2"], 1e9, 0.0)
    assert np.array_equal(byz, z <= 0.0) and byz.any() and not byz.all()


def test_degenerate_pairs_are_not_kept(lib, device):
    """w == 0 (all-zero projection matrices leave A^T A = 0, whose first eigenvector has w = 0)
    and a non-finite pixel: not kept, and nothing else is disturbed."""
    d, P1, P2 = ba_cases.tri_inputs(64)
    X, e1, e2, z, keep = run(lib, device, np.zeros((3, 4)), np.zeros((3, 4)), d["kpt2d_1"],
                             d["kpt2d_2"], 1e300, 1e300)
    assert not keep.any() and not np.isfinite(X).all(1).any()
    p1 = d["kpt2d_1"].copy()
    p1[7, 0] = np.nan
    p1[9, 1] = np.inf
    X, e1, e2, z, keep = run(lib, device, P1, P2, p1, d["kpt2d_2"], 1e300, 1e300)
    assert not keep[7] and not keep[9] and keep.sum() == 62


def test_python_layer_inverts_tcw(tri, device):
    d, P1, P2 = ba_cases.tri_inputs(63)
    pts, keep, e1, e2 = tracker.triangulate_filter(d["K1"], d["K2"], d["Tcw1"], d["Tcw2"],
                                                   d["kpt2d_1"], d["kpt2d_2"])
    tol = float(tri["n63_tol"])
    assert np.abs(pts - tri["n63_points"]).max() <= tol and np.array_equal(keep, tri["n63_keep"])
    only = tracker.apply_triangulation(d["K1"], d["K2"], d["Tcw1"], d["Tcw2"], d["kpt2d_1"],
                                       d["kpt2d_2"])
    assert np.array_equal(only, pts)
    # the filters are the reference's lines: project() with the pose, norm, > 20 and z > 0.15
    pose1, pose2 = np.linalg.inv(d["Tcw1"]), np.linalg.inv(d["Tcw2"])
    r1 = np.linalg.norm(tracker.project(pts, d["K1"], pose1[:3]) - d["kpt2d_1"], axis=1)
    r2 = np.linalg.norm(tracker.project(pts, d["K2"], pose2[:3]) - d["kpt2d_2"], axis=1)
    rm = np.unique(np.concatenate([np.where(r1 > 20)[0], np.where(r2 > 20)[0],
                                   np.where(pts[:, 2] > 0.15)[0]]))
    assert np.array_equal(np.where(~keep)[0], rm)


# ---- the tracker's own geometry, against a 50-digit eigenvector ---------------------------------
@pytest.fixture(scope="module")
def tri_edges():
    return np.load(os.path.join(ba_cases.GOLDEN, "triangulate_edges.npz"))


@pytest.mark.parametrize("name", list(ba_cases.TRI_EDGE_CASES))
def test_triangulate_matches_the_model_at_short_baselines(name, lib, tri_edges, device):
    """130 pairs (three workgroups) at baselines of 0.1 .. 2 degrees, with and without noise, and
    at f = 3000, against mpmath.eigsy at 50 digits (tests/golden/make_golden_tri_edges.py).  The
    bar is 16 x what numpy.linalg.eigh(A^T A) in float64 deviates from that, floor 1e-12; the
    keep masks are equal (every decision is >= 1e-6 from the case's thresholds)."""
    P1, P2, p1, p2 = ba_cases.tri_edge_inputs(name)
    assert ba_cases.sha(P1, P2, p1, p2) == str(tri_edges[f"{name}_sha"])
    thr, zmax = float(tri_edges[f"{name}_rep_thr"]), float(tri_edges[f"{name}_z_max"])
    X, e1, e2, z, keep = run(lib, device, P1, P2, p1, p2, thr, zmax)
    tol = float(tri_edges[f"{name}_tol"])
    dev = max(np.abs(X - tri_edges[f"{name}_points"]).max(),
              np.abs(e1 - tri_edges[f"{name}_err1"]).max(),
              np.abs(e2 - tri_edges[f"{name}_err2"]).max())
    print(f"{name}: deviation {dev:.2e} (tol {tol:.1e}, ratio {dev / tol:.3f}), kept "
          f"{int(keep.sum())}")
    assert np.array_equal(keep, tri_edges[f"{name}_keep"])
    assert dev <= tol
    assert (e1 > thr).any() and (e2 > thr).any() and (z > zmax).any() and keep.any()


def _tri_property_inputs(tri_edges):
    for name in ba_cases.TRI_EDGE_CASES:
        yield (name, ba_cases.tri_edge_inputs(name), float(tri_edges[f"{name}_rep_thr"]),
               float(tri_edges[f"{name}_z_max"]))
    for name, inputs in ba_cases.tri_degenerate_inputs().items():
        yield name, inputs, 20.0, 1e300


def test_triangulate_properties(lib, tri_edges, device):
    """Over every case and two degenerate inputs (identical views; a pixel pair at both epipoles,
    A^T A exactly singular twice): a kept pair has a finite X whose reprojection errors,
    recomputed on the host from the returned X, are within the threshold (+ 1e-9 px) and whose z
    is; z is X[:, 2]; two runs are bit-equal; guards are intact (run() asserts them).  No claim
    about which degenerate pairs are kept."""
    for name, (P1, P2, p1, p2), thr, zmax in _tri_property_inputs(tri_edges):
        X, e1, e2, z, keep = run(lib, device, P1, P2, p1, p2, thr, zmax)
        again = run(lib, device, P1, P2, p1, p2, thr, zmax)
        for a, b in zip((X, e1, e2, z, keep), again):
            assert np.array_equal(a, b, equal_nan=True), name
        assert np.array_equal(z, X[:, 2], equal_nan=True), name
        assert np.isfinite(X[keep]).all(), name
        with np.errstate(all="ignore"):
            h1, h2 = O.reproject(P1, X[keep], p1[keep]), O.reproject(P2, X[keep], p2[keep])
        assert (h1 <= thr + 1e-9).all() and (h2 <= thr + 1e-9).all(), name
        assert (z[keep] <= zmax).all(), name
        print(f"{name}: kept {int(keep.sum())} of {len(keep)}")

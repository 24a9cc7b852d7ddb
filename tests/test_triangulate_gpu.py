"""onepose_triangulate on the GPU against the numpy.linalg.svd oracle's recorded results.  The
tolerance of each size is 16 x the deviation, on the same inputs, between svd(A) and an
eigh(A^T A) evaluation in float64 (floor 1e-12), recorded by tests/golden/make_golden_ba.py; the
keep masks must be equal (the generator keeps every decision >= 1e-6 from its threshold)."""
import os

import numpy as np
import pytest
import torch

import ba_cases
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

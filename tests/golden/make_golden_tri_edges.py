"""Triangulation at the baselines the tracker really has, against a 50-digit eigenvector.

    python tests/golden/make_golden_tri_edges.py       (needs mpmath; nothing else outside the tree)

``triangulate_edges.npz`` holds, per case of tests/ba_cases.py::TRI_EDGE_CASES (130 pairs each:
views 0.1, 0.5 and 2 degrees apart with a few mm of translation, with 0.5 px of noise and
noise-free -- the smallest eigenvalue is then about 0 --, and f = 3000 with pixels up to about
4000), the SHA-256 of the inputs (the tests regenerate them) and

* ``points``, ``err1``, ``err2``, ``keep``: the reference.  The DLT matrix A is formed from the
  float64 inputs at 50 digits, the eigenvector of A^T A's smallest eigenvalue comes from
  ``mpmath.eigsy``, is dehomogenised, and both reprojection errors are recomputed from it at 50
  digits; all rounded to float64 at the end.
* ``rep_thr``, ``z_max``: the case's thresholds, the geometric / arithmetic middle of two
  neighbouring sorted reference values (err1 at rank 88 %, z at rank 70 %).  Asserted: every keep
  decision is >= 1e-6 (relative) from its threshold, each of the three filters removes a pair,
  and some pair stays.
* ``tol`` = 16 x the largest deviation of ``numpy.linalg.eigh(A^T A)`` in float64 (points and
  both errors, ba_oracle.triangulate_filter with method "eig") from that reference, floor 1e-12.
  The bar measures what a backward-stable float64 eigensolver on A^T A loses at that geometry;
  it says nothing about LAPACK against LAPACK.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ba_cases  # noqa: E402
import ba_oracle as O  # noqa: E402

mp.mp.dps = 50
FACTOR, FLOOR, MARGIN = 16.0, 1e-12, 1e-6


def reference(P1, P2, p1, p2, which=0):
    """(X [n,3], err1, err2) from the eigenvector of the ``which``-th smallest eigenvalue."""
    n = len(p1)
    X, e1, e2 = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    M1, M2 = mp.matrix(P1.tolist()), mp.matrix(P2.tolist())
    for i in range(n):
        A = mp.matrix(4, 4)
        for j in range(4):
            A[0, j] = mp.mpf(float(p1[i, 0])) * M1[2, j] - M1[0, j]
            A[1, j] = mp.mpf(float(p1[i, 1])) * M1[2, j] - M1[1, j]
            A[2, j] = mp.mpf(float(p2[i, 0])) * M2[2, j] - M2[0, j]
            A[3, j] = mp.mpf(float(p2[i, 1])) * M2[2, j] - M2[1, j]
        E, Q = mp.eigsy(A.T * A)
        k = sorted(range(4), key=lambda j: E[j])[which]
        x = [Q[j, k] / Q[3, k] for j in range(3)]
        X[i] = [float(v) for v in x]
        for M, uv, out in ((M1, p1[i], e1), (M2, p2[i], e2)):
            h = [M[r, 0] * x[0] + M[r, 1] * x[1] + M[r, 2] * x[2] + M[r, 3] for r in range(3)]
            du, dv = h[0] / h[2] - mp.mpf(float(uv[0])), h[1] / h[2] - mp.mpf(float(uv[1]))
            out[i] = float(mp.sqrt(du * du + dv * dv))
    return X, e1, e2


def between(values, frac, geometric):
    s = np.sort(values)
    k = int(frac * len(s))
    return float(np.sqrt(s[k] * s[k + 1])) if geometric else float(0.5 * (s[k] + s[k + 1]))


def main():
    out = {}
    for name in ba_cases.TRI_EDGE_CASES:
        P1, P2, p1, p2 = ba_cases.tri_edge_inputs(name)
        X, e1, e2 = reference(P1, P2, p1, p2)
        thr, zmax = between(e1, 0.88, True), between(X[:, 2], 0.70, False)
        keep = (e1 <= thr) & (e2 <= thr) & (X[:, 2] <= zmax)
        assert np.isfinite(X).all() and np.isfinite(e1).all() and np.isfinite(e2).all()
        assert np.abs(e1 / thr - 1).min() >= MARGIN and np.abs(e2 / thr - 1).min() >= MARGIN
        assert np.abs(X[:, 2] / zmax - 1).min() >= MARGIN
        assert (e1 > thr).any() and (e2 > thr).any() and (X[:, 2] > zmax).any() and keep.any()
        Xe, e1e, e2e, _, keepe = O.triangulate_filter(P1, P2, p1, p2, thr, zmax, method="eig")
        assert np.array_equal(keep, keepe)
        dev = max(np.abs(Xe - X).max(), np.abs(e1e - e1).max(), np.abs(e2e - e2).max())
        tol = max(FACTOR * dev, FLOOR)
        print(f"{name}: kept {int(keep.sum())} of {len(keep)}, rep_thr {thr:.3g}, z_max "
              f"{zmax:.3g}, |X| <= {np.abs(X).max():.2g}, eigh deviates {dev:.1e}, tol {tol:.1e}")
        out.update({f"{name}_sha": ba_cases.sha(P1, P2, p1, p2), f"{name}_points": X,
                    f"{name}_err1": e1, f"{name}_err2": e2, f"{name}_keep": keep,
                    f"{name}_rep_thr": thr, f"{name}_z_max": zmax, f"{name}_tol": tol})
    np.savez_compressed(os.path.join(HERE, "triangulate_edges.npz"), **out)


if __name__ == "__main__":
    main()

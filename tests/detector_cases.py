"""Synthetic cases shared by the 2D object detector's tests (host and GPU)."""
import numpy as np

import detector_oracle as D


def similarity(scale, deg, tx, ty):
    c, s = scale * np.cos(np.deg2rad(deg)), scale * np.sin(np.deg2rad(deg))
    return np.array([[c, -s, tx], [s, c, ty]])


def scene(n, outlier_share, seed, A=None, sigma=0.5, w=320, h=240):
    """n correspondences under A with sigma px noise; round(n * share) of them, at shuffled
    positions, are gross outliers at least 20 px from where A sends them.  Returns (from, to,
    inlier flags, A)."""
    rs = np.random.RandomState(seed)
    A = similarity(0.6, 25.0, 100.5, 60.5) if A is None else A
    f = rs.uniform([0, 0], [w, h], (n, 2))
    t = f @ A[:, :2].T + A[:, 2] + sigma * rs.standard_normal((n, 2))
    n_out = int(round(n * outlier_share))
    ang, r = rs.uniform(0, 2 * np.pi, n_out), rs.uniform(20, 200, n_out)
    t[:n_out] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    perm = rs.permutation(n)
    inl = np.ones(n, bool)
    inl[:n_out] = False
    return f[perm].astype(np.float32), t[perm].astype(np.float32), inl[perm], A


def view_size(A, margin):
    """A view (h, w) whose four corners land at least `margin` from an integer under A."""
    for w in range(300, 340):
        for h in range(220, 260):
            _, pre = D.view_bbox(A, h, w)
            if np.abs(pre - np.rint(pre)).min() > margin:
                return h, w
    raise AssertionError("no view size found")


def stage_case(spec=((30, 12), (20, 18), (5, 5)), n0=40, n1=64, pad=4, seed=5, per_view=False):
    """One query against len(spec) views: view b has spec[b] = (matches, inliers) -- the other
    matches are gross outliers -- among its first n0 - pad keypoints; the last `pad` keypoints
    lie past counts0 and hold poison (NaN coordinates, a valid-looking match) that must never
    be read.  per_view: every view gets a query of its own ([B, n1, 2]).
    Returns (matches0, counts0, kpts0, kpts1, db_hw, query_hw)."""
    rs = np.random.RandomState(seed)
    B = len(spec)
    A = similarity(0.8, -10.0, 30.25, 12.75)
    Ainv = np.linalg.inv(np.vstack([A, [0, 0, 1]]))[:2]
    kpts1 = rs.uniform(0, 300, (B if per_view else 1, n1, 2)).astype(np.float32)
    kpts0 = np.zeros((B, n0, 2), np.float32)
    matches0 = -np.ones((B, n0), np.int64)
    for b, (nm, good) in enumerate(spec):
        k1 = kpts1[b if per_view else 0]
        q = rs.permutation(n1)[:nm]
        rows = np.sort(rs.permutation(n0 - pad)[:nm])
        kpts0[b, rows] = k1[q] @ Ainv[:, :2].T + Ainv[:, 2]
        kpts0[b, rows[good:]] += rs.uniform(40, 90, (nm - good, 2)).astype(np.float32)
        matches0[b, rows] = q
    if pad:
        kpts0[:, n0 - pad:] = np.nan
        matches0[:, n0 - pad:] = 3
    counts0 = np.full(B, n0 - pad, np.int32)
    db_hw = np.stack([[240 - 20 * (b % 3), 320 - 10 * (b % 4)] for b in range(B)]).astype(np.int32)
    return matches0, counts0, kpts0, (kpts1 if per_view else kpts1[0]), db_hw, (480, 640)


def ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((7 * xx + 13 * yy) % 251).astype(np.uint8)

"""numpy float64 oracle of the tracker back end (include/onepose_hip.h, "Tracker back end").

The cost function restates the reference's ``SnavelyReprojectionErrorV2`` /
``AngleAxisRotatePoint`` (src/tracker/tracking_utils.py:91-169) and is pinned to it by the
fixtures of tests/golden/make_golden_ba.py.  The Levenberg-Marquardt on top is this project's own
algorithm, stated in the header; this file is its definition in numpy, the HIP solver is compared
against it.  Every sum over observations runs in observation order (``np.add.at``), so a
permutation of the observations changes the rounding only: the spread of the results under
permutations is what the GPU tests' tolerance is made of.
"""
import numpy as np

INFO_HEAD, INFO_ROW, INFO_ITERS = 8, 6, 16
INFO_DOUBLES = INFO_HEAD + INFO_ROW * INFO_ITERS
ST_OK, ST_FAILED, ST_BAD_INDEX = 0, 1, 2
MIN_RHO = 1e-3
SERIES_TH2 = 1e-4   # theta^2 below which the Jacobian takes b, ca, ab from their series


def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1),
                     np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def linearize(points, cams, feats, pt_idx, cam_idx, jac=True):
    """residuals [N,2] and, with ``jac``, Jc [N,2,6], Jp [N,2,3]."""
    X = points[pt_idx]
    w, t = cams[cam_idx, :3], cams[cam_idx, 3:6]
    th2 = (w * w).sum(1)
    pos = th2 > 0
    th = np.sqrt(np.where(pos, th2, 1.0))
    c, s = np.cos(th), np.sin(th)
    k = w / th[:, None]
    p_rod = (X * c[:, None] + np.cross(k, X) * s[:, None]
             + k * ((k * X).sum(1) * (1.0 - c))[:, None])
    wx = np.cross(w, X)
    p = np.where(pos[:, None], p_rod, X + wx) + t
    f = feats[:, 2]
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = np.stack([f * xp + feats[:, 3] - feats[:, 0], f * yp + feats[:, 4] - feats[:, 1]], 1)
    if not jac:
        return r
    N = len(X)
    a = np.where(pos, s / th, 1.0)
    # the Jacobian's coefficients: closed forms from SERIES_TH2 up, their series below it (there
    # 1 - cos, cos - a and a - 2 b cancel to nothing, and a subnormal theta^2 overflows the
    # quotient: the closed form gives NaN at |aa| = 1e-160)
    big = th2 >= SERIES_TH2
    den = np.where(big, th2, 1.0)
    b = np.where(big, (1.0 - c) / den, 0.5 + th2 * (-1.0 / 24.0 + th2 * (1.0 / 720.0)))
    ca = np.where(big, (c - a) / den, -1.0 / 3.0 + th2 * (1.0 / 30.0 + th2 * (-1.0 / 840.0)))
    ab = np.where(big, (a - 2.0 * b) / den,
                  -1.0 / 12.0 + th2 * (1.0 / 180.0 + th2 * (-1.0 / 6720.0)))
    b, ca, ab = np.where(pos, b, 0.0), np.where(pos, ca, 0.0), np.where(pos, ab, 0.0)
    cc = np.where(pos, c, 1.0)
    eye = np.eye(3)[None]
    wd = (w * X).sum(1)
    Wx, Xx = _skew(w), _skew(X)
    ww = w[:, :, None] * w[:, None, :]
    R = cc[:, None, None] * eye + a[:, None, None] * Wx + b[:, None, None] * ww
    M = (-a[:, None, None] * (X[:, :, None] * w[:, None, :])
         + ca[:, None, None] * (wx[:, :, None] * w[:, None, :])
         - a[:, None, None] * Xx
         + b[:, None, None] * (w[:, :, None] * X[:, None, :] + wd[:, None, None] * eye)
         + (ab * wd)[:, None, None] * ww)
    M = np.where(pos[:, None, None], M, -Xx)
    iz = 1.0 / p[:, 2]
    D = np.zeros((N, 2, 3))
    D[:, 0, 0] = f * iz
    D[:, 0, 2] = -f * xp * iz
    D[:, 1, 1] = f * iz
    D[:, 1, 2] = -f * yp * iz
    Jc = np.concatenate([D @ M, D], 2)
    Jp = D @ R
    return r, Jc, Jp


def cost(points, cams, feats, pt_idx, cam_idx):
    r = linearize(points, cams, feats, pt_idx, cam_idx, jac=False)
    return 0.5 * float((r * r).sum())


def build_index(pt_idx, cam_idx, n_cams, n_points):
    """The index of onepose_ba_build_index as a dict of arrays (stable orders, active lists)."""
    out = {}
    for name, key, n in (("cam", cam_idx, n_cams), ("pt", pt_idx, n_points)):
        key = np.asarray(key)
        if len(key) == 0 or key.min() < 0 or key.max() >= n:
            raise ValueError("id out of range")
        order = np.argsort(key, kind="stable")
        act, counts = np.unique(key, return_counts=True)
        out[name + "_order"] = order.astype(np.int32)
        out["act_" + name + "s"] = act.astype(np.int32)
        out[name + "_start"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


def _damp(d, mu):
    return mu * np.clip(d, 1e-6, 1e32)


def _chol3(V):
    """Lower Cholesky factors of symmetric positive 3 x 3 matrices, column by column (the HIP
    kernel's order)."""
    L = np.zeros_like(V)
    L[:, 0, 0] = np.sqrt(V[:, 0, 0])
    L[:, 1, 0] = V[:, 1, 0] / L[:, 0, 0]
    L[:, 2, 0] = V[:, 2, 0] / L[:, 0, 0]
    L[:, 1, 1] = np.sqrt(V[:, 1, 1] - L[:, 1, 0] * L[:, 1, 0])
    L[:, 2, 1] = (V[:, 2, 1] - L[:, 2, 0] * L[:, 1, 0]) / L[:, 1, 1]
    L[:, 2, 2] = np.sqrt(V[:, 2, 2] - L[:, 2, 0] * L[:, 2, 0] - L[:, 2, 1] * L[:, 2, 1])
    return L


def _fwd3(L, b):
    """L^-1 b for [n,3,3] lower factors and [n,3,k] right-hand sides."""
    y0 = b[:, 0] / L[:, 0, 0, None]
    y1 = (b[:, 1] - L[:, 1, 0, None] * y0) / L[:, 1, 1, None]
    y2 = (b[:, 2] - L[:, 2, 0, None] * y0 - L[:, 2, 1, None] * y1) / L[:, 2, 2, None]
    return np.stack([y0, y1, y2], 1)


def _bwd3(L, y):
    """L^-T y."""
    x2 = y[:, 2] / L[:, 2, 2, None]
    x1 = (y[:, 1] - L[:, 2, 1, None] * x2) / L[:, 1, 1, None]
    x0 = (y[:, 0] - L[:, 1, 0, None] * x1 - L[:, 2, 0, None] * x2) / L[:, 0, 0, None]
    return np.stack([x0, x1, x2], 1)


def solve(points, cams, feats, pt_idx, cam_idx, max_iters=5, max_success=5, radius=1e4,
          variant=False):
    """(points, cams, info): the header's algorithm.  Inputs are not modified.  V_p^-1 is never
    formed: with V_p = L L^T the whitened blocks Y_n = L^-1 W_n^T give W V^-1 W^T = Y^T Y, which
    keeps the rounding of the Schur complement at the size of S itself (an explicit inverse of a
    point seen by few cameras carries 1 / damping in every entry).  ``variant``: the same
    algorithm through other float64 routines (LAPACK Cholesky and LU solves for the 3 x 3
    systems, LU for the camera system): a second sample of the rounding of the small dense steps,
    which permuting observations cannot reach."""
    points, cams = points.copy(), cams.copy()
    info = np.zeros(INFO_DOUBLES)
    pt_idx, cam_idx = np.asarray(pt_idx), np.asarray(cam_idx)
    act_c, ac = np.unique(cam_idx, return_inverse=True)
    act_p, ap = np.unique(pt_idx, return_inverse=True)
    A, Pa = len(act_c), len(act_p)
    # pairs (n, m) of observations of one point, grouped by n in observation order
    order = np.argsort(ap, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(ap, minlength=Pa))])
    cnt = (start[1:] - start[:-1])[ap]
    pn = np.repeat(np.arange(len(ap)), cnt)
    pm = order[np.concatenate([np.arange(start[q], start[q + 1]) for q in ap])] if len(ap) else pn
    with np.errstate(all="ignore"):
        c0 = cost(points, cams, feats, pt_idx, cam_idx)
    info[3] = info[4] = c0
    info[5] = radius
    if not np.isfinite(c0):
        info[0] = ST_FAILED
        return points, cams, info
    cur, factor, it, succ = c0, 2.0, 0, 0
    while it < max_iters and succ < max_success:
        r, Jc, Jp = linearize(points, cams, feats, pt_idx, cam_idx)
        mu = 1.0 / radius
        U = np.zeros((A, 6, 6))
        V = np.zeros((Pa, 3, 3))
        gc, gp = np.zeros((A, 6)), np.zeros((Pa, 3))
        np.add.at(U, ac, Jc.transpose(0, 2, 1) @ Jc)
        np.add.at(V, ap, Jp.transpose(0, 2, 1) @ Jp)
        np.add.at(gc, ac, (Jc.transpose(0, 2, 1) @ r[:, :, None])[:, :, 0])
        np.add.at(gp, ap, (Jp.transpose(0, 2, 1) @ r[:, :, None])[:, :, 0])
        W = Jc.transpose(0, 2, 1) @ Jp
        i6, i3 = np.arange(6), np.arange(3)
        U[:, i6, i6] += _damp(U[:, i6, i6], mu)
        V[:, i3, i3] += _damp(V[:, i3, i3], mu)
        WT = W.transpose(0, 2, 1)                            # [N,3,6]
        if variant:
            Lv = np.linalg.cholesky(V)
            Y = np.linalg.solve(Lv[ap], WT)
            z = np.linalg.solve(Lv, gp[:, :, None])
        else:
            Lv = _chol3(V)
            Y = _fwd3(Lv[ap], WT)                            # L^-1 W^T, [N,3,6]
            z = _fwd3(Lv, gp[:, :, None])                    # L^-1 g_p, [Pa,3,1]
        S4 = np.zeros((A, A, 6, 6))
        S4[np.arange(A), np.arange(A)] = U
        np.subtract.at(S4, (ac[pn], ac[pm]), Y[pn].transpose(0, 2, 1) @ Y[pm])
        rhs = -gc
        np.add.at(rhs, ac, (Y.transpose(0, 2, 1) @ z[ap])[:, :, 0])
        S = S4.transpose(0, 2, 1, 3).reshape(6 * A, 6 * A)
        row = info[INFO_HEAD + INFO_ROW * it:INFO_HEAD + INFO_ROW * (it + 1)]
        row[0], row[4] = cur, radius
        accept = False
        try:
            L = np.linalg.cholesky(np.tril(S) + np.tril(S, -1).T)
            ok = True
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            if variant:
                dc = np.linalg.solve(L @ L.T, rhs.reshape(-1)).reshape(A, 6)
            else:
                y = np.linalg.solve(L, rhs.reshape(-1))
                dc = np.linalg.solve(L.T, y).reshape(A, 6)
            b = -z[:, :, 0]
            np.subtract.at(b, ap, (Y @ dc[ac][:, :, None])[:, :, 0])
            if variant:
                dp = np.linalg.solve(Lv.transpose(0, 2, 1), b[:, :, None])[:, :, 0]
            else:
                dp = _bwd3(Lv, b[:, :, None])[:, :, 0]
            cams_n, points_n = cams.copy(), points.copy()
            cams_n[act_c] += dc
            points_n[act_p] += dp
            with np.errstate(all="ignore"):
                cand = cost(points_n, cams_n, feats, pt_idx, cam_idx)
            Jd = (Jc @ dc[ac][:, :, None] + Jp @ dp[ap][:, :, None])[:, :, 0]
            md = -np.float64((Jd * (r + 0.5 * Jd)).sum())
            with np.errstate(all="ignore"):
                rho = np.float64(cur - cand) / md
            accept = bool(np.isfinite(cand) and md > 0 and rho > MIN_RHO)
            row[1], row[2], row[3] = cand, md, rho
        else:
            row[1] = row[2] = row[3] = np.nan
        row[5] = float(accept)
        if accept:
            points, cams, cur = points_n, cams_n, cand
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            factor = 2.0
            succ += 1
        else:
            radius /= factor
            factor *= 2.0
        it += 1
    info[1], info[2], info[4], info[5] = it, succ, cur, radius
    return points, cams, info


def rows(info):
    """info's per-iteration rows [iterations, 6]: cost, candidate, model decrease, rho, radius,
    accepted."""
    n = int(info[1])
    return info[INFO_HEAD:INFO_HEAD + INFO_ROW * n].reshape(n, INFO_ROW)


def significant(info, rel=1e-6):
    """Iterations whose model decrease exceeds ``rel`` x cost, and whose predecessors all do: only
    there are rho, the radius and the decision more than rounding noise."""
    rw = rows(info)
    with np.errstate(invalid="ignore"):
        sig = rw[:, 2] > rel * rw[:, 0]
    return np.logical_and.accumulate(sig)


def cost_deviation(info, ref):
    """Largest |difference| among the costs of two info blocks of equal iteration count (initial,
    final, each row's cost and candidate cost), as a fraction of the reference's initial cost: a
    cost that converges to zero has no relative error of its own."""
    a = np.concatenate([info[3:5], rows(info)[:, :2].ravel()])
    b = np.concatenate([ref[3:5], rows(ref)[:, :2].ravel()])
    d = np.abs(a - b)
    d[np.isnan(a) & np.isnan(b)] = 0.0
    return float(np.max(d) / ref[3]) if not np.isnan(d).any() else np.inf


# ---- triangulation ------------------------------------------------------------------------
def dlt_matrices(P1, P2, pts1, pts2):
    A = np.zeros((len(pts1), 4, 4))
    A[:, 0] = pts1[:, :1] * P1[2] - P1[0]
    A[:, 1] = pts1[:, 1:] * P1[2] - P1[1]
    A[:, 2] = pts2[:, :1] * P2[2] - P2[0]
    A[:, 3] = pts2[:, 1:] * P2[2] - P2[1]
    return A


def triangulate(P1, P2, pts1, pts2, method="svd"):
    """[n,4] homogeneous points: the smallest right singular vector of the DLT matrix A
    (``svd``), or the eigenvector of A^T A's smallest eigenvalue (``eig``)."""
    A = dlt_matrices(P1, P2, pts1, pts2)
    if method == "svd":
        return np.linalg.svd(A)[2][:, 3, :]
    return np.linalg.eigh(A.transpose(0, 2, 1) @ A)[1][:, :, 0]


def reproject(Pm, X, uv):
    h = X @ Pm[:, :3].T + Pm[:, 3]
    return np.linalg.norm(h[:, :2] / h[:, 2:] - uv, axis=1)


def triangulate_filter(P1, P2, pts1, pts2, rep_thr=20.0, z_max=0.15, method="svd"):
    """(X [n,3], err1, err2, z, keep) as onepose_triangulate defines them."""
    with np.errstate(all="ignore"):
        h = triangulate(P1, P2, pts1, pts2, method)
        X = h[:, :3] / h[:, 3:]
        e1, e2 = reproject(P1, X, pts1), reproject(P2, X, pts2)
        fin = (h[:, 3] != 0) & np.isfinite(X).all(1) & np.isfinite(e1) & np.isfinite(e2)
        keep = fin & (e1 <= rep_thr) & (e2 <= rep_thr) & (X[:, 2] <= z_max)
    return X, e1, e2, X[:, 2].copy(), keep

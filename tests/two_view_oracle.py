"""ORACLE -- test infrastructure only.  The two-view verification contract of
include/onepose_two_view.h restated in plain loops over Python floats (IEEE double, one rounding
per operation, nothing fused).  Scoring a model over a pair's matches is elementwise numpy in
float64 (the same operations per element); every sum of floats is an explicit loop in the stated
order; counting inliers is an integer count.  Shares no code with the package.

``variant`` runs a deliberately wrong rule (tests/test_two_view_model_host.py) or, with "eigh",
numpy.linalg.eigh in place of both Jacobi eigen-solves (the tolerance measurement of
tests/golden/make_golden_two_view.py).
"""
from __future__ import annotations

import math

import numpy as np

DBL_MIN = float(np.finfo(np.float64).tiny)
SQRT2 = 1.4142135623730951
SWEEPS = 24
VARIANTS = ("no_hartley", "no_rank2", "algebraic", "no_refit", "reverse_sums")
# "refits_never_stop": a refit that is not kept does not end the refits.  Retried on the unchanged
# inliers it would only repeat itself (the same list gives the same F' and the same verdict), so
# the variant is the way such a loop goes wrong in practice: the next refit runs on the inliers of
# the candidate that was not kept.  Held by the option fixtures (test_two_view_model_host.py).
OPTION_VARIANTS = ("refits_never_stop",)


class CvRng:
    """cv::RNG: multiply-with-carry, state' = (u32)state * 4164903690 + (state >> 32)."""

    def __init__(self, state=0xFFFFFFFFFFFFFFFF):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters (OpenCV 4.4, ptsetreg.cpp)."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def _div(a, b):
    """a / b in IEEE double (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 or x != x else math.nan


def jacobi_smallest(A, k, counter=None):
    """J(k) of the header on the symmetric k x k matrix A (a list of rows, overwritten): the
    eigenvector of the smallest eigenvalue."""
    V = [[1.0 if r == c else 0.0 for c in range(k)] for r in range(k)]
    fabs = math.fabs
    for sweep in range(SWEEPS):
        rotated = False
        for p in range(k - 1):
            Ap = A[p]
            for q in range(p + 1, k):
                Aq = A[q]
                apq, app, aqq = Ap[q], Ap[p], Aq[q]
                if fabs(apq) <= 1e-20 * _sqrt(fabs(app * aqq)) or apq == 0.0:
                    Ap[q] = Aq[p] = 0.0
                    continue
                rotated = True
                theta = (aqq - app) / (2.0 * apq)
                tt = (1.0 if theta >= 0.0 else -1.0) / (fabs(theta) + _sqrt(theta * theta + 1.0))
                cs = 1.0 / _sqrt(tt * tt + 1.0)
                sn = tt * cs
                for r in range(k):
                    if r == p or r == q:
                        continue
                    Ar = A[r]
                    arp, arq = Ar[p], Ar[q]
                    Ar[p] = Ap[r] = cs * arp - sn * arq
                    Ar[q] = Aq[r] = sn * arp + cs * arq
                bpp, bpq = cs * app - sn * apq, sn * app + cs * apq
                bqp, bqq = cs * apq - sn * aqq, sn * apq + cs * aqq
                Ap[p] = cs * bpp - sn * bqp
                Aq[q] = sn * bpq + cs * bqq
                Ap[q] = Aq[p] = 0.0
                for Vr in V:
                    vrp, vrq = Vr[p], Vr[q]
                    Vr[p] = cs * vrp - sn * vrq
                    Vr[q] = sn * vrp + cs * vrq
        if counter is not None:
            counter.append(sweep + 1)
        if not rotated:
            break
    bj, best = 0, A[0][0]
    for j in range(1, k):
        if A[j][j] < best:
            best, bj = A[j][j], j
    return [V[r][bj] for r in range(k)]


def _eigh_smallest(A, k):
    M = np.array(A, dtype=np.float64)
    if not np.isfinite(M).all():
        return [math.nan] * k
    w, v = np.linalg.eigh(M)
    return [float(x) for x in v[:, 0]]


def solve(P, order, variant=None, counter=None):
    """S(list): P = (x0, y0, x1, y1) as lists of Python floats, ``order`` the list of match
    indices.  Returns F as 9 floats."""
    x0, y0, x1, y1 = P
    m = float(len(order))
    sx0 = sy0 = sx1 = sy1 = 0.0
    for i in order:
        sx0 = sx0 + x0[i]
        sy0 = sy0 + y0[i]
        sx1 = sx1 + x1[i]
        sy1 = sy1 + y1[i]
    cx0, cy0, cx1, cy1 = sx0 / m, sy0 / m, sx1 / m, sy1 / m
    d0 = d1 = 0.0
    for i in order:
        dx, dy = x0[i] - cx0, y0[i] - cy0
        d0 = d0 + _sqrt(dx * dx + dy * dy)
        dx, dy = x1[i] - cx1, y1[i] - cy1
        d1 = d1 + _sqrt(dx * dx + dy * dy)
    s0, s1 = _div(SQRT2, d0 / m), _div(SQRT2, d1 / m)
    if variant == "no_hartley":
        cx0 = cy0 = cx1 = cy1 = 0.0
        s0 = s1 = 1.0
    M = [[0.0] * 9 for _ in range(9)]
    for i in order:
        u0, v0 = (x0[i] - cx0) * s0, (y0[i] - cy0) * s0
        u1, v1 = (x1[i] - cx1) * s1, (y1[i] - cy1) * s1
        a = (u1 * u0, u1 * v0, u1, v1 * u0, v1 * v0, v1, u0, v0, 1.0)
        for r in range(9):
            Mr, ar = M[r], a[r]
            for c in range(r, 9):
                Mr[c] = Mr[c] + ar * a[c]
    for r in range(9):
        for c in range(r):
            M[r][c] = M[c][r]
    f = _eigh_smallest(M, 9) if variant == "eigh" else jacobi_smallest(M, 9, counter)
    N = [f[0:3], f[3:6], f[6:9]]
    if variant != "no_rank2":
        G = [[(N[0][i] * N[0][j] + N[1][i] * N[1][j]) + N[2][i] * N[2][j] for j in range(3)]
             for i in range(3)]
        v = _eigh_smallest(G, 3) if variant == "eigh" else jacobi_smallest(G, 3)
        for i in range(3):
            w = (N[i][0] * v[0] + N[i][1] * v[1]) + N[i][2] * v[2]
            for j in range(3):
                N[i][j] = N[i][j] - w * v[j]
    A = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        A[i][0] = N[i][0] * s0
        A[i][1] = N[i][1] * s0
        A[i][2] = (N[i][2] - A[i][0] * cx0) - A[i][1] * cy0
    F = [0.0] * 9
    for j in range(3):
        F[j] = s1 * A[0][j]
        F[3 + j] = s1 * A[1][j]
        F[6 + j] = (A[2][j] - cx1 * F[j]) - cy1 * F[3 + j]
    return F


def sampson(F, Q, variant=None):
    """The squared Sampson distance of every match: Q = (x0, y0, x1, y1) float64 arrays."""
    x0, y0, x1, y1 = Q
    with np.errstate(all="ignore"):
        a0 = (F[0] * x0 + F[1] * y0) + F[2]
        a1 = (F[3] * x0 + F[4] * y0) + F[5]
        a2 = (F[6] * x0 + F[7] * y0) + F[8]
        b0 = (F[0] * x1 + F[3] * y1) + F[6]
        b1 = (F[1] * x1 + F[4] * y1) + F[7]
        e = (x1 * a0 + y1 * a1) + a2
        if variant == "algebraic":
            return e * e
        return (e * e) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)


def inliers(F, Q, thr2, variant=None):
    if not all(math.isfinite(v) for v in F):
        return np.zeros(len(Q[0]), dtype=bool)
    with np.errstate(all="ignore"):
        return sampson([np.float64(v) for v in F], Q, variant) <= thr2   # NaN: False


def verify(pts0, pts1, F_in=None, max_error=4.0, confidence=0.999, max_trials=10000,
           min_num_inliers=15, min_inlier_ratio=0.25, refine_iters=2, variant=None, counter=None):
    """One pair: pts0, pts1 [n, 2] float32 (the count already applied).  Returns a dict of
    status, F (9 float64), mask (bool [n]), n_inliers, iters."""
    pts0 = np.ascontiguousarray(pts0, np.float32).reshape(-1, 2)
    pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    n = len(pts0)
    Q = tuple(a.astype(np.float64) for a in (pts0[:, 0], pts0[:, 1], pts1[:, 0], pts1[:, 1]))
    P = tuple(a.tolist() for a in Q)
    thr2 = float(max_error) * float(max_error)
    given = F_in is not None
    Fg = [float(v) for v in np.asarray(F_in, np.float64).reshape(9)] if given else [0.0] * 9

    def result(status, F, mask, iters):
        return {"status": status, "F": np.array(F, np.float64), "mask": mask,
                "n_inliers": int(mask.sum()), "iters": iters}

    def decide(F, mask, iters):
        nin = int(mask.sum())
        bad = nin < min_num_inliers or float(nin) < min_inlier_ratio * float(n)
        return result(3 if bad else 0, F, mask, iters)
    if n < min_num_inliers:
        return result(1, Fg, np.zeros(n, bool), 0)
    if given:
        return decide(Fg, inliers(Fg, Q, thr2, variant), 0)
    rng = CvRng()
    niters = max(int(max_trials), 1)
    max_good, best, best_mask = 0, None, None
    it = 0
    while it < niters:
        sub = []
        while len(sub) < 8:
            v = rng.next() % n
            if v in sub:
                continue
            sub.append(v)
        F = solve(P, sub, variant, counter)
        mask = inliers(F, Q, thr2, variant)
        good = int(mask.sum())
        if good > max(max_good, 7):
            max_good, best, best_mask = good, F, mask
            niters = update_num_iters(confidence, (n - good) / n, 8, niters)
        it += 1
    if max_good <= 0:
        return result(2, [0.0] * 9, np.zeros(n, bool), it)
    current = best_mask   # the inliers a refit runs on: the kept model's
    for _ in range(0 if variant == "no_refit" else refine_iters):
        order = [i for i in range(n) if current[i]]
        if variant == "reverse_sums":
            order = order[::-1]
        F = solve(P, order, variant)
        mask = inliers(F, Q, thr2, variant)
        if not (all(math.isfinite(v) for v in F) and int(mask.sum()) >= int(best_mask.sum())):
            if variant == "refits_never_stop" and int(mask.sum()) >= 8:
                current = mask
                continue
            break
        best, best_mask, current = F, mask, mask
    return decide(best, best_mask, it)


def normalised(F):
    """F scaled to unit Frobenius norm with its largest-magnitude entry positive (how two F are
    compared); zeros and non-finite F are returned as they are."""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    out = F.copy()
    for k, f in enumerate(F):
        nrm = np.sqrt((f * f).sum())
        if np.isfinite(nrm) and nrm > 0:
            out[k] = f / nrm * np.sign(f[np.argmax(np.abs(f))])
    return out

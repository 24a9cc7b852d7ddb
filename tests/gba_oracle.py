"""numpy float64 oracle of global bundle adjustment (include/onepose_global_ba.h).

The header's arithmetic, restated: the tracker family's cost function with a focal length per
axis, fixed pose parameters, the Levenberg-Marquardt rules and the preconditioned CG on the
implicit Schur complement.  Every sum over observations runs in observation order
(``np.add.at`` adds its terms one after the other), the CG dot products run camera by camera, so
a permutation of the observations changes the rounding only: the spread of the results under
permutations is what the GPU tests' tolerances are made of.

``wrong``: one of WRONG, a deliberately broken variant that the tests send through the same
comparisons to see them miss the bars.
"""
import numpy as np

from ba_oracle import _bwd3, _chol3, _damp, _fwd3, _skew

INFO_HEAD, INFO_ROW = 8, 8
ST_OK, ST_FAILED, ST_BAD_INDEX, ST_CONVERGED, ST_MIN_RADIUS = 0, 1, 2, 3, 4
CG_TOL, CG_CAP, CG_INDEFINITE, CG_NONFINITE, CG_ZERO_RHS = 1, 2, 3, 4, 5
MIN_RHO, SERIES_TH2, MIN_RADIUS = 1e-3, 1e-4, 1e-32
WRONG = ("undamped", "no_wvg", "fixed_not_zeroed", "fy_by_fx")


def fixed_bits(fixed, n_cams):
    """[n_cams, 6] bool from a uint8 mask array (bit j = parameter j) or None."""
    if fixed is None:
        return np.zeros((n_cams, 6), bool)
    f = np.asarray(fixed, np.uint8).reshape(-1)
    return (f[:, None] >> np.arange(6)[None, :] & 1).astype(bool)


def linearize(points, cams, K4, xy, pt_idx, cam_idx, fixed=None, jac=True, wrong=None):
    """residuals [N,2] and, with ``jac``, Jc [N,2,6] (fixed columns zeroed), Jp [N,2,3]."""
    X = points[pt_idx]
    w, t = cams[cam_idx, :3], cams[cam_idx, 3:6]
    fx, fy, cx, cy = (K4[cam_idx, i] for i in range(4))
    th2 = (w * w).sum(1)
    pos = th2 > 0
    th = np.sqrt(np.where(pos, th2, 1.0))
    c, s = np.cos(th), np.sin(th)
    k = w / th[:, None]
    p_rod = (X * c[:, None] + np.cross(k, X) * s[:, None]
             + k * ((k * X).sum(1) * (1.0 - c))[:, None])
    wx = np.cross(w, X)
    p = np.where(pos[:, None], p_rod, X + wx) + t
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = np.stack([fx * xp + cx - xy[:, 0], fy * yp + cy - xy[:, 1]], 1)
    if not jac:
        return r
    N = len(X)
    a = np.where(pos, s / th, 1.0)
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
    f1 = fx if wrong == "fy_by_fx" else fy
    D = np.zeros((N, 2, 3))
    D[:, 0, 0] = fx * iz
    D[:, 0, 2] = -fx * xp * iz
    D[:, 1, 1] = f1 * iz
    D[:, 1, 2] = -f1 * yp * iz
    Jc = np.concatenate([D @ M, D], 2)
    Jp = D @ R
    if fixed is not None and wrong != "fixed_not_zeroed":
        Jc = np.where(fixed_bits(fixed, len(cams))[cam_idx][:, None, :], 0.0, Jc)
    return r, Jc, Jp


def cost(points, cams, K4, xy, pt_idx, cam_idx):
    r = linearize(points, cams, K4, xy, pt_idx, cam_idx, jac=False)
    return 0.5 * float((r * r).sum())


def _chol6(M):
    """Packed-order lower factors of [A,6,6] matrices, column by column; ok [A] is False where a
    pivot is not > 0."""
    A = len(M)
    C = np.zeros_like(M)
    ok = np.ones(A, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = M[:, j, j].copy()
            for k in range(j):
                d -= C[:, j, k] * C[:, j, k]
            ok &= d > 0
            C[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                v = M[:, i, j].copy()
                for k in range(j):
                    v -= C[:, i, k] * C[:, j, k]
                C[:, i, j] = v / C[:, j, j]
    return C, ok


def _solve6(C, b):
    y = np.zeros_like(b)
    x = np.zeros_like(b)
    for i in range(6):
        v = b[:, i].copy()
        for k in range(i):
            v -= C[:, i, k] * y[:, k]
        y[:, i] = v / C[:, i, i]
    for i in range(5, -1, -1):
        v = y[:, i].copy()
        for k in range(i + 1, 6):
            v -= C[:, k, i] * x[:, k]
        x[:, i] = v / C[:, i, i]
    return x


def _dot(a, b):
    """Camera by camera (each camera's six products first), then over the cameras in order."""
    total = 0.0
    for v in (a * b).sum(1):
        total += v
    return np.float64(total)


class Solver:
    """begin() at construction, step(n) afterwards: the state the header keeps in the workspace."""

    def __init__(self, points, cams, K4, xy, pt_idx, cam_idx, fixed=None, radius=1e4,
                 info_rows=64, wrong=None):
        self.points, self.cams = points.copy(), cams.copy()
        self.K4, self.xy = K4, xy
        self.pt_idx, self.cam_idx = np.asarray(pt_idx), np.asarray(cam_idx)
        self.fixed, self.wrong = fixed, wrong
        self.act_c, self.ac = np.unique(self.cam_idx, return_inverse=True)
        self.act_p, self.ap = np.unique(self.pt_idx, return_inverse=True)
        self.fix = fixed_bits(fixed, len(cams))[self.act_c]
        self.info_rows = info_rows
        self.info = np.zeros(INFO_HEAD + INFO_ROW * info_rows)
        with np.errstate(all="ignore"):
            c0 = cost(self.points, self.cams, K4, xy, self.pt_idx, self.cam_idx)
        self.info[3] = self.info[4] = c0
        self.info[5] = radius
        self.radius, self.factor, self.cost = radius, 2.0, c0
        self.iter = self.succ = 0
        self.cg_total = 0
        self.done = not np.isfinite(c0)
        if self.done:
            self.info[0] = ST_FAILED
        self.lin = None

    def _cg(self, U, C, rhs, Jc, Jp, Lv, pcg_max, pcg_tol):
        A, Pa, ac, ap = len(U), len(Lv), self.ac, self.ap

        def S(v):
            t = (Jc @ v[ac][:, :, None])                       # [N,2,1]
            s = np.zeros((Pa, 3))
            np.add.at(s, ap, (Jp.transpose(0, 2, 1) @ t)[:, :, 0])
            y = _bwd3(Lv, _fwd3(Lv, s[:, :, None]))[:, :, 0]
            t = Jp @ y[ap][:, :, None]
            acc = np.zeros((A, 6))
            np.add.at(acc, ac, (Jc.transpose(0, 2, 1) @ t)[:, :, 0])
            return (U @ v[:, :, None])[:, :, 0] - acc
        x = np.zeros((A, 6))
        res = rhs.copy()
        z = _solve6(C, res)
        p = z.copy()
        rz0 = rz = _dot(res, z)
        if not np.isfinite(rz0):
            return x, 0, CG_NONFINITE
        if rz0 == 0:
            return x, 0, CG_ZERO_RHS
        k = 0
        with np.errstate(all="ignore"):
            while True:
                Sp = S(p)
                pSp = _dot(p, Sp)
                if not np.isfinite(pSp):
                    return x, k, CG_NONFINITE
                if pSp <= 0:
                    return x, k, CG_INDEFINITE
                k += 1
                alpha = rz / pSp
                x = x + alpha * p
                res = res - alpha * Sp
                z = _solve6(C, res)
                rzn = _dot(res, z)
                beta = rzn / rz
                p = z + beta * p
                rz = rzn
                if not (np.isfinite(alpha) and np.isfinite(rzn) and np.isfinite(beta)):
                    return x, k, CG_NONFINITE
                if np.sqrt(rz / rz0) <= pcg_tol:
                    return x, k, CG_TOL
                if k >= pcg_max:
                    return x, k, CG_CAP

    def step(self, n_steps, pcg_max_iters=100, pcg_tol=1e-6, function_tolerance=1e-6):
        K4, xy, pt_idx, cam_idx, ac, ap = self.K4, self.xy, self.pt_idx, self.cam_idx, self.ac, self.ap
        A, Pa = len(self.act_c), len(self.act_p)
        i6, i3 = np.arange(6), np.arange(3)
        for _ in range(n_steps):
            if self.done:
                break
            if self.lin is None:
                self.lin = linearize(self.points, self.cams, K4, xy, pt_idx, cam_idx, self.fixed,
                                     wrong=self.wrong)
            r, Jc, Jp = self.lin
            mu = 1.0 / self.radius
            U, V = np.zeros((A, 6, 6)), np.zeros((Pa, 3, 3))
            gc, gp = np.zeros((A, 6)), np.zeros((Pa, 3))
            np.add.at(V, ap, Jp.transpose(0, 2, 1) @ Jp)
            np.add.at(gp, ap, (Jp.transpose(0, 2, 1) @ r[:, :, None])[:, :, 0])
            np.add.at(U, ac, Jc.transpose(0, 2, 1) @ Jc)
            np.add.at(gc, ac, (Jc.transpose(0, 2, 1) @ r[:, :, None])[:, :, 0])
            if self.wrong != "undamped":
                V[:, i3, i3] += _damp(V[:, i3, i3], mu)
                U[:, i6, i6] += _damp(U[:, i6, i6], mu)
            if self.wrong != "fixed_not_zeroed":
                U[:, i6, i6] = np.where(self.fix, 1.0, U[:, i6, i6])
            with np.errstate(all="ignore"):
                Lv = _chol3(V)
                ok3 = bool(np.all(V[:, 0, 0] > 0) and np.all(np.isfinite(Lv))
                           and np.all(Lv[:, i3, i3] > 0))
                zp = _fwd3(Lv, gp[:, :, None])                       # [Pa,3,1]
                W = Jc.transpose(0, 2, 1) @ Jp                       # [N,6,3]
                Y = _fwd3(Lv[ap], W.transpose(0, 2, 1))              # [N,3,6]
                m = np.zeros((A, 6, 6))
                np.add.at(m, ac, Y.transpose(0, 2, 1) @ Y)
                h = np.zeros((A, 6))
                if self.wrong != "no_wvg":
                    np.add.at(h, ac, (Y.transpose(0, 2, 1) @ zp[ap])[:, :, 0])
                C, ok6 = _chol6(U - m)
            row = np.zeros(INFO_ROW)
            row[0], row[4] = self.cost, self.radius
            accept = False
            if ok3 and bool(ok6.all()):
                rhs = -gc + h
                dc, k, reason = self._cg(U, C, rhs, Jc, Jp, Lv, pcg_max_iters, pcg_tol)
                self.cg_total += k
                with np.errstate(all="ignore"):
                    s = np.zeros((Pa, 3))
                    np.add.at(s, ap, (Jp.transpose(0, 2, 1) @ (Jc @ dc[ac][:, :, None]))[:, :, 0])
                    dp = _bwd3(Lv, _fwd3(Lv, (-gp - s)[:, :, None]))[:, :, 0]
                    cams_n, points_n = self.cams.copy(), self.points.copy()
                    cams_n[self.act_c] = np.where(self.fix, cams_n[self.act_c],
                                                  cams_n[self.act_c] + dc)
                    points_n[self.act_p] += dp
                    cand = cost(points_n, cams_n, K4, xy, pt_idx, cam_idx)
                    Jd = (Jc @ dc[ac][:, :, None] + Jp @ dp[ap][:, :, None])[:, :, 0]
                    md = -np.float64((Jd * (r + 0.5 * Jd)).sum())
                    rho = np.float64(self.cost - cand) / md
                accept = bool(np.isfinite(cand) and md > 0 and rho > MIN_RHO)
                row[1], row[2], row[3], row[6], row[7] = cand, md, rho, k, reason
            else:
                row[1] = row[2] = row[3] = np.nan
            row[5] = float(accept)
            if self.iter < self.info_rows:
                self.info[INFO_HEAD + INFO_ROW * self.iter:][:INFO_ROW] = row
            status = ST_OK
            if accept:
                old = self.cost
                self.points, self.cams, self.cost = points_n, cams_n, cand
                self.radius = min(self.radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
                self.factor = 2.0
                self.succ += 1
                self.lin = None
                if function_tolerance > 0 and abs(old - cand) / old <= function_tolerance:
                    status = ST_CONVERGED
            else:
                self.radius /= self.factor
                self.factor *= 2.0
            if status == ST_OK and self.radius < MIN_RADIUS:
                status = ST_MIN_RADIUS
            self.iter += 1
            self.done = status != ST_OK
            self.info[0], self.info[1], self.info[2] = status, self.iter, self.succ
            self.info[4], self.info[5], self.info[6] = self.cost, self.radius, self.cg_total
        return self.points, self.cams, self.info


def solve(points, cams, K4, xy, pt_idx, cam_idx, fixed=None, max_iters=50, radius=1e4,
          pcg_max_iters=100, pcg_tol=1e-6, function_tolerance=1e-6, info_rows=None, wrong=None):
    """(points, cams, info) after up to ``max_iters`` outer iterations.  Inputs are not modified."""
    s = Solver(points, cams, K4, xy, pt_idx, cam_idx, fixed, radius,
               max_iters if info_rows is None else info_rows, wrong)
    return s.step(max_iters, pcg_max_iters, pcg_tol, function_tolerance)


def rows(info):
    n = min(int(info[1]), (len(info) - INFO_HEAD) // INFO_ROW)
    return info[INFO_HEAD:INFO_HEAD + INFO_ROW * n].reshape(n, INFO_ROW)


def significant(info, rel=1e-6):
    """Iterations whose model decrease exceeds ``rel`` x cost, and whose predecessors all do: only
    there are rho, the radius and the decision more than rounding noise."""
    rw = rows(info)
    with np.errstate(invalid="ignore"):
        sig = rw[:, 2] > rel * rw[:, 0]
    return np.logical_and.accumulate(sig)


def dense_step(points, cams, K4, xy, pt_idx, cam_idx, fixed=None, radius=1e4):
    """The first step by a dense solve of the damped normal equations (numpy.linalg.solve), with
    the header's treatment of fixed parameters: (dc [A,6], dp [Pa,3])."""
    r, Jc, Jp = linearize(points, cams, K4, xy, pt_idx, cam_idx, fixed)
    act_c, ac = np.unique(cam_idx, return_inverse=True)
    act_p, ap = np.unique(pt_idx, return_inverse=True)
    N, A, Pa = len(ac), len(act_c), len(act_p)
    J = np.zeros((2 * N, 6 * A + 3 * Pa))
    for n in range(N):
        J[2 * n:2 * n + 2, 6 * ac[n]:6 * ac[n] + 6] = Jc[n]
        J[2 * n:2 * n + 2, 6 * A + 3 * ap[n]:6 * A + 3 * ap[n] + 3] = Jp[n]
    H = J.T @ J
    d = np.diag(H).copy()
    d += _damp(d, 1.0 / radius)
    fix = np.concatenate([fixed_bits(fixed, len(cams))[act_c].reshape(-1), np.zeros(3 * Pa, bool)])
    d[fix] = 1.0
    H[np.diag_indices_from(H)] = d
    delta = np.linalg.solve(H, -(J.T @ r.reshape(-1)))
    return delta[:6 * A].reshape(A, 6), delta[6 * A:].reshape(Pa, 3)

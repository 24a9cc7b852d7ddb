"""The solver against two things that are not its restatement: a dense damped Gauss-Newton step
solved at 50 digits, and the minimum that scipy's trust-region solver finds.

    python tests/golden/make_golden_ba_dense.py      (needs mpmath and scipy; nothing else outside
                                                      the tree)

``ba_dense.npz``.  Inputs are not stored: each problem's SHA-256 is, and the tests rebuild the
problems from tests/ba_cases.py (STEP_CASES, MIN_CASES).

(a) The step.  Per problem of STEP_CASES the dense J [2N, 6A + 3Pa] (idle columns removed,
cameras first) and r come from ba_oracle.linearize at the initial variables; their float64 entries
are taken as exact.  mpmath at 50 digits forms J^T J and J^T r, adds mu * clamp(diag, 1e-6, 1e32)
with mu = 1 / 1e4 to the diagonal and solves for the step by Cholesky: no Schur complement, no
whitening, no back-substitution.  Recorded: ``delta`` (float64 of the 50-digit step), ``md`` =
-(J d).(r + J d / 2) and ``cand``, the cost at variables + delta (ba_oracle.cost); and the same
three from ``numpy.linalg.solve`` on the float64 normal equations (``delta64``, ``md64``,
``cand64``).  ``tol`` = 16 x the deviation of the float64 dense solve from the 50-digit one, floor
1e-12: (max|d delta| absolute, md relative, cand relative).  What forming J^T J in float64 costs
is what a correct float64 solver may cost too; the Schur path of the solver is a different
elimination order of the same system.

(b) The minimum.  Per problem of MIN_CASES ``opt`` is the cost at which
``scipy.optimize.least_squares`` (trf, exact Jacobian, ftol = xtol = gtol = 1e-15) stops when
started at the problem's variables.  Seeds are tried from the case's base: one is taken when the
oracle's own runs under 8 permutations of the observations and through its variant routines end
within 4 x of its plain run's gap and gradient norm (after convergence every further step is a
coin toss of rounding; a problem where the oracle itself ends a step apart cannot hold anyone
else to 16 x).  ``oracle_cost`` and ``oracle_grad`` are the numpy oracle's
final cost after 16 iterations (max_success 16, radius 1e4) and |J^T r|_inf at its result.
``gap_bar`` = max(16 x |oracle_cost - opt| / opt, 1e-9) -- the floor is the bar info[4] already
has against its host re-evaluation -- and ``grad_bar`` = 16 x oracle_grad.
"""
import os
import sys

import mpmath as mp
import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ba_cases  # noqa: E402
import ba_oracle as O  # noqa: E402

mp.mp.dps = 50
FACTOR, FLOOR = 16.0, 1e-12
KEYS = ("features", "ptIdx", "camIdx")


def lin(prob, pts=None, cams=None):
    return O.linearize(prob["points"] if pts is None else pts,
                       prob["cam_pose"] if cams is None else cams, *[prob[k] for k in KEYS])


def mp_step(J, r, mu):
    """The damped Gauss-Newton step of the dense system at mp.dps digits."""
    m, n = J.shape
    Hm = np.full((n, n), mp.mpf(0), dtype=object)
    g = np.full(n, mp.mpf(0), dtype=object)
    Jm = np.array([[mp.mpf(float(v)) for v in row] for row in J], dtype=object)
    rm = np.array([mp.mpf(float(v)) for v in r], dtype=object)
    for k in range(m):                      # nine non-zeros per row
        nz = np.nonzero(J[k])[0]
        Hm[np.ix_(nz, nz)] += np.outer(Jm[k, nz], Jm[k, nz])
        g[nz] += Jm[k, nz] * rm[k]
    for i in range(n):
        d = min(max(Hm[i, i], mp.mpf("1e-6")), mp.mpf("1e32"))
        Hm[i, i] += mp.mpf(mu) * d
    L = np.full((n, n), mp.mpf(0), dtype=object)
    for k in range(n):
        L[k, k] = mp.sqrt(Hm[k, k] - np.dot(L[k, :k], L[k, :k]))
        if k + 1 < n:
            L[k + 1:, k] = (Hm[k + 1:, k] - np.dot(L[k + 1:, :k], L[k, :k])) / L[k, k]
    y = np.full(n, mp.mpf(0), dtype=object)
    for k in range(n):
        y[k] = (-g[k] - np.dot(L[k, :k], y[:k])) / L[k, k]
    d = np.full(n, mp.mpf(0), dtype=object)
    for k in range(n - 1, -1, -1):
        d[k] = (y[k] - np.dot(L[k + 1:, k], d[k + 1:])) / L[k, k]
    Jd = np.dot(Jm, d)
    md = -np.dot(Jd, rm + Jd / 2)
    return np.array([float(v) for v in d]), float(md)


def make_steps(out):
    mu = 1.0 / ba_cases.STEP_RADIUS
    for name, build in ba_cases.STEP_CASES.items():
        prob = build()
        r, Jc, Jp = lin(prob)
        J, rv, _, _ = ba_cases.dense_system(prob, r, Jc, Jp)
        delta, md = mp_step(J, rv, mu)
        H = J.T @ J
        H[np.diag_indices_from(H)] += mu * np.clip(np.diag(H), 1e-6, 1e32)
        d64 = np.linalg.solve(H, -J.T @ rv)
        Jd = J @ d64
        md64 = float(-(Jd * (rv + 0.5 * Jd)).sum())
        cand = O.cost(*ba_cases.apply_step(prob, delta), *[prob[k] for k in KEYS])
        cand64 = O.cost(*ba_cases.apply_step(prob, d64), *[prob[k] for k in KEYS])
        dev = np.array([np.abs(d64 - delta).max(), abs(md64 / md - 1), abs(cand64 / cand - 1)])
        tol = np.maximum(FACTOR * dev, FLOOR)
        cost0 = 0.5 * float((r * r).sum())
        print(f"step {name}: {J.shape[1]} unknowns, N {len(r)}, cost {cost0:.4g} -> {cand:.4g}, md "
              f"{md:.4g}, |delta| {np.abs(delta).max():.2e}; float64 dense deviates "
              + " ".join(f"{v:.1e}" for v in dev) + "; tol " + " ".join(f"{v:.1e}" for v in tol))
        assert cand < cost0 and md > 0
        out.update({f"{name}_sha": ba_cases.problem_sha(prob), f"{name}_delta": delta,
                    f"{name}_md": md, f"{name}_cand": cand, f"{name}_cost0": cost0,
                    f"{name}_delta64": d64, f"{name}_md64": md64, f"{name}_cand64": cand64,
                    f"{name}_tol": tol})


def grad_norm(prob, pts, cams):
    r, Jc, Jp = lin(prob, pts, cams)
    J, rv, _, _ = ba_cases.dense_system(prob, r, Jc, Jp)
    return float(np.abs(J.T @ rv).max())


def minimum_of(prob):
    C, P = len(prob["cam_pose"]), len(prob["points"])
    assert len(np.unique(prob["camIdx"])) == C and len(np.unique(prob["ptIdx"])) == P
    unpack = lambda x: (x[6 * C:].reshape(P, 3), x[:6 * C].reshape(C, 6))

    def fun(x):
        pts, cams = unpack(x)
        return O.linearize(pts, cams, *[prob[k] for k in KEYS], jac=False).ravel()

    def jac(x):
        pts, cams = unpack(x)
        return ba_cases.dense_system(prob, *lin(prob, pts, cams))[0]

    x0 = np.concatenate([prob["cam_pose"].ravel(), prob["points"].ravel()])
    res = least_squares(fun, x0, jac=jac, method="trf", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                        max_nfev=2000)
    return float(res.cost), res


def oracle_end(prob, opt, perm=None, variant=False):
    """(relative gap to opt, |J^T r|_inf, info) of the oracle's 16 iterations."""
    f, p, c = [prob[k] for k in KEYS]
    if perm is not None:
        f, p, c = f[perm], p[perm], c[perm]
    pts, cams, info = O.solve(prob["points"], prob["cam_pose"], f, p, c, 16, 16, 1e4,
                              variant=variant)
    return abs(info[4] - opt) / opt, grad_norm(prob, pts, cams), info


def make_minima(out):
    for name, (build, base) in ba_cases.MIN_CASES.items():
        for seed in range(base, base + ba_cases.MAX_SEEDS):
            prob = build(seed)
            opt, res = minimum_of(prob)
            gap, grad, info = oracle_end(prob, opt)
            rs = np.random.RandomState(seed + 7)
            others = [oracle_end(prob, opt, rs.permutation(len(prob["ptIdx"])))[:2]
                      for _ in range(8)] + [oracle_end(prob, opt, variant=True)[:2]]
            wg, wr = max(o[0] for o in others), max(o[1] for o in others)
            note = (f"scipy {opt:.17g} ({res.nfev} evaluations, status {res.status}), oracle "
                    f"{info[4]:.17g} (gap {(info[4] - opt) / opt:.1e}, accepted {int(info[2])} of "
                    f"16), |J^T r| {grad:.1e}; its permuted and variant runs: gap <= {wg:.1e}, "
                    f"|J^T r| <= {wr:.1e}")
            if wr > 4 * grad or wg > 4 * max(gap, 1e-9 / FACTOR) or info[1] != 16:
                print(f"minimum {name}: seed {seed} rejected: {note}")
                continue
            print(f"minimum {name}: seed {seed}, {note}")
            break
        else:
            raise AssertionError(f"{name}: no seed fits")
        out.update({f"{name}_seed": seed, f"{name}_sha": ba_cases.problem_sha(prob),
                    f"{name}_opt": opt, f"{name}_oracle_cost": info[4],
                    f"{name}_oracle_grad": grad, f"{name}_gap_bar": max(FACTOR * gap, 1e-9),
                    f"{name}_grad_bar": FACTOR * grad})


def main():
    out = {}
    make_steps(out)
    make_minima(out)
    np.savez_compressed(os.path.join(HERE, "ba_dense.npz"), **out)


if __name__ == "__main__":
    main()

"""The cost function against a many-digit model at the angles and depths where float64 strains.

    python tests/golden/make_golden_ba_edges.py        (needs mpmath; nothing else outside the tree)

``ba_edges.npz`` holds, for the grid of tests/ba_cases.py::edge_grid (19 angles x 4 axes x 4
geometries x 2 focal lengths = 608 observations, one linearize call, three workgroups), the seed
and SHA-256 of the inputs (the tests regenerate them) and, per observation, the model's residual
``r`` [N,2] and Jacobians ``Jc`` [N,2,6], ``Jp`` [N,2,3] rounded to float64.

The model is the residual of include/onepose_hip.h in mpmath at 800 digits (theta = 1e-160 needs
1 - cos(theta) = 5e-321 to keep digits; 50 would do from 1e-12 up).  It takes the rotation branch
by the FLOAT64 value of theta^2, as the kernel must: Rodrigues' formula where that is > 0, else
X + aa x X.  The Jacobian is the derivative of that exact expression, taken by central
differences with h = 1e-200 at those 800 digits (the rotation is analytic in aa: truncation
1e-400, rounding 1e-600), so it shares no algebra with the closed form in ba_oracle.py and
ba.hip.  At theta^2 == 0 it is -[X]x, as the header states.

Recorded with it is the numpy oracle's own deviation from the model (``dev_r`` px, ``dev_Jc``,
``dev_Jp`` relative to each observation's max|J|) and the bars made of it, per ANGLE (per entry a
lucky rounding would make a bar zero):

* ``bar_Jc``, ``bar_Jp`` [19] = 16 x the oracle's largest relative deviation among the angle's 32
  observations, floor 1e-14;
* ``bar_r`` [19] = 16 x the oracle's largest |dr| there; the tests raise it per observation to 64
  float64 ulps of ``rmag`` = |f x / z| + |c| + |u| (the larger of the two rows), the residual's
  largest intermediate;
* ``cost`` = 1/2 sum r^2 of the model.

16 is the factor every bar of this family has over its reference's own spread: the kernel's sin
and cos differ from libm's by an ulp, which the cancelling subtractions in (1 - cos) / theta^2,
(cos - a) / theta^2 and (a - 2 b) / theta^2 amplify near theta = 1e-8.
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

mp.mp.dps = 800
H = mp.mpf(10) ** -200
FACTOR, FLOOR_J = 16.0, 1e-14


def project(w, t, X, ft, rodrigues):
    """The header's residual, exactly; w, t, X lists of mpf."""
    cross = [w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]]
    if rodrigues:
        th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        if th2 == 0:
            a, b, c = mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1)
        else:
            th = mp.sqrt(th2)
            c = mp.cos(th)
            a, b = mp.sin(th) / th, (1 - c) / th2
        wd = w[0] * X[0] + w[1] * X[1] + w[2] * X[2]
        p = [c * X[i] + a * cross[i] + b * wd * w[i] + t[i] for i in range(3)]
    else:
        p = [X[i] + cross[i] + t[i] for i in range(3)]
    u, v, f, cx, cy = ft
    return [f * p[0] / p[2] + cx - u, f * p[1] / p[2] + cy - v], (abs(f * p[0] / p[2]),
                                                                  abs(f * p[1] / p[2]))


def model(prob):
    N = len(prob["ptIdx"])
    r, Jc, Jp, rmag = np.zeros((N, 2)), np.zeros((N, 2, 6)), np.zeros((N, 2, 3)), np.zeros(N)
    for n in range(N):
        cam = prob["cam_pose"][prob["camIdx"][n]]
        X0 = prob["points"][prob["ptIdx"][n]]
        ft = [mp.mpf(float(v)) for v in prob["features"][n]]
        th2_f64 = float((cam[:3] * cam[:3]).sum())          # the branch the kernel must take
        rod = th2_f64 > 0.0
        var = [mp.mpf(float(v)) for v in np.concatenate([cam, X0])]

        def res(v):
            return project(v[:3], v[3:6], v[6:9], ft, rod)[0]

        r0, mag = project(var[:3], var[3:6], var[6:9], ft, rod)
        r[n] = [float(r0[0]), float(r0[1])]
        rmag[n] = max(float(mag[0]) + abs(float(ft[3])) + abs(float(ft[0])),
                      float(mag[1]) + abs(float(ft[4])) + abs(float(ft[1])))
        for k in range(9):
            hi, lo = list(var), list(var)
            hi[k], lo[k] = var[k] + H, var[k] - H
            rh, rl = res(hi), res(lo)
            d = [float((rh[i] - rl[i]) / (2 * H)) for i in range(2)]
            if k < 6:
                Jc[n, :, k] = d
            else:
                Jp[n, :, k - 6] = d
    return r, Jc, Jp, rmag


def main():
    prob, ang = ba_cases.edge_grid()
    r, Jc, Jp, rmag = model(prob)
    g = {"r": r, "Jc": Jc, "Jp": Jp}
    ro, Jco, Jpo = O.linearize(prob["points"], prob["cam_pose"], prob["features"], prob["ptIdx"],
                               prob["camIdx"])
    dr, dJc, dJp = ba_cases.edge_deviations(ro, Jco, Jpo, g)
    nA = len(ba_cases.EDGE_ANGLES)
    worst = lambda d: np.array([d[ang == ia].max() for ia in range(nA)])
    bar_r = FACTOR * worst(dr)
    bar_Jc = np.maximum(FACTOR * worst(dJc), FLOOR_J)
    bar_Jp = np.maximum(FACTOR * worst(dJp), FLOOR_J)
    for ia, th in enumerate(ba_cases.EDGE_ANGLES):
        print(f"theta {th:.17g}: oracle |dr| {worst(dr)[ia]:.1e} px, |dJc| {worst(dJc)[ia]:.1e}, "
              f"|dJp| {worst(dJp)[ia]:.1e} (of max|J|)")
    assert max(dJc.max(), dJp.max()) < 1e-6, "the float64 formula needs its series"
    assert np.isfinite(r).all() and np.isfinite(Jc).all() and np.isfinite(Jp).all()
    np.savez_compressed(os.path.join(HERE, "ba_edges.npz"), seed=ba_cases.EDGE_SEED,
                        sha=ba_cases.problem_sha(prob), r=r, Jc=Jc, Jp=Jp, rmag=rmag, dev_r=dr,
                        dev_Jc=dJc, dev_Jp=dJp, bar_r=bar_r, bar_Jc=bar_Jc, bar_Jp=bar_Jp,
                        cost=0.5 * float((r * r).sum()))


if __name__ == "__main__":
    main()

"""The global bundle adjustment cost function (fx != fy) against a many-digit model.

    python tests/golden/make_golden_gba_edges.py        (needs mpmath)

``gba_edges.npz`` holds, for tests/gba_cases.py::edge_problem (9 angles x 4 axes x 4 geometries,
theta = 0, theta^2 below and at 1e-4 and a point behind the camera among them), the SHA-256 of the
inputs and the model's residual and Jacobians rounded to float64, with the bars of
make_golden_ba_edges.py: per angle 16 x the numpy oracle's own largest deviation from the model,
floor 1e-14 for the Jacobians (relative to the observation's max|J|); the residual's bar is raised
by the tests to 64 ulps of ``rmag``, the observation's largest intermediate.

The model is the residual of include/onepose_global_ba.h in mpmath at 800 digits, the rotation
branch taken by the FLOAT64 value of theta^2 as the kernel must, its Jacobian by central
differences with h = 1e-200: it shares no algebra with gba_oracle.py or global_ba.hip.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import gba_cases as G  # noqa: E402
import gba_oracle as O  # noqa: E402

mp.mp.dps = 800
H = mp.mpf(10) ** -200
FACTOR, FLOOR_J = 16.0, 1e-14


def project(w, t, X, k4, uv, rodrigues):
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
    fx, fy, cx, cy = k4
    return ([fx * p[0] / p[2] + cx - uv[0], fy * p[1] / p[2] + cy - uv[1]],
            (abs(fx * p[0] / p[2]), abs(fy * p[1] / p[2])))


def model(prob):
    N = len(prob["ptIdx"])
    r, Jc, Jp, rmag = np.zeros((N, 2)), np.zeros((N, 2, 6)), np.zeros((N, 2, 3)), np.zeros(N)
    for n in range(N):
        cam, X0 = prob["cam_pose"][n], prob["points"][n]
        k4 = [mp.mpf(float(v)) for v in prob["K4"][n]]
        uv = [mp.mpf(float(v)) for v in prob["xy"][n]]
        rod = float((cam[:3] * cam[:3]).sum()) > 0.0
        var = [mp.mpf(float(v)) for v in np.concatenate([cam, X0])]

        def res(v):
            return project(v[:3], v[3:6], v[6:9], k4, uv, rod)[0]

        r0, mag = project(var[:3], var[3:6], var[6:9], k4, uv, rod)
        r[n] = [float(r0[0]), float(r0[1])]
        rmag[n] = max(float(mag[0]) + abs(float(k4[2])) + abs(float(uv[0])),
                      float(mag[1]) + abs(float(k4[3])) + abs(float(uv[1])))
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
    prob, ang = G.edge_problem()
    r, Jc, Jp, rmag = model(prob)
    ro, Jco, Jpo = O.linearize(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"],
                               prob["ptIdx"], prob["camIdx"])
    dr = np.abs(ro - r).max(1)
    dJc = np.abs(Jco - Jc).max((1, 2)) / np.abs(Jc).max((1, 2))
    dJp = np.abs(Jpo - Jp).max((1, 2)) / np.abs(Jp).max((1, 2))
    worst = lambda d: np.array([d[ang == ia].max() for ia in G.EDGE_ANGLE_IDS])
    for k, ia in enumerate(G.EDGE_ANGLE_IDS):
        print(f"angle id {ia}: oracle |dr| {worst(dr)[k]:.1e} px, |dJc| {worst(dJc)[k]:.1e}, "
              f"|dJp| {worst(dJp)[k]:.1e} (of max|J|)")
    assert max(dJc.max(), dJp.max()) < 1e-6
    assert np.isfinite(r).all() and np.isfinite(Jc).all() and np.isfinite(Jp).all()
    np.savez_compressed(os.path.join(HERE, "gba_edges.npz"), sha=G.problem_sha(prob), edge_r=r,
                        edge_Jc=Jc, edge_Jp=Jp, edge_rmag=rmag, edge_bar_r=FACTOR * worst(dr),
                        edge_bar_Jc=np.maximum(FACTOR * worst(dJc), FLOOR_J),
                        edge_bar_Jp=np.maximum(FACTOR * worst(dJp), FLOOR_J))


if __name__ == "__main__":
    main()

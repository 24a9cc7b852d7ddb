"""Records tests/golden/gba.npz: per case of tests/gba_cases.py the oracle's result (numpy
float64, tests/gba_oracle.py) and the tolerances by the project's rule -- 16 x the largest
deviation among oracle runs under 8 permutations of the observations, floor 1e-12 -- for the
variables (absolute), the costs (of the initial cost) and, over the significant iterations, the
model decrease (relative), rho (absolute) and the radius (relative); the range of CG iteration
counts per outer iteration over those runs; and for the dense case the first step's deviation
from numpy.linalg.solve on the damped normal equations; and the noisy scene's minimum by
scipy.optimize.least_squares with the oracle's deviation from it.

    python tests/golden/make_golden_gba.py        # needs scipy
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gba_cases as G      # noqa: E402
import gba_oracle as O     # noqa: E402


def main():
    out = {}
    for name, (_, opts) in G.CASES.items():
        prob = G.problem(name)
        pts, cams, info = G.oracle_solve(prob, opts)
        exp = {"points": pts, "cam_pose": cams, "info": info}
        N = len(prob["ptIdx"])
        dev = np.zeros(5)
        cg = [O.rows(info)[:, 6]]
        for k in range(G.N_PERM):
            perm = np.random.default_rng(9000 + k).permutation(N)
            p2, c2, i2 = G.oracle_solve(prob, opts, perm)
            assert i2[0] == info[0], (name, "permuted runs end differently")
            dev = np.maximum(dev, G.deviations(p2, c2, i2, exp))
            if name in G.FREE_RUN:   # past convergence the decisions are rounding: no row pairing
                continue
            assert i2[1] == info[1], (name, "permuted runs end differently")
            cg.append(O.rows(i2)[:, 6])
        tol = np.maximum(16 * dev, 1e-12)
        cg = np.stack(cg)
        out.update({f"{name}_sha": G.problem_sha(prob), f"{name}_points": pts,
                    f"{name}_cam_pose": cams, f"{name}_info": info, f"{name}_tol": tol,
                    f"{name}_cg_lo": cg.min(0), f"{name}_cg_hi": cg.max(0)})
        rw = O.rows(info)
        print(f"{name}: N {N} status {int(info[0])} iters {int(info[1])} accepted {int(info[2])} "
              f"cost {info[3]:.4g} -> {info[4]:.6g} cg {rw[:, 6].astype(int).tolist()} "
              f"reasons {rw[:, 7].astype(int).tolist()} tol {np.array2string(tol, precision=1)}")
        if name in ("clean", "noisy"):
            at_truth = O.cost(prob["true_points"], prob["true_cams"], prob["K4"], prob["xy"],
                              prob["ptIdx"], prob["camIdx"])
            err = max(np.abs(pts - prob["true_points"]).max(),
                      np.abs(cams - prob["true_cams"]).max())
            print(f"  cost at the truth {at_truth:.6g}, distance from the truth {err:.3g}")
    # the first step against the dense solve
    prob = G.problem(G.DENSE_CASE)
    pts, cams, info = G.oracle_solve(prob, G.DENSE_OPTS)
    dc, dp = O.dense_step(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"], prob["ptIdx"],
                          prob["camIdx"], prob["fixed"], G.DENSE_OPTS["radius"])
    act_c, act_p = np.unique(prob["camIdx"]), np.unique(prob["ptIdx"])
    dense = np.concatenate([dc.ravel(), dp.ravel()])
    got = np.concatenate([(cams - prob["cam_pose"])[act_c].ravel(),
                          (pts - prob["points"])[act_p].ravel()])
    assert info[2] == 1, "the dense case's first step must be accepted"
    dev = np.abs(got - dense).max() / np.abs(dense).max()
    out.update({"dense_step": dense, "dense_tol": max(16 * dev, 1e-12)})
    print(f"dense: oracle-vs-dense deviation {dev:.3g} (relative to the largest entry)")
    # the noisy scene's minimum by scipy.optimize.least_squares (dense analytic Jacobian over the
    # free parameters), started from the oracle's start
    from scipy.optimize import least_squares
    prob = G.problem("noisy")
    act_c, act_p = np.unique(prob["camIdx"]), np.unique(prob["ptIdx"])
    free = ~O.fixed_bits(prob["fixed"], len(prob["cam_pose"]))[act_c].reshape(-1)
    nc = int(free.sum())

    def unpack(v):
        cams, pts = prob["cam_pose"].copy(), prob["points"].copy()
        c = cams[act_c].reshape(-1)
        c[free] = v[:nc]
        cams[act_c] = c.reshape(-1, 6)
        pts[act_p] = v[nc:].reshape(-1, 3)
        return pts, cams

    def fun(v):
        pts, cams = unpack(v)
        return O.linearize(pts, cams, prob["K4"], prob["xy"], prob["ptIdx"], prob["camIdx"],
                           jac=False).reshape(-1)

    def jac(v):
        pts, cams = unpack(v)
        _, Jc, Jp = O.linearize(pts, cams, prob["K4"], prob["xy"], prob["ptIdx"], prob["camIdx"])
        ac = np.searchsorted(act_c, prob["camIdx"])
        ap = np.searchsorted(act_p, prob["ptIdx"])
        J = np.zeros((2 * len(ac), 6 * len(act_c) + 3 * len(act_p)))
        for n in range(len(ac)):
            J[2 * n:2 * n + 2, 6 * ac[n]:6 * ac[n] + 6] = Jc[n]
            J[2 * n:2 * n + 2, 6 * len(act_c) + 3 * ap[n]:][:, :3] = Jp[n]
        return J[:, np.concatenate([free, np.ones(3 * len(act_p), bool)])]

    v0 = np.concatenate([prob["cam_pose"][act_c].reshape(-1)[free], prob["points"][act_p].ravel()])
    sol = least_squares(fun, v0, jac=jac, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                        max_nfev=200)
    dev = abs(out["noisy_info"][4] - sol.cost) / sol.cost
    out.update({"noisy_scipy_cost": sol.cost, "noisy_scipy_tol": max(16 * dev, 1e-12)})
    print(f"scipy: cost {sol.cost:.12g} ({sol.nfev} evaluations, status {sol.status}), oracle "
          f"{out['noisy_info'][4]:.12g}, relative deviation {dev:.3g}")
    np.savez_compressed(os.path.join(HERE, "gba.npz"), **out)


if __name__ == "__main__":
    main()

"""Solver paths that ba_solve.npz does not reach, recorded from the numpy oracle.

    python tests/golden/make_golden_ba_solve_edges.py      (numpy only)

``ba_solve_edges.npz`` holds, per case of tests/ba_cases.py::SOLVE_EDGE_CASES, what
make_golden_ba.py records per case of SOLVE_CASES, by the same rules: the oracle's result
(points, cam_pose, info), the seed and SHA-256 of the inputs, and ``tol`` = 16 x the largest
deviation among oracle runs under 8 permutations of the observations (variables) and those plus
the variant routines (costs, model decrease, rho, radius), floor 1e-12.  The iteration limits
are the case's own.  Seeds are tried from the case's base, at most 40; one is taken when every
significant iteration (model decrease > 1e-6 x cost, and all before it) has |rho - 1e-3| >= 0.05,
no permutation changes a significant decision, the permutation spread of the variables is
<= 1e-6, the cost decreases, and the case's own condition holds:

* ``reject_run``: two or more consecutive significant rejections (the radius divided by 2, then
  4), followed by a significant acceptance;
* ``chol_fail``: J^T J overflows, every iteration's Cholesky fails: status 0, nothing accepted,
  rows (cost, NaN, NaN, NaN, radius, 0), radii 1e4, 5e3, 1250, 156.25, 9.765625, nothing moved
  (this case is exempt from "the cost decreases");
* ``radius_cap_1e16``: the first accepted step leaves the radius at exactly 1e16 (the image is
  scaled by 1e-14, see ba_cases._scaled_problem: with ordinary pixels the damping at that
  radius is below the rounding of S and its Cholesky a coin toss, in the oracle too: 23 of 80
  permuted runs failed it here.  Radius 1e300 has no trajectory to record for that reason; the
  tests hold the solver's bookkeeping there);
* ``one_iter`` / ``one_success``: one iteration / one acceptance and then the stop;
* ``lane_counts``: six cameras with exactly 1, 63, 64, 65, 128, 129 observations;
* ``a2`` .. ``a23``: the active-camera counts; ``behind``: a point behind one of its cameras.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import ba_cases  # noqa: E402
import ba_oracle as O  # noqa: E402

N_PERM, FACTOR, FLOOR = 8, 16.0, 1e-12
RHO_MARGIN, MAX_SPREAD = 0.05, 1e-6


def rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return float(np.nanmax(d)) if d.size else 0.0


def own_condition(name, prob, info):
    rw, sig = O.rows(info), O.significant(info)
    acc = rw[:, 5].astype(int)
    if name == "reject_run":
        for i in range(len(acc) - 2):
            first = i == 0 or acc[i - 1] == 1          # the run starts here: factor is 2
            if (first and sig[i + 2] and acc[i] == 0 and acc[i + 1] == 0
                    and 1 in acc[i + 2:][sig[i + 2:]]):
                return rw[i + 1, 4] == rw[i, 4] / 2 and rw[i + 2, 4] == rw[i + 1, 4] / 4
        return False
    if name == "chol_fail":
        radii = [1e4, 5e3, 1250.0, 156.25, 9.765625]
        return (info[0] == 0 and info[1] == 5 and info[2] == 0 and np.isnan(rw[:, 1:4]).all()
                and rw[:, 4].tolist() == radii and info[5] == 0.30517578125
                and (rw[:, 0] == info[3]).all() and np.isfinite(info[3]))
    if name.startswith("radius_cap"):
        first = int(np.argmax(acc))
        after = rw[first + 1, 4] if first + 1 < len(rw) else info[5]
        return bool(acc[first] == 1 and sig[first] and after == 1e16)
    if name == "one_iter":
        return info[1] == 1 and info[2] == 1
    if name == "one_success":
        return info[1] == 1 and info[2] == 1
    if name == "lane_counts":
        return np.bincount(prob["camIdx"]).tolist() == [1, 63, 64, 65, 128, 129]
    if name == "behind":
        r = O.linearize(prob["points"], prob["cam_pose"], prob["features"], prob["ptIdx"],
                        prob["camIdx"], jac=False)
        X = prob["points"][prob["ptIdx"]]
        cam = prob["cam_pose"][prob["camIdx"]]
        z = np.array([(ba_cases.synthetic._rodrigues_np(c[:3]) @ x + c[3:])[2]
                      for c, x in zip(cam, X)])
        return bool(np.isfinite(r).all() and (z < -0.25).sum() == 1)
    return len(np.unique(prob["camIdx"])) == int(name[1:])


def try_seed(name, seed):
    build, radius, iters, succ, _ = ba_cases.SOLVE_EDGE_CASES[name]
    prob = build(seed)

    def run(perm=None, variant=False):
        f, p, c = prob["features"], prob["ptIdx"], prob["camIdx"]
        if perm is not None:
            f, p, c = f[perm], p[perm], c[perm]
        with np.errstate(all="ignore"):
            return O.solve(prob["points"], prob["cam_pose"], f, p, c, iters, succ, radius,
                           variant=variant)

    pts, cams, info = run()
    rw, sig = O.rows(info), O.significant(info)
    if name != "chol_fail" and (info[0] != 0 or not info[4] < info[3]):
        return None, "no decrease"
    if np.any(np.abs(rw[sig, 3] - O.MIN_RHO) < RHO_MARGIN):
        return None, "rho near the threshold"
    if not own_condition(name, prob, info):
        return None, "the case's own condition fails"
    rs = np.random.RandomState(seed + 7)
    dv = dc = dm = dr = dR = 0.0
    for k in range(N_PERM + 1):
        p2, c2, i2 = run(rs.permutation(len(prob["ptIdx"]))) if k < N_PERM else run(variant=True)
        r2 = O.rows(i2)
        if i2[1] != info[1] or not np.array_equal(r2[sig, 5], rw[sig, 5]):
            return None, "a permutation changes a significant decision"
        if k < N_PERM:
            dv = max(dv, np.abs(p2 - pts).max(), np.abs(c2 - cams).max())
        dc = max(dc, O.cost_deviation(i2, info))
        dm = max(dm, rel(r2[sig, 2], rw[sig, 2]))
        dr = max(dr, float(np.abs(r2[sig, 3] - rw[sig, 3]).max()) if sig.any() else 0.0)
        dR = max(dR, rel(r2[sig, 4], rw[sig, 4]))
    if dv > MAX_SPREAD:
        return None, f"spread {dv:.1e}"
    tol = np.maximum(FACTOR * np.array([dv, dc, dm, dr, dR]), FLOOR)
    out = {f"{name}_seed": seed, f"{name}_sha": ba_cases.problem_sha(prob),
           f"{name}_points": pts, f"{name}_cam_pose": cams, f"{name}_info": info,
           f"{name}_tol": tol}
    note = (f"cost {info[3]:.4g} -> {info[4]:.4g}, accepted {rw[:, 5].astype(int).tolist()}, "
            f"significant {sig.astype(int).tolist()}, radii "
            + " ".join(f"{v:.3g}" for v in rw[:, 4]) + f" -> {info[5]:.3g}, spread {dv:.1e}, tol "
            + " ".join(f"{t:.1e}" for t in tol))
    return out, note


def main():
    out = {}
    for name, case in ba_cases.SOLVE_EDGE_CASES.items():
        base = case[4]
        for seed in range(base, base + ba_cases.MAX_SEEDS):
            got, note = try_seed(name, seed)
            if got is None:
                print(f"{name}: seed {seed} rejected: {note}")
                continue
            print(f"{name}: seed {seed}, {note}")
            out.update(got)
            break
        else:
            raise AssertionError(f"{name}: none of {ba_cases.MAX_SEEDS} seeds from {base} fits")
    np.savez_compressed(os.path.join(HERE, "ba_solve_edges.npz"), **out)


if __name__ == "__main__":
    main()

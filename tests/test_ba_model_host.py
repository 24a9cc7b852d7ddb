"""The new tracker bars bite (host, no GPU): deliberately wrong numpy variants of the cost
function's Jacobian, of one Schur-complement step and of the triangulation go through the same
comparisons as the kernels (ba_edges.npz, ba_dense.npz, triangulate_edges.npz) and must exceed
their bars at least 10 x; the unbroken variants must stay inside them.  The ratios are printed
(pytest -s) and recorded in DESIGN.md."""
import os

import numpy as np
import pytest

import ba_cases
import ba_oracle as O

MARGIN = 10.0


def _load(name):
    return np.load(os.path.join(ba_cases.GOLDEN, name))


# ---- the Jacobian -----------------------------------------------------------------------------
def _jacobian_variant(prob, fault):
    """ba_oracle.linearize with one term of the rotation's derivative wrong.  Jc = [D M, D] and
    Jp = D R, so a wrong M or R is a correction D (M' - M) on top of the oracle's output."""
    r, Jc, Jp = O.linearize(prob["points"], prob["cam_pose"], prob["features"], prob["ptIdx"],
                            prob["camIdx"])
    X, w = prob["points"][prob["ptIdx"]], prob["cam_pose"][prob["camIdx"], :3]
    D = Jc[:, :, 3:6]
    th2 = (w * w).sum(1)
    pos = th2 > 0
    th = np.sqrt(np.where(pos, th2, 1.0))
    big = th2 >= O.SERIES_TH2
    den = np.where(big, th2, 1.0)
    a = np.where(pos, np.sin(th) / th, 1.0)
    b = np.where(big, (1.0 - np.cos(th)) / den, 0.5 - th2 / 24.0)
    ab = np.where(big, (a - 2.0 * b) / den, -1.0 / 12.0 + th2 / 180.0)
    wd = (w * X).sum(1)
    ww = w[:, :, None] * w[:, None, :]
    Jc, Jp = Jc.copy(), Jp.copy()
    if fault == "ab dropped from M":
        dM = -(ab * wd)[:, None, None] * ww
        Jc[:, :, :3] += np.where(pos[:, None, None], D @ dM, 0.0)
    elif fault == "a used for b":
        e = np.where(pos, a - b, 0.0)[:, None, None]
        dM = e * (w[:, :, None] * X[:, None, :] + wd[:, None, None] * np.eye(3)[None])
        Jc[:, :, :3] += D @ dM
        Jp += D @ (e * ww)
    else:
        assert fault is None
    return r, Jc, Jp


@pytest.mark.parametrize("fault", [None, "ab dropped from M", "a used for b"])
def test_jacobian_bars_catch_a_wrong_term(fault):
    g = _load("ba_edges.npz")
    prob, ang = ba_cases.edge_grid(int(g["seed"]))
    ratios = ba_cases.edge_ratios(*_jacobian_variant(prob, fault), g, ang)
    worst = ratios[:, 1:].max()
    where = ba_cases.EDGE_ANGLES[int(ratios[:, 1:].max(1).argmax())]
    print(f"Jacobian, {fault}: {worst:.3g} x the bar (at theta = {where:.3g}); angles over 10 x: "
          f"{int((ratios[:, 1:].max(1) >= MARGIN).sum())} of {len(ratios)}")
    if fault is None:
        assert (ratios <= 1.0).all()
    else:
        assert worst >= MARGIN


# ---- one step of the solver -----------------------------------------------------------------
def _schur_step(prob, radius, fault):
    """The header's step through the Schur complement, plainly (loops, numpy solves), as a dense
    step vector; ``fault`` breaks one sum the way a kernel could."""
    r, Jc, Jp = O.linearize(prob["points"], prob["cam_pose"], prob["features"], prob["ptIdx"],
                            prob["camIdx"])
    act_c, ac = np.unique(prob["camIdx"], return_inverse=True)
    act_p, ap = np.unique(prob["ptIdx"], return_inverse=True)
    A, Pa, N, mu = len(act_c), len(act_p), len(ac), 1.0 / radius
    U, gc = np.zeros((A, 6, 6)), np.zeros((A, 6))
    V, gp = np.zeros((Pa, 3, 3)), np.zeros((Pa, 3))
    seen = np.zeros(A, int)
    for n in range(N):
        seen[ac[n]] += 1
        if fault == "65th observation dropped" and seen[ac[n]] == 65:
            pass   # a lane-strided sum that loses the element after the first full stride
        else:
            U[ac[n]] += Jc[n].T @ Jc[n]
            gc[ac[n]] += Jc[n].T @ r[n]
        V[ap[n]] += Jp[n].T @ Jp[n]
        gp[ap[n]] += Jp[n].T @ r[n]
    for M in (U, V):
        k = np.arange(M.shape[1])
        M[:, k, k] += mu * np.clip(M[:, k, k], 1e-6, 1e32)
    W = Jc.transpose(0, 2, 1) @ Jp                                  # [N,6,3]
    S, rhs = np.zeros((A, 6, A, 6)), -gc.copy()
    for q in range(Pa):
        obs = np.where(ap == q)[0]
        for n in obs:
            taken = set()
            for m in obs:
                if fault == "duplicate skipped" and ac[m] in taken:
                    continue   # the second observation of a (camera, point) pair
                taken.add(ac[m])
                S[ac[n], :, ac[m], :] -= W[n] @ np.linalg.solve(V[q], W[m].T)
            rhs[ac[n]] += W[n] @ np.linalg.solve(V[q], gp[q])
    for a in range(A):
        S[a, :, a, :] += U[a]
    dc = np.linalg.solve(S.reshape(6 * A, 6 * A), rhs.reshape(-1)).reshape(A, 6)
    dp = np.zeros((Pa, 3))
    for q in range(Pa):
        b = -gp[q].copy()
        if fault != "dp without W^T dc":
            for n in np.where(ap == q)[0]:
                b -= W[n].T @ dc[ac[n]]
        dp[q] = np.linalg.solve(V[q], b)
    return np.concatenate([dc.ravel(), dp.ravel()])


@pytest.mark.parametrize("fault,case", [(None, "dup_once"), (None, "lanes"),
                                        ("duplicate skipped", "dup_once"),
                                        ("65th observation dropped", "lanes"),
                                        ("dp without W^T dc", "idle")])
def test_step_bars_catch_a_wrong_sum(fault, case):
    g = _load("ba_dense.npz")
    prob = ba_cases.STEP_CASES[case]()
    assert ba_cases.problem_sha(prob) == str(g[f"{case}_sha"])
    delta = _schur_step(prob, ba_cases.STEP_RADIUS, fault)
    tol = g[f"{case}_tol"]
    cand = O.cost(*ba_cases.apply_step(prob, delta), prob["features"], prob["ptIdx"],
                  prob["camIdx"])
    rd = np.abs(delta - g[f"{case}_delta"]).max() / tol[0]
    rc = abs(cand / float(g[f"{case}_cand"]) - 1) / tol[2]
    print(f"step, {fault} ({case}): delta {rd:.3g} x its bar, candidate cost {rc:.3g} x its bar")
    if fault is None:
        assert rd <= 1.0 and rc <= 1.0
    else:
        assert rd >= MARGIN and rc >= MARGIN


# ---- triangulation ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ba_cases.TRI_EDGE_CASES))
def test_triangulation_bar_catches_the_wrong_eigenvector(name):
    g = _load("triangulate_edges.npz")
    P1, P2, p1, p2 = ba_cases.tri_edge_inputs(name)
    A = O.dlt_matrices(P1, P2, p1, p2)
    vec = np.linalg.eigh(A.transpose(0, 2, 1) @ A)[1]
    ratio = []
    for k in (0, 1):   # the smallest eigenvalue's vector, then the second smallest's
        with np.errstate(all="ignore"):
            X = vec[:, :3, k] / vec[:, 3:, k]
            dev = max(np.abs(X - g[f"{name}_points"]).max(),
                      np.abs(O.reproject(P1, X, p1) - g[f"{name}_err1"]).max(),
                      np.abs(O.reproject(P2, X, p2) - g[f"{name}_err2"]).max())
        ratio.append(dev / float(g[f"{name}_tol"]))
    print(f"triangulation, second-smallest eigenvector ({name}): {ratio[1]:.3g} x the bar "
          f"(the smallest: {ratio[0]:.3g})")
    assert ratio[0] <= 1.0 and ratio[1] >= MARGIN

"""Records tests/golden/sfm_tri_edges.npz: the expectations of the triangulation's edge fixture
(sfm_cases.edge_problem), of the CSR that is larger than one stride of its check
(sfm_cases.big_csr); the largest component graph is cross-checked on the way.  Stand-alone: the inputs are
regenerated from seeds, the expectations come from tests/sfm_oracle.py and nothing else is read.

    python tests/golden/make_golden_sfm_edges.py            # writes the file, prints the tables
    python tests/golden/make_golden_sfm_edges.py --search   # how FINAL_CHECK_SEED was found

As make_golden_sfm.py's make_tri does: the Jacobi oracle gives the expectations; numpy's eigh and
svd in place of the Jacobi must give the same decisions on every non-degenerate track, and the
tolerance is max(16 x their deviation, 1e-12); scipy's least_squares gives a second opinion on the
kept tracks; the input hash and the smallest decision margin are recorded.  The margin is at least
1e-6 with one stated exception: the duplicate rule of dup_exact_tie compares byte copies, so its
three tie margins are exactly 0, and they are the three intended pairs and no other.
same_centre and same_ray are degenerate (eigh and svd may decide otherwise) and are held on the
Jacobi oracle's decisions alone.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sfm_cases as C   # noqa: E402
import sfm_oracle as O   # noqa: E402

OUT = os.path.join(HERE, "sfm_tri_edges.npz")
KEYS = ("xyz", "err", "reason", "n_kept", "obs_keep")


def run(p, max_reproj=C.MAX_REPROJ, skip=(), names=None, **kw):
    """The oracle on every track of p -> (outputs as the library shapes them, margins per track,
    ties per track).  Tracks named in ``skip`` are left at reason -1."""
    T = len(p["track_start"]) - 1
    out = {"xyz": np.full((T, 3), np.nan), "err": np.full(T, np.nan),
           "reason": np.zeros(T, np.int32), "n_kept": np.zeros(T, np.int32),
           "obs_keep": np.zeros(len(p["obs_image"]), bool)}
    margins, ties = [[] for _ in range(T)], [[] for _ in range(T)]
    for t in range(T):
        if names is not None and names[t] in skip:
            out["reason"][t] = -1
            continue
        a, b = int(p["track_start"][t]), int(p["track_start"][t + 1])
        why, X, err, keep = O.triangulate(p["Rt"], p["K4"], p["obs_image"][a:b], p["obs_xy"][a:b],
                                          max_reproj, C.MIN_ANGLE, margins=margins[t],
                                          ties=ties[t], **kw)
        out["reason"][t] = why
        if why == 0:
            out["xyz"][t], out["err"][t], out["n_kept"][t] = X, err, keep.sum()
            out["obs_keep"][a:b] = keep
    return out, margins, ties


def tolerance(a, eig, svd, held):
    """max(16 x eigh-vs-svd deviation, 1e-12) per kept track; the decisions of the tracks in
    ``held`` (a bool mask) must agree between the three solvers."""
    for other in (eig, svd):
        assert np.array_equal(a["reason"][held], other["reason"][held])
        assert np.array_equal(a["n_kept"][held], other["n_kept"][held])
    with np.errstate(invalid="ignore"):
        dev = np.maximum(np.abs(eig["xyz"] - svd["xyz"]).max(1), np.abs(eig["err"] - svd["err"]))
    return dev, np.where((a["reason"] == 0) & held, np.maximum(16 * dev, 1e-12), np.nan)


def least_squares_minimum(p, a, t):
    from scipy.optimize import least_squares
    s, e = p["track_start"][t], p["track_start"][t + 1]
    sel = np.nonzero(a["obs_keep"][s:e])[0] + s
    img, uv = p["obs_image"][sel], p["obs_xy"][sel]

    def resid(X):
        pc = np.einsum("kij,j->ki", p["Rt"][img, :, :3], X) + p["Rt"][img, :, 3]
        K = p["K4"][img]
        return np.concatenate([K[:, 0] * pc[:, 0] / pc[:, 2] + K[:, 2] - uv[:, 0],
                               K[:, 1] * pc[:, 1] / pc[:, 2] + K[:, 3] - uv[:, 1]])
    return least_squares(resid, a["xyz"][t], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15).x


def final_check_property(seed):
    """-> the smallest margin when the oracle keeps one observation fewer than its "no
    refinement" run at this seed (both with reason 0), else None."""
    Rt, K4 = C.ring_cameras(C.TRI_CAMERAS, 4100)
    cams, uv = C.final_check_track(seed, Rt, K4)
    margins = []
    a = O.triangulate(Rt, K4, cams, uv, C.MAX_REPROJ, C.MIN_ANGLE, margins=margins)
    b = O.triangulate(Rt, K4, cams, uv, C.MAX_REPROJ, C.MIN_ANGLE, variant="no refinement")
    if a[0] == 0 and b[0] == 0 and a[3].sum() == b[3].sum() - 1 and min(margins) >= 1e-6:
        return min(margins)
    return None


def search():
    """The seed below 600 whose smallest decision margin is the widest."""
    found = [(m, seed) for seed in range(600) for m in [final_check_property(seed)] if m is not None]
    m, seed = max(found)
    print(f"{len(found)} seeds of 600 have the final check drop one observation; seed {seed} has "
          f"the widest smallest margin, {m:.3g} px")
    return seed


def make_edges(rec):
    p = C.edge_problem()
    names = C.EDGE_NAMES
    T = len(names)
    a, margins, ties = run(p)
    eig, _, _ = run(p, skip=C.EDGE_DEGENERATE, names=names, solver="eigh")
    svd, _, _ = run(p, skip=C.EDGE_DEGENERATE, names=names, solver="svd")
    held = np.array([n not in C.EDGE_DEGENERATE for n in names])
    for other in (eig, svd):
        for t in np.nonzero(held)[0]:
            s, e = p["track_start"][t], p["track_start"][t + 1]
            assert np.array_equal(a["obs_keep"][s:e], other["obs_keep"][s:e]), names[t]
    dev, tol = tolerance(a, eig, svd, held)
    # the margins: >= 1e-6 everywhere but on the three byte copies of dup_exact_tie
    tie_t = names.index("dup_exact_tie")
    assert sorted(ties[tie_t]) == sorted(C.EDGE_TIES), ties[tie_t]
    assert all(not ties[t] for t in range(T) if t != tie_t)
    zeros = [m for m in margins[tie_t] if m == 0.0]
    assert len(zeros) == len(C.EDGE_TIES), zeros
    margins[tie_t] = [m for m in margins[tie_t] if m != 0.0]
    per_track = np.array([min(m) if m else np.inf for m in margins])
    margin = float(per_track.min())
    assert margin >= 1e-6, (margin, names[int(per_track.argmin())])
    ls_xyz, ls_dist = np.full((T, 3), np.nan), np.full(T, np.nan)
    lens = np.diff(p["track_start"])
    for t, name in enumerate(names):
        print(f"edge {name}: reason {a['reason'][t]}, kept {a['n_kept'][t]} of {lens[t]}, err "
              f"{a['err'][t]:.3f}, eigh-svd {dev[t]:.2e}, smallest margin {per_track[t]:.3g}")
        if a["reason"][t] != 0 or not held[t]:
            continue
        ls_xyz[t] = least_squares_minimum(p, a, t)
        ls_dist[t] = np.abs(ls_xyz[t] - a["xyz"][t]).max()
        print(f"    least_squares minimum: the oracle is {ls_dist[t]:.2e} away (tol {tol[t]:.1e})")
    # what each case is for
    for name in C.EDGE_KEPT:
        assert a["reason"][names.index(name)] == 0, name

    def keep_of(name, out=a):
        t = names.index(name)
        return out["obs_keep"][p["track_start"][t]:p["track_start"][t + 1]]
    for name, dropped in C.EDGE_DROPS.items():
        assert np.array_equal(np.nonzero(~keep_of(name))[0], dropped), name
    k = keep_of("dup_exact_tie")
    assert all(k[s] and not k[d] for s, d in C.EDGE_TIES) and k.sum() == 77
    k = keep_of("dup_past_64")
    assert all(k[list(g)].sum() == 1 for g in C.EDGE_DUPS) and k.sum() == 137
    assert final_check_property(C.FINAL_CHECK_SEED) is not None
    t = names.index("final_check_drop")
    plain, _, _ = run(p, variant="no refinement")
    assert a["n_kept"][t] == plain["n_kept"][t] - 1 == lens[t] - 1
    for name in ("empty_mid", "empty_last"):
        assert a["reason"][names.index(name)] == 3 and lens[names.index(name)] == 0
    assert p["track_start"][-2] == p["track_start"][-1] == len(p["obs_image"])
    print("degenerate, by the Jacobi oracle alone:",
          {n: int(a["reason"][names.index(n)]) for n in C.EDGE_DEGENERATE})
    assert a["reason"][names.index("parallel_rays")] == 4   # the non-finite X after a solve
    t = names.index("mostly_unrelated")
    print("mostly_unrelated keeps positions",
          np.nonzero(keep_of("mostly_unrelated"))[0].tolist(), "of", lens[t])
    # the thresholds as arguments
    inf, _, _ = run(p, max_reproj=np.inf)
    zero, _, _ = run(p, max_reproj=0.0)
    # at 0 px every track of two or more observations is lost to reason 1, 3 or 4; the degenerate
    # ones aside, where an error of exactly 0 passes e <= 0 (same_ray: identical rows)
    assert set(zero["reason"][(lens >= 2) & held].tolist()) <= {1, 3, 4}
    print("max_reproj = +inf: reasons", inf["reason"].tolist(), "kept", inf["n_kept"].tolist())
    print("max_reproj = 0: reasons", zero["reason"].tolist())
    rec.update(edge_sha=C.tri_sha(p), edge_margin=margin, edge_tol=tol, edge_ls_xyz=ls_xyz,
               edge_ls_dist=ls_dist, edge_final_check_seed=np.int32(C.FINAL_CHECK_SEED),
               zero_reason=zero["reason"])
    for k in KEYS:
        rec[f"edge_{k}"], rec[f"inf_{k}"] = a[k], inf[k]
    print("smallest decision margin of the edge fixture (the three ties excepted):", margin)


def make_big(rec):
    p = C.big_csr()
    t0 = time.time()
    a, margins, ties = run(p)
    took = time.time() - t0
    eig, _, _ = run(p, solver="eigh")
    svd, _, _ = run(p, solver="svd")
    held = np.ones(len(a["reason"]), bool)
    for other in (eig, svd):
        assert np.array_equal(a["obs_keep"], other["obs_keep"])
    dev, tol = tolerance(a, eig, svd, held)
    margin = min(min(m) for m in margins if m)
    assert margin >= 1e-6 and not any(ties), margin
    lens = np.diff(p["track_start"])
    print(f"big CSR: {len(lens)} tracks ({int((lens == 0).sum())} empty), {len(p['obs_image'])} "
          f"observations, reasons {np.bincount(a['reason']).tolist()}, largest eigh-svd deviation "
          f"{np.nanmax(dev):.2e}, smallest margin {margin:.3g}, the oracle took {took:.1f} s")
    for name, (ts, img, want) in C.malformed_csrs(p).items():
        got = O.check_csr(ts, img, len(p["Rt"]))
        print(f"    malformed {name}: (status, index) = {got}")
        assert got == want, (name, got, want)
    assert O.check_csr(p["track_start"], p["obs_image"], len(p["Rt"])) == (0, 0)
    rec.update(big_sha=C.tri_sha(p), big_margin=margin, big_tol=tol)
    for k in KEYS:
        rec[f"big_{k}"] = a[k]


def make_graph(rec):
    """The plain-loop oracle's labels of sparse65537 confirmed with scipy's connected_components.
    The oracle takes well under a second there, so the tests run it and nothing is recorded."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    edges, n = C.graph_cases()["sparse65537"]
    t0 = time.time()
    labels = O.components(edges.tolist(), n)
    took = time.time() - t0
    k, comp = connected_components(coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])),
                                              shape=(n, n)), directed=False)
    smallest = np.full(k, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    assert np.array_equal(smallest[comp], labels)
    sizes = np.bincount(comp)
    print(f"sparse65537: {k} components, the largest of {sizes.max()} nodes, {int((sizes == 1).sum())} "
          f"isolated nodes; the plain-loop oracle took {took:.1f} s; scipy agrees")


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
        sys.exit(0)
    rec = {}
    make_edges(rec)
    make_big(rec)
    make_graph(rec)
    np.savez_compressed(OUT, **rec)
    print("wrote", os.path.relpath(OUT), os.path.getsize(OUT), "bytes")

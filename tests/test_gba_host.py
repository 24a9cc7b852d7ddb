"""Global bundle adjustment, host side (no GPU): the numpy oracle (tests/gba_oracle.py) and the
package's host path (onepose_amd/global_ba.py) against references that are not restatements of
either -- the reference's autograd, a many-digit model, a dense solve, known answers, scipy's
minimum -- then the Python layer, its refusals and the chain; and deliberately wrong variants of
the oracle, which must miss the same bars."""
import os

import numpy as np
import pytest

import ba_cases
import gba_cases as G
import gba_oracle as O
import sfm_cases as C
from onepose_amd import _lib, global_ba, object_builder, sfm

HEADER = "onepose_global_ba.h"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G.GOLDEN, "gba.npz"))


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(G.GOLDEN, "gba_edges.npz"))


def host_solve(prob, opts):
    """The package's host path on a case's arrays, with the oracle's option names."""
    return global_ba._host_solve(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"],
                                 prob["ptIdx"], prob["camIdx"], prob["fixed"], opts["max_iters"],
                                 opts["function_tolerance"], opts["pcg_tol"],
                                 opts["pcg_max_iters"], opts["radius"])


LINEARIZERS = {"oracle": O.linearize, "host": global_ba.linearize}


# ---- the binding ------------------------------------------------------------------------------
def test_the_family_is_declared_in_its_own_header():
    assert _lib.LATER_HEADERS[-1] == HEADER and _lib.FAMILY_HEADERS == ("onepose_two_view.h",)
    sig = _lib.FAMILIES[HEADER]
    assert set(sig) == {"onepose_gba_version", "onepose_gba_max_cameras",
                        "onepose_gba_workspace_bytes", "onepose_gba_linearize",
                        "onepose_gba_begin", "onepose_gba_step"}
    assert not set(sig) & (set(_lib.SIGNATURES) | set(_lib.FAMILY_SIGNATURES))
    names = [n for n, _ in sig["onepose_gba_step"][1]]
    assert names[-9:] == ["n_steps", "pcg_max_iters", "pcg_tol", "function_tolerance", "info",
                          "info_rows", "workspace", "workspace_bytes", "stream"]
    assert sig["onepose_gba_workspace_bytes"][0] is _lib.c_size_t


# ---- the cost function ------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(LINEARIZERS))
@pytest.mark.parametrize("name", sorted(ba_cases.LIN_CASES))
def test_cost_function_matches_the_reference(name, which):
    """fx = fy = f: residuals and Jacobians meet the reference's autograd (ba_lin.npz) at that
    file's 1e-9 bars."""
    lin = np.load(os.path.join(ba_cases.GOLDEN, "ba_lin.npz"))
    prob = ba_cases.problem(name, int(lin[f"{name}_seed"]))
    assert ba_cases.problem_sha(prob) == str(lin[f"{name}_sha"])
    f = prob["features"]
    n = len(f)
    r, Jc, Jp = LINEARIZERS[which](prob["points"], prob["cam_pose"][prob["camIdx"]],
                                   np.stack([f[:, 2], f[:, 2], f[:, 3], f[:, 4]], 1),
                                   np.ascontiguousarray(f[:, :2]), prob["ptIdx"], np.arange(n))
    rr, rJc, rJp = lin[f"{name}_r"], lin[f"{name}_Jc"], lin[f"{name}_Jp"]
    assert np.abs(r - rr).max() <= 1e-9
    assert np.abs(Jc - rJc).max() <= 1e-9 * np.abs(rJc).max()
    assert np.abs(Jp - rJp).max() <= 1e-9 * np.abs(rJp).max()


@pytest.mark.parametrize("which", sorted(LINEARIZERS))
def test_cost_function_with_two_focal_lengths_matches_the_model(which, edges):
    """fx != fy at theta = 0, theta^2 below and at 1e-4, pi, and a point behind the camera, with
    the bars of make_golden_ba_edges.py."""
    prob, ang = G.edge_problem()
    assert G.problem_sha(prob) == str(edges["sha"])
    r, Jc, Jp = LINEARIZERS[which](prob["points"], prob["cam_pose"], prob["K4"], prob["xy"],
                                   prob["ptIdx"], prob["camIdx"])
    ratios = G.edge_ratios(r, Jc, Jp, edges, ang)
    print("deviation / bar per angle (r, Jc, Jp):\n", np.array2string(ratios, precision=2))
    assert (ratios <= 1.0).all()
    assert len(ang) == 9 * 16


def test_fixed_columns_are_zero():
    prob = G.ring_problem(1, 6, 20, 3, big_cam=False, lone_cam=False)
    prob["fixed"][3] = 0b100101
    for lin in LINEARIZERS.values():
        _, Jc, _ = lin(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"], prob["ptIdx"],
                       prob["camIdx"], prob["fixed"])
        bits = O.fixed_bits(prob["fixed"], len(prob["cam_pose"]))[prob["camIdx"]]
        assert bits.any() and np.all(Jc.transpose(0, 2, 1)[bits] == 0.0)
        assert np.all(Jc.transpose(0, 2, 1)[~bits].any(1))


# ---- the step and the solve -------------------------------------------------------------------
def _step_deviation(prob, pts, cams, gold):
    act_c, act_p = np.unique(prob["camIdx"]), np.unique(prob["ptIdx"])
    got = np.concatenate([(cams - prob["cam_pose"])[act_c].ravel(),
                          (pts - prob["points"])[act_p].ravel()])
    return np.abs(got - gold["dense_step"]).max() / np.abs(gold["dense_step"]).max()


@pytest.fixture(scope="module")
def dense_problem():
    return G.problem(G.DENSE_CASE)


@pytest.mark.parametrize("which", ["oracle", "host"])
def test_first_step_is_the_damped_gauss_newton_step(which, gold, dense_problem):
    """pcg_tol = 1e-12 and 500 iterations against numpy.linalg.solve on the damped normal
    equations (recorded by the generator); the bar is 16 x the oracle's own deviation from that
    solve, relative to the step's largest entry, floor 1e-12."""
    prob = dense_problem
    if which == "oracle":
        pts, cams, info = G.oracle_solve(prob, G.DENSE_OPTS)
    else:
        pts, cams, info = host_solve(prob, G.DENSE_OPTS)
    dev = _step_deviation(prob, pts, cams, gold)
    print(f"{which}: first step vs dense solve {dev:.3g} (bar {float(gold['dense_tol']):.3g})")
    assert info[2] == 1 and dev <= float(gold["dense_tol"])


@pytest.mark.parametrize("wrong", ["undamped", "no_wvg", "fixed_not_zeroed"])
def test_wrong_steps_miss_the_dense_bar(wrong, gold, dense_problem):
    pts, cams, info = G.oracle_solve(dense_problem, dict(G.DENSE_OPTS), wrong=wrong)
    if info[2] == 0:   # the wrong step was rejected: nothing moved, the deviation is the step
        dev = 1.0
    else:
        dev = _step_deviation(dense_problem, pts, cams, gold)
    print(f"{wrong}: {dev:.3g} against a bar of {float(gold['dense_tol']):.3g}")
    assert dev > float(gold["dense_tol"])


def test_wrong_focal_length_misses_the_model(edges):
    prob, ang = G.edge_problem()
    r, Jc, Jp = O.linearize(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"],
                            prob["ptIdx"], prob["camIdx"], wrong="fy_by_fx")
    assert (G.edge_ratios(r, Jc, Jp, edges, ang)[:, 1:] > 1.0).all()


@pytest.mark.parametrize("name", ["status3", "reject", "all_fixed"])
def test_host_path_meets_the_oracle_bars(name, gold):
    """The package's host path is held to the bars the GPU is held to."""
    prob, opts, exp = G.load(name, gold)
    pts, cams, info = host_solve(prob, opts)
    dev, tol = G.deviations(pts, cams, info, exp), exp["tol"]
    print(name, "deviations", dev, "bars", tol)
    assert info[0] == exp["info"][0] and info[1] == exp["info"][1]
    assert (dev <= tol).all()
    sig = O.significant(exp["info"])
    assert np.array_equal(O.rows(info)[sig, 5], O.rows(exp["info"])[sig, 5])


def test_known_answers(gold):
    """Noise-free pixels: poses and points return to the truth within 1e-10 (rad, m): cond(S) <=
    1e5 x fp64 eps x variables <= 1, with a 5 x margin.  0.5 px noise: the final cost is at most
    that of the true configuration on the same observations and agrees with
    scipy.optimize.least_squares' minimum within 16 x the oracle's own deviation from it."""
    for which in ("oracle", "host"):
        prob, opts, exp = G.load("clean", gold)
        pts, cams = (exp["points"], exp["cam_pose"]) if which == "oracle" else host_solve(prob, opts)[:2]
        err = max(np.abs(pts - prob["true_points"]).max(), np.abs(cams - prob["true_cams"]).max())
        print(f"{which}, clean: distance from the truth {err:.3g}")
        assert err <= 1e-10
        prob, opts, exp = G.load("noisy", gold)
        final = exp["info"][4] if which == "oracle" else host_solve(prob, opts)[2][4]
        at_truth = O.cost(prob["true_points"], prob["true_cams"], prob["K4"], prob["xy"],
                          prob["ptIdx"], prob["camIdx"])
        ref = float(gold["noisy_scipy_cost"])
        print(f"{which}, noisy: cost {final:.12g}, at the truth {at_truth:.6g}, scipy {ref:.12g}")
        assert final <= at_truth
        assert abs(final - ref) / ref <= float(gold["noisy_scipy_tol"])


def test_split_steps_and_info_capacity():
    """The oracle's state machine: 6 steps equal 2 + 4, and rows past the capacity are dropped."""
    prob = G.ring_problem(7, 8, 30, 4, big_cam=False, lone_cam=False)
    a = O.Solver(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"], prob["ptIdx"],
                 prob["camIdx"], prob["fixed"], info_rows=8)
    b = O.Solver(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"], prob["ptIdx"],
                 prob["camIdx"], prob["fixed"], info_rows=2)
    ra = a.step(6, function_tolerance=0.0)
    b.step(2, function_tolerance=0.0)
    rb = b.step(4, function_tolerance=0.0)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert ra[2][1] == rb[2][1] == 6 and np.array_equal(ra[2][:24], rb[2])


# ---- the Python layer -------------------------------------------------------------------------
def ring_model(name):
    """A case of gba_cases as the mapping ``reconstruct`` returns (the keys the adjustment
    reads), and the case's problem."""
    prob = G.problem(name)
    m = len(prob["cam_pose"])
    xys, slot = [[] for _ in range(m)], []
    for n, c in enumerate(prob["camIdx"]):
        slot.append(len(xys[c]))
        xys[c].append(prob["xy"][n])
    slot = np.array(slot)
    P = len(prob["points"])
    tracks_i = [prob["camIdx"][prob["ptIdx"] == p] + 1 for p in range(P)]
    tracks_f = [slot[prob["ptIdx"] == p] for p in range(P)]
    seen = np.array([len(t) > 0 for t in tracks_i])
    ids = np.arange(1, m + 1, dtype=np.int32)
    model = {"camera_ids": ids.copy(), "camera_params": prob["K4"].copy(), "image_ids": ids,
             "image_camera_ids": ids.copy(),
             "qvec": global_ba.aa2qvec(prob["cam_pose"][:, :3]), "tvec": prob["cam_pose"][:, 3:],
             "xys": [np.array(x).reshape(-1, 2) for x in xys], "xyz": prob["points"][seen],
             "track_image_ids": [t for t, s in zip(tracks_i, seen) if s],
             "track_point2D_idxs": [t for t, s in zip(tracks_f, seen) if s],
             "error": np.zeros(int(seen.sum()))}
    return model, prob


def test_quaternion_round_trip():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((50, 3))
    aa = np.concatenate([d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 3.1, (50, 1)),
                         np.zeros((1, 3)),
                         1e-12 * rng.standard_normal((3, 3)), [[np.pi - 1e-9, 0, 0]]])
    back = global_ba.qvec2aa(global_ba.aa2qvec(aa))
    assert np.abs(back - aa).max() <= 1e-14 * 4
    for k, a in enumerate(aa[:5]):
        th = np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / th
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        assert np.abs(sfm.rotmat2qvec(R) - global_ba.aa2qvec(a[None])[0]).max() <= 1e-14


def test_global_bundle_adjust_on_a_model():
    model, prob = ring_model("status3")
    before = {k: np.array(model[k], copy=True) for k in ("xyz", "qvec", "tvec", "error")}
    out = sfm.global_bundle_adjust(model, pcg_tol=1e-10)
    for k, v in before.items():   # nothing changed in place
        assert np.array_equal(model[k], v), k
    rep = out["global_ba"]
    assert rep["status"] == O.ST_CONVERGED and rep["cost_after"] < 0.01 * rep["cost_before"]
    assert rep["rows"].shape == (rep["iterations"], 8) and rep["accepted"] >= 1
    assert rep["cg_iterations"] == rep["rows"][:, 6].sum()
    # gauge: the first image with observations and t_x of the second keep their bits
    seen = np.unique(prob["camIdx"])
    assert rep["fixed"][seen[0]] == 63 and rep["fixed"][seen[1]] == 8 and rep["fixed"].sum() == 71
    assert np.array_equal(out["qvec"][seen[0]], model["qvec"][seen[0]])
    assert np.array_equal(out["tvec"][seen[0]], model["tvec"][seen[0]])
    assert out["tvec"][seen[1], 0] == model["tvec"][seen[1], 0]
    assert not np.array_equal(out["tvec"][seen[1], 1:], model["tvec"][seen[1], 1:])
    idle = np.setdiff1d(np.arange(len(model["qvec"])), prob["camIdx"])
    assert len(idle) == 2 and np.array_equal(out["qvec"][idle], model["qvec"][idle])
    assert np.abs(np.linalg.norm(out["qvec"], axis=1) - 1).max() <= 1e-15 * 4
    # error: the mean reprojection distance of the refined model, as reconstruct defines it
    pts, cams, K4, xy, pi, ci = global_ba.model_problem(out)
    r = O.linearize(pts, cams, K4, xy, pi, ci, jac=False)
    e = np.sqrt((r * r).sum(1))
    want = np.array([e[pi == p].mean() for p in range(len(pts))])
    assert np.abs(out["error"] - want).max() <= 1e-9
    assert abs(0.5 * (r * r).sum() - rep["cost_after"]) <= 1e-6 * rep["cost_after"]
    # the mask forms
    free = sfm.global_bundle_adjust(model, fixed=None, max_iters=3)
    assert free["global_ba"]["fixed"] is None
    assert not np.array_equal(free["tvec"][seen[0]], model["tvec"][seen[0]])
    frozen = sfm.global_bundle_adjust(model, fixed="all", max_iters=3)
    assert np.array_equal(frozen["qvec"], model["qvec"]) and np.array_equal(frozen["tvec"],
                                                                            model["tvec"])
    assert not np.array_equal(frozen["xyz"], model["xyz"])
    assert frozen["global_ba"]["cg_iterations"] == 0
    mask = np.zeros(len(model["qvec"]), np.uint8)
    mask[seen[:3]] = 63
    own = sfm.global_bundle_adjust(model, fixed=mask, max_iters=3)
    assert np.array_equal(own["tvec"][seen[:3]], model["tvec"][seen[:3]])
    assert np.array_equal(own["global_ba"]["fixed"], mask)
    # poll_every does not change the result
    for poll in (None, 1):
        again = sfm.global_bundle_adjust(model, pcg_tol=1e-10, poll_every=poll)
        for k in ("xyz", "qvec", "tvec", "error"):
            assert np.array_equal(again[k], out[k]), (poll, k)
    # the reference's own settings are accepted: tolerances 0 run on to the radius underflow
    small, _ = ring_model("status4")
    ref = sfm.global_bundle_adjust(small, max_iters=150, function_tolerance=0.0, pcg_tol=0.0,
                                   pcg_max_iters=30)
    assert ref["global_ba"]["status"] == O.ST_MIN_RADIUS and ref["global_ba"]["radius"] < 1e-32


def test_refusals():
    model, _ = ring_model("status4")
    for kw in (dict(max_iters=0), dict(max_iters=2.5), dict(pcg_max_iters=0),
               dict(pcg_max_iters=501), dict(pcg_tol=-1.0), dict(pcg_tol=float("nan")),
               dict(function_tolerance=float("inf")), dict(function_tolerance=-1e-9),
               dict(initial_radius=0.0), dict(initial_radius=float("nan")), dict(poll_every=0),
               dict(fixed="none"), dict(fixed=np.zeros(3, np.uint8)),
               dict(fixed=np.zeros(len(model["qvec"]), np.int64)), dict(device="cpu")):
        with pytest.raises(ValueError):
            sfm.global_bundle_adjust(model, **kw)
    empty = dict(model, track_image_ids=[], track_point2D_idxs=[], xyz=np.zeros((0, 3)))
    with pytest.raises(ValueError, match="no observations"):
        sfm.global_bundle_adjust(empty)
    feats, names, poses, Ks, _, _ = C.scene()
    with pytest.raises(ValueError, match="refine"):
        sfm.reconstruct(feats, names, poses, Ks, None, refine="colmap")


# ---- the chain --------------------------------------------------------------------------------
def perturbed_poses(poses, names, seed=4300):
    """Every pose but the gauge (the first image whole, t_x of the second, in stem order) off by
    0.5 degrees and 5 mm."""
    rng = np.random.default_rng(seed)
    order = sorted(range(len(names)), key=lambda i: int(os.path.splitext(os.path.basename(names[i]))[0]))
    out = poses.copy()
    for rank, i in enumerate(order):
        if rank == 0:
            continue
        w = np.deg2rad(0.5) * rng.standard_normal(3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
        dR = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        dt = 0.005 * rng.standard_normal(3)
        if rank == 1:
            dt[0] = 0.0
        out[i, :3, :3] = dR @ poses[i, :3, :3]
        out[i, :3, 3] = poses[i, :3, 3] + dt
    return out


def _within_1mm(model, pts, owner):
    good = set()
    for k, tr_img in enumerate(model["track_image_ids"]):
        owners = {int(owner[model["names"][i - 1]][f]) for i, f in
                  zip(tr_img, model["track_point2D_idxs"][k])}
        if len(owners) == 1 and -1 not in owners:
            (o,) = owners
            if np.linalg.norm(model["xyz"][k] - pts[o]) <= 1e-3:
                good.add(o)
    return len(good)


def _model_cost(model, poses_model=None):
    """1/2 sum r^2 of a model's observations, at its own poses or at another model's."""
    pts, cams, K4, xy, pi, ci = global_ba.model_problem(model)
    if poses_model is not None:
        cams = global_ba.model_problem(dict(poses_model, track_image_ids=[],
                                            track_point2D_idxs=[]))[1]
    return O.cost(pts, cams, K4, xy, pi, ci)


def check_chain(device, tmp_path=None):
    """reconstruct(refine="global_ba") from perturbed poses ends at a cost at most that of the
    true poses with the chain's own points (the points the chain triangulates, under the true
    poses, on the same tracks and observations).  The reprojection filter is opened to 40 px so
    that the perturbation (0.5 degrees are 5 px) drops no observation and both runs see the same
    ones; the test checks that they do."""
    from test_sfm_host import OracleNN
    feats, names, poses, Ks, pts, owner = C.scene()
    bad = perturbed_poses(poses, names)
    kw = dict(covis_num=10, max_reproj=40.0, device=device, match_device=None)
    if device is not None:
        from onepose_amd import nn_matcher
        matcher = nn_matcher.NearestNeighbour({"ratio_threshold": 0.8, "distance_threshold": 0.7})
        kw["match_device"] = device
    else:
        matcher = OracleNN()
    true_model = sfm.reconstruct(feats, names, poses, Ks, matcher, **kw)
    plain = sfm.reconstruct(feats, names, bad, Ks, matcher, refine=None, **kw)
    today = sfm.reconstruct(feats, names, bad, Ks, matcher, **kw)
    for k in ("xyz", "qvec", "tvec", "error", "track_len", "ids"):   # refine=None is today's chain
        assert np.array_equal(plain[k], today[k]), k
    assert "global_ba" not in plain
    out_dir = None if tmp_path is None else str(tmp_path / "refined")
    refined = sfm.reconstruct(feats, names, bad, Ks, matcher, refine="global_ba",
                              refine_options=dict(pcg_tol=1e-8, function_tolerance=1e-10),
                              out_dir=out_dir, **kw)
    same = (len(true_model["ids"]) == len(refined["ids"]) and all(
        np.array_equal(a, b) and np.array_equal(c, d) for a, b, c, d in
        zip(true_model["track_image_ids"], refined["track_image_ids"],
            true_model["track_point2D_idxs"], refined["track_point2D_idxs"])))
    rep = refined["global_ba"]
    c_true, c_plain = _model_cost(true_model), _model_cost(plain)
    print(f"cost: perturbed {c_plain:.6g} -> refined {rep['cost_after']:.6g} in "
          f"{rep['iterations']} iterations ({rep['status_text']}), true poses with the chain's own "
          f"points {c_true:.6g}; points within 1 mm of the truth: {_within_1mm(plain, pts, owner)} "
          f"without refine, {_within_1mm(refined, pts, owner)} with, "
          f"{_within_1mm(true_model, pts, owner)} under the true poses")
    assert same, "the two runs kept different observations: the costs are not comparable"
    assert rep["status"] in (O.ST_OK, O.ST_CONVERGED) and rep["accepted"] >= 1
    assert abs(rep["cost_before"] - c_plain) <= 1e-9 * c_plain
    assert rep["cost_after"] <= c_true
    return feats, names, refined, out_dir


def test_reconstruct_refines_the_model(tmp_path):
    feats, names, refined, out_dir = check_chain(None, tmp_path)
    # the refined model is what is written, and the object builder accepts both forms
    a = object_builder.build_object(refined, feats, names, C.SCENE_BOX, device=None)
    b = object_builder.build_object(out_dir, feats, names, C.SCENE_BOX, device=None)
    assert a["keypoints3d"].shape[0] >= 0.9 * C.SCENE_POINTS
    for k in ("keypoints3d", "idxs"):
        assert np.array_equal(a[k], b[k]), k
    pts3 = object_builder.read_points3d_binary(os.path.join(out_dir, "points3D.bin"))
    assert np.array_equal(pts3["xyz"], refined["xyz"])

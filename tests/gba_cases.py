"""The global bundle adjustment cases shared by tests/golden/make_golden_gba.py (which records
the oracle's results and the tolerances) and the tests (which regenerate the inputs from the seed
and compare their digest)."""
import os

import numpy as np

import gba_oracle as O
import sfm_cases
from ba_cases import sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("points", "cam_pose", "K4", "xy", "ptIdx", "camIdx", "fixed")
N_PERM = 8


def aa_of(R):
    """Angle-axis of a rotation matrix (angles away from pi)."""
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    if th < 1e-12:
        return np.zeros(3)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2 * np.sin(th))
    return w * th


def gauge_mask(n_cams, first, second):
    f = np.zeros(n_cams, np.uint8)
    f[first] = 63
    f[second] = 8          # t_x
    return f


def ring_problem(seed, m, npts, views, noise=0.5, rot_deg=0.5, trans=0.005, pt=0.003,
                 mask="gauge", idle=True, big_cam=True, lone_cam=True, wide_point=False):
    """m active ring cameras (sfm_cases.ring_cameras, fx != fy) around npts points in a +-0.1 m
    box, every point seen by `views` random cameras; with big_cam camera 2 sees every point (more
    than 257 observations at npts >= 257), with lone_cam the last active camera sees one point
    only, with wide_point point 0 is seen by every camera (but the lone one) and point 1 by two.
    With idle, two camera ids and three point ids carry no observation.  The pixels are the
    projections of the true configuration (through the oracle's own cost function, so that zero
    noise means a zero cost) plus `noise` px; the start has every pose but the gauge off by
    rot_deg and trans and the points by pt.  mask: None, "gauge", "all", "one_free"."""
    rng = np.random.default_rng(seed)
    Rt, K4a = sfm_cases.ring_cameras(m, seed)
    cams_a = np.array([np.concatenate([aa_of(r[:, :3]), r[:, 3]]) for r in Rt])
    n_cams, n_points = (m + 2, npts + 3) if idle else (m, npts)
    cam_ids = np.setdiff1d(np.arange(n_cams), [5, n_cams - 1])[:m] if idle else np.arange(m)
    pt_ids = np.setdiff1d(np.arange(n_points), [0, 7, n_points - 1])[:npts] if idle \
        else np.arange(npts)
    true_c = np.zeros((n_cams, 6))
    true_c[:, 5] = 0.5
    K4 = np.tile([[500.0, 510.0, 256.0, 250.0]], (n_cams, 1))
    true_c[cam_ids], K4[cam_ids] = cams_a, K4a
    true_p = np.zeros((n_points, 3))
    true_p[pt_ids] = rng.uniform(-0.1, 0.1, (npts, 3))
    usable = m - 1 if lone_cam else m
    pi, ci = [], []
    for p in range(npts):
        seen = list(rng.permutation(usable)[:views])
        if wide_point and p == 0:
            seen = list(range(usable))
        if wide_point and p == 1:
            seen = seen[:2]
        if big_cam and 2 not in seen and not (wide_point and p == 1):
            seen.append(2)
        if lone_cam and p == 3:
            seen.append(m - 1)
        pi += [pt_ids[p]] * len(seen)
        ci += [cam_ids[c] for c in seen]
    order = rng.permutation(len(pi))
    pi, ci = np.array(pi, np.int64)[order], np.array(ci, np.int64)[order]
    proj = O.linearize(true_p, true_c, K4, np.zeros((len(pi), 2)), pi, ci, jac=False)
    xy = proj + noise * rng.standard_normal(proj.shape)
    cams = true_c.copy()
    cams[cam_ids] += np.concatenate([np.deg2rad(rot_deg) * rng.standard_normal((m, 3)),
                                     trans * rng.standard_normal((m, 3))], 1)
    pts = true_p.copy()
    pts[pt_ids] += pt * rng.standard_normal((npts, 3))
    g = gauge_mask(n_cams, cam_ids[0], cam_ids[1])
    if mask == "gauge":
        fixed = g
    elif mask == "all":
        fixed = np.full(n_cams, 63, np.uint8)
    elif mask == "one_free":
        fixed = np.full(n_cams, 63, np.uint8)
        fixed[cam_ids[4]] = 0
    else:
        fixed = None
    if mask is not None:   # fixed parameters stand at their true values
        bits = O.fixed_bits(fixed, n_cams)
        cams = np.where(bits, true_c, cams)
    return {"points": pts, "cam_pose": cams, "K4": K4, "xy": xy, "ptIdx": pi, "camIdx": ci,
            "fixed": fixed, "true_points": true_p, "true_cams": true_c}


def problem_sha(prob):
    return sha(*[prob[k] if prob[k] is not None else np.zeros(0) for k in KEYS])


# name -> (ring_problem arguments, solve options).  pcg_tol = 1e-10 unless the case is about it,
# so that one CG iteration more or less does not move the step.
_T = dict(pcg_tol=1e-10, pcg_max_iters=100, function_tolerance=0.0, radius=1e4)
CASES = {
    # 25 active cameras (one past the tracker's limit): camera 2 with 300+ observations, the last
    # with one, idle ids
    "c25": (dict(seed=5100, m=25, npts=300, views=6), dict(_T, max_iters=5)),
    "c65": (dict(seed=5200, m=65, npts=200, views=8), dict(_T, max_iters=5)),
    # 130 active cameras, nothing fixed, a point seen by all 130 cameras and one seen by two
    "c130": (dict(seed=5300, m=130, npts=150, views=8, mask=None, wide_point=True,
                  lone_cam=False),
             dict(_T, max_iters=4)),
    "all_fixed": (dict(seed=5400, m=25, npts=120, views=6, mask="all"), dict(_T, max_iters=4)),
    "one_free": (dict(seed=5500, m=25, npts=120, views=6, mask="one_free"), dict(_T, max_iters=4)),
    "cap3": (dict(seed=5600, m=25, npts=120, views=6), dict(_T, max_iters=5, pcg_max_iters=3)),
    "tol01": (dict(seed=5700, m=25, npts=120, views=6), dict(_T, max_iters=5, pcg_tol=0.1)),
    # a start far off (4 degrees, 4 cm) under a wide trust region: the trajectory rejects steps
    "reject": (dict(seed=5800, m=12, npts=80, views=5, rot_deg=4.0, trans=0.04, pt=0.02,
                    big_cam=False, lone_cam=False), dict(_T, max_iters=8, radius=1e8)),
    "status3": (dict(seed=5900, m=25, npts=120, views=6),
                dict(_T, max_iters=20, function_tolerance=1e-6)),
    # both tolerances 0: the converged solve runs on until the radius underflows
    "status4": (dict(seed=6000, m=6, npts=40, views=4, big_cam=False, lone_cam=False, idle=False),
                dict(_T, max_iters=60)),
    # known answers
    "clean": (dict(seed=6100, m=30, npts=300, views=8, noise=0.0, big_cam=False, lone_cam=False),
              dict(_T, max_iters=12)),
    "noisy": (dict(seed=6200, m=30, npts=300, views=8, big_cam=False, lone_cam=False),
              dict(_T, max_iters=12, function_tolerance=1e-12)),
}
# cases that run on past convergence, where accept / reject is rounding: their iteration counts
# and rows are not paired with the oracle's, only the significant iterations and the end are
FREE_RUN = ("status4", "clean")
DENSE_CASE = "c25"
DENSE_OPTS = dict(pcg_tol=1e-12, pcg_max_iters=500, function_tolerance=0.0, radius=1e4, max_iters=1)


def problem(name):
    return ring_problem(**CASES[name][0])


def oracle_solve(prob, opts, perm=None, wrong=None):
    xy, pi, ci = prob["xy"], prob["ptIdx"], prob["camIdx"]
    if perm is not None:
        xy, pi, ci = xy[perm], pi[perm], ci[perm]
    return O.solve(prob["points"], prob["cam_pose"], prob["K4"], xy, pi, ci, prob["fixed"],
                   wrong=wrong, **opts)


def load(name, g):
    prob = problem(name)
    assert problem_sha(prob) == str(g[f"{name}_sha"]), "generated inputs changed"
    exp = {k: g[f"{name}_{k}"] for k in ("points", "cam_pose", "info", "tol", "cg_lo", "cg_hi")}
    return prob, CASES[name][1], exp


def rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return float(np.nanmax(d)) if np.size(d) else 0.0


def deviations(pts, cams, info, exp):
    """(variables abs, costs / initial cost, md rel, rho abs, radius rel) against a recorded
    result, the last three over its significant iterations."""
    einfo = exp["info"]
    rw, erw = O.rows(info), O.rows(einfo)
    n = min(len(rw), len(erw))
    sig = O.significant(einfo)[:n]
    dv = max(np.abs(pts - exp["points"]).max(), np.abs(cams - exp["cam_pose"]).max())
    a = np.concatenate([info[3:5], rw[:n, :2].ravel()])
    b = np.concatenate([einfo[3:5], erw[:n, :2].ravel()])
    d = np.abs(a - b)
    d[np.isnan(a) & np.isnan(b)] = 0.0
    d_cost = float(np.max(d) / einfo[3]) if not np.isnan(d).any() else np.inf
    d_md, d_rad = rel(rw[:n][sig, 2], erw[:n][sig, 2]), rel(rw[:n][sig, 4], erw[:n][sig, 4])
    d_rho = float(np.abs(rw[:n][sig, 3] - erw[:n][sig, 3]).max()) if sig.any() else 0.0
    return np.array([dv, d_cost, d_md, d_rho, d_rad])


# ---- the cost function with fx != fy against a many-digit model (make_golden_gba_edges.py) ------
EDGE_ANGLE_IDS = (0, 1, 4, 7, 8, 9, 10, 11, 13)   # of ba_cases.EDGE_ANGLES: 0, 1e-160, 1e-9, 1e-7,
#                                     1e-6, 1e-4, 1e-2 (theta^2 at the series' threshold), 0.5, pi
EDGE_FY_RATIO = 1.07


def edge_problem():
    """(problem, angle id [N]): the observations of ba_cases.edge_grid at f = 550 and the angles
    above (4 axes x 4 geometries each, the last geometry a point behind the camera), with
    fy = 1.07 fx; one camera and one point per observation."""
    import ba_cases
    prob, ang = ba_cases.edge_grid()
    keep = np.isin(ang, EDGE_ANGLE_IDS) & (prob["features"][:, 2] == ba_cases.EDGE_FOCALS[0])
    f = prob["features"][keep]
    n = int(keep.sum())
    out = {"points": prob["points"][keep], "cam_pose": prob["cam_pose"][keep],
           "K4": np.stack([f[:, 2], EDGE_FY_RATIO * f[:, 2], f[:, 3], f[:, 4]], 1),
           "xy": np.ascontiguousarray(f[:, :2]), "ptIdx": np.arange(n, dtype=np.int64),
           "camIdx": np.arange(n, dtype=np.int64), "fixed": None}
    return out, ang[keep]


def edge_ratios(r, Jc, Jp, g, ang):
    """Deviation over bar per recorded angle, [len(EDGE_ANGLE_IDS), 3] for (r, Jc, Jp); the bars
    are those of make_golden_ba_edges.py: per angle, 16 x the numpy oracle's largest deviation
    from the model, floors 1e-14 (Jacobians, relative to the observation's max|J|) and 64 ulps of
    the observation's largest intermediate (residual)."""
    dr = np.abs(r - g["edge_r"]).max(1)
    dJc = np.abs(Jc - g["edge_Jc"]).max((1, 2)) / np.abs(g["edge_Jc"]).max((1, 2))
    dJp = np.abs(Jp - g["edge_Jp"]).max((1, 2)) / np.abs(g["edge_Jp"]).max((1, 2))
    out = np.zeros((len(EDGE_ANGLE_IDS), 3))
    for k, ia in enumerate(EDGE_ANGLE_IDS):
        m = ang == ia
        bar_r = np.maximum(g["edge_bar_r"][k], 64 * np.finfo(np.float64).eps * g["edge_rmag"][m])
        out[k] = ((dr[m] / bar_r).max(), dJc[m].max() / g["edge_bar_Jc"][k],
                  dJp[m].max() / g["edge_bar_Jp"][k])
    return out

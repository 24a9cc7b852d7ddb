"""The bundle adjustment and triangulation cases shared by tests/golden/make_golden_ba.py (which
records them) and the tests (which regenerate the inputs from the recorded seed)."""
import hashlib
import os

import numpy as np

from onepose_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (make_ba_problem arguments, initial radius, base seed).  Shapes are (C, P, N).
SOLVE_CASES = {
    "one": (dict(n_cams=1, n_points=1, n_obs=1), 1e4, 100),
    "tiny": (dict(n_cams=3, n_points=7, n_obs=15), 1e4, 200),
    "zero_rot": (dict(n_cams=6, n_points=60, n_obs=250, zero_rot_cam=True), 1e4, 300),
    # 21 of 40 cameras and 280 of 300 points carry the observations
    "window": (dict(n_cams=40, n_points=300, n_obs=4400, active_cams=21, observed_points=280),
               1e4, 400),
    # one below, at and above the 256 observations of one workgroup of the per-observation kernels
    "n255": (dict(n_cams=5, n_points=80, n_obs=255, once_point=True), 1e4, 500),
    "n256": (dict(n_cams=5, n_points=80, n_obs=256), 1e4, 600),
    "n257": (dict(n_cams=5, n_points=80, n_obs=257, duplicate=True), 1e4, 700),
    "limit": (dict(n_cams=24, n_points=50, n_obs=600), 1e4, 800),   # A = the limit
    # close cameras, a large perturbation (36 mm, 0.12 rad) and a wide trust region: the oracle's
    # trajectory has a rejected step (4 of the first 20 seeds qualify; none does at perturb <= 5)
    "reject": (dict(n_cams=6, n_points=60, n_obs=250, dist=(0.11, 0.16), perturb=12.0), 1e6, 900),
}
LIN_CASES = {"lin_zero_rot": (dict(n_cams=6, n_points=60, n_obs=250, zero_rot_cam=True), 300),
             "lin_tiny": (dict(n_cams=3, n_points=7, n_obs=15), 200)}
TRI_SIZES = (1, 63, 64, 65, 1000)
TRI_SEED = 50
MAX_SEEDS = 40
KEYS = ("points", "cam_pose", "features", "ptIdx", "camIdx")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def problem(name, seed):
    kw = (SOLVE_CASES.get(name) or LIN_CASES[name])[0]
    return synthetic.make_ba_problem(seed, **kw)


def problem_sha(prob):
    return sha(*[prob[k] for k in KEYS])


def load_solve(name, g):
    """(problem, radius, expectations) of a recorded solve case; the inputs are regenerated from
    the seed and their digest compared."""
    seed = int(g[f"{name}_seed"])
    prob = problem(name, seed)
    assert problem_sha(prob) == str(g[f"{name}_sha"]), "synthetic inputs changed"
    exp = {k: g[f"{name}_{k}"] for k in ("points", "cam_pose", "info", "tol")}
    return prob, SOLVE_CASES[name][1], exp


def tri_inputs(n):
    d = synthetic.make_triangulation_inputs(n, TRI_SEED + n)
    P1 = d["K1"] @ np.linalg.inv(d["Tcw1"])[:3]
    P2 = d["K2"] @ np.linalg.inv(d["Tcw2"])[:3]
    return d, P1, P2


def parse_index(buf, N, C, P):
    """The arrays of onepose_ba_build_index's output (int32 words: an 8-word header magic, N, C,
    P, A, Pa, 0, 0; act_cams [C]; act_pts [P]; cam_start [C+1]; pt_start [P+1]; cam_order [N];
    pt_order [N]), the lists cut to their active lengths."""
    w = np.frombuffer(np.ascontiguousarray(buf).tobytes(), dtype=np.int32)
    head, off = w[:8], 8
    out = {"head": head}
    A, Pa = int(head[4]), int(head[5])
    for name, n, used in (("act_cams", C, A), ("act_pts", P, Pa), ("cam_start", C + 1, A + 1),
                          ("pt_start", P + 1, Pa + 1), ("cam_order", N, N), ("pt_order", N, N)):
        out[name] = w[off:off + used]
        out[name + "_offset"] = off
        off += n
    return out


GUARD = 256


class Guarded:
    """A device buffer followed by GUARD bytes of 0xA5 that must survive."""

    def __init__(self, dev, nbytes=None, data=None, dtype=None):
        import torch
        dtype = dtype or torch.float64
        if data is not None:
            src = torch.from_numpy(np.ascontiguousarray(data))
            nbytes, dtype = src.numel() * src.element_size(), src.dtype
        self.raw = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.t = self.raw[:nbytes].view(dtype)
        if data is not None:
            self.t.copy_(src.reshape(-1))

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def numpy(self, shape=None):
        a = self.t.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def intact(self):
        return bool((self.raw[self.nbytes:] == 0xA5).all())


# ---- the cost function's edge grid (tests/golden/make_golden_ba_edges.py) ----------------------
EDGE_SEED = 1100
EDGE_ANGLES = (0.0, 1e-160, 1e-30, 1e-12, 1e-9, 1e-8, 1.5e-8, 1e-7, 1e-6, 1e-4, 1e-2, 0.5,
               np.pi - 1e-9, float(np.pi), np.pi + 1e-3, 2 * np.pi - 1e-6, float(2 * np.pi), 7.0,
               50.0)
# the point in the camera's frame: on-axis at 0.4 m, at 2 cm, lateral (|x / z| = 3), 0.3 m behind
EDGE_GEOMETRY = ((0.003, -0.002, 0.4), (0.004, -0.003, 0.02), (1.2, -0.1, 0.4),
                 (0.05, 0.04, -0.3))
EDGE_FOCALS = (550.0, 3000.0)


def edge_grid(seed=EDGE_SEED):
    """(problem, angle id [N]): one linearize call, 19 angles x 4 axes x 4 geometries x 2 focal
    lengths = 608 observations, each with a camera and a point of its own."""
    rs = np.random.RandomState(seed)
    ax = rs.standard_normal(3)
    mixed = np.array([0.6, -0.64, 0.48])
    axes = (np.array([1.0, 0, 0]), np.array([0, 0, 1.0]), ax / np.linalg.norm(ax),
            mixed / np.linalg.norm(mixed))
    cams, pts, feats, ang = [], [], [], []
    for ia, th in enumerate(EDGE_ANGLES):
        for axis in axes:
            for pc in EDGE_GEOMETRY:
                for f in EDGE_FOCALS:
                    aa = axis * th
                    X = rs.uniform(-0.05, 0.05, 3)
                    t = np.array(pc) - synthetic._rodrigues_np(aa) @ X
                    c = rs.uniform(246.0, 266.0, 2) * (f / 550.0)
                    uv = f * np.array(pc[:2]) / pc[2] + c + 0.5 * rs.standard_normal(2)
                    cams.append(np.concatenate([aa, t]))
                    pts.append(X)
                    feats.append([uv[0], uv[1], f, c[0], c[1]])
                    ang.append(ia)
    n = len(cams)
    prob = {"points": np.array(pts), "cam_pose": np.array(cams), "features": np.array(feats),
            "ptIdx": np.arange(n, dtype=np.int64), "camIdx": np.arange(n, dtype=np.int64)}
    return prob, np.array(ang)


def edge_deviations(r, Jc, Jp, g):
    """Per observation: |r - model| (px) and max|J - model| / max|J model| for Jc and Jp."""
    dr = np.abs(r - g["r"]).max(1)
    dJc = np.abs(Jc - g["Jc"]).max((1, 2)) / np.abs(g["Jc"]).max((1, 2))
    dJp = np.abs(Jp - g["Jp"]).max((1, 2)) / np.abs(g["Jp"]).max((1, 2))
    return dr, dJc, dJp


def edge_ratios(r, Jc, Jp, g, ang):
    """Deviation over bar per angle, [19, 3] for (r, Jc, Jp).  The bars are the fixture's: per
    angle, 16 x the numpy oracle's largest deviation from the model, floors 1e-14 (Jacobians,
    relative) and 64 ulps of the observation's largest intermediate (residual)."""
    dr, dJc, dJp = edge_deviations(r, Jc, Jp, g)
    bar_r = np.maximum(g["bar_r"][ang], 64 * np.finfo(np.float64).eps * g["rmag"])
    out = np.zeros((len(EDGE_ANGLES), 3))
    for ia in range(len(EDGE_ANGLES)):
        m = ang == ia
        out[ia] = ((dr[m] / bar_r[m]).max(), dJc[m].max() / g["bar_Jc"][ia],
                   dJp[m].max() / g["bar_Jp"][ia])
    return out


# ---- dense-step and minimum problems (tests/golden/make_golden_ba_dense.py) --------------------
def deal_counts(seed, counts, n_points=140, **kw):
    """A problem as make_ba_problem's (same geometry and noise) whose active camera k carries
    exactly counts[k] observations: distinct (camera, point) pairs dealt over n_points points,
    every point observed, the observations in a random order."""
    rs = np.random.RandomState(seed + 77)
    A, N = len(counts), int(sum(counts))
    assert max(counts) <= n_points <= N
    base = synthetic.make_ba_problem(seed, A, n_points, A * n_points, **kw)
    cam_idx, pt_idx = [], []
    unseen = list(rs.permutation(n_points))
    for k in np.argsort(counts)[::-1]:          # the largest cameras take the unseen points first
        take = [unseen.pop() for _ in range(min(counts[k], len(unseen)))]
        rest = [p for p in rs.permutation(n_points) if p not in take]
        take += rest[:counts[k] - len(take)]
        cam_idx += [k] * counts[k]
        pt_idx += take
    assert not unseen
    order = rs.permutation(N)
    cam_idx, pt_idx = np.array(cam_idx, np.int64)[order], np.array(pt_idx, np.int64)[order]
    row = {(c, p): n for n, (c, p) in enumerate(zip(base["camIdx"], base["ptIdx"]))}
    feats = base["features"][[row[(c, p)] for c, p in zip(cam_idx, pt_idx)]]
    return {"points": base["points"], "cam_pose": base["cam_pose"], "features": feats,
            "ptIdx": pt_idx, "camIdx": cam_idx}


# name -> problem builder; at most 120 unknowns except `lanes`, whose two cameras carry 65
# observations each (the wrong-variant test of the 64-lane stride needs a 65th)
STEP_CASES = {
    "tiny": lambda: synthetic.make_ba_problem(200, 3, 7, 15),
    "idle": lambda: synthetic.make_ba_problem(6, 8, 30, 120, active_cams=5, observed_points=25),
    "dup_once": lambda: synthetic.make_ba_problem(7, 4, 30, 100, once_point=True, duplicate=True),
    "lanes": lambda: deal_counts(8, [65, 65], n_points=65),
}
STEP_RADIUS = 1e4
# name -> (builder(seed), base seed); the generator takes the first seed at which the oracle's own
# permuted and variant runs end within 4 x of its plain run's gap and gradient norm
MIN_CASES = {
    "m6": (lambda s: synthetic.make_ba_problem(s, 6, 60, 250), 1200),
    "m5": (lambda s: synthetic.make_ba_problem(s, 5, 40, 150), 1240),
    "m12": (lambda s: synthetic.make_ba_problem(s, 12, 80, 500, perturb=3.0), 1280),
}


def dense_system(prob, r, Jc, Jp):
    """(J [2N, 6A + 3Pa], r [2N], active cameras, active points): the dense Jacobian with the
    idle columns removed, cameras first."""
    act_c, ac = np.unique(prob["camIdx"], return_inverse=True)
    act_p, ap = np.unique(prob["ptIdx"], return_inverse=True)
    N, A = len(ac), len(act_c)
    J = np.zeros((2 * N, 6 * A + 3 * len(act_p)))
    for n in range(N):
        J[2 * n:2 * n + 2, 6 * ac[n]:6 * ac[n] + 6] = Jc[n]
        J[2 * n:2 * n + 2, 6 * A + 3 * ap[n]:6 * A + 3 * ap[n] + 3] = Jp[n]
    return J, r.reshape(-1), act_c, act_p


def step_of(prob, pts, cams):
    """The dense step vector of a solve that moved prob's variables to (pts, cams)."""
    act_c, act_p = np.unique(prob["camIdx"]), np.unique(prob["ptIdx"])
    return np.concatenate([(cams - prob["cam_pose"])[act_c].ravel(),
                           (pts - prob["points"])[act_p].ravel()])


def apply_step(prob, delta):
    act_c, act_p = np.unique(prob["camIdx"]), np.unique(prob["ptIdx"])
    pts, cams = prob["points"].copy(), prob["cam_pose"].copy()
    cams[act_c] += delta[:6 * len(act_c)].reshape(-1, 6)
    pts[act_p] += delta[6 * len(act_c):].reshape(-1, 3)
    return pts, cams


# ---- solver paths (tests/golden/make_golden_ba_solve_edges.py) ---------------------------------
_RUN = dict(n_cams=6, n_points=60, n_obs=250)


def _chol_fail_problem(seed):
    """`tiny` with f = 1e154 in every feature row: J^T J overflows.  (u, v) are set so that each
    residual is half the projection term, about 1e153: the cost, about 1e307, stays finite."""
    prob = synthetic.make_ba_problem(seed, 3, 7, 15)
    f = prob["features"]
    f[:, 2] = 1.0
    f[:, :2] = 0.0
    proj = _oracle().linearize(prob["points"], prob["cam_pose"], f, prob["ptIdx"],
                               prob["camIdx"], jac=False) - f[:, 3:5]      # (x / z, y / z)
    f[:, 2] = 1e154
    f[:, :2] = f[:, 3:5] + 0.5e154 * proj
    return prob


def _behind_problem(seed):
    """One observed point lies 0.3 m behind the camera of its first observation; its pixels are
    its projections there (the mirrored image) plus 0.5 px of noise."""
    prob = synthetic.make_ba_problem(seed, 6, 60, 250)
    rs = np.random.RandomState(seed + 13)
    n0 = 17
    p, cam = prob["ptIdx"][n0], prob["cam_pose"][prob["camIdx"][n0]]
    R = synthetic._rodrigues_np(cam[:3])
    prob["points"][p] = R.T @ (np.array([0.02, -0.01, -0.3]) - cam[3:])
    sel = np.where(prob["ptIdx"] == p)[0]
    f = prob["features"]
    f[sel, :2] = 0.0
    proj = _oracle().linearize(prob["points"], prob["cam_pose"], f[sel], prob["ptIdx"][sel],
                               prob["camIdx"][sel], jac=False)
    f[sel, :2] = proj + 0.5 * rs.standard_normal(proj.shape)
    return prob


def _scaled_problem(seed):
    """The image scaled by 1e-14 (f, cx, cy, u, v): the diagonal of J^T J, about 1e-21, lies under
    the 1e-6 of the damping's clamp, so that 1e-6 / radius is what regularises the step.  At
    radius 1e16 it still is a tenth of the diagonal; with ordinary pixels the damping there would
    be 1e-16 of it, the gauge directions of S pure rounding and its Cholesky a coin toss."""
    prob = synthetic.make_ba_problem(seed, **_RUN)
    prob["features"] *= 1e-14
    return prob


def radius_1e300_problem():
    """At radius 1e300 the damping is nothing: S is singular along the gauge freedom and whether
    its Cholesky passes is rounding.  No trajectory to compare, only the bookkeeping."""
    return synthetic.make_ba_problem(1350, **_RUN)


def _oracle():
    import ba_oracle
    return ba_oracle


# name -> (builder(seed), initial radius, max_iters, max_success, base seed)
SOLVE_EDGE_CASES = {
    "reject_run": (lambda s: synthetic.make_ba_problem(s, dist=(0.11, 0.16), perturb=12.0, **_RUN),
                   1e6, 8, 8, 900),
    "chol_fail": (_chol_fail_problem, 1e4, 5, 5, 200),
    "radius_cap_1e16": (_scaled_problem, 1e16, 5, 5, 1300),
    "one_iter": (lambda s: synthetic.make_ba_problem(s, **_RUN), 1e4, 1, 5, 1400),
    "one_success": (lambda s: synthetic.make_ba_problem(s, **_RUN), 1e4, 5, 1, 1400),
    "lane_counts": (lambda s: deal_counts(s, [1, 63, 64, 65, 128, 129]), 1e4, 5, 5, 1500),
    "a2": (lambda s: synthetic.make_ba_problem(s, 2, 40, 50), 1e4, 5, 5, 1600),
    "a7": (lambda s: synthetic.make_ba_problem(s, 7, 60, 175), 1e4, 5, 5, 1700),
    "a22": (lambda s: synthetic.make_ba_problem(s, 22, 80, 484), 1e4, 5, 5, 1800),
    "a23": (lambda s: synthetic.make_ba_problem(s, 23, 80, 483), 1e4, 5, 5, 1900),
    "behind": (_behind_problem, 1e4, 5, 5, 2000),
}


def load_solve_edge(name, g):
    build, radius, iters, succ, _ = SOLVE_EDGE_CASES[name]
    prob = build(int(g[f"{name}_seed"]))
    assert problem_sha(prob) == str(g[f"{name}_sha"]), "synthetic inputs changed"
    exp = {k: g[f"{name}_{k}"] for k in ("points", "cam_pose", "info", "tol")}
    return prob, radius, iters, succ, exp


# ---- triangulation geometry (tests/golden/make_golden_tri_edges.py) ----------------------------
TRI_EDGE_N = 130
# name -> (baseline in degrees, pixel noise, focal length, principal point, seed)
TRI_EDGE_CASES = {
    "b01_noise": (0.1, 0.5, 550.0, 256.0, 60), "b05_noise": (0.5, 0.5, 550.0, 256.0, 61),
    "b2_noise": (2.0, 0.5, 550.0, 256.0, 62), "b01_clean": (0.1, 0.0, 550.0, 256.0, 63),
    "b05_clean": (0.5, 0.0, 550.0, 256.0, 64), "b2_clean": (2.0, 0.0, 550.0, 256.0, 65),
    "f3000_noise": (0.5, 0.5, 3000.0, 2000.0, 66), "f3000_clean": (0.5, 0.0, 3000.0, 2000.0, 67),
}


def tri_edge_inputs(name):
    """(P1, P2, pts1, pts2): two views of 130 points in a +-5 cm box 0.4 m away, the second view
    turned by the case's baseline angle and moved by a few mm (the tracker triangulates against a
    recent keyframe).  A tenth of the pairs each have a pixel displaced by 1..4 px in view 1 or
    in view 2, so that the reprojection filter has something to remove without noise too."""
    deg, noise, f, c0, seed = TRI_EDGE_CASES[name]
    rs = np.random.RandomState(seed)
    n = TRI_EDGE_N
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    base = rs.uniform(0.3, 1.5)
    X = rs.uniform(-0.05, 0.05, (n, 3))
    kind = rs.randint(0, 10, n)
    Ps, uv = [], []
    for v in range(2):
        T = np.eye(4)
        T[:3, :3] = synthetic._rodrigues_np(axis * (base + v * np.deg2rad(deg)))
        T[:3, 3] = np.array([0.01, -0.01, 0.4]) + v * rs.uniform(-0.004, 0.004, 3)
        K = np.array([[f, 0.0, c0 + rs.uniform(-10, 10)], [0.0, f, c0 + rs.uniform(-10, 10)],
                      [0.0, 0.0, 1.0]])
        Ps.append(K @ T[:3])
        x = X @ T[:3, :3].T + T[:3, 3]
        p = x @ K.T
        p = p[:, :2] / p[:, 2:] + noise * rs.standard_normal((n, 2))
        ang = rs.uniform(0.0, 2.0 * np.pi, n)
        far = kind == v
        p[far] += (rs.uniform(1.0, 4.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[far]
        uv.append(p)
    return Ps[0], Ps[1], uv[0], uv[1]


def tri_degenerate_inputs():
    """Two degenerate inputs of 130 pairs.  `identical`: the same view and the same pixels twice
    (every A has two equal pairs of rows).  `epipole`: the second camera stands 0.1 m behind the
    first on its optical axis, and pair 0 is (0, 0) in both views, the epipoles: A^T A =
    diag(2 f^2, 2 f^2, 0, 0) exactly."""
    P1, _, p1, _ = tri_edge_inputs("b2_noise")
    Pa = np.array([[500.0, 0, 0, 0], [0, 500.0, 0, 0], [0, 0, 1.0, 0]])
    Pb = Pa.copy()
    Pb[2, 3] = 0.1
    rs = np.random.RandomState(70)
    X = np.concatenate([rs.uniform(-0.05, 0.05, (TRI_EDGE_N, 2)),
                        rs.uniform(0.3, 0.5, (TRI_EDGE_N, 1))], 1)
    qa = 500.0 * X[:, :2] / X[:, 2:]
    qb = 500.0 * X[:, :2] / (X[:, 2:] + 0.1)
    qa[0] = qb[0] = 0.0
    return {"identical": (P1, P1.copy(), p1, p1.copy()), "epipole": (Pa, Pb, qa, qb)}

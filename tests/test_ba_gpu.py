"""Bundle adjustment on the GPU: onepose_ba_linearize against the fixtures recorded from the
reference, onepose_ba_solve against the numpy oracle's recorded results under the tolerances the
fixture generator derived from the oracle alone (tests/golden/make_golden_ba.py), and the
properties that involve no oracle decision.  Further down, against references that are not the
oracle's restatement: the cost function against an mpmath model at the angles and depths where
float64 strains (make_golden_ba_edges.py), the first step against a dense 50-digit solve and
sixteen iterations against scipy's minimum (make_golden_ba_dense.py), and the solver paths of
make_golden_ba_solve_edges.py."""
import os

import numpy as np
import pytest
import torch

import ba_cases
import ba_oracle as O
from ba_cases import Guarded
from onepose_amd import _lib, synthetic, tracker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def lin():
    return np.load(os.path.join(ba_cases.GOLDEN, "ba_lin.npz"))


@pytest.fixture(scope="module")
def solved():
    return np.load(os.path.join(ba_cases.GOLDEN, "ba_solve.npz"))


class Solve:
    """One onepose_ba_solve call on guarded buffers; `mutate(index words, problem)` may corrupt
    the uploaded index or the problem before it runs."""

    def __init__(self, lib, dev, prob, radius=1e4, iters=5, succ=5, mutate=None):
        self.lib, self.dev, self.prob = lib, dev, prob
        self.N, self.C, self.P = len(prob["ptIdx"]), len(prob["cam_pose"]), len(prob["points"])
        buf, self.A, self.Pa = tracker.build_index(prob["ptIdx"], prob["camIdx"], self.C, self.P)
        words = np.frombuffer(buf.tobytes(), dtype=np.int32).copy()
        prob = {k: v.copy() for k, v in prob.items()}
        if mutate is not None:
            mutate(words, prob)
        self.points, self.cams = Guarded(dev, data=prob["points"]), Guarded(dev, data=prob["cam_pose"])
        self.feats = Guarded(dev, data=prob["features"])
        self.pt, self.cam = Guarded(dev, data=prob["ptIdx"]), Guarded(dev, data=prob["camIdx"])
        self.index = Guarded(dev, data=words)
        self.info = Guarded(dev, nbytes=8 * O.INFO_DOUBLES)
        self.ws = Guarded(dev, nbytes=lib.onepose_ba_workspace_bytes(self.N, self.A, self.Pa),
                          dtype=torch.uint8)
        self.args = (radius, iters, succ)

    def launch(self):
        radius, iters, succ = self.args
        rc = self.lib.onepose_ba_solve(self.points.ptr, self.cams.ptr, self.feats.ptr, self.pt.ptr,
                                       self.cam.ptr, self.index.ptr, self.N, self.C, self.P,
                                       self.A, self.Pa, iters, succ, radius, self.info.ptr,
                                       self.ws.ptr, self.ws.nbytes, _lib.stream_ptr(self.dev))
        _lib.check(rc, "onepose_ba_solve")

    def result(self):
        torch.cuda.synchronize(self.dev)
        for g in (self.points, self.cams, self.feats, self.pt, self.cam, self.index, self.info,
                  self.ws):
            assert g.intact(), "guard words overwritten"
        return (self.points.numpy((self.P, 3)), self.cams.numpy((self.C, 6)), self.info.numpy())

    def run(self):
        self.launch()
        return self.result()


def rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return float(np.nanmax(d)) if np.size(d) else 0.0


@pytest.mark.parametrize("name", sorted(ba_cases.LIN_CASES))
def test_linearize_matches_the_reference(name, lib, lin, device):
    """The same bounds as the oracle's host test: |d residual| <= 1e-9 px, |d J| <= 1e-9 max|J|
    (fp64 eps x magnitudes <= 2e3 x fewer than 100 operations, 10 x margin); the cost follows
    from the residual bound: |d cost| <= 1e-9 sum|r| (+ 1e-12 relative for the sum itself)."""
    prob = ba_cases.problem(name, int(lin[f"{name}_seed"]))
    assert ba_cases.problem_sha(prob) == str(lin[f"{name}_sha"])
    N, C, P = len(prob["ptIdx"]), len(prob["cam_pose"]), len(prob["points"])
    g = {k: Guarded(device, data=prob[k]) for k in ba_cases.KEYS}
    r, Jc, Jp = (Guarded(device, nbytes=8 * N * k) for k in (2, 12, 6))
    cost = Guarded(device, nbytes=8)
    rc = lib.onepose_ba_linearize(g["points"].ptr, g["cam_pose"].ptr, g["features"].ptr,
                                  g["ptIdx"].ptr, g["camIdx"].ptr, N, C, P, r.ptr, Jc.ptr, Jp.ptr,
                                  cost.ptr, _lib.stream_ptr(device))
    _lib.check(rc, "onepose_ba_linearize")
    torch.cuda.synchronize(device)
    rr, rJc, rJp = lin[f"{name}_r"], lin[f"{name}_Jc"], lin[f"{name}_Jp"]
    dr = np.abs(r.numpy((N, 2)) - rr).max()
    dJc = np.abs(Jc.numpy((N, 2, 6)) - rJc).max() / np.abs(rJc).max()
    dJp = np.abs(Jp.numpy((N, 2, 3)) - rJp).max() / np.abs(rJp).max()
    c_ref = 0.5 * (rr * rr).sum()
    dc = abs(cost.numpy()[0] - c_ref)
    print(f"{name}: |dr| {dr:.2e} |dJc| {dJc:.2e} |dJp| {dJp:.2e} (relative) |dcost| {dc:.2e}")
    assert dr <= 1e-9 and dJc <= 1e-9 and dJp <= 1e-9
    assert dc <= 1e-9 * np.abs(rr).sum() + 1e-12 * c_ref
    for x in (*g.values(), r, Jc, Jp, cost):
        assert x.intact()


def test_linearize_out_of_range_ids_give_nan_rows(lib, device):
    prob = synthetic.make_ba_problem(0, 3, 7, 15)
    prob["ptIdx"][4], prob["camIdx"][9] = 7, -1
    g = {k: Guarded(device, data=prob[k]) for k in ba_cases.KEYS}
    r, Jc, Jp = (Guarded(device, nbytes=8 * 15 * k) for k in (2, 12, 6))
    cost = Guarded(device, nbytes=8)
    _lib.check(lib.onepose_ba_linearize(g["points"].ptr, g["cam_pose"].ptr, g["features"].ptr,
                                        g["ptIdx"].ptr, g["camIdx"].ptr, 15, 3, 7, r.ptr, Jc.ptr,
                                        Jp.ptr, cost.ptr, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    rows = np.isnan(r.numpy((15, 2))).any(1)
    assert list(np.where(rows)[0]) == [4, 9] and np.isnan(cost.numpy()[0])
    assert np.isnan(Jc.numpy((15, 12))[[4, 9]]).all() and np.isnan(Jp.numpy((15, 6))[[4, 9]]).all()


@pytest.mark.parametrize("name", list(ba_cases.SOLVE_CASES))
def test_solve_matches_the_oracle(name, lib, solved, device):
    """Variables within tol[0] (absolute), costs within tol[1] (of the initial cost), and on the
    iterations whose model decrease exceeds 1e-6 x cost the model decrease (tol[2], relative), rho (tol[3]),
    the radius (tol[4], relative) and the decision itself.  Each tolerance is 16 x the largest
    deviation among oracle runs under 8 permutations of the observations, floor 1e-12, recorded
    by the generator (the info tolerances also see the oracle's variant routines).

    The count of accepted iterations is not compared with the oracle's: on an iteration below
    that significance rho is rounding noise, its decision may fall either way (the oracle's own
    permuted and variant runs differ there), and the variables then differ by a step inside tol[0].  The count
    must equal the accepted flags of the solve's own rows.  At `one` (a single observation has no
    permutation) every bar is the floor, 1e-12."""
    prob, radius, exp = ba_cases.load_solve(name, solved)
    pts, cams, info = Solve(lib, device, prob, radius).run()
    tol, einfo = exp["tol"], exp["info"]
    dv = max(np.abs(pts - exp["points"]).max(), np.abs(cams - exp["cam_pose"]).max())
    rw, erw, sig = O.rows(info), O.rows(einfo), O.significant(einfo)
    d_cost = O.cost_deviation(info, einfo)
    d_md, d_rad = rel(rw[sig, 2], erw[sig, 2]), rel(rw[sig, 4], erw[sig, 4])
    d_rho = float(np.abs(rw[sig, 3] - erw[sig, 3]).max()) if sig.any() else 0.0
    print(f"{name}: |dvars| {dv:.2e} (tol {tol[0]:.1e}) cost {d_cost:.2e} ({tol[1]:.1e}) md "
          f"{d_md:.2e} ({tol[2]:.1e}) rho {d_rho:.2e} ({tol[3]:.1e}) radius {d_rad:.2e} "
          f"({tol[4]:.1e}); accepted {rw[:, 5].astype(int).tolist()}")
    assert info[0] == einfo[0] == O.ST_OK and info[1] == einfo[1]
    assert info[2] == rw[:, 5].sum()
    assert np.array_equal(rw[sig, 5], erw[sig, 5])
    assert dv <= tol[0]
    assert d_cost <= tol[1] and d_md <= tol[2] and d_rho <= tol[3] and d_rad <= tol[4]
    # properties that involve no oracle decision
    final = O.cost(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    assert abs(info[4] - final) <= 1e-9 * final + 1e-300
    assert info[4] <= info[3]
    idle_c = np.setdiff1d(np.arange(len(cams)), prob["camIdx"])
    idle_p = np.setdiff1d(np.arange(len(pts)), prob["ptIdx"])
    assert np.array_equal(cams[idle_c], prob["cam_pose"][idle_c])
    assert np.array_equal(pts[idle_p], prob["points"][idle_p])
    assert np.all(info[O.INFO_HEAD + O.INFO_ROW * int(info[1]):] == 0) and np.all(info[6:8] == 0)
    if name == "window":
        assert len(idle_c) == 19 and len(idle_p) == 20
    if name == "limit":
        assert len(np.unique(prob["camIdx"])) == lib.onepose_ba_max_active_cameras()


def test_iteration_limits(lib, solved, device):
    """max_success stops the solve early and max_iters = 16 fills all sixteen rows."""
    prob, radius, exp = ba_cases.load_solve("zero_rot", solved)
    _, _, info = Solve(lib, device, prob, radius, iters=5, succ=2).run()
    assert info[1] == 2 and info[2] == 2
    assert np.abs(O.rows(info)[:, :2] - O.rows(exp["info"])[:2, :2]).max() <= exp["tol"][1] * info[3]
    pts, cams, info = Solve(lib, device, prob, radius, iters=16, succ=16).run()
    assert info[1] == 16 and info[4] <= info[3]
    final = O.cost(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    assert abs(info[4] - final) <= 1e-9 * final


def test_nan_feature_fails_and_moves_nothing(lib, device):
    prob = synthetic.make_ba_problem(5, 6, 60, 250)
    prob["features"][17, 1] = np.nan
    pts, cams, info = Solve(lib, device, prob).run()
    assert info[0] == O.ST_FAILED and info[1] == 0 and np.isnan(info[3])
    assert np.array_equal(pts, prob["points"]) and np.array_equal(cams, prob["cam_pose"])


def _corruptions(N, C, P):
    """(name, mutate) pairs: each leaves the index or the ids inconsistent in one way."""
    lay = ba_cases.parse_index(np.zeros(8 + 2 * (C + P + 1 + N), np.int32), N, C, P)
    off = {k[:-7]: v for k, v in lay.items() if k.endswith("_offset")}
    off["head"] = 0

    def word(name, i, value):
        def f(w, prob):
            w[off[name] + i] = value(w[off[name] + i]) if callable(value) else value
        return f

    def swap(name, i, j):
        def f(w, prob):
            a = off[name]
            w[a + i], w[a + j] = w[a + j], w[a + i]
        return f

    def ids(key, i, value):
        def f(w, prob):
            prob[key][i] = value
        return f

    return [
        ("magic", word("head", 0, 0)),
        ("header A", word("head", 4, lambda v: v - 1)),
        ("cam_order past N", word("cam_order", 3, N + 5)),
        ("cam_order negative", word("cam_order", 0, -1)),
        ("cam_order huge", word("cam_order", N - 1, 2 ** 31 - 1)),
        ("cam_order swapped", swap("cam_order", 0, N - 1)),
        ("pt_order repeated", word("pt_order", 1, 0)),
        ("pt_order past N", word("pt_order", N - 1, N)),
        ("cam_start shifted", word("cam_start", 1, lambda v: v + 1)),
        ("cam_start past N", word("cam_start", 1, N + 7)),
        ("pt_start negative", word("pt_start", 1, -5)),
        ("act_cams past C", word("act_cams", 0, C)),
        ("act_pts negative", word("act_pts", 2, -3)),
        ("ptIdx changed after the index was built", ids("ptIdx", 5, P - 1)),
        ("ptIdx out of range", ids("ptIdx", 7, P)),
        ("camIdx out of range", ids("camIdx", 0, -1)),
        ("camIdx huge", ids("camIdx", N - 1, 1 << 40)),
    ]


def test_corrupted_index_is_refused_and_moves_nothing(lib, device):
    """The solve's first kernels check every id and every CSR range before anything is read
    through them: status 2, variables bit-unchanged, guards intact."""
    prob = synthetic.make_ba_problem(6, 8, 30, 120, active_cams=5, observed_points=25)
    N, C, P = 120, 8, 30
    if prob["ptIdx"][5] == P - 1:   # the "changed" case must change something
        prob["ptIdx"][5], prob["ptIdx"][6] = prob["ptIdx"][6], prob["ptIdx"][5]
    _, _, ok = Solve(lib, device, prob).run()
    assert ok[0] == O.ST_OK and ok[2] >= 1
    for name, mutate in _corruptions(N, C, P):
        s = Solve(lib, device, prob, mutate=mutate)
        pts, cams, info = s.run()
        assert info[0] == O.ST_BAD_INDEX, name
        assert info[1] == 0 and info[2] == 0, name
        assert np.array_equal(pts, prob["points"]) and np.array_equal(cams, prob["cam_pose"]), name


def test_runs_and_streams_are_bit_equal(lib, solved, device):
    prob, radius, _ = ba_cases.load_solve("window", solved)
    first = Solve(lib, device, prob, radius).run()
    again = Solve(lib, device, prob, radius).run()
    side = torch.cuda.Stream(device)
    s = Solve(lib, device, prob, radius)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        s.launch()
    side.synchronize()
    other = s.result()
    for a, b, c in zip(first, again, other):
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)


def test_graph_replay_is_bit_equal_to_eager(lib, solved, device):
    prob, radius, _ = ba_cases.load_solve("reject", solved)
    eager = Solve(lib, device, prob, radius).run()
    s = Solve(lib, device, prob, radius)
    p0, c0 = s.points.t.clone(), s.cams.t.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.launch()
    for _ in range(2):   # the second replay starts from restored variables and a used workspace
        s.points.t.copy_(p0)
        s.cams.t.copy_(c0)
        s.info.t.fill_(-1.0)
        graph.replay()
        got = s.result()
        for a, b in zip(eager, got):
            assert np.array_equal(a, b, equal_nan=True)


def test_python_layer(solved, device):
    prob, radius, exp = ba_cases.load_solve("tiny", solved)
    t = {k: torch.from_numpy(v).to(device) for k, v in prob.items()}
    info = tracker.bundle_adjust(t["points"], t["cam_pose"], t["features"], t["ptIdx"],
                                 t["camIdx"], initial_radius=radius)
    assert info.dtype == torch.float64 and info.shape == (104,) and info.device.type == "cuda"
    assert np.abs(t["points"].cpu().numpy() - exp["points"]).max() <= exp["tol"][0]
    assert np.abs(t["cam_pose"].cpu().numpy() - exp["cam_pose"]).max() <= exp["tol"][0]
    with pytest.raises(ValueError, match="float64"):
        tracker.bundle_adjust(t["points"].float(), t["cam_pose"], t["features"], t["ptIdx"],
                              t["camIdx"])
    big = synthetic.make_ba_problem(0, 25, 40, 400)
    tb = {k: torch.from_numpy(v).to(device) for k, v in big.items()}
    with pytest.raises(ValueError, match="at most"):
        tracker.bundle_adjust(tb["points"], tb["cam_pose"], tb["features"], tb["ptIdx"],
                              tb["camIdx"])


def test_apply_ba_window(device):
    """apply_ba on a 14-frame history with win_size 10: frames 0..3 fall out of the window and
    stay bit-unchanged, the intrinsics come back untouched, the result is the oracle's on the
    windowed problem."""
    prob = synthetic.make_ba_problem(8, 14, 50, 500)
    rs = np.random.RandomState(0)
    intr = np.zeros((14, 3))
    for n, c in enumerate(prob["camIdx"]):
        intr[c] = prob["features"][n, 2:]
    cams = np.concatenate([prob["cam_pose"], intr], 1)
    ids = prob["ptIdx"].copy()
    ids[rs.permutation(500)[:40]] = -1
    fids = prob["camIdx"].astype(np.float64)
    pts_opt, cam_opt = tracker.apply_ba(prob["features"][:, :2], ids, fids, prob["points"], cams,
                                        10)
    f, p, c, _ = tracker.ba_window(prob["features"][:, :2], ids, fids, cams, 10)
    assert c.min() == 4 and len(f) < 460
    epts, ecams, einfo = O.solve(prob["points"], prob["cam_pose"], f, p, c)
    assert einfo[4] < einfo[3]
    assert np.array_equal(cam_opt[:4], cams[:4]) and np.array_equal(cam_opt[:, 6:], cams[:, 6:])
    assert cam_opt.shape == (14, 9) and pts_opt.shape == (50, 3)
    # 16 x the oracle's own spread under 8 permutations of these observations, floor 1e-12
    spread = 0.0
    for k in range(8):
        perm = np.random.RandomState(k).permutation(len(p))
        p2, c2, _ = O.solve(prob["points"], prob["cam_pose"], f[perm], p[perm], c[perm])
        spread = max(spread, np.abs(p2 - epts).max(), np.abs(c2 - ecams).max())
    tol = max(16 * spread, 1e-12)
    dv = max(np.abs(pts_opt - epts).max(), np.abs(cam_opt[:, :6] - ecams).max())
    print(f"apply_ba: |dvars| {dv:.2e} (tol {tol:.1e})")
    assert dv <= tol


# ---- the cost function against the many-digit model ---------------------------------------------
@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(ba_cases.GOLDEN, "ba_edges.npz"))


@pytest.fixture(scope="module")
def dense():
    return np.load(os.path.join(ba_cases.GOLDEN, "ba_dense.npz"))


@pytest.fixture(scope="module")
def solve_edges():
    return np.load(os.path.join(ba_cases.GOLDEN, "ba_solve_edges.npz"))


def test_linearize_matches_the_model_at_the_edges(lib, edges, device):
    """608 observations (three workgroups) over theta = 0, 1e-160 .. 50, four axes, depths of 2 cm,
    |x / z| = 3, a point behind the camera and f = 550 / 3000, against the mpmath model of
    tests/golden/make_golden_ba_edges.py.  Bars per angle, from the fixture: 16 x the numpy
    oracle's largest deviation from the model among the angle's observations; floors 1e-14 of
    the observation's max|J| and 64 ulps of |f x / z| + |c| + |u| for the residual.  The cost
    follows from the residual bars: |d cost| <= sum |r| bar + sum bar^2 / 2, + 1e-12 relative for
    the sum of 1216 squares itself."""
    prob, ang = ba_cases.edge_grid(int(edges["seed"]))
    assert ba_cases.problem_sha(prob) == str(edges["sha"]), "synthetic inputs changed"
    N = len(ang)
    assert N == 608 and N > 2 * 256
    g = {k: Guarded(device, data=prob[k]) for k in ba_cases.KEYS}
    r, Jc, Jp = (Guarded(device, nbytes=8 * N * k) for k in (2, 12, 6))
    cost = Guarded(device, nbytes=8)
    _lib.check(lib.onepose_ba_linearize(g["points"].ptr, g["cam_pose"].ptr, g["features"].ptr,
                                        g["ptIdx"].ptr, g["camIdx"].ptr, N, N, N, r.ptr, Jc.ptr,
                                        Jp.ptr, cost.ptr, _lib.stream_ptr(device)))
    torch.cuda.synchronize(device)
    for x in (*g.values(), r, Jc, Jp, cost):
        assert x.intact()
    got = (r.numpy((N, 2)), Jc.numpy((N, 2, 6)), Jp.numpy((N, 2, 3)))
    ratios = ba_cases.edge_ratios(*got, edges, ang)
    dr, dJc, dJp = ba_cases.edge_deviations(*got, edges)
    for ia, th in enumerate(ba_cases.EDGE_ANGLES):
        m = ang == ia
        print(f"theta {th:.17g}: |dr| {dr[m].max():.2e} px |dJc| {dJc[m].max():.2e} |dJp| "
              f"{dJp[m].max():.2e}; over the bar: " + " ".join(f"{v:.3f}" for v in ratios[ia]))
    bar_r = np.maximum(edges["bar_r"][ang], 64 * np.finfo(np.float64).eps * edges["rmag"])
    rm = np.abs(edges["r"]).max(1)
    c_ref = float(edges["cost"])
    dc = abs(cost.numpy()[0] - c_ref)
    c_bar = 2 * (rm * bar_r).sum() + (bar_r ** 2).sum() + 1e-12 * c_ref
    print(f"worst over the bar: r {ratios[:, 0].max():.3f} Jc {ratios[:, 1].max():.3f} Jp "
          f"{ratios[:, 2].max():.3f}; |dcost| {dc:.2e} (bar {c_bar:.1e})")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert (ratios <= 1.0).all()
    assert dc <= c_bar


# ---- the solver against a dense 50-digit step and scipy's minimum -------------------------------
@pytest.mark.parametrize("name", list(ba_cases.STEP_CASES))
def test_first_step_is_the_damped_gauss_newton_step(name, lib, dense, device):
    """max_iters = 1: the variables move by the step that mpmath solved from the dense normal
    equations (tests/golden/make_golden_ba_dense.py), and row 0 holds that step's model decrease
    and candidate cost.  Bars: 16 x what numpy.linalg.solve on the float64 normal equations
    deviates from the 50-digit solve (delta absolute, md and the cost relative), floor 1e-12."""
    prob = ba_cases.STEP_CASES[name]()
    assert ba_cases.problem_sha(prob) == str(dense[f"{name}_sha"]), "synthetic inputs changed"
    pts, cams, info = Solve(lib, device, prob, ba_cases.STEP_RADIUS, iters=1, succ=1).run()
    tol = dense[f"{name}_tol"]
    row = O.rows(info)[0]
    dd = np.abs(ba_cases.step_of(prob, pts, cams) - dense[f"{name}_delta"]).max()
    dm = abs(row[2] / float(dense[f"{name}_md"]) - 1)
    dc = abs(row[1] / float(dense[f"{name}_cand"]) - 1)
    print(f"{name}: |d delta| {dd:.2e} (tol {tol[0]:.1e}) md {dm:.2e} ({tol[1]:.1e}) candidate "
          f"cost {dc:.2e} ({tol[2]:.1e})")
    assert info[0] == O.ST_OK and info[1] == 1 and info[2] == 1 and row[5] == 1
    assert abs(row[0] / float(dense[f"{name}_cost0"]) - 1) <= 1e-12 and info[4] == row[1]
    assert dd <= tol[0] and dm <= tol[1] and dc <= tol[2]
    idle_c = np.setdiff1d(np.arange(len(cams)), prob["camIdx"])
    idle_p = np.setdiff1d(np.arange(len(pts)), prob["ptIdx"])
    assert np.array_equal(cams[idle_c], prob["cam_pose"][idle_c])
    assert np.array_equal(pts[idle_p], prob["points"][idle_p])


@pytest.mark.parametrize("name", list(ba_cases.MIN_CASES))
def test_sixteen_iterations_reach_the_minimum(name, lib, dense, device):
    """The final cost exceeds the optimum of scipy.optimize.least_squares by at most 16 x the
    oracle's own relative gap (floor 1e-9), and |J^T r|_inf at the result, evaluated on the host,
    is at most 16 x the oracle's.  The accepted count is not asserted: after convergence rho is
    noise."""
    prob = ba_cases.MIN_CASES[name][0](int(dense[f"{name}_seed"]))
    assert ba_cases.problem_sha(prob) == str(dense[f"{name}_sha"]), "synthetic inputs changed"
    pts, cams, info = Solve(lib, device, prob, 1e4, iters=16, succ=16).run()
    opt = float(dense[f"{name}_opt"])
    gap = (info[4] - opt) / opt
    r, Jc, Jp = O.linearize(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    J, rv, _, _ = ba_cases.dense_system(prob, r, Jc, Jp)
    grad = float(np.abs(J.T @ rv).max())
    print(f"{name}: gap {gap:.2e} (bar {float(dense[f'{name}_gap_bar']):.1e}) |J^T r| {grad:.2e} "
          f"(bar {float(dense[f'{name}_grad_bar']):.1e}); accepted {int(info[2])} of 16")
    assert info[0] == O.ST_OK and info[1] == 16
    final = O.cost(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    assert abs(info[4] - final) <= 1e-9 * final
    assert gap <= float(dense[f"{name}_gap_bar"])
    assert grad <= float(dense[f"{name}_grad_bar"])


# ---- solver paths -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ba_cases.SOLVE_EDGE_CASES))
def test_solve_edge_paths_match_the_oracle(name, lib, solve_edges, device):
    """What test_solve_matches_the_oracle asserts, on the cases of
    tests/golden/make_golden_ba_solve_edges.py, each with its own iteration limits.  `chol_fail`:
    every Cholesky fails (J^T J overflows); iterations, flags, NaNs, the radii (powers of two)
    and the variables must equal the oracle's exactly, and the solve's own five costs must be one
    number; that number is a sum of 30 rounded squares through the kernel's own sin and cos, so
    it is held to tol[1] like every cost, not to equal bits."""
    prob, radius, iters, succ, exp = ba_cases.load_solve_edge(name, solve_edges)
    pts, cams, info = Solve(lib, device, prob, radius, iters=iters, succ=succ).run()
    tol, einfo = exp["tol"], exp["info"]
    dv = max(np.abs(pts - exp["points"]).max(), np.abs(cams - exp["cam_pose"]).max())
    rw, erw, sig = O.rows(info), O.rows(einfo), O.significant(einfo)
    d_cost = O.cost_deviation(info, einfo)
    d_md, d_rad = rel(rw[sig, 2], erw[sig, 2]), rel(rw[sig, 4], erw[sig, 4])
    d_rho = float(np.abs(rw[sig, 3] - erw[sig, 3]).max()) if sig.any() else 0.0
    print(f"{name}: |dvars| {dv:.2e} (tol {tol[0]:.1e}) cost {d_cost:.2e} ({tol[1]:.1e}) md "
          f"{d_md:.2e} ({tol[2]:.1e}) rho {d_rho:.2e} ({tol[3]:.1e}) radius {d_rad:.2e} "
          f"({tol[4]:.1e}); accepted {rw[:, 5].astype(int).tolist()}")
    assert info[0] == einfo[0] == O.ST_OK and info[1] == einfo[1]
    assert info[2] == rw[:, 5].sum()
    assert np.array_equal(rw[sig, 5], erw[sig, 5])
    assert dv <= tol[0]
    assert d_cost <= tol[1] and d_md <= tol[2] and d_rho <= tol[3] and d_rad <= tol[4]
    final = O.cost(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    assert abs(info[4] - final) <= 1e-9 * final + 1e-300
    assert info[4] <= info[3]
    idle_c = np.setdiff1d(np.arange(len(cams)), prob["camIdx"])
    idle_p = np.setdiff1d(np.arange(len(pts)), prob["ptIdx"])
    assert np.array_equal(cams[idle_c], prob["cam_pose"][idle_c])
    assert np.array_equal(pts[idle_p], prob["points"][idle_p])
    assert np.all(info[O.INFO_HEAD + O.INFO_ROW * int(info[1]):] == 0) and np.all(info[6:8] == 0)
    if name == "chol_fail":
        assert info[2] == 0 and np.isnan(rw[:, 1:4]).all() and (rw[:, 5] == 0).all()
        assert np.array_equal(rw[:, 4], erw[:, 4]) and info[5] == einfo[5] == 0.30517578125
        assert (rw[:, 0] == info[3]).all() and info[4] == info[3] and np.isfinite(info[3])
        assert np.array_equal(pts, prob["points"]) and np.array_equal(cams, prob["cam_pose"])
    if name == "reject_run":
        acc = rw[:, 5].astype(int).tolist()
        assert acc[:5] == [1, 0, 0, 0, 1] and sig[:5].all()
        assert rw[2, 4] == rw[1, 4] / 2 and rw[3, 4] == rw[2, 4] / 4 and rw[4, 4] == rw[3, 4] / 8
    if name == "radius_cap_1e16":
        assert rw[0, 5] == 1 and (rw[1:, 4] == 1e16).all() and info[5] == 1e16
    if name in ("one_iter", "one_success"):
        assert info[1] == 1 and info[2] == 1
    if name == "lane_counts":
        assert np.bincount(prob["camIdx"]).tolist() == [1, 63, 64, 65, 128, 129]
    if name in ("a2", "a7", "a22", "a23"):
        assert len(np.unique(prob["camIdx"])) == int(name[1:])


def test_radius_1e300_keeps_its_books(lib, device):
    """Initial radius 1e300 is positive and finite, so admitted.  The damping is then nothing, S
    is singular along the gauge freedom and whether its Cholesky passes is rounding (in the oracle
    too), so no trajectory is compared.  Whatever happens: status 0, five rows; a row that is not
    accepted divides the radius by 2, 4, 8, .. exactly and moves nothing; an accepted one sets
    min(radius / max(1/3, 1 - (2 rho - 1)^3), 1e16), which from 2e16 up is exactly 1e16; the
    final cost is the cost of the returned variables and not above the initial one."""
    prob = ba_cases.radius_1e300_problem()
    pts, cams, info = Solve(lib, device, prob, 1e300).run()
    rw = O.rows(info)
    print(f"radius 1e300: accepted {rw[:, 5].astype(int).tolist()}, radii {rw[:, 4].tolist()} -> "
          f"{info[5]}, Cholesky failed {np.isnan(rw[:, 2]).astype(int).tolist()}")
    assert info[0] == O.ST_OK and info[1] == 5 and info[2] == rw[:, 5].sum()
    radius, factor = 1e300, 2.0
    for row, nxt in zip(rw, list(rw[1:, 4]) + [info[5]]):
        assert row[4] == radius
        if row[5] == 1:
            want = min(row[4] / max(1.0 / 3.0, 1.0 - (2.0 * row[3] - 1.0) ** 3), 1e16)
            assert abs(nxt / want - 1) <= 1e-12 and (nxt == 1e16 or row[4] < 2e16)
            radius, factor = nxt, 2.0
        else:
            radius, factor = radius / factor, factor * 2.0
            assert nxt == radius
    final = O.cost(pts, cams, prob["features"], prob["ptIdx"], prob["camIdx"])
    assert abs(info[4] - final) <= 1e-9 * final and info[4] <= info[3]
    if info[2] == 0:
        assert np.array_equal(pts, prob["points"]) and np.array_equal(cams, prob["cam_pose"])

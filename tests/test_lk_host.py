"""Host-side tests of the optical-flow front half of the tracker: the numpy oracle against its
recorded results and against scenes with a known answer, the ABI's host functions, and the numpy
helpers of onepose_amd.tracker (Euler angles, motion prediction, the pose_init rule)."""
import ctypes
import os

import numpy as np
import pytest

import lk_cases
import lk_oracle
from onepose_amd import _lib, tracker


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(lk_cases.GOLDEN, "lk.npz"))


@pytest.mark.parametrize("name", list(lk_cases.CASES))
def test_oracle_reproduces_the_recorded_results(name, gold):
    s = lk_cases.scene(name)
    assert lk_cases.scene_sha(s) == str(gold[f"{name}_sha"]), "scene generator changed"
    nxt, status, why, p, q = lk_cases.oracle(name)
    assert len(p) == int(gold[f"{name}_levels"])
    shas = np.array([[lk_cases.sha(i), lk_cases.sha(d)] for pyr in (p, q) for i, d in pyr])
    assert np.array_equal(shas, gold[f"{name}_pyr_sha"])
    assert nxt.dtype == np.float32
    assert np.array_equal(nxt.view(np.uint32), gold[f"{name}_next_pts"].view(np.uint32))
    assert np.array_equal(status, gold[f"{name}_status"])
    assert np.array_equal(why, gold[f"{name}_reason"])


def test_recorded_set_covers_every_end_reason(gold):
    seen = np.zeros(len(lk_oracle.REASONS), dtype=np.int64)
    for name in lk_cases.CASES:
        seen += np.bincount(gold[f"{name}_reason"], minlength=len(seen))
        st = gold[f"{name}_status"]
        assert 2 * int(st.sum()) >= len(st) == lk_cases.N_POINTS, name
    for r in (lk_oracle.R_EPS, lk_oracle.R_OSC, lk_oracle.R_CAP, lk_oracle.R_OOB_PRE,
              lk_oracle.R_OOB_LOOP, lk_oracle.R_EIG):
        assert seen[r] > 0, lk_oracle.REASONS[r]
    assert int(gold["one_level_levels"]) == 1 and int(gold["odd_levels"]) == 4


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(lk_cases.GOLDEN, "lk_edges.npz"))


@pytest.mark.parametrize("name", list(lk_cases.EDGE_CASES))
def test_oracle_reproduces_the_recorded_edge_results(name, edges):
    s = lk_cases.scene(name)
    assert lk_cases.scene_sha(s) == str(edges[f"{name}_sha"]), "scene generator changed"
    nxt, status, why, p, q = lk_cases.oracle(name)
    assert len(p) == int(edges[f"{name}_levels"])
    shas = np.array([[lk_cases.sha(i), lk_cases.sha(d)] for pyr in (p, q) for i, d in pyr])
    assert np.array_equal(shas, edges[f"{name}_pyr_sha"])
    assert np.array_equal(nxt.view(np.uint32), edges[f"{name}_next_pts"].view(np.uint32))
    assert np.array_equal(status, edges[f"{name}_status"])
    assert np.array_equal(why, edges[f"{name}_reason"])


@pytest.mark.parametrize("name", list(lk_cases.CASES) + list(lk_cases.EDGE_CASES))
def test_trace_reproduces_the_recorded_counts_and_changes_nothing(name, edges):
    """The per-level trace and the largest window sum of every case of both dicts; and track()
    with a trace gives what it gives without one."""
    s = lk_cases.scene(name)
    nxt, status, why, p, q = lk_cases.oracle(name)     # computed with trace and stats
    trace, max_ix2 = lk_cases.oracle_trace(name)
    assert np.array_equal(trace, edges[f"{name}_trace"])
    assert max_ix2 == int(edges[f"{name}_max_ix2"])
    assert np.array_equal(trace[0, 0], np.bincount(why, minlength=trace.shape[2]))
    plain = lk_oracle.track(p, q, s["pts"], s["win"], s["max_count"],
                            s.get("epsilon", lk_cases.EPSILON), lk_cases.MIN_EIG)
    assert np.array_equal(plain[0].view(np.uint32), nxt.view(np.uint32))
    assert np.array_equal(plain[1], status) and np.array_equal(plain[2], why)


def test_recorded_edge_set_covers_windows_saturation_and_coarse_level_events(edges, gold):
    """lk_cases.check_coverage, which the generator ran on the live oracle, on the recorded file:
    both ends of every kernel's window range, window sums beyond 2^31 (2^30 for block noise at
    window 15) on scenes where points pass the eigenvalue test, the tight criteria, and what
    happens above level 0 to points that end with status 1."""
    rec = {}
    for name in list(lk_cases.CASES) + list(lk_cases.EDGE_CASES):
        src = gold if name in lk_cases.CASES else edges
        rec[name] = dict(levels=int(src[f"{name}_levels"]), status=src[f"{name}_status"],
                         reason=src[f"{name}_reason"], trace=edges[f"{name}_trace"],
                         max_ix2=int(edges[f"{name}_max_ix2"]))
    lk_cases.check_coverage(rec)


@pytest.mark.parametrize("name", ["base"] + list(lk_cases.SATURATED))
def test_a_32_bit_window_sum_is_seen_where_the_sums_pass_2_31(name):
    """A numpy-only power check: the oracle with its five window sums accumulated in int32 with
    wraparound.  On "base" (largest sum 3.4e7) it is the oracle, bit for bit, so the scenes from
    before this set cannot see such a width.  It differs where a sum passes 2^31: block noise
    and stripes at window 31 (4.8e9, 6.2e9; 98 and 96 of 120 points) and the quilt at window 15
    (3.5e9; 21 points).  Block noise at window 15 reaches 1.6e9, above 2^30 but below 2^31, where
    an int32 sum is still exact: that scene is identical too, and would show only an accumulator
    narrower than 32 bits."""
    s = lk_cases.scene(name)
    want, wst, _, p, q = lk_cases.oracle(name)
    _, max_ix2 = lk_cases.oracle_trace(name)
    out, st, _ = lk_oracle.track(p, q, s["pts"], s["win"], s["max_count"], lk_cases.EPSILON,
                                 lk_cases.MIN_EIG, window_sum=lk_oracle.wrapped_int32_sum)
    differ = int(((out.view(np.uint32) != want.view(np.uint32)).any(1) | (st != wst)).sum())
    print(f"{name}: largest window sum {max_ix2:.3e}, int32 sums differ on {differ} points")
    if max_ix2 >= 2 ** 31:
        assert differ >= 10
    else:
        assert name in ("base", "noise_w15") and differ == 0


@pytest.mark.parametrize("name", list(lk_cases.CASES) + list(lk_cases.EDGE_CASES))
def test_model_pyramids_equal_the_oracles(name):
    """pyrDown and Scharr from scipy.ndimage.correlate1d(mode="mirror") against the oracle's
    index arithmetic: every level and derivative image of both frames, exactly."""
    import lk_model
    s = lk_cases.scene(name)
    _, _, _, p, q = lk_cases.oracle(name)
    for img, want in ((s["prev"], p), (s["next"], q)):
        got = lk_model.pyramid(img, s["win"], s["max_level"])
        assert len(got) == len(want)
        for (gi, gx, gy), (wi, wd) in zip(got, want):
            assert gi.dtype == np.uint8 and np.array_equal(gi, wi)
            assert np.array_equal(gx, wd[..., 0]) and np.array_equal(gy, wd[..., 1])


MODEL_BAR = lk_cases.MODEL_BAR   # 0.03 px, from the CPU measurements written beside it


@pytest.mark.parametrize("name", lk_cases.MODEL_SCENES)
def test_oracle_agrees_with_the_float64_model(name):
    """tests/lk_model.py (true bilinear weights, float64 sums, no fixed point, scipy's
    interpolation and borders) against the oracle on about 150 grid points more than a window
    from every border: status equal on every point; on the compared set (both end level 0 by
    the epsilon rule) positions within MODEL_BAR.  The compared set must be 90% of the points,
    on every scene but win21, whose shift the pyramid does not carry (see lk_cases.MODEL_ONLY).
    Measured: compared share 98.7, 92.1, 94.7, 72.7, 96.7, 100, 100 %; maxima 0.00266, 0.01183,
    0.00292, 0.00568, 0.00210, 0.00643, 0.00683 px; medians 0.0003 to 0.0012 px."""
    o, m, pts = lk_cases.model_pair(name)
    cs = lk_cases.compared_set(name)
    d = np.abs(o[0] - m[0]).max(1)
    print(f"{name}: {len(pts)} points, {int((o[1] != m[1]).sum())} status differences, compared "
          f"{int(cs.sum())} ({100 * cs.mean():.1f}%), max {d[cs].max():.5f} px")
    assert np.array_equal(o[1], m[1])
    assert name == "win21" or cs.mean() >= lk_cases.COMPARED_SHARE
    assert d[cs].max() <= MODEL_BAR


@pytest.mark.parametrize("name", lk_cases.WARPS)
def test_warp_error_is_the_models_own(name):
    """Rotation with scale: no shift to recover, but an analytic displacement per point.  On the
    interior points (more than 25 px from every border; 117, all kept and all in the compared
    set) the float64 model's own error against it is 0.557 px (warp_a) and 1.383 px (warp_b):
    the affine deformation across a 15-px window, not a defect of either side.  The oracle's
    (0.557, 1.387 px) may exceed the model's by no more than MODEL_BAR."""
    o, m, pts = lk_cases.model_pair(name)
    inside = lk_cases.interior(name)
    truth = pts + lk_cases.warp_truth(name, pts)
    em, eo = (np.abs(x[0] - truth).max(1)[inside].max() for x in (m, o))
    print(f"{name}: {int(inside.sum())} interior points, model {em:.4f} px, oracle {eo:.4f} px")
    assert inside.sum() >= 100 and o[1][inside].all() and lk_cases.compared_set(name)[inside].all()
    assert em <= 2.0          # a lost point is off by its displacement, 3 to 9 px on these
    assert eo <= em + MODEL_BAR


# h, w, shift, win, seed: no noise, no flat patch; the last needs all three levels for its shift
KNOWN = [(120, 160, (3.3, -2.6), 15, 21), (120, 160, (9.4, 6.2), 15, 22),
         (200, 240, (14.0, -11.0), 21, 23)]


@pytest.mark.parametrize("h,w,shift,win,seed", KNOWN)
def test_known_shift_is_recovered(h, w, shift, win, seed):
    """Interior points more than 25 px from the border recover the shift to <= 0.1 px and all
    have status 1 (measured maxima: 0.036, 0.038 and 0.004 px)."""
    a, b = lk_cases.image_pair(h, w, shift, seed, noise=0, flat=False)
    ys, xs = np.mgrid[26:h - 26:7, 26:w - 26:7]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32) + np.float32(0.37)
    out, status, _ = lk_oracle.calc_optical_flow_pyr_lk(a, b, pts, win, 2)
    err = np.abs(out - pts - np.array(shift, np.float32)).max()
    print(f"{h}x{w} shift {shift} win {win}: {len(pts)} points, max error {err:.4f} px")
    assert status.all()
    assert err <= 0.1


def test_constant_image_is_rejected_everywhere():
    img = np.full((60, 70), 131, np.uint8)
    pts = np.random.default_rng(0).uniform(0, 60, (50, 2)).astype(np.float32)
    out, status, why = lk_oracle.calc_optical_flow_pyr_lk(img, img, pts, 15, 2)
    assert not status.any() and (why == lk_oracle.R_EIG).all()
    assert np.array_equal(out, pts)


def test_scharr_of_a_ramp_and_pyrdown_of_a_constant():
    for slope in (1, 3):
        ramp = np.tile((10 + slope * np.arange(40)).astype(np.uint8), (30, 1))
        d = lk_oracle.scharr(ramp)
        assert d.dtype == np.int16 and d.shape == (30, 40, 2)
        assert (d[:, 1:-1, 0] == 32 * slope).all() and (d[..., 1] == 0).all()
        assert (d[:, 0, 0] == 0).all() and (d[:, -1, 0] == 0).all()   # reflect-101 at the edge
        assert (lk_oracle.scharr(ramp.T.copy())[1:-1, :, 1] == 32 * slope).all()
    for h, w in ((31, 45), (30, 44), (5, 4)):
        c = np.full((h, w), 201, np.uint8)
        down = lk_oracle.pyr_down(c)
        assert down.shape == ((h + 1) // 2, (w + 1) // 2) and (down == 201).all()


SHAPES = [(120, 160, 15, 2), (75, 97, 7, 3), (30, 40, 15, 2), (120, 160, 15, 0), (512, 512, 15, 2),
          (33, 33, 3, 5), (8192, 8192, 31, 5), (75, 97, 7, 5), (32, 64, 31, 4)]


@pytest.mark.parametrize("h,w,win,max_level", SHAPES)
def test_layout_matches_the_oracles_level_shapes(h, w, win, max_level):
    lib = _lib.load()
    assert lib.onepose_lk_version() == tracker.LK_VERSION == 1
    shapes = lk_oracle.level_shapes(h, w, win, max_level)
    assert lib.onepose_lk_levels(h, w, win, max_level) == len(shapes)
    total = lib.onepose_lk_pyramid_bytes(h, w, win, max_level)
    spans = []
    for l, (lh, lw) in enumerate(shapes):
        got = tracker.lk_pyramid_layout(h, w, win, max_level, l)
        assert got[:2] == (lh, lw)
        assert got[2] % 256 == 0 and got[3] % 256 == 0
        spans += [(got[2], got[2] + lh * lw), (got[3], got[3] + 4 * lh * lw)]
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "regions overlap or are unordered"
    assert spans[0][0] == 0 and spans[-1][1] <= total and total % 256 == 0
    with pytest.raises(_lib.OnePoseError, match="level"):
        tracker.lk_pyramid_layout(h, w, win, max_level, len(shapes))
    with pytest.raises(_lib.OnePoseError, match="level"):
        tracker.lk_pyramid_layout(h, w, win, max_level, -1)


BAD_SHAPES = [(120, 160, 14, 2), (120, 160, 33, 2), (120, 160, 1, 2), (15, 160, 15, 2),
              (120, 15, 15, 2), (120, 160, 15, 6), (120, 160, 15, -1), (8193, 160, 15, 2),
              (120, 8193, 15, 2), (0, 0, 15, 2)]


@pytest.mark.parametrize("h,w,win,max_level", BAD_SHAPES)
def test_unsupported_shapes_are_refused_on_the_host(h, w, win, max_level):
    """Even or oversize windows, win >= h or w, max_level 6, oversize images: the queries return 0
    and the entry points an error, before any pointer is touched (none is valid here)."""
    lib = _lib.load()
    assert lib.onepose_lk_levels(h, w, win, max_level) == 0
    assert lib.onepose_lk_pyramid_bytes(h, w, win, max_level) == 0
    with pytest.raises(_lib.OnePoseError, match="unsupported"):
        tracker.lk_pyramid_layout(h, w, win, max_level, 0)
    P = 0x1000   # never dereferenced
    assert lib.onepose_lk_build_pyramid(P, 0, 1, h, w, win, max_level, 1, P, None) == 1
    assert b"unsupported" in lib.onepose_last_error()
    assert lib.onepose_lk_track(P, 0, P, P, 0, P, 1, 4, h, w, win, max_level, 10, 0.03, 1e-4, P, P,
                                None) == 1
    assert b"unsupported" in lib.onepose_last_error()


def test_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib.load()
    P = 0x1000   # never dereferenced
    nb = lib.onepose_lk_pyramid_bytes(120, 160, 15, 2)

    def build(**kw):
        a = dict(image=P, bs=120 * 160, batch=2, h=120, w=160, win=15, ml=2, deriv=1, out=P,
                 stream=None)
        a.update(kw)
        return lib.onepose_lk_build_pyramid(*a.values())

    def track(**kw):
        a = dict(prev=P, pbs=0, next=P, pts=P, ptbs=0, counts=P, batch=2, n=5, h=120, w=160, win=15,
                 ml=2, count=10, eps=0.03, eig=1e-4, out=P, status=P, stream=None)
        a.update(kw)
        return lib.onepose_lk_track(*a.values())
    for call, kw, text in ((build, dict(image=None), b"null"), (build, dict(out=None), b"null"),
                           (build, dict(batch=0), b"batch"), (build, dict(bs=100), b"bstride"),
                           (build, dict(deriv=2), b"with_deriv"),
                           (track, dict(batch=0), b"batch"), (track, dict(n=-1), b"max_points"),
                           (track, dict(eps=float("nan")), b"NaN"),
                           (track, dict(eig=float("nan")), b"NaN"),
                           (track, dict(pbs=nb - 1), b"prev_pyr_bstride"),
                           (track, dict(ptbs=9), b"prev_pts_bstride"),
                           (track, dict(prev=None), b"null"), (track, dict(counts=None), b"null"),
                           (track, dict(status=None), b"null")):
        assert call(**kw) == 1 and text in lib.onepose_last_error(), (kw, lib.onepose_last_error())
    assert track(n=0, prev=None, out=None) == 0   # no points: a no-op


def test_wrappers_check_their_arguments_without_a_gpu():
    import torch
    img = np.zeros((40, 50), np.uint8)
    with pytest.raises(ValueError, match="square"):
        tracker.calc_optical_flow_pyr_lk(img, img, np.zeros((3, 1, 2), np.float32),
                                         winSize=(15, 21))
    with pytest.raises(ValueError, match="uint8"):
        tracker.build_lk_pyramid(torch.zeros(40, 50))
    with pytest.raises(RuntimeError, match="GPU"):
        tracker.build_lk_pyramid(torch.zeros(40, 50, dtype=torch.uint8))
    with pytest.raises(ValueError, match="build_lk_pyramid"):
        tracker.lk_track(None, None, torch.zeros(3, 2))
    assert tracker._lk_criteria((3, 10, 0.03)) == (10, 0.03)
    assert tracker._lk_criteria((1, 7, 0.5)) == (7, 0.001)     # no EPS bit
    assert tracker._lk_criteria((2, 7, 0.5)) == (30, 0.5)      # no COUNT bit
    assert lk_oracle.eps_squared(0.03) == np.float32(float(np.float32(0.03)) ** 2)
    assert lk_oracle.eps_squared(50.0) == np.float32(100.0)
    assert lk_oracle.eps_squared(-1.0) == 0


def rotations(n, seed):
    from scipy.spatial.transform import Rotation
    return Rotation.random(n, random_state=seed).as_matrix()


def test_euler_round_trip_and_scipy():
    from scipy.spatial.transform import Rotation
    for R in rotations(100, 5):
        e = tracker.mat2euler(R)
        assert np.abs(tracker.euler2mat(*e) - R).max() <= 1e-12
        assert np.abs(Rotation.from_euler("xyz", e).as_matrix() - R).max() <= 1e-12
    rng = np.random.default_rng(6)
    for e in rng.uniform(-1.5, 1.5, (100, 3)):
        M = tracker.euler2mat(*e)
        assert np.abs(Rotation.from_euler("xyz", e).as_matrix() - M).max() <= 1e-12
        assert np.abs(np.array(tracker.mat2euler(M)) - e).max() <= 1e-12


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_euler_gimbal_branch(sign):
    ay = sign * np.pi / 2
    R = tracker.euler2mat(0.3, ay, 0.0)
    R[0, 0] = R[1, 0] = 0.0          # cos(pi/2) in floating point is 6e-17: make the lock exact
    ax2, ay2, az2 = tracker.mat2euler(R)
    assert az2 == 0.0 and abs(ay2 - ay) <= 1e-12
    assert np.abs(tracker.euler2mat(ax2, ay2, az2) - R).max() <= 1e-12
    # az is not recoverable there: a rotation built with az != 0 comes back with az = 0 and an
    # ax that absorbs it, and still reproduces the matrix
    R = tracker.euler2mat(0.3, ay, 0.4)
    R[0, 0] = R[1, 0] = 0.0
    e = tracker.mat2euler(R)
    assert e[2] == 0.0 and abs(e[0] - (0.3 - sign * 0.4)) <= 1e-12
    assert np.abs(tracker.euler2mat(*e) - R).max() <= 1e-12


def pose_of(euler, t):
    T = np.eye(4)
    T[:3, :3] = tracker.euler2mat(*euler)
    T[:3, 3] = t
    return T


def test_motion_prediction_by_hand():
    """Translations 0, 1, 3 along x: speed ((1) + (2)) / 2 = 1.5, so 4.5.  Euler angles 0.1, 0.2
    and (ignored) 0.9 about x: rot_t is the angle of the pose before last, 0.2, plus the speed
    ((0.2 - 0.1) + (0.2 - 0.2)) / 2 = 0.05, so 0.25."""
    poses = [pose_of((0.1, 0, 0), (0, 0, 0)), pose_of((0.2, 0, 0), (1, 0, 0)),
             pose_of((0.9, 0, 0), (3, 0, 0))]
    new = tracker.motion_prediction(poses)
    assert np.allclose(new[:3, 3], (4.5, 0, 0), atol=1e-15)
    assert np.abs(new[:3, :3] - tracker.euler2mat(0.25, 0, 0)).max() <= 1e-15
    assert np.array_equal(new[3], (0, 0, 0, 1))
    # the quirk: the rotation of the last pose does not enter at all
    other = tracker.motion_prediction(poses[:2] + [pose_of((-0.4, 0.3, 1.0), (3, 0, 0))])
    assert np.array_equal(other, new)
    # only the last three poses count
    assert np.array_equal(tracker.motion_prediction([pose_of((1, 1, 1), (9, 9, 9))] + poses), new)


def test_select_pose_init_truth_table():
    last = np.eye(4)[:3]
    near = pose_of((0.05, 0, 0), (0.02, 0, 0))[:3]      # 2 cm, 2.9 deg
    jump = pose_of((0.25, 0, 0), (0.02, 0, 0))[:3]      # 14.3 deg: > 10, < 20
    jump_t = pose_of((0, 0, 0), (0.15, 0, 0))[:3]       # 15 cm
    far = pose_of((0.5, 0, 0), (0.02, 0, 0))[:3]        # 28.6 deg: > 20
    mo = "motion"
    sel = tracker.select_pose_init
    for cnt in (0, 2, 5):
        got = sel(last, near, 3.0, mo, cnt)
        assert got[0] is near and got[1] == 0
        got = sel(last, near, 10.5, mo, cnt)              # kpt_dist > 10 wins whatever else
        assert got == (mo, cnt + 1)
        got = sel(last, far, 3.0, mo, cnt)                # beyond 20: motion in both branches
        assert got == (mo, cnt + 1)
    assert sel(last, near, 10.0, mo, 0)[0] is near        # kpt_dist > 10 is strict
    for p in (jump, jump_t):
        for cnt in (0, 1, 2):
            assert sel(last, p, 3.0, mo, cnt) == (mo, cnt + 1)
        got = sel(last, p, 3.0, mo, 3)                    # use_motion_cnt reached 3: flow again
        assert got[0] is p and got[1] == 0
    assert sel(last, far, 3.0, mo, 3) == (mo, 4)


def test_cm_degree_5_metric_known_pair():
    a = pose_of((0, 0, 0), (0.01, 0.02, 0.02))[:3]
    b = pose_of((0, 0, np.deg2rad(12.0)), (0.01, -0.01, -0.02))[:3]
    t, r = tracker.cm_degree_5_metric(a, b)
    assert abs(t - 5.0) <= 1e-12 and abs(r - 12.0) <= 1e-9
    t, r = tracker.cm_degree_5_metric(a, a)
    assert t == 0.0 and r == 0.0

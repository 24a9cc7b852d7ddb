"""GPU RANSAC-EPnP (libonepose_hip) vs the C oracle (oracle/epnp_ransac.c).

Both restate OpenCV 4.4's solvePnPRansac(SOLVEPNP_EPNP) with the same cv::RNG stream, so
they must pick the same model: identical status, inlier mask and inlier count, and poses
within 1e-6 rad / 1e-6 m (both are double-precision; only operation order differs).  The
north-star bound (1e-4 rad, 1e-3 m) is asserted too.  Parity against OpenCV itself is
unpinned (cv2 is not installed); tests/test_pnp_oracle.py pins the oracle on known-answer
scenes."""
import numpy as np
import pytest
import torch

from onepose_amd import pose as P
from onepose_amd import synthetic as S
from oracle import pnp_oracle as O

pytestmark = pytest.mark.gpu


# fx != fy and cx != cy, and a different K per frame, as real OnePose crops have: with
# crop_intrinsics() (fx = fy = 600, cx = cy = 256) for every frame, a kernel that swaps the two
# focal lengths or the principal point's coordinates, or reads frame 0's K for every frame,
# gives the right answer (tests/test_pnp_oracle.py: 2 to 10 deg off under these).
K_A = np.array([[640.0, 0.0, 231.5], [0.0, 565.0, 287.25], [0.0, 0.0, 1.0]])
K_B = np.array([[310.0, 0.0, 100.0], [0.0, 295.0, 140.0], [0.0, 0.0, 1.0]])
K_0 = S.crop_intrinsics()


def scene(seed, n, outlier_frac=0.3, px_noise=0.5, K=None):
    rs = np.random.RandomState(seed)
    K = S.crop_intrinsics() if K is None else np.array(K, np.float64)
    R = S.random_rotation(rs)
    t = np.array([rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), rs.uniform(0.35, 0.55)])
    pose = np.concatenate([R, t[:, None]], 1)
    pts = rs.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    uv = S.project(K, pose, pts.astype(np.float64)) + rs.normal(0, px_noise, (n, 2))
    out = rs.rand(n) < outlier_frac
    uv[out] = rs.uniform(0, 512, (out.sum(), 2))
    p2 = uv.astype(np.float32)
    p3 = (pts.astype(np.float64) * 1000.0).astype(np.float32)
    return p2, p3, K, pose, ~out


def rot_angle(Ra, Rb):
    c = (np.trace(Ra @ Rb.T) - 1) / 2
    return np.arccos(np.clip(c, -1, 1))


def run_gpu(scenes, device, max_points=None, pad=0.0, K=None, scale=1000.0, **ransac):
    """The scenes as one batch: entries past counts[b] are `pad`; K per frame ([B,3,3], each
    scene's own), or the one shared [3,3] `K` (K_bstride 0); `ransac`: ransac_pnp_batch's
    reprojection_error / iterations_count / confidence."""
    B = len(scenes)
    M = max_points or max(s[0].shape[0] for s in scenes)
    p2 = np.full((B, M, 2), pad, np.float32)
    p3 = np.full((B, M, 3), pad, np.float32)
    Ks = np.zeros((B, 3, 3))
    counts = np.zeros(B, np.int32)
    for b, s in enumerate(scenes):
        n = s[0].shape[0]
        p2[b, :n], p3[b, :n], Ks[b], counts[b] = s[0], s[1], s[2], n
    pose, mask, nin, status = P.ransac_pnp_batch(
        torch.from_numpy(p2).to(device), torch.from_numpy(p3).to(device),
        torch.from_numpy(counts).to(device),
        torch.from_numpy(Ks if K is None else np.array(K, np.float64)).to(device), scale=scale,
        **ransac)
    torch.cuda.synchronize()
    return pose.cpu().numpy(), mask.cpu().numpy().astype(bool), nin.cpu().numpy(), status.cpu().numpy()


def oracle(s, K=None, scale=1000.0, reprojection_error=5.0, iterations_count=10000,
           confidence=0.99):
    """The C oracle on one scene, called as run_gpu calls the kernel."""
    return O.pnp_ransac(s[0], s[1], s[2] if K is None else K, scale, reprojection_error,
                        iterations_count, confidence)


def assert_frame_equals_oracle(b, got, s, want, what=""):
    """The file's bars: identical status, inlier mask and count, pose within 1e-6 rad / 1e-6 m
    of the oracle (the identity pose, bit for bit, on failure); nothing past the count."""
    pose, mask, nin, status = got
    st, opose, omask, onin, _ = want
    n = s[0].shape[0]
    assert status[b] == st, (what, b, status[b], st)
    assert nin[b] == onin, (what, b, nin[b], onin)
    np.testing.assert_array_equal(mask[b, :n], omask, err_msg=f"{what} frame {b}")
    assert not mask[b, n:].any(), (what, b)
    assert np.isfinite(pose[b]).all(), (what, b)
    if st == 0:
        assert rot_angle(pose[b, :, :3], opose[:, :3]) < 1e-6, (what, b)
        assert np.abs(pose[b, :, 3] - opose[:, 3]).max() < 1e-6, (what, b)
    else:
        np.testing.assert_array_equal(pose[b], np.eye(4)[:3], err_msg=f"{what} frame {b}")
        assert onin == 0 and not mask[b].any(), (what, b)


def degenerate_scenes():
    """100-point sets (K_A, exact projections of one pose) on which EPnP has no unique answer
    or RANSAC has nothing to find."""
    _, _, K, pose, _ = scene(700, 100, 0.0, 0.0, K=K_A)
    rs = np.random.RandomState(701)

    def corr(pts_m):
        pts_m = pts_m.astype(np.float32)
        uv = S.project(K, pose, pts_m.astype(np.float64)).astype(np.float32)
        return uv, (pts_m.astype(np.float64) * 1000.0).astype(np.float32), K, pose, None

    flat = rs.uniform(-0.1, 0.1, (100, 3))
    flat[:, 2] = 0.0
    line = np.linspace(-0.1, 0.1, 100)[:, None] * np.array([[0.6, -0.3, 0.74]])
    cloud = corr(rs.uniform(-0.1, 0.1, (10, 3)))
    return {
        "coplanar": corr(flat),
        "collinear": corr(line),
        "one_point": tuple(np.repeat(a[:1], 100, axis=0) for a in cloud[:2]) + cloud[2:],
        "all_outliers": scene(702, 100, 1.0, 0.0, K=K_A),
        "ten_by_ten": tuple(np.repeat(a, 10, axis=0) for a in cloud[:2]) + cloud[2:],
    }


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_ransac_matches_oracle(outliers, device):
    scenes = [scene(100 + i, n, outliers) for i, n in enumerate([40, 200, 700, 1024])]
    pose, mask, nin, status = run_gpu(scenes, device)
    for b, (p2, p3, K, gt, inl) in enumerate(scenes):
        st, opose, omask, onin, iters = O.pnp_ransac(p2, p3, K, scale=1000.0)
        n = p2.shape[0]
        assert status[b] == st == 0
        assert nin[b] == onin
        np.testing.assert_array_equal(mask[b, :n], omask)
        assert not mask[b, n:].any()
        assert rot_angle(pose[b, :, :3], opose[:, :3]) < 1e-6
        assert np.abs(pose[b, :, 3] - opose[:, 3]).max() < 1e-6
        # north-star bound vs the oracle, and GT recovered to the noise level
        assert rot_angle(pose[b, :, :3], gt[:, :3]) < np.deg2rad(1.0)
        assert np.abs(pose[b, :, 3] - gt[:, 3]).max() < 0.01


def collect(failures, *args):
    """assert_frame_equals_oracle, with a failure noted instead of raised (so that a batch or a
    sweep reports every case that disagrees, not the first)."""
    try:
        assert_frame_equals_oracle(*args)
    except AssertionError as e:
        failures.append(" ".join(str(e).split())[:160])


def per_frame_K_scenes():
    Ks = [K_A, K_B, K_0, K_B, K_A, K_0]
    return [scene(400 + b, n, 0.3, K=K) for b, (n, K) in
            enumerate(zip([40, 150, 300, 450, 600, 700], Ks))]


def test_ransac_per_frame_intrinsics(device):
    """Six frames, each under its own K ([B,3,3]): every frame equals the oracle under that
    frame's K.  The control: under frame 0's K the oracle keeps a different inlier set for
    frames 1-3, so a kernel reading K[0] for every frame fails here."""
    scenes = per_frame_K_scenes()
    own = [oracle(s) for s in scenes]
    for b in (1, 2, 3):
        assert (oracle(scenes[b], K=scenes[0][2])[2] != own[b][2]).any(), b
    got = run_gpu(scenes, device)
    for b, s in enumerate(scenes):
        assert own[b][0] == 0
        assert_frame_equals_oracle(b, got, s, own[b], "per-frame K")
        assert rot_angle(got[0][b, :, :3], s[3][:, :3]) < np.deg2rad(1.0)
        assert np.abs(got[0][b, :, 3] - s[3][:, 3]).max() < 0.01


def test_ransac_shared_intrinsics(device):
    """The same six frames with one shared [3,3] K_A (K_bstride 0): every frame equals the
    oracle under K_A.  Frames 0 and 4 were made under K_A; the other four are solved under a K
    they were not made with, so no pose fits them and every 5-point model is a poor one.

    This test found that a 5-point EPnP model was not a function of its five points.  Before
    canon_null2 (pnp.hip, oracle/epnp_ransac.c) frame 1 (150 points made under K_B) had status
    0 and 84 inliers on both sides but 40 of its 150 mask entries differed: M^T M of five
    points has an exactly two-dimensional null space, the kernel's eigensolver and the oracle's
    Jacobi sweeps returned different bases of it, and on subsets that no pose fits
    Gauss-Newton's five fixed iterations end at different models from different bases
    (docs/EXPERIMENTS.md section 5b).  Both now use a canonical basis of that plane."""
    scenes = per_frame_K_scenes()
    got = run_gpu(scenes, device, K=K_A)
    failures = []
    for b, s in enumerate(scenes):
        collect(failures, b, got, s, oracle(s, K=K_A), "shared K_A")
    assert not failures, "\n".join(failures)


SWEEP = [(cap, reproj, conf) for cap in (1, 10, 63, 64, 65, 100, 10000)
         for reproj in (1.0, 5.0, 20.0) for conf in (0.5, 0.99, 0.999999)]


def test_ransac_parameter_sweep(device):
    """iterations_count x reprojection_error x confidence, one launch each, on two noisy
    300-point scenes under K_A (30% and 60% outliers).  The kernel judges 64-iteration rounds
    16 iterations at a time; these reach a cap inside a round and on its boundary (10, 63, 64,
    65, 100), a cap that leaves no model (status 2), the confidence rule stopping after 5, 31
    and exactly 128 iterations, and runs of 2839 and 5678 iterations (the oracle's
    iterations_run, pinned in tests/test_pnp_oracle.py and below).

    Before canon_null2 12 of the 126 runs disagreed, all of them the 60% scene at 20 px (19
    inliers against the oracle's 20 at caps 63, 64 and 65, 29 against 30 at cap 100): there the
    best model comes from a subset with outliers in it, which no pose fits (see
    test_ransac_shared_intrinsics)."""
    scenes = [scene(5, 300, f, 0.5, K=K_A) for f in (0.3, 0.6)]
    p2 = torch.from_numpy(np.stack([s[0] for s in scenes])).to(device)
    p3 = torch.from_numpy(np.stack([s[1] for s in scenes])).to(device)
    counts = torch.tensor([300, 300], dtype=torch.int32, device=device)
    K = torch.from_numpy(np.stack([K_A, K_A])).to(device)
    seen, n_fail, failures = set(), 0, []
    for cap, reproj, conf in SWEEP:
        out = P.ransac_pnp_batch(p2, p3, counts, K, scale=1000.0, reprojection_error=reproj,
                                 iterations_count=cap, confidence=conf)
        got = (out[0].cpu().numpy(), out[1].cpu().numpy().astype(bool), out[2].cpu().numpy(),
               out[3].cpu().numpy())
        for b, s in enumerate(scenes):
            want = oracle(s, reprojection_error=reproj, iterations_count=cap, confidence=conf)
            collect(failures, b, got, s, want, f"cap {cap} reproj {reproj} conf {conf}")
            seen.add(want[4])
            n_fail += want[0] == 2
    assert {1, 5, 31, 63, 64, 65, 128} <= seen and max(seen) > 64 * 40
    assert n_fail >= 18 + 2 * 5 * 3   # cap 1 everywhere; 60% outliers at reproj 1 and 5 below 10000
    assert not failures, f"{len(failures)} of {2 * len(SWEEP)} disagree:\n" + "\n".join(failures)


@pytest.mark.parametrize("pad", [np.nan, 1e30])
def test_ransac_ignores_padding(pad, device):
    """Entries past counts[b] are never read: NaN or 1e30 there gives the bits of the
    zero-padded run, and no inlier past the count."""
    scenes = [scene(100 + i, n, 0.3) for i, n in enumerate([40, 200, 700, 1024])]
    zero = run_gpu(scenes, device)
    got = run_gpu(scenes, device, pad=pad)
    assert zero[3].tolist() == [0] * 4
    for a, b in zip(zero, got):
        assert a.tobytes() == b.tobytes()
    for b, s in enumerate(scenes):
        assert not got[1][b, s[0].shape[0]:].any()


def test_ransac_mixed_counts_in_one_batch(device):
    """Counts 0, 3, 4, 5, 6 and 300 side by side under max_points 300 (too few points, the
    P3P gate, one EPnP over all five, RANSAC), NaN past each count: each as the oracle."""
    scenes = [scene(20 + i, n, 0.0 if n < 300 else 0.3, K=K_A)
              for i, n in enumerate([0, 3, 4, 5, 6, 300])]
    got = run_gpu(scenes, device, max_points=300, pad=np.nan)
    want = [oracle(s) for s in scenes]
    assert [w[0] for w in want] == [1, 1, 0, 0, 0, 0]
    for b, s in enumerate(scenes):
        n = s[0].shape[0]
        if n == 4:   # EPnP on four points is rank-deficient: form only (the P3P gate test)
            assert got[3][b] == 0 and got[2][b] == 4 and got[1][b, :4].all()
            assert not got[1][b, 4:].any() and np.isfinite(got[0][b]).all()
            continue
        assert_frame_equals_oracle(b, got, s, want[b], "mixed counts")
    zero = run_gpu(scenes, device, max_points=300)
    for a, b in zip(zero, got):
        assert a.tobytes() == b.tobytes()


def test_ransac_max_points_limit(device):
    """onepose_pnp_max_points() is the largest max_points whose points fit in LDS beside the
    solver's state (documented in the header): one more is refused by the host check, and a
    batch of 2048, 4096 and exactly that many points (config 5 runs n1 = 2048) equals the
    oracle."""
    from onepose_amd import _lib
    limit = _lib.load().onepose_pnp_max_points()
    assert 4096 < limit < 8192
    big = scene(1, 8, 0.0)
    with pytest.raises(_lib.OnePoseError, match="onepose_pnp_max_points"):
        run_gpu([big], device, max_points=limit + 1)
    scenes = [scene(500 + b, n, 0.4, K=K_A) for b, n in enumerate([2048, 4096, limit])]
    got = run_gpu(scenes, device)
    for b, s in enumerate(scenes):
        want = oracle(s)
        assert want[0] == 0
        assert_frame_equals_oracle(b, got, s, want, "sizes")
        assert rot_angle(got[0][b, :, :3], s[3][:, :3]) < np.deg2rad(1.0)


def test_ransac_scale_one(device):
    """Points in metres and scale 1 (ransac_PnP's default): t is divided by 1."""
    p2, p3, K, gt, inl = scene(600, 200, 0.2, K=K_A)
    s = (p2, (p3.astype(np.float64) / 1000.0).astype(np.float32), K, gt, inl)
    got = run_gpu([s], device, scale=1.0)
    want = oracle(s, scale=1.0)
    assert want[0] == 0
    assert_frame_equals_oracle(0, got, s, want, "scale 1")
    assert rot_angle(got[0][0, :, :3], gt[:, :3]) < np.deg2rad(1.0)
    assert np.abs(got[0][0, :, 3] - gt[:, 3]).max() < 0.01


@pytest.mark.parametrize("name", ["coplanar", "collinear", "one_point", "all_outliers",
                                  "ten_by_ten"])
def test_degenerate_geometry_keeps_the_contract(name, device):
    """Sets on which EPnP's system is rank-deficient or RANSAC has nothing to find.  Every loop
    of the kernel on these paths has a fixed trip count (Jacobi sweeps, bisection steps, the
    iteration cap), so the call returns; the contract holds as for the 4-point gate: status 0
    or 2, finite outputs, a proper rotation, the identity pose and an empty mask on failure.
    The oracle gives status 2 after all 10000 iterations for the coplanar, collinear, one-point
    and all-outlier sets and status 0 with 100 inliers after 2 iterations for ten
    correspondences repeated ten times.  The all-outlier and repeated sets are well-conditioned
    and must equal the oracle; on coplanar and collinear points rounding decides, so agreement
    is printed (docs/EXPERIMENTS.md section 5b), not asserted."""
    s = degenerate_scenes()[name]
    want = oracle(s)
    got = run_gpu([s], device, max_points=128, pad=np.nan)
    pose, mask, nin, status = got
    assert status[0] in (0, 2)
    assert np.isfinite(pose[0]).all()
    R = pose[0, :, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0
    assert not mask[0, 100:].any() and nin[0] == mask[0].sum()
    if status[0] == 2:
        np.testing.assert_array_equal(pose[0], np.eye(4)[:3])
        assert nin[0] == 0 and not mask[0].any()
    print(f"degenerate {name}: gpu status {status[0]} inliers {nin[0]}; "
          f"oracle status {want[0]} inliers {want[3]} iterations {want[4]}")
    if name in ("all_outliers", "ten_by_ten"):
        assert want[0] == (2 if name == "all_outliers" else 0)
        assert_frame_equals_oracle(0, got, s, want, name)


def test_ransac_small_sets_and_many_rounds(device):
    """The round's cv::RNG draws are generated in parallel by jump-ahead and dealt out by one
    lane: small point sets redraw duplicates often (n = 6..16 runs past the generated draws
    into the sequential fallback), and 50-70% outliers keep RANSAC going for several
    64-iteration rounds (jump-ahead from a mid-stream state).  Same model as the oracle."""
    cases = [(6, 0.0), (7, 0.3), (9, 0.3), (12, 0.4), (16, 0.5), (60, 0.6), (300, 0.7),
             (500, 0.5)]
    scenes = [scene(300 + i, n, f) for i, (n, f) in enumerate(cases)]
    pose, mask, nin, status = run_gpu(scenes, device)
    for b, (p2, p3, K, gt, inl) in enumerate(scenes):
        st, opose, omask, onin, iters = O.pnp_ransac(p2, p3, K, scale=1000.0)
        n = p2.shape[0]
        assert status[b] == st, b
        assert nin[b] == onin, b
        np.testing.assert_array_equal(mask[b, :n], omask)
        if st == 0:
            assert rot_angle(pose[b, :, :3], opose[:, :3]) < 1e-6
            assert np.abs(pose[b, :, 3] - opose[:, 3]).max() < 1e-6
    assert O.pnp_ransac(*scenes[-2][:3], scale=1000.0)[4] > 64   # several rounds


def test_ransac_edge_counts(device):
    s5 = scene(7, 5, 0.0)
    s4 = scene(8, 4, 0.0)
    s3 = scene(9, 3, 0.0)
    s6 = scene(10, 6, 0.0)
    pose, mask, nin, status = run_gpu([s5, s4, s3, s6], device, max_points=8)
    # exactly 5 points: EPnP on all of them, every point an inlier
    st, opose, omask, onin, _ = O.pnp_ransac(s5[0], s5[1], s5[2], scale=1000.0)
    assert status[0] == 0 and nin[0] == 5 and mask[0, :5].all()
    assert rot_angle(pose[0, :, :3], opose[:, :3]) < 1e-6
    # exactly 4 points: the P3P gate passes, EPnP over all four (status / inliers as the oracle)
    st4, opose4, _, onin4, _ = O.pnp_ransac(s4[0], s4[1], s4[2], scale=1000.0)
    assert status[1] == st4 == 0 and nin[1] == onin4 == 4 and mask[1, :4].all()
    assert status[2] == P.STATUS_TOO_FEW and nin[2] == 0
    np.testing.assert_allclose(pose[2], np.eye(4)[:3])
    st6, opose6, omask6, onin6, _ = O.pnp_ransac(s6[0], s6[1], s6[2], scale=1000.0)
    assert status[3] == st6 and nin[3] == onin6


def test_drop_in_ransac_PnP(device):
    p2, p3, K, gt, inl = scene(3, 300, 0.25)
    pts3d_m = p3.astype(np.float64) / 1000.0
    pose, pose_homo, inliers = P.ransac_PnP(K, p2.astype(np.float64), pts3d_m, scale=1000)
    assert pose.shape == (3, 4) and pose_homo.shape == (4, 4)
    assert inliers.dtype == np.int32 and inliers.shape[1] == 1
    assert rot_angle(pose[:, :3], gt[:, :3]) < np.deg2rad(0.5)
    few = P.ransac_PnP(K, p2[:3], pts3d_m[:3], scale=1000)
    np.testing.assert_allclose(few[0], np.eye(4)[:3])
    assert few[2] == []


def test_four_point_p3p_gate_matches_oracle(device):
    """solvePnPRansac's 4-point branch on many scenes: exact, noisy, degenerate-looking ones (all
    image points on one pixel, solved by a far-away triangle; random sets, a few with no
    positive P3P root -> no model); status, inlier mask and count as the oracle's.  The pose
    of a 4-point solve is EPnP on a rank-deficient system (M is 8 x 12: a 4-dimensional null
    space), which amplifies rounding into degrees -- the oracle itself lands up to ~80 deg
    from the truth on exact data, and OpenCV's answer depends on its SVD -- so the pose is
    checked for form only: a finite rotation and translation."""
    scenes = [scene(200 + i, 4, 0.0 if i % 2 else 0.5) for i in range(12)]
    p2, p3, K, gt, inl = scene(7, 4, 0.0)
    scenes.append((np.repeat(p2[:1], 4, axis=0), p3, K, gt, inl))   # one pixel: a far solution
    rs = np.random.RandomState(5)
    for i in range(64):   # random 4-point sets: a few have no positive P3P solution
        q3 = rs.uniform(-100, 100, (4, 3)).astype(np.float32)
        q3[:, 2] += 400
        scenes.append((rs.uniform(0, 512, (4, 2)).astype(np.float32), q3, K, gt, inl))
    pose, mask, nin, status = run_gpu(scenes, device, max_points=4)
    n_fail = 0
    for b, (q2, q3, Kb, _, _) in enumerate(scenes):
        st, opose, omask, onin, _ = O.pnp_ransac(q2, q3, Kb, scale=1000.0)
        assert status[b] == st and nin[b] == onin, b
        np.testing.assert_array_equal(mask[b, :4], omask)
        assert np.isfinite(pose[b]).all()
        R = pose[b, :, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.linalg.det(R) > 0
        if st != 0:
            np.testing.assert_array_equal(pose[b], np.eye(4)[:3])
        n_fail += st != 0
    assert 0 < n_fail < len(scenes)

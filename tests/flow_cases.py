"""The synthetic keyframe / query pairs of the flow_track tests: about 300 points of
onepose_amd.synthetic's kind (uniform in a 0.2 m box) seen from 0.6 m, each rendered as a
Gaussian splat of its own brightness, in two poses.  ``near`` moves the object by 3 degrees and a
few millimetres, which optical flow follows; ``far`` by 35 degrees and 6 cm, which it cannot."""
import numpy as np

from onepose_amd import synthetic

SIZE, N_POINTS, SIGMA = 384, 300, 2.0


def _pose(euler_deg, t):
    from onepose_amd.tracker import euler2mat
    T = np.eye(4)
    T[:3, :3] = euler2mat(*np.deg2rad(euler_deg))
    T[:3, 3] = t
    return T


POSE_KF = _pose((20.0, -30.0, 10.0), (0.0, 0.0, 0.6))
POSES = {"near": _pose((22.0, -28.0, 11.5), (0.004, -0.003, 0.605)),
         "far": _pose((50.0, -5.0, 30.0), (0.05, 0.03, 0.62))}


def render(uv, amp):
    """uint8 [SIZE, SIZE]: background 40 plus one Gaussian per point."""
    img = np.full((SIZE, SIZE), 40.0)
    r = int(4 * SIGMA)
    for (u, v), a in zip(uv, amp):
        x0, y0 = int(round(u)), int(round(v))
        xs = np.arange(max(x0 - r, 0), min(x0 + r + 1, SIZE))
        ys = np.arange(max(y0 - r, 0), min(y0 + r + 1, SIZE))
        if len(xs) == 0 or len(ys) == 0:
            continue
        g = np.exp(-((xs[None, :] - u) ** 2 + (ys[:, None] - v) ** 2) / (2 * SIGMA ** 2))
        img[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += a * g
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pair(which, seed=3):
    """(kf_frame_info, frame_info_dict) as BATracker.flow_track reads them."""
    obj = synthetic.make_object(N_POINTS, seed=seed)
    K = synthetic.crop_intrinsics(SIZE, 600.0)
    pts3d = obj.keypoints3d.astype(np.float64)
    amp = np.random.default_rng(seed).uniform(70.0, 170.0, N_POINTS)
    uv_kf = synthetic.project(K, POSE_KF[:3], pts3d)
    uv_q = synthetic.project(K, POSES[which][:3], pts3d)
    kf = dict(im_path=render(uv_kf, amp), mkpts2d=uv_kf.astype(np.float32), mkpts3d=pts3d,
              K_crop=K, pose_gt=POSE_KF)
    query = dict(im_path=render(uv_q, amp), K_crop=K, pose_gt=POSES[which])
    return kf, query

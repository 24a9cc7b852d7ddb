"""The numeric stages of ``BATracker.track`` (src/tracker/ba_tracker.py) on libonepose_hip
(MI355X): the front half that produces ``pose_init`` (pyramidal Lucas-Kanade optical flow, the
flow -> PnP -> accept chain, motion prediction) and the back half after matching and PnP (bundle
adjustment and triangulation, float64).

* ``build_lk_pyramid`` / ``lk_track`` / ``calc_optical_flow_pyr_lk`` stand where the reference
  calls ``cv2.calcOpticalFlowPyrLK`` (:113-126); include/onepose_hip.h states the arithmetic
  (cv2 is not available here, so parity with it is pinned by known-answer scenes only).
* ``kpt_flow_track`` (:113-126), ``flow_track`` (:295-356 without the drawing),
  ``motion_prediction`` (:275-293), ``select_pose_init`` (:742-750), ``cm_degree_5_metric``
  (:105-111), ``mat2euler`` / ``euler2mat`` (transforms3d's default 'sxyz' convention).

* ``bundle_adjust`` stands where the reference calls DeepLM's ``Solve`` (:401-407): same
  arguments, variables updated in place.  The cost function is the reference's
  ``SnavelyReprojectionErrorV2`` (tracking_utils.py:142-169); the Levenberg-Marquardt on top is
  this project's own (include/onepose_hip.h states it; DeepLM's source is not part of the
  reference tree, so parity with its iterates is not verified).
* ``apply_ba`` is ``BATracker.apply_ba``'s body (:358-441) with ``win_size`` as an argument in
  place of ``self``.
* ``apply_triangulation`` / ``triangulate_filter`` replace ``cv2.triangulatePoints`` as
  ``apply_triangulation`` uses it (:267-273) and fuse track_ba's filters (:556-571).
* ``get_cam_param`` / ``get_cam_params_back`` (:443-466) with Rodrigues in numpy, ``project``
  (tracking_utils.py:74-88).

Every numeric stage of ``track`` is here; the ``BATracker`` class itself (``add_kf``,
``update_kf``, ``track_ba``'s bookkeeping) is not part of this package.  There is no CPU path:
the GPU entry points raise on CPU tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

BA_VERSION = 1
INFO_DOUBLES = 104
STATUS_OK, STATUS_FAILED, STATUS_BAD_INDEX = 0, 1, 2


def build_index(ptIdx, camIdx, n_cams: int, n_points: int):
    """onepose_ba_build_index on host arrays: (index as a uint8 numpy array, active cameras,
    active points).  Needs no GPU."""
    lib = _lib.load()
    pt = np.ascontiguousarray(ptIdx, dtype=np.int64)
    cam = np.ascontiguousarray(camIdx, dtype=np.int64)
    if pt.ndim != 1 or pt.shape != cam.shape:
        raise ValueError("ptIdx and camIdx must be 1-D and of equal length")
    nbytes = lib.onepose_ba_index_bytes(len(pt), n_cams, n_points)
    if nbytes == 0:
        raise ValueError(f"bundle_adjust: unsupported shape N={len(pt)}, C={n_cams}, P={n_points}")
    buf = np.zeros(nbytes, dtype=np.uint8)
    a, pa = ctypes.c_int(0), ctypes.c_int(0)
    _lib.run("onepose_ba_build_index", ptIdx=pt.ctypes.data, camIdx=cam.ctypes.data, n_obs=len(pt),
             n_cams=n_cams, n_points=n_points, index=buf.ctypes.data, index_bytes=nbytes,
             n_active_cams=ctypes.byref(a), n_active_points=ctypes.byref(pa))
    return buf, int(a.value), int(pa.value)


def _need_gpu(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("onepose_amd.tracker runs on a ROCm GPU only; move the inputs "
                               "with .cuda()")


def _f64(t, shape, name):
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape[1:]) != shape:
        raise ValueError(f"{name}: expected a contiguous float64 tensor [n, "
                         f"{', '.join(map(str, shape))}], got {t.dtype} {tuple(t.shape)}")


def bundle_adjust(points, cam_pose, features, ptIdx, camIdx, numIterations=5,
                  numSuccessIterations=5, initial_radius=1e4, index=None):
    """``Solve(variables=[points, cam_pose], constants=[features], indices=[ptIdx, camIdx],
    fn=SnavelyReprojectionErrorV2, ...)``: CUDA float64 ``points [P,3]``, ``cam_pose [C,6]``
    (updated in place), ``features [N,5]``, int64 ``ptIdx`` / ``camIdx [N]``.  Returns the info
    block (float64 [104] on the device; layout in include/onepose_hip.h).  The index structures
    are sorted on the host, which copies the two index tensors back once; pass ``index`` (the
    triple of ``build_index``) when they are already at hand there, as in ``apply_ba``."""
    _need_gpu(points, cam_pose, features, ptIdx, camIdx)
    _f64(points, (3,), "points")
    _f64(cam_pose, (6,), "cam_pose")
    _f64(features, (5,), "features")
    if ptIdx.dtype != torch.int64 or camIdx.dtype != torch.int64:
        raise ValueError("ptIdx and camIdx must be int64")
    ptIdx, camIdx = ptIdx.contiguous(), camIdx.contiguous()
    N, C, P = features.shape[0], cam_pose.shape[0], points.shape[0]
    if ptIdx.shape != (N,) or camIdx.shape != (N,):
        raise ValueError("ptIdx and camIdx must have one entry per row of features")
    if index is None:
        index = build_index(ptIdx.cpu().numpy(), camIdx.cpu().numpy(), C, P)
    buf, A, Pa = index
    lib = _lib.load()
    dev = points.device
    if A > lib.onepose_ba_max_active_cameras():
        raise ValueError(f"bundle_adjust: {A} cameras carry observations, at most "
                         f"{lib.onepose_ba_max_active_cameras()} are supported")
    with torch.cuda.device(dev):
        ix = torch.from_numpy(buf).to(dev)
        ws = torch.empty(lib.onepose_ba_workspace_bytes(N, A, Pa), dtype=torch.uint8, device=dev)
        info = torch.empty(INFO_DOUBLES, dtype=torch.float64, device=dev)
        _lib.run("onepose_ba_solve", points=points, cam_pose=cam_pose, features=features,
                 ptIdx=ptIdx, camIdx=camIdx, index=ix, n_obs=N, n_cams=C, n_points=P,
                 n_active_cams=A, n_active_points=Pa, max_iters=int(numIterations),
                 max_success=int(numSuccessIterations), initial_radius=float(initial_radius),
                 info=info, workspace=ws, workspace_bytes=ws.numel(), stream=_lib.stream_ptr(dev))
    return info


def ba_window(kpt2ds, kpt2d3d_ids, kpt2d_fids, cams, win_size):
    """The host half of ``apply_ba`` (:362-370): the observations with a 3D point, inside the
    window ``fids > max - win_size`` once ``max > win_size`` -> (features [N,5], ptIdx, camIdx,
    valid2d_idx)."""
    valid2d_idx = np.where(kpt2d3d_ids != -1)[0]
    if np.max(kpt2d_fids) > win_size:
        valid_idx_fid = np.where(kpt2d_fids > np.max(kpt2d_fids) - win_size)
        valid2d_idx = np.intersect1d(valid_idx_fid, valid2d_idx)
    fids = np.array(kpt2d_fids[valid2d_idx], dtype=int)
    ks = cams[fids, 6:]
    features = np.concatenate([kpt2ds[valid2d_idx], ks], axis=1).astype(np.float64)
    return (features, np.asarray(kpt2d3d_ids[valid2d_idx], dtype=np.int64),
            fids.astype(np.int64), valid2d_idx)


def apply_ba(kpt2ds, kpt2d3d_ids, kpt2d_fids, kpt3d_list, cams, win_size, verbose=False,
             device="cuda"):
    """``BATracker.apply_ba``: numpy in, ``(points_opt_np, cam_opt)`` out, with ``cam_opt`` the
    optimised ``cams[:, :6]`` beside the untouched intrinsics ``cams[:, 6:]``."""
    if not torch.cuda.is_available():
        raise RuntimeError("onepose_amd.tracker runs on a ROCm GPU only")
    cams = np.asarray(cams, dtype=np.float64)
    features, pt_idx, cam_idx, _ = ba_window(kpt2ds, kpt2d3d_ids, kpt2d_fids, cams, win_size)
    points = torch.tensor(np.asarray(kpt3d_list), device=device, dtype=torch.float64)
    cam_pose = torch.tensor(cams[:, :6], device=device, dtype=torch.float64)
    index = build_index(pt_idx, cam_idx, cam_pose.shape[0], points.shape[0])
    info = bundle_adjust(points, cam_pose, torch.from_numpy(features).to(device),
                         torch.from_numpy(pt_idx).to(device), torch.from_numpy(cam_idx).to(device),
                         5, 5, index=index)
    if verbose:
        h = info.cpu().numpy()
        print(f"BA status {int(h[0])}: {int(h[1])} iterations, {int(h[2])} accepted, "
              f"cost {h[3]:.6g} -> {h[4]:.6g}")
    points_opt_np = points.cpu().numpy()
    cam_opt = np.concatenate([cam_pose.cpu().numpy(), cams[:, 6:]], axis=1)
    return points_opt_np, cam_opt


def triangulate_filter(K1, K2, Tcw1, Tcw2, kpt2d_1, kpt2d_2, rep_thr=20.0, z_max=0.15,
                       device="cuda"):
    """Triangulation with track_ba's filters (:556-571): ``(point_3d_w [n,3], keep [n] bool,
    err1, err2)`` as numpy arrays.  ``keep`` = both reprojection errors <= ``rep_thr`` and z <=
    ``z_max`` and a finite point."""
    if not torch.cuda.is_available():
        raise RuntimeError("onepose_amd.tracker runs on a ROCm GPU only")
    P1 = np.dot(K1, np.linalg.inv(Tcw1)[:3, :])
    P2 = np.dot(K2, np.linalg.inv(Tcw2)[:3, :])
    out = triangulate_points(torch.as_tensor(P1, dtype=torch.float64, device=device),
                             torch.as_tensor(P2, dtype=torch.float64, device=device),
                             torch.as_tensor(np.asarray(kpt2d_1), dtype=torch.float64,
                                             device=device),
                             torch.as_tensor(np.asarray(kpt2d_2), dtype=torch.float64,
                                             device=device), rep_thr, z_max)
    return (out["points"].cpu().numpy(), out["keep"].cpu().numpy().astype(bool),
            out["err1"].cpu().numpy(), out["err2"].cpu().numpy())


def apply_triangulation(K1, K2, Tcw1, Tcw2, kpt2d_1, kpt2d_2):
    """``BATracker.apply_triangulation``: the [n,3] points alone."""
    return triangulate_filter(K1, K2, Tcw1, Tcw2, kpt2d_1, kpt2d_2)[0]


def triangulate_points(P1, P2, pts1, pts2, rep_thr=20.0, z_max=0.15):
    """onepose_triangulate on device tensors: float64 ``P1, P2 [3,4]``, ``pts1, pts2 [n,2]`` ->
    dict of points [n,3], err1, err2, z [n] float64 and keep [n] uint8."""
    _need_gpu(P1, P2, pts1, pts2)
    for t, shape, name in ((P1, (3, 4), "P1"), (P2, (3, 4), "P2")):
        if t.dtype != torch.float64 or tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected float64 [3, 4]")
    _f64(pts1, (2,), "pts1")
    _f64(pts2, (2,), "pts2")
    n = pts1.shape[0]
    if pts2.shape[0] != n:
        raise ValueError("pts1 and pts2 differ in length")
    dev = pts1.device
    P1, P2 = P1.contiguous(), P2.contiguous()
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        out = {"points": torch.empty(n, 3, **f64), "err1": torch.empty(n, **f64),
               "err2": torch.empty(n, **f64), "z": torch.empty(n, **f64),
               "keep": torch.empty(n, dtype=torch.uint8, device=dev)}
        _lib.run("onepose_triangulate", P1=P1, P2=P2, pts1=pts1, pts2=pts2, n=n,
                 rep_thr=float(rep_thr), z_max=float(z_max), X=out["points"], err1=out["err1"],
                 err2=out["err2"], z=out["z"], keep=out["keep"], stream=_lib.stream_ptr(dev))
    return out


def rodrigues(r):
    """cv2.Rodrigues in numpy, both ways: a 3-vector gives the 3 x 3 matrix, a 3 x 3 rotation its
    [3,1] vector (the shape cv2 returns)."""
    r = np.asarray(r, dtype=np.float64)
    if r.shape == (3, 3):
        cos = np.clip((np.trace(r) - 1.0) / 2.0, -1.0, 1.0)
        ax = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
        s = np.linalg.norm(ax) / 2.0
        th = np.arctan2(s, cos)   # accurate at small angles and near pi, where arccos is not
        if s < 1e-10:
            if cos > 0:
                return np.zeros((3, 1))
            d = np.sqrt(np.maximum((np.diag(r) + 1.0) / 2.0, 0.0))   # theta = pi: R = 2 k k^T - I
            if d[0] >= d[1] and d[0] >= d[2]:
                d[1:] *= np.sign([r[0, 1], r[0, 2]]) + (np.array([r[0, 1], r[0, 2]]) == 0)
            elif d[1] >= d[2]:
                sg = np.sign([r[0, 1], r[1, 2]]) + (np.array([r[0, 1], r[1, 2]]) == 0)
                d[0] *= sg[0]
                d[2] *= sg[1]
            else:
                d[:2] *= np.sign([r[0, 2], r[1, 2]]) + (np.array([r[0, 2], r[1, 2]]) == 0)
            return (th * d / np.linalg.norm(d)).reshape(3, 1)
        return (ax / (2.0 * s) * th).reshape(3, 1)
    r = r.reshape(3)
    th = np.linalg.norm(r)
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def get_cam_params_back(cam_params):
    """BAL format (rvec, t, f, cx, cy) -> (K, 4 x 4 pose) (:443-457)."""
    f, k1, k2 = cam_params[6], cam_params[7], cam_params[8]
    K = np.array([[f, 0, k1], [0, f, k2], [0, 0, 1]])
    pose_mat = np.eye(4)
    pose_mat[:3, :3] = rodrigues(cam_params[:3])
    pose_mat[:3, 3] = cam_params[3:6]
    return K, pose_mat


def get_cam_param(K, pose):
    """(K, pose) -> BAL format (:459-466)."""
    R = rodrigues(pose[:3, :3])
    return np.concatenate([R.flatten(), pose[:3, 3], [K[0, 0], K[0, 2], K[1, 2]]])


def project(xyz, K, RT, need_depth=False):
    """tracking_utils.project (:74-88)."""
    xyz = np.dot(xyz, RT[:, :3].T) + RT[:, 3:].T
    depth = xyz[:, 2:].flatten()
    xyz = np.dot(xyz, K.T)
    xy = xyz[:, :2] / xyz[:, 2:]
    return (xy, depth) if need_depth else xy


# ---- the front half of BATracker.track: optical flow, flow_track, motion prediction ----

LK_VERSION = 1
TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2   # cv2.TERM_CRITERIA_*


class LKPyramid:
    """The blob(s) of ``onepose_lk_build_pyramid`` with the shape they were built for: ``blob``
    uint8 [B, pyramid_bytes] on the device.  ``level(l)`` gives plain views of it."""

    def __init__(self, blob, h, w, win, max_level, with_deriv):
        self.blob, self.h, self.w, self.win, self.max_level = blob, h, w, win, max_level
        self.with_deriv = bool(with_deriv)
        self.levels = _lib.load().onepose_lk_levels(h, w, win, max_level)

    @property
    def batch(self):
        return self.blob.shape[0]

    def level(self, l):
        """(image uint8 [B, lh, lw], derivative int16 [B, lh, lw, 2]) of level ``l``."""
        lh, lw, io, do = lk_pyramid_layout(self.h, self.w, self.win, self.max_level, l)
        img = self.blob[:, io:io + lh * lw].view(self.batch, lh, lw)
        der = self.blob[:, do:do + lh * lw * 4].view(torch.int16).view(self.batch, lh, lw, 2)
        return img, der


def lk_pyramid_layout(h, w, win, max_level, level):
    """onepose_lk_pyramid_layout (a host function): (lh, lw, image offset, derivative offset)."""
    lh, lw = ctypes.c_int(0), ctypes.c_int(0)
    io, do = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.run("onepose_lk_pyramid_layout", h=h, w=w, win=win, max_level=max_level, level=level,
             lh=ctypes.byref(lh), lw=ctypes.byref(lw), image_offset=ctypes.byref(io),
             deriv_offset=ctypes.byref(do))
    return int(lh.value), int(lw.value), int(io.value), int(do.value)


def build_lk_pyramid(image_u8, win=15, max_level=2, with_deriv=True):
    """The image pyramid (and, with ``with_deriv``, its Scharr derivatives) of a CUDA uint8 image
    ``[h, w]`` or batch ``[B, h, w]`` -> ``LKPyramid``.  Build a keyframe's once and reuse it for
    every frame tracked against it; the second image of a pair needs no derivatives."""
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 \
            or image_u8.dim() not in (2, 3):
        raise ValueError("build_lk_pyramid: expected a uint8 tensor [h, w] or [B, h, w]")
    _need_gpu(image_u8)
    img = image_u8[None] if image_u8.dim() == 2 else image_u8
    img = img.contiguous()
    B, h, w = img.shape
    lib = _lib.load()
    nbytes = lib.onepose_lk_pyramid_bytes(h, w, int(win), int(max_level))
    if nbytes == 0 or B == 0:
        raise ValueError(f"build_lk_pyramid: unsupported h={h} w={w} win={win} "
                         f"max_level={max_level} (win odd in 3..31, max_level in 0..5, "
                         "win < h, w <= 8192)")
    dev = img.device
    with torch.cuda.device(dev):
        blob = torch.empty(B, nbytes, dtype=torch.uint8, device=dev)
        _lib.run("onepose_lk_build_pyramid", image=img, image_bstride=h * w, batch=B, h=h, w=w,
                 win=int(win), max_level=int(max_level), with_deriv=int(bool(with_deriv)),
                 pyramids=blob, stream=_lib.stream_ptr(dev))
    return LKPyramid(blob, h, w, int(win), int(max_level), with_deriv)


def lk_track(prev_pyr, next_pyr, prev_pts, counts=None, max_count=10, epsilon=0.03,
             min_eig_threshold=1e-4):
    """onepose_lk_track: ``prev_pts`` CUDA float32 ``[n, 2]`` or ``[B, n, 2]`` tracked from
    ``prev_pyr`` (built with derivatives) into each image of ``next_pyr`` -> ``(next_pts
    [B, n, 2] float32, status [B, n] uint8)`` with B = ``next_pyr.batch``.  A ``prev_pyr`` of one
    image and 2-D ``prev_pts`` are shared by the batch.  ``counts`` (CUDA int32 [B]) limits the
    points of each item; the rows beyond keep ``prev_pts`` and status 0."""
    if not isinstance(prev_pyr, LKPyramid) or not isinstance(next_pyr, LKPyramid):
        raise ValueError("lk_track: prev_pyr and next_pyr come from build_lk_pyramid")
    if (prev_pyr.h, prev_pyr.w, prev_pyr.win, prev_pyr.max_level) != \
            (next_pyr.h, next_pyr.w, next_pyr.win, next_pyr.max_level):
        raise ValueError("lk_track: the two pyramids differ in shape, window or levels")
    if not prev_pyr.with_deriv:
        raise ValueError("lk_track: prev_pyr was built without derivatives")
    if not isinstance(prev_pts, torch.Tensor) or prev_pts.dtype != torch.float32 \
            or prev_pts.dim() not in (2, 3) or prev_pts.shape[-1] != 2:
        raise ValueError("lk_track: prev_pts must be float32 [n, 2] or [B, n, 2]")
    _need_gpu(prev_pts, prev_pyr.blob, next_pyr.blob)
    B, n = next_pyr.batch, prev_pts.shape[-2]
    if prev_pyr.batch not in (1, B):
        raise ValueError(f"lk_track: prev_pyr holds {prev_pyr.batch} images, next_pyr {B}")
    if prev_pts.dim() == 3 and prev_pts.shape[0] not in (1, B):
        raise ValueError(f"lk_track: prev_pts holds {prev_pts.shape[0]} items, next_pyr {B}")
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                               or tuple(counts.shape) != (B,)):
        raise ValueError("lk_track: counts must be an int32 tensor [B]")
    prev_pts = prev_pts.contiguous()
    shared_pts = prev_pts.dim() == 2 or prev_pts.shape[0] == 1
    dev = prev_pts.device
    with torch.cuda.device(dev):
        if counts is None:
            counts = torch.full((B,), n, dtype=torch.int32, device=dev)
            next_pts = torch.empty(B, n, 2, dtype=torch.float32, device=dev)
            status = torch.empty(B, n, dtype=torch.uint8, device=dev)
        else:
            _need_gpu(counts)
            next_pts = prev_pts.reshape(-1, n, 2).expand(B, n, 2).clone()
            status = torch.zeros(B, n, dtype=torch.uint8, device=dev)
        _lib.run("onepose_lk_track", prev_pyr=prev_pyr.blob,
                 prev_pyr_bstride=0 if prev_pyr.batch == 1 else prev_pyr.blob.shape[1],
                 next_pyr=next_pyr.blob, prev_pts=prev_pts,
                 prev_pts_bstride=0 if shared_pts else 2 * n, counts=counts, batch=B,
                 max_points=n, h=prev_pyr.h, w=prev_pyr.w, win=prev_pyr.win,
                 max_level=prev_pyr.max_level, max_count=int(max_count), epsilon=float(epsilon),
                 min_eig_threshold=float(min_eig_threshold), next_pts=next_pts, status=status,
                 stream=_lib.stream_ptr(dev))
    return next_pts, status


def _lk_criteria(criteria):
    """cv2's TermCriteria as calcOpticalFlowPyrLK reads it: without COUNT the count is 30,
    without EPS the epsilon is 0.001."""
    kind, count, eps = criteria
    return (int(count) if int(kind) & TERM_CRITERIA_COUNT else 30,
            float(eps) if int(kind) & TERM_CRITERIA_EPS else 0.001)


def _as_gray_gpu(img, device, name):
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError(f"{name}: expected an 8-bit single-channel image [h, w], got "
                             f"{img.dtype} {img.shape}")
        return torch.from_numpy(np.ascontiguousarray(img)).to(device)
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 2:
        raise ValueError(f"{name}: expected an 8-bit single-channel image [h, w]")
    _need_gpu(img)
    return img


def _check_win(winSize):
    if len(winSize) != 2 or winSize[0] != winSize[1]:
        raise ValueError(f"winSize {tuple(winSize)}: only square windows are supported")
    return int(winSize[0])


def calc_optical_flow_pyr_lk(prev_img, next_img, prev_pts, winSize=(15, 15), maxLevel=2,
                             criteria=(3, 10, 0.03), minEigThreshold=1e-4, kf_pyramid=None,
                             device="cuda"):
    """``cv2.calcOpticalFlowPyrLK(prev_img, next_img, prev_pts, None, winSize=, maxLevel=,
    criteria=, minEigThreshold=)`` -> ``(next_pts [n, 1, 2] float32, status [n, 1] uint8,
    None)``: numpy in gives numpy out, CUDA tensors in give CUDA tensors out.  ``prev_pts`` is
    ``[n, 1, 2]`` or ``[n, 2]``.  cv2's ``err`` is not produced and its flags are not supported.
    Two arguments are this package's own: ``kf_pyramid`` (an ``LKPyramid`` of ``prev_img`` with
    derivatives, same window and levels) spares rebuilding it, and ``prev_img`` is then not
    read; ``device`` is where numpy inputs are uploaded to (tensor inputs stay where they
    are)."""
    win = _check_win(winSize)
    max_count, eps = _lk_criteria(criteria)
    as_numpy = not isinstance(prev_pts, torch.Tensor)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("onepose_amd.tracker runs on a ROCm GPU only")
        pts = np.ascontiguousarray(prev_pts, dtype=np.float32)
        if pts.size % 2:
            raise ValueError("prev_pts must be [n, 1, 2] or [n, 2]")
        pts = torch.from_numpy(pts.reshape(-1, 2)).to(device)
    else:
        _need_gpu(prev_pts)
        if prev_pts.dtype != torch.float32 or prev_pts.numel() % 2:
            raise ValueError("prev_pts must be float32 [n, 1, 2] or [n, 2]")
        pts = prev_pts.reshape(-1, 2)
    dev = pts.device
    nxt = build_lk_pyramid(_as_gray_gpu(next_img, dev, "next_img"), win, maxLevel, False)
    if kf_pyramid is None:
        kf_pyramid = build_lk_pyramid(_as_gray_gpu(prev_img, dev, "prev_img"), win, maxLevel, True)
    n = pts.shape[0]
    if n == 0:
        out = torch.empty(0, 1, 2, dtype=torch.float32, device=dev)
        st = torch.empty(0, 1, dtype=torch.uint8, device=dev)
    else:
        o, s = lk_track(kf_pyramid, nxt, pts, None, max_count, eps, minEigThreshold)
        out, st = o.reshape(n, 1, 2), s.reshape(n, 1)
    if as_numpy:
        return out.cpu().numpy(), st.cpu().numpy(), None
    return out, st, None


def kpt_flow_track(im_kf, im_query, kpt2d_last, kf_pyramid=None):
    """``BATracker.kpt_flow_track`` (:113-126): winSize 15 x 15, maxLevel 2, criteria (EPS | COUNT,
    10, 0.03) -> ``(kpt_new [n, 2], valid_id)`` with ``valid_id`` the ``np.where`` tuple of status
    == 1.  ``kf_pyramid``: the keyframe's ``build_lk_pyramid(im_kf)``, built once per keyframe."""
    kpt_last = np.expand_dims(np.asarray(kpt2d_last, dtype=np.float32), axis=1)
    kpt_new, status, _ = calc_optical_flow_pyr_lk(
        im_kf, im_query, kpt_last, winSize=(15, 15), maxLevel=2,
        criteria=(TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, 10, 0.03), kf_pyramid=kf_pyramid)
    valid_id = np.where(status.flatten() == 1)
    return np.squeeze(kpt_new, axis=1), valid_id


def cm_degree_5_metric(pose_pred, pose_target):
    """The tracker's pose distance (``BATracker.cm_degree_5_metric``, :105-111) between two
    ``[3, 4]`` (or 4 x 4, first three rows) poses: (translation distance in cm, rotation angle in
    degrees).  As in the reference the trace is limited from above only (and NaN counts as 3), so
    a trace below -1 gives NaN."""
    P, G = np.asarray(pose_pred)[:3], np.asarray(pose_target)[:3]
    cm = 100 * np.linalg.norm(P[:, 3] - G[:, 3])
    tr = (P[:, :3] @ G[:, :3].T).trace()
    cos_angle = (tr - 1.0) / 2.0 if tr <= 3 else 1.0
    return cm, np.degrees(np.arccos(cos_angle))


ACCEPT_CM = ACCEPT_DEG = 7.0   # flow_track's acceptance rule (:351)
ACCEPT_KPT_DIST = 10.0


def flow_track(frame_info_dict, kf_frame_info):
    """What ``BATracker.flow_track`` (:295-356) computes, without its drawing and timers: the
    keyframe's ``mkpts2d`` are followed into the query image by optical flow, the points that
    kept status 1 go with their ``mkpts3d`` through ``pose.ransac_PnP`` (``K_crop`` of the query,
    scale 1), and the pose is judged by the mean reprojection distance of those points and by its
    cm / degree distance to the query's ``pose_gt``.  Returns ``(pose_init_homo [4, 4], kpt_dist,
    accepted)``; accepted means at most 7 cm and 7 degrees and ``kpt_dist`` below 10 px, and then
    ``mkpts3d`` / ``mkpts2d`` (the tracked subset) are written into ``frame_info_dict``, which
    the caller keeps as its ``last_kf_info``.

    There is no image loader here: the caller puts the images themselves, uint8 ``[h, w]`` numpy
    arrays or CUDA tensors, under the reference's key ``im_path`` of both dicts.  An optional
    ``lk_pyramid`` entry of ``kf_frame_info`` is the keyframe's ``build_lk_pyramid`` result,
    built once per keyframe."""
    from . import pose as _pose
    K = frame_info_dict["K_crop"]
    tracked, keep = kpt_flow_track(kf_frame_info["im_path"], frame_info_dict["im_path"],
                                   kf_frame_info["mkpts2d"], kf_frame_info.get("lk_pyramid"))
    pts2d, pts3d = tracked[keep], kf_frame_info["mkpts3d"][keep]
    pose34, pose44, _ = _pose.ransac_PnP(K, pts2d, pts3d)
    residual = project(pts3d, K, pose34) - pts2d
    kpt_dist = np.linalg.norm(residual, axis=1).mean()
    cm, deg = cm_degree_5_metric(pose44, frame_info_dict["pose_gt"])
    accepted = bool(cm <= ACCEPT_CM and deg <= ACCEPT_DEG and kpt_dist < ACCEPT_KPT_DIST)
    if accepted:
        frame_info_dict["mkpts3d"], frame_info_dict["mkpts2d"] = pts3d, pts2d
    return pose44, kpt_dist, accepted


_EULER_EPS4 = float(np.finfo(np.float64).eps) * 4.0


def mat2euler(R):
    """transforms3d.euler.mat2euler with its default axes 'sxyz': (ax, ay, az) with
    R = Rz(az) Ry(ay) Rx(ax); at the gimbal lock (cy <= 4 eps) az = 0."""
    R = np.asarray(R, dtype=np.float64)[:3, :3]
    cy = np.hypot(R[0, 0], R[1, 0])
    if cy > _EULER_EPS4:
        ax = np.arctan2(R[2, 1], R[2, 2])
        ay = np.arctan2(-R[2, 0], cy)
        az = np.arctan2(R[1, 0], R[0, 0])
    else:
        ax = np.arctan2(-R[1, 2], R[1, 1])
        ay = np.arctan2(-R[2, 0], cy)
        az = 0.0
    return float(ax), float(ay), float(az)


def euler2mat(ax, ay, az):
    """transforms3d.euler.euler2mat with its default axes 'sxyz': Rz(az) Ry(ay) Rx(ax)."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def motion_prediction(pose_list):
    """Constant-velocity extrapolation of the last three 4 x 4 poses, as
    ``BATracker.motion_prediction`` (:275-293) computes it: the translation of the last pose
    advanced by the mean of the last two translation steps, and Euler angles ('sxyz') advanced
    the same way.  The reference's quirk is kept: the angles it advances, its ``rot_t``, are
    read from ``pose_list[-2]``, not ``[-1]`` (:285).  So the second angle step is zero, the
    last pose's rotation never enters, and the result is the rotation of the pose before last
    plus half the step that led to it."""
    first, second, last = (np.asarray(p, dtype=np.float64) for p in pose_list[-3:])
    t0, t1, t2 = first[:3, 3], second[:3, 3], last[:3, 3]
    e0 = np.array(mat2euler(first))
    e1 = np.array(mat2euler(second))
    e2 = e1   # the quirk: not mat2euler(last)
    out = np.eye(4)
    out[:3, :3] = euler2mat(*(e2 + ((e1 - e0) + (e2 - e1)) / 2))
    out[:3, 3] = t2 + ((t1 - t0) + (t2 - t1)) / 2
    return out


JUMP, LOST = 10.0, 20.0   # cm and degrees against the last pose (:742, :745)
MAX_MOTION_FRAMES = 3


def select_pose_init(pose_last, pose_ftk, kpt_dist, pose_mo, use_motion_cnt):
    """Which pose starts the frame (``BATracker.track``, :734-750): the flow pose ``pose_ftk`` or
    the motion-predicted ``pose_mo`` -> ``(pose_init, use_motion_cnt)``.  The flow pose is
    measured against ``pose_last`` in cm / degrees.  A jump (more than 10 on either) is answered
    with the motion pose for at most 3 frames in a row; a keypoint distance above 10 px always
    is; otherwise the flow pose is taken while both distances are below 20, and the motion pose
    beyond.  Taking the motion pose counts ``use_motion_cnt`` up, the flow pose resets it."""
    cm, deg = cm_degree_5_metric(pose_last, pose_ftk)
    jumped = cm > JUMP or deg > JUMP
    distrust_flow = kpt_dist > ACCEPT_KPT_DIST or (jumped and use_motion_cnt < MAX_MOTION_FRAMES)
    if not distrust_flow and cm < LOST and deg < LOST:
        return pose_ftk, 0
    return pose_mo, use_motion_cnt + 1

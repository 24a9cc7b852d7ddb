"""The numeric stages of ``BATracker.track_ba`` (src/tracker/ba_tracker.py) after matching and
PnP, on libonepose_hip (MI355X): bundle adjustment and triangulation, float64.

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

The ``BATracker`` class itself, LK optical flow and motion prediction are not part of this
package.  There is no CPU path: the GPU entry points raise on CPU tensors.
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
    _lib.check(lib.onepose_ba_build_index(pt.ctypes.data, cam.ctypes.data, len(pt), n_cams,
                                          n_points, buf.ctypes.data, nbytes, ctypes.byref(a),
                                          ctypes.byref(pa)), "onepose_ba_build_index")
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
        rc = lib.onepose_ba_solve(points.data_ptr(), cam_pose.data_ptr(), features.data_ptr(),
                                  ptIdx.data_ptr(), camIdx.data_ptr(), ix.data_ptr(), N, C, P, A,
                                  Pa, int(numIterations), int(numSuccessIterations),
                                  float(initial_radius), info.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "onepose_ba_solve")
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
    lib = _lib.load()
    dev = pts1.device
    P1, P2 = P1.contiguous(), P2.contiguous()
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        out = {"points": torch.empty(n, 3, **f64), "err1": torch.empty(n, **f64),
               "err2": torch.empty(n, **f64), "z": torch.empty(n, **f64),
               "keep": torch.empty(n, dtype=torch.uint8, device=dev)}
        rc = lib.onepose_triangulate(P1.data_ptr(), P2.data_ptr(), pts1.data_ptr(),
                                     pts2.data_ptr(), n, float(rep_thr), float(z_max),
                                     out["points"].data_ptr(), out["err1"].data_ptr(),
                                     out["err2"].data_ptr(), out["z"].data_ptr(),
                                     out["keep"].data_ptr(), _lib.stream_ptr(dev))
        _lib.check(rc, "onepose_triangulate")
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

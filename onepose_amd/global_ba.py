"""Global bundle adjustment of an SfM model (``include/onepose_global_ba.h``).

The reference's last SfM stage, ``src/sfm/global_ba.py``, shells out to COLMAP's
``bundle_adjuster`` (extrinsics refined, intrinsics fixed).  **This project's own** solver takes
its place: Levenberg-Marquardt on the tracker's angle-axis reprojection cost with fx != fy, the
camera step by preconditioned CG on the implicit Schur complement.  No parity with COLMAP or
Ceres is claimed; no robust loss, no refinement of intrinsics, no filtering or re-triangulation
afterwards.

``global_bundle_adjust`` takes ``device=``: with a GPU device the kernels of
``csrc/global_ba.hip`` run; with ``device=None`` the same contract runs in numpy float64 on the
host (it need not give the GPU's bits).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

INFO_HEAD, INFO_ROW = 8, 8
STATUS = {0: "ran", 1: "non-finite initial cost", 2: "bad index", 3: "converged",
          4: "radius underflow"}
CG_REASONS = {0: "not run", 1: "tolerance", 2: "iteration cap", 3: "p.Sp <= 0", 4: "non-finite",
              5: "zero right-hand side"}
MIN_RHO, SERIES_TH2, MIN_RADIUS = 1e-3, 1e-4, 1e-32
MAX_STEPS_PER_CALL, MAX_INFO_ROWS = 1024, 65536


# ------------------------------------------------------------------ poses
def qvec2aa(q):
    """Angle-axis [n, 3] of unit quaternions (w, x, y, z) [n, 4], angle in [0, pi]."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    q = np.where(q[:, :1] < 0, -q, q)
    n = np.linalg.norm(q[:, 1:], axis=1)
    ang = 2.0 * np.arctan2(n, q[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(n > 1e-150, ang / n, 2.0 / np.maximum(q[:, 0], 1e-300))
    return q[:, 1:] * k[:, None]


def aa2qvec(aa):
    """Unit quaternions (w, x, y, z) [n, 4], w >= 0, of angle-axis vectors [n, 3]."""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(aa, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(th > 1e-8, np.sin(0.5 * th) / th, 0.5 - th * th / 48.0)
    q = np.concatenate([np.cos(0.5 * th)[:, None], aa * k[:, None]], axis=1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.where(q[:, :1] < 0, -q, q)


# ------------------------------------------------------------------ the host path
def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def fixed_bits(fixed, n_cams):
    if fixed is None:
        return np.zeros((n_cams, 6), bool)
    f = np.asarray(fixed, np.uint8).reshape(-1)
    return (f[:, None] >> np.arange(6)[None, :] & 1).astype(bool)


def linearize(points, cams, K4, xy, pt_idx, cam_idx, fixed=None, jac=True):
    """The header's cost function: residuals [N, 2] and, with ``jac``, Jc [N, 2, 6] (fixed
    columns zeroed) and Jp [N, 2, 3]."""
    X = points[pt_idx]
    w, t = cams[cam_idx, :3], cams[cam_idx, 3:6]
    fx, fy, cx, cy = (K4[cam_idx, i] for i in range(4))
    th2 = (w * w).sum(1)
    pos = th2 > 0
    th = np.sqrt(np.where(pos, th2, 1.0))
    c, s = np.cos(th), np.sin(th)
    k = w / th[:, None]
    p_rod = (X * c[:, None] + np.cross(k, X) * s[:, None]
             + k * ((k * X).sum(1) * (1.0 - c))[:, None])
    wx = np.cross(w, X)
    p = np.where(pos[:, None], p_rod, X + wx) + t
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = np.stack([fx * xp + cx - xy[:, 0], fy * yp + cy - xy[:, 1]], 1)
    if not jac:
        return r
    a = np.where(pos, s / th, 1.0)
    big = th2 >= SERIES_TH2
    den = np.where(big, th2, 1.0)
    b = np.where(big, (1.0 - c) / den, 0.5 + th2 * (-1.0 / 24.0 + th2 * (1.0 / 720.0)))
    ca = np.where(big, (c - a) / den, -1.0 / 3.0 + th2 * (1.0 / 30.0 + th2 * (-1.0 / 840.0)))
    ab = np.where(big, (a - 2.0 * b) / den,
                  -1.0 / 12.0 + th2 * (1.0 / 180.0 + th2 * (-1.0 / 6720.0)))
    b, ca, ab = np.where(pos, b, 0.0), np.where(pos, ca, 0.0), np.where(pos, ab, 0.0)
    cc = np.where(pos, c, 1.0)
    eye = np.eye(3)[None]
    wd = (w * X).sum(1)
    Wx, Xx = _skew(w), _skew(X)
    ww = w[:, :, None] * w[:, None, :]
    R = cc[:, None, None] * eye + a[:, None, None] * Wx + b[:, None, None] * ww
    M = (-a[:, None, None] * (X[:, :, None] * w[:, None, :])
         + ca[:, None, None] * (wx[:, :, None] * w[:, None, :])
         - a[:, None, None] * Xx
         + b[:, None, None] * (w[:, :, None] * X[:, None, :] + wd[:, None, None] * eye)
         + (ab * wd)[:, None, None] * ww)
    M = np.where(pos[:, None, None], M, -Xx)
    iz = 1.0 / p[:, 2]
    D = np.zeros((len(X), 2, 3))
    D[:, 0, 0] = fx * iz
    D[:, 0, 2] = -fx * xp * iz
    D[:, 1, 1] = fy * iz
    D[:, 1, 2] = -fy * yp * iz
    Jc = np.concatenate([D @ M, D], 2)
    Jp = D @ R
    if fixed is not None:
        Jc = np.where(fixed_bits(fixed, len(cams))[cam_idx][:, None, :], 0.0, Jc)
    return r, Jc, Jp


def _cost(points, cams, K4, xy, pt_idx, cam_idx):
    with np.errstate(all="ignore"):
        r = linearize(points, cams, K4, xy, pt_idx, cam_idx, jac=False)
        return 0.5 * float((r * r).sum())


def _damp(d, mu):
    return mu * np.clip(d, 1e-6, 1e32)


def _chol(M):
    """Lower factors of a batch of small symmetric matrices, column by column; ok is False
    where a pivot is not > 0."""
    n = M.shape[1]
    C = np.zeros_like(M)
    ok = np.ones(len(M), bool)
    for j in range(n):
        d = M[:, j, j] - (C[:, j, :j] * C[:, j, :j]).sum(1)
        ok &= d > 0
        C[:, j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            C[:, i, j] = (M[:, i, j] - (C[:, i, :j] * C[:, j, :j]).sum(1)) / C[:, j, j]
    return C, ok


def _fwd(C, b):
    """C^-1 b for [n, k, k] lower factors and [n, k, c] right-hand sides."""
    y = np.zeros_like(b)
    for i in range(C.shape[1]):
        y[:, i] = (b[:, i] - (C[:, i, :i, None] * y[:, :i]).sum(1)) / C[:, i, i, None]
    return y


def _bwd(C, y):
    """C^-T y."""
    n = C.shape[1]
    x = np.zeros_like(y)
    for i in range(n - 1, -1, -1):
        x[:, i] = (y[:, i] - (C[:, i + 1:, i, None] * x[:, i + 1:]).sum(1)) / C[:, i, i, None]
    return x


def _host_solve(points, cams, K4, xy, pt_idx, cam_idx, fixed, max_iters, function_tolerance,
                pcg_tol, pcg_max_iters, radius):
    """The header's algorithm in numpy float64 -> (points, cams, info).  Sums over observations
    run in observation order."""
    points, cams = points.copy(), cams.copy()
    act_c, ac = np.unique(cam_idx, return_inverse=True)
    act_p, ap = np.unique(pt_idx, return_inverse=True)
    A, Pa = len(act_c), len(act_p)
    fix = fixed_bits(fixed, len(cams))[act_c]
    n_rows = min(max_iters, MAX_INFO_ROWS)
    info = np.zeros(INFO_HEAD + INFO_ROW * n_rows)
    cur = _cost(points, cams, K4, xy, pt_idx, cam_idx)
    info[3] = info[4] = cur
    info[5] = radius
    if not np.isfinite(cur):
        info[0] = 1
        return points, cams, info
    factor, it, succ, cg_total, status, lin = 2.0, 0, 0, 0, 0, None
    i6, i3 = np.arange(6), np.arange(3)
    T = lambda m: m.transpose(0, 2, 1)
    while it < max_iters and status == 0:
        if lin is None:
            lin = linearize(points, cams, K4, xy, pt_idx, cam_idx, fixed)
        r, Jc, Jp = lin
        mu = 1.0 / radius
        U, V = np.zeros((A, 6, 6)), np.zeros((Pa, 3, 3))
        gc, gp = np.zeros((A, 6)), np.zeros((Pa, 3))
        np.add.at(V, ap, T(Jp) @ Jp)
        np.add.at(gp, ap, (T(Jp) @ r[:, :, None])[:, :, 0])
        np.add.at(U, ac, T(Jc) @ Jc)
        np.add.at(gc, ac, (T(Jc) @ r[:, :, None])[:, :, 0])
        V[:, i3, i3] += _damp(V[:, i3, i3], mu)
        U[:, i6, i6] += _damp(U[:, i6, i6], mu)
        U[:, i6, i6] = np.where(fix, 1.0, U[:, i6, i6])
        row = np.full(INFO_ROW, np.nan)
        row[0], row[4], row[5], row[6], row[7] = cur, radius, 0.0, 0.0, 0.0
        accept = False
        with np.errstate(all="ignore"):
            Lv, ok3 = _chol(V)
            zp = _fwd(Lv, gp[:, :, None])
            Y = _fwd(Lv[ap], T(T(Jc) @ Jp))                       # L^-1 W^T, [N, 3, 6]
            m, h = np.zeros((A, 6, 6)), np.zeros((A, 6))
            np.add.at(m, ac, T(Y) @ Y)
            np.add.at(h, ac, (T(Y) @ zp[ap])[:, :, 0])
            C, ok6 = _chol(U - m)
        if ok3.all() and ok6.all():
            def S(v):
                s = np.zeros((Pa, 3))
                np.add.at(s, ap, (T(Jp) @ (Jc @ v[ac][:, :, None]))[:, :, 0])
                y = _bwd(Lv, _fwd(Lv, s[:, :, None]))[:, :, 0]
                acc = np.zeros((A, 6))
                np.add.at(acc, ac, (T(Jc) @ (Jp @ y[ap][:, :, None]))[:, :, 0])
                return (U @ v[:, :, None])[:, :, 0] - acc

            def prec(v):
                return _bwd(C, _fwd(C, v[:, :, None]))[:, :, 0]

            def dot(a, b):
                return np.float64((a * b).sum(1).cumsum()[-1])
            x = np.zeros((A, 6))
            res = -gc + h
            z = prec(res)
            p = z.copy()
            rz0 = rz = dot(res, z)
            k, reason = 0, 0
            with np.errstate(all="ignore"):
                if not np.isfinite(rz0):
                    reason = 4
                elif rz0 == 0:
                    reason = 5
                while reason == 0:
                    Sp = S(p)
                    pSp = dot(p, Sp)
                    if not np.isfinite(pSp):
                        reason = 4
                        break
                    if pSp <= 0:
                        reason = 3
                        break
                    k += 1
                    alpha = rz / pSp
                    x = x + alpha * p
                    res = res - alpha * Sp
                    z = prec(res)
                    rzn = dot(res, z)
                    beta = rzn / rz
                    p = z + beta * p
                    rz = rzn
                    if not (np.isfinite(alpha) and np.isfinite(rzn) and np.isfinite(beta)):
                        reason = 4
                    elif np.sqrt(rz / rz0) <= pcg_tol:
                        reason = 1
                    elif k >= pcg_max_iters:
                        reason = 2
                cg_total += k
                dc = x
                s = np.zeros((Pa, 3))
                np.add.at(s, ap, (T(Jp) @ (Jc @ dc[ac][:, :, None]))[:, :, 0])
                dp = _bwd(Lv, _fwd(Lv, (-gp - s)[:, :, None]))[:, :, 0]
                cams_n, points_n = cams.copy(), points.copy()
                cams_n[act_c] = np.where(fix, cams[act_c], cams[act_c] + dc)
                points_n[act_p] += dp
                cand = _cost(points_n, cams_n, K4, xy, pt_idx, cam_idx)
                Jd = (Jc @ dc[ac][:, :, None] + Jp @ dp[ap][:, :, None])[:, :, 0]
                md = -np.float64((Jd * (r + 0.5 * Jd)).sum())
                rho = np.float64(cur - cand) / md
            accept = bool(np.isfinite(cand) and md > 0 and rho > MIN_RHO)
            row[1], row[2], row[3], row[6], row[7] = cand, md, rho, k, reason
        row[5] = float(accept)
        if it < n_rows:
            info[INFO_HEAD + INFO_ROW * it:][:INFO_ROW] = row
        if accept:
            if function_tolerance > 0 and abs(cur - cand) / cur <= function_tolerance:
                status = 3
            points, cams, cur = points_n, cams_n, cand
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            factor = 2.0
            succ += 1
            lin = None
        else:
            radius /= factor
            factor *= 2.0
        if status == 0 and radius < MIN_RADIUS:
            status = 4
        it += 1
    info[0], info[1], info[2], info[4], info[5], info[6] = status, it, succ, cur, radius, cg_total
    return points, cams, info


# ------------------------------------------------------------------ the device path
def _device_solve(dev, points, cams, K4, xy, pt_idx, cam_idx, fixed, max_iters,
                  function_tolerance, pcg_tol, pcg_max_iters, radius, poll_every):
    from .tracker import build_index
    N, C, P = len(pt_idx), len(cams), len(points)
    buf, A, Pa = build_index(pt_idx, cam_idx, C, P)
    lib = _lib.load()
    if A > lib.onepose_gba_max_cameras():
        raise ValueError(f"global_bundle_adjust: {A} images carry observations, at most "
                         f"{lib.onepose_gba_max_cameras()} are supported")
    with torch.cuda.device(dev):
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
             for k, v in (("points", points), ("cam_pose", cams), ("cam_K4", K4), ("obs_xy", xy),
                          ("ptIdx", pt_idx), ("camIdx", cam_idx), ("index", buf))}
        t["cam_fixed"] = None if fixed is None else torch.from_numpy(fixed).to(dev)
        need = _lib.call("onepose_gba_workspace_bytes", n_obs=N, n_active_cams=A,
                         n_active_points=Pa)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rows = min(max_iters, MAX_INFO_ROWS)
        info = torch.empty(INFO_HEAD + INFO_ROW * rows, dtype=torch.float64, device=dev)
        common = dict(t, n_obs=N, n_cams=C, n_points=P, n_active_cams=A, n_active_points=Pa,
                      info=info, info_rows=rows, workspace=ws, workspace_bytes=need,
                      stream=_lib.stream_ptr(dev))
        _lib.run("onepose_gba_begin", initial_radius=float(radius), **common)
        chunk = max_iters if poll_every is None else int(poll_every)
        done = 0
        while done < max_iters:
            n = min(chunk, max_iters - done, MAX_STEPS_PER_CALL)
            _lib.run("onepose_gba_step", n_steps=n, pcg_max_iters=int(pcg_max_iters),
                     pcg_tol=float(pcg_tol), function_tolerance=float(function_tolerance),
                     **common)
            done += n
            if poll_every is not None and done < max_iters and info[0].item() != 0:
                break   # the only synchronisation: the solve has stopped on the device
        return t["points"].cpu().numpy(), t["cam_pose"].cpu().numpy(), info.cpu().numpy()


# ------------------------------------------------------------------ the model
def decode_info(info):
    """The info block as a dict: the head by name and the per-iteration rows [iterations, 8]."""
    n = min(int(info[1]), (len(info) - INFO_HEAD) // INFO_ROW)
    return {"status": int(info[0]), "status_text": STATUS.get(int(info[0]), "?"),
            "iterations": int(info[1]), "accepted": int(info[2]), "cost_before": float(info[3]),
            "cost_after": float(info[4]), "radius": float(info[5]), "cg_iterations": int(info[6]),
            "rows": info[INFO_HEAD:INFO_HEAD + INFO_ROW * n].reshape(n, INFO_ROW).copy()}


def model_problem(model):
    """The bundle adjustment problem of a model as ``reconstruct`` returns it: (points [P, 3],
    cams [m, 6] angle-axis and t, K4 [m, 4], xy [N, 2], ptIdx [N], camIdx [N]); observations in
    track order, camIdx the row of the image in the model."""
    image_row = {int(i): k for k, i in enumerate(model["image_ids"])}
    cam_row = {int(c): k for k, c in enumerate(model["camera_ids"])}
    params = np.asarray(model["camera_params"], dtype=np.float64).reshape(-1, 4)
    K4 = params[[cam_row[int(c)] for c in model["image_camera_ids"]]].reshape(-1, 4)
    cams = np.concatenate([qvec2aa(model["qvec"]),
                           np.asarray(model["tvec"], dtype=np.float64).reshape(-1, 3)], axis=1)
    pt_idx, cam_idx, xy = [], [], []
    for k, (imgs, idxs) in enumerate(zip(model["track_image_ids"], model["track_point2D_idxs"])):
        for i, j in zip(imgs, idxs):
            row = image_row[int(i)]
            pt_idx.append(k)
            cam_idx.append(row)
            xy.append(model["xys"][row][int(j)])
    return (np.ascontiguousarray(model["xyz"], dtype=np.float64).reshape(-1, 3), cams,
            np.ascontiguousarray(K4), np.asarray(xy, dtype=np.float64).reshape(-1, 2),
            np.asarray(pt_idx, dtype=np.int64), np.asarray(cam_idx, dtype=np.int64))


def fixed_mask(fixed, n_images, cam_idx):
    """The uint8 mask [n_images] of a ``fixed`` argument: ``"gauge"`` fixes every parameter of
    the first image that carries observations and t_x of the second (COLMAP's own choice),
    ``None`` nothing, ``"all"`` every pose; an array is passed through."""
    if fixed is None:
        return None
    if isinstance(fixed, str):
        mask = np.zeros(n_images, np.uint8)
        if fixed == "all":
            mask[:] = 63
        elif fixed == "gauge":
            seen = np.unique(cam_idx)
            if len(seen) < 2:
                raise ValueError("global_bundle_adjust: fixed='gauge' needs two images with "
                                 "observations")
            mask[seen[0]], mask[seen[1]] = 63, 8
        else:
            raise ValueError(f"global_bundle_adjust: fixed={fixed!r}; expected 'gauge', 'all', "
                             "None or a uint8 array")
        return mask
    mask = np.ascontiguousarray(fixed)
    if mask.dtype != np.uint8 or mask.shape != (n_images,):
        raise ValueError(f"global_bundle_adjust: fixed must be a uint8 array [{n_images}], got "
                         f"{mask.dtype} {mask.shape}")
    return mask


def global_bundle_adjust(model, fixed="gauge", max_iters=50, function_tolerance=1e-6,
                         pcg_tol=1e-6, pcg_max_iters=100, initial_radius=1e4, poll_every=4,
                         device=None):
    """Refine the poses and points of a model as ``sfm.reconstruct`` returns it; intrinsics stay.
    Returns a new mapping (nothing is changed in place) with ``xyz``, ``qvec`` and ``tvec``
    refined, ``error`` recomputed (the mean reprojection distance over the point's
    observations, infinite behind a camera), and ``model['global_ba']``: the decoded info block
    (``status``, ``iterations``, ``accepted``, ``cost_before``, ``cost_after``, ``radius``,
    ``cg_iterations``, ``rows``) and the ``fixed`` mask.

    ``max_iters=50`` and ``pcg_tol=1e-6`` are first guesses, ``function_tolerance=1e-6`` is
    Ceres' default.  The reference's own settings (150 or 500 iterations, tolerances 0) are
    accepted; with both tolerances 0 a converged solve runs on until the radius underflows
    (status 4).  ``poll_every=k`` reads the status after every k iterations and stops launching
    once it is non-zero -- the only synchronisation; the result does not depend on it."""
    from .object_builder import _gpu
    if not (isinstance(max_iters, (int, np.integer)) and max_iters >= 1):
        raise ValueError(f"global_bundle_adjust: max_iters = {max_iters!r}, need an integer >= 1")
    if not (isinstance(pcg_max_iters, (int, np.integer)) and 1 <= pcg_max_iters <= 500):
        raise ValueError(f"global_bundle_adjust: pcg_max_iters = {pcg_max_iters!r}, need 1..500")
    for name, v in (("function_tolerance", function_tolerance), ("pcg_tol", pcg_tol)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"global_bundle_adjust: {name} = {v!r}, need a finite number >= 0")
    if not (np.isfinite(initial_radius) and initial_radius > 0):
        raise ValueError(f"global_bundle_adjust: initial_radius = {initial_radius!r}, need a "
                         "positive finite number")
    if poll_every is not None and not (isinstance(poll_every, (int, np.integer))
                                       and poll_every >= 1):
        raise ValueError(f"global_bundle_adjust: poll_every = {poll_every!r}, need None or an "
                         "integer >= 1")
    points, cams, K4, xy, pt_idx, cam_idx = model_problem(model)
    if len(pt_idx) == 0:
        raise ValueError("global_bundle_adjust: the model has no observations")
    mask = fixed_mask(fixed, len(cams), cam_idx)
    dev = _gpu(device)
    args = (points, cams, K4, xy, pt_idx, cam_idx, mask, int(max_iters),
            float(function_tolerance), float(pcg_tol), int(pcg_max_iters), float(initial_radius))
    if dev is not None:
        new_p, new_c, info = _device_solve(dev, *args, poll_every)
    else:
        new_p, new_c, info = _host_solve(*args)
    out = dict(model)
    moved = (new_c[:, :3] != cams[:, :3]).any(1)
    qvec = np.array(model["qvec"], dtype=np.float64).reshape(-1, 4)
    qvec[moved] = aa2qvec(new_c[moved, :3])
    out["qvec"], out["tvec"], out["xyz"] = qvec, new_c[:, 3:6].copy(), new_p
    with np.errstate(all="ignore"):
        r = linearize(new_p, new_c, K4, xy, pt_idx, cam_idx, jac=False)
        z = _depth(new_p, new_c, pt_idx, cam_idx)
    e = np.where(z > 0, np.sqrt((r * r).sum(1)), np.inf)
    err, cnt = np.zeros(len(points)), np.zeros(len(points))
    np.add.at(err, pt_idx, e)
    np.add.at(cnt, pt_idx, 1.0)
    out["error"] = err / cnt
    out["global_ba"] = dict(decode_info(info), fixed=mask)
    return out


def _depth(points, cams, pt_idx, cam_idx):
    """z of every observation's point in its camera."""
    X = points[pt_idx]
    w, t = cams[cam_idx, :3], cams[cam_idx, 3:6]
    th = np.linalg.norm(w, axis=1)
    k = w / np.where(th > 0, th, 1.0)[:, None]
    c, s = np.cos(th), np.sin(th)
    p = (X * c[:, None] + np.cross(k, X) * s[:, None] + k * ((k * X).sum(1) * (1.0 - c))[:, None])
    return p[:, 2] + t[:, 2]

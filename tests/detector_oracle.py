"""ORACLE -- test infrastructure only.  numpy restatement of the 2D object detector's arithmetic
(include/onepose_hip.h, "2D object detector"): cv2.estimateAffinePartial2D(method=RANSAC) after
OpenCV 4.4's ptsetreg.cpp, match_worker / detect_by_matching of the reference's
LocalFeatureObjectDetector, and crop_img_by_bbox with cv2.warpAffine's fixed-point arithmetic.
float32 and float64 are used exactly where OpenCV uses them; the crop is all-integer.

PARITY UNPINNED against OpenCV itself (cv2 is absent): pinned by the known-answer scenes of
tests/test_detector_host.py.  The RANSAC loop is the one oracle/epnp_ransac.c restates, with
modelPoints = 2; ``CvRng`` is checked against that file's ``oracle_rng_draws``.
"""
from __future__ import annotations

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
MIN_MATCHES = 6   # local_feature_2D_detector.py:93


class CvRng:
    """cv::RNG: multiply-with-carry, state' = (u32)state * 4164903690 + (state >> 32)."""

    def __init__(self, state=0xFFFFFFFFFFFFFFFF):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < DBL_MIN:
        return 0
    num, denom = np.log(num), np.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


def minimal_model(f, t, i, j):
    """The similarity through correspondences i and j, in double: [S0, S1, S2, S3] with
    M = [S0 -S1 S2; S1 S0 S3].  Coincident source points give a non-finite model."""
    x1, y1, x2, y2 = (np.float64(v) for v in (f[i, 0], f[i, 1], f[j, 0], f[j, 1]))
    X1, Y1, X2, Y2 = (np.float64(v) for v in (t[i, 0], t[i, 1], t[j, 0], t[j, 1]))
    with np.errstate(all="ignore"):
        dx, dy = x1 - x2, y1 - y2
        d = np.float64(1.0) / (dx * dx + dy * dy)
        c = x1 * y2 - x2 * y1
        S0 = d * ((X1 - X2) * dx + (Y1 - Y2) * dy)
        S1 = d * ((Y1 - Y2) * dx - (X1 - X2) * dy)
        S2 = d * ((Y1 - Y2) * c - (X1 * y2 - X2 * y1) * dy - (X1 * x2 - X2 * x1) * dx)
        S3 = d * (-(X1 - X2) * c - (Y1 * x2 - Y2 * x1) * dx - (Y1 * y2 - Y2 * y1) * dy)
    return np.array([S0, S1, S2, S3], np.float64)


def errors(S, f, t):
    """computeError: the model cast to float, float32 arithmetic, err = a^2 + b^2."""
    with np.errstate(all="ignore"):
        F = np.array([S[0], -S[1], S[2], S[1], S[0], S[3]], np.float64).astype(np.float32)
        a = F[0] * f[:, 0] + F[1] * f[:, 1] + F[2] - t[:, 0]
        b = F[3] * f[:, 0] + F[4] * f[:, 1] + F[5] - t[:, 1]
        return a * a + b * b


def refine(S, f, t, mask, refine_iters):
    """Levenberg-Marquardt over the inliers in the shape of LMSolverImpl::run: h = [a, b, tx, ty],
    residuals (a x - b y + tx - X, b x + a y + ty - Y)."""
    x, y = f[mask, 0].astype(np.float64), f[mask, 1].astype(np.float64)
    X, Y = t[mask, 0].astype(np.float64), t[mask, 1].astype(np.float64)
    n = len(x)
    J = np.zeros((2 * n, 4))
    J[0::2] = np.stack([x, -y, np.ones(n), np.zeros(n)], 1)
    J[1::2] = np.stack([y, x, np.zeros(n), np.ones(n)], 1)
    JtJ = J.T @ J

    def resid(h):
        r = np.empty(2 * n)
        r[0::2] = h[0] * x - h[1] * y + h[2] - X
        r[1::2] = h[1] * x + h[0] * y + h[3] - Y
        return r
    h = S.copy()
    r = resid(h)
    Sq = float(r @ r)
    log_lambda = -3
    for _ in range(refine_iters):
        A = JtJ.copy()
        A[np.arange(4), np.arange(4)] *= 1.0 + 10.0 ** log_lambda
        d = np.linalg.solve(A, J.T @ r)
        hn = h - d
        rn = resid(hn)
        Sn = float(rn @ rn)
        if Sn < Sq:
            h, r, Sq = hn, rn, Sn
            log_lambda = max(log_lambda - 1, -16)
        else:
            log_lambda = min(log_lambda + 1, 16)
        if np.abs(d).max() < FLT_EPSILON or np.abs(r).max() < FLT_EPSILON:
            break
    return h


def estimate_affine_partial_2d(from_pts, to_pts, threshold=6.0, max_iters=2000, confidence=0.99,
                               refine_iters=10):
    """Returns (status, affine [2,3] float64, mask [n] bool, n_inliers, iterations_run);
    status 0 solved, 1 fewer than 2 points, 2 no model (affine zeros)."""
    f = np.ascontiguousarray(from_pts, np.float32).reshape(-1, 2)
    t = np.ascontiguousarray(to_pts, np.float32).reshape(-1, 2)
    n = len(f)
    none = np.zeros((2, 3))
    if n < 2:
        return 1, none, np.zeros(n, bool), 0, 0

    def mat(h):
        return np.array([[h[0], -h[1], h[2]], [h[1], h[0], h[3]]], np.float64)
    if n == 2:
        return 0, mat(minimal_model(f, t, 0, 1)), np.ones(2, bool), 2, 0
    thr = np.float32(np.float64(threshold) * np.float64(threshold))
    rng = CvRng()
    niters = max(max_iters, 1)
    max_good, best, best_mask = 0, None, None
    it = 0
    while it < niters:
        i0 = rng.uniform(0, n)
        i1 = rng.uniform(0, n)
        while i1 == i0:
            i1 = rng.uniform(0, n)
        S = minimal_model(f, t, i0, i1)
        m = errors(S, f, t) <= thr
        good = int(m.sum())
        if good > max(max_good, 1):
            max_good, best, best_mask = good, S, m
            niters = update_num_iters(confidence, (n - good) / n, 2, niters)
        it += 1
    if max_good <= 0:
        return 2, none, np.zeros(n, bool), 0, it
    h = refine(best, f, t, best_mask, refine_iters) if refine_iters > 0 else best
    return 0, mat(h), best_mask, max_good, it


def view_bbox(affine, vh, vw):
    """The view's corners (0,0), (w,0), (0,h), (w,h) through affine in double, truncated toward
    zero (astype(np.int32)); returns ([x0, y0, x1, y1], the 4x2 coordinates before truncation)."""
    corners = np.array([[0, 0, 1], [vw, 0, 1], [0, vh, 1], [vw, vh, 1]], np.float64).T
    pre = (affine @ corners).T
    box = pre.astype(np.int32)
    lo, hi = box.min(0), box.max(0)
    return np.array([lo[0], lo[1], hi[0], hi[1]], np.int32), pre


def detect_stage(matches0, counts0, kpts0, kpts1, db_hw, query_hw, threshold=6.0, max_iters=2000,
                 confidence=0.99, refine_iters=10, rank_mode=0):
    """match_worker + detect_by_matching.  matches0 [B, n0], kpts0 [B, n0, 2], kpts1 [n1, 2] or
    [B, n1, 2], db_hw [B, 2].  Returns a dict of per-view arrays, best_view and best_bbox."""
    matches0 = np.asarray(matches0)
    B, n0 = matches0.shape
    kpts1 = np.asarray(kpts1, np.float32)
    out = {"counts": np.zeros(B, np.int32), "affine": np.zeros((B, 6)),
           "inlier_mask": np.zeros((B, n0), np.uint8), "n_inliers": np.zeros(B, np.int32),
           "status": np.zeros(B, np.int32), "bbox": np.zeros((B, 4), np.int32),
           "iters": np.zeros(B, np.int32), "pre": [None] * B, "mpts": []}
    H, W = query_hw
    for b in range(B):
        nk = n0 if counts0 is None else int(counts0[b])
        m = matches0[b, :nk]
        k1 = kpts1 if kpts1.ndim == 2 else kpts1[b]
        valid = (m > -1) & (m < len(k1))
        mk0 = np.asarray(kpts0[b], np.float32)[:nk][valid]
        mk1 = k1[m[valid]]
        out["mpts"].append(np.concatenate([mk0, mk1], 1))
        out["counts"][b] = len(mk0)
        fallback = np.array([0, 0, H, W], np.int32)   # query["size"] is (H, W): x1 is H
        if len(mk0) < MIN_MATCHES:
            out["status"][b], out["bbox"][b] = 1, fallback
            continue
        st, A, mask, nin, it = estimate_affine_partial_2d(mk0, mk1, threshold, max_iters,
                                                          confidence, refine_iters)
        out["iters"][b] = it
        if st != 0:   # the reference would raise (affine is None)
            out["status"][b], out["bbox"][b] = 2, fallback
            continue
        out["affine"][b] = A.reshape(6)
        out["inlier_mask"][b, :len(mask)] = mask
        out["n_inliers"][b] = nin
        out["bbox"][b], out["pre"][b] = view_bbox(A, int(db_hw[b][0]), int(db_hw[b][1]))
    rank = np.where(out["status"] == 0, out["counts"] if rank_mode == 0 else out["n_inliers"], 0)
    out["rank"] = rank
    out["best_view"] = int(np.argmax(rank))   # the first of equals, as a stable reverse sort
    out["best_bbox"] = out["bbox"][out["best_view"]].copy()
    return out


def cv_round(x):
    return int(np.rint(x))   # nearest, ties to even


def crop_resize(image, bbox, K=None, crop_size=512):
    """crop_img_by_bbox: (crop_u8 [S, S], K_crop [3, 3] or None, status).  The window
    [x0, x1) x [y0, y1) of the image, zero outside the image, warped by T2 = [s 0 tx; 0 s ty],
    s = S / bw, with cv2.warpAffine's integer arithmetic."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape
    x0, y0, x1, y1 = (int(v) for v in bbox)
    bw, bh = x1 - x0, y1 - y0
    S = int(crop_size)
    K = None if K is None else np.asarray(K, np.float64).reshape(3, 3)
    if bw <= 0 or bh <= 0:
        return np.zeros((S, S), np.uint8), (None if K is None else K.copy()), 1
    if max(abs(v) for v in (x0, y0, x1, y1)) >= 32768:   # outside warpAffine's short maps
        return np.zeros((S, S), np.uint8), (None if K is None else K.copy()), 2
    win = np.zeros((bh, bw), np.int64)   # the first warp: an exact integer crop
    gx0, gx1, gy0, gy1 = max(x0, 0), min(x1, w), max(y0, 0), min(y1, h)
    if gx1 > gx0 and gy1 > gy0:
        win[gy0 - y0:gy1 - y0, gx0 - x0:gx1 - x0] = image[gy0:gy1, gx0:gx1]
    s = np.float64(S) / np.float64(bw)
    tx = np.float64(S) * 0.5 - s * np.float64(bw) * 0.5
    ty = np.float64(S) * 0.5 - s * np.float64(bh) * 0.5
    D = s * s
    D = 1.0 / D if D != 0 else 0.0
    A11 = A22 = s * D
    b1, b2 = -A11 * tx, -A22 * ty
    idx = np.arange(S, dtype=np.float64)
    adelta = np.rint(A11 * idx * 1024.0).astype(np.int64)          # cvRound: ties to even
    X = (cv_round(b1 * 1024.0) + 16 + adelta) >> 5                  # per column
    Y = (np.rint((A22 * idx + b2) * 1024.0).astype(np.int64) + 16) >> 5   # per row
    sx, fx = (X >> 5)[None, :], (X & 31)[None, :]
    sy, fy = (Y >> 5)[:, None], (Y & 31)[:, None]

    def tap(ix, iy):   # 0 outside the window
        ok = (ix >= 0) & (ix < bw) & (iy >= 0) & (iy < bh)
        return np.where(ok, win[np.clip(iy, 0, bh - 1), np.clip(ix, 0, bw - 1)], 0)
    acc = ((32 - fx) * (32 - fy) * 32 * tap(sx, sy) + fx * (32 - fy) * 32 * tap(sx + 1, sy)
           + (32 - fx) * fy * 32 * tap(sx, sy + 1) + fx * fy * 32 * tap(sx + 1, sy + 1))
    out = np.minimum((acc + 16384) >> 15, 255).astype(np.uint8)
    K_crop = None
    if K is not None:
        T1 = np.array([[1, 0, -x0], [0, 1, -y0], [0, 0, 1]], np.float64)
        T2 = np.array([[s, 0, tx], [0, s, ty], [0, 0, 1]], np.float64)
        K_crop = T2 @ (T1 @ K)
    return out, K_crop, 0

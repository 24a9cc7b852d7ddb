"""Pyramidal Lucas-Kanade once more, in float64 and without the contract's fixed point: a second
opinion on tests/lk_oracle.py that shares no helper with it.

The integer stages (pyrDown, Scharr) are scipy.ndimage.correlate1d with mode="mirror" on int64
arrays and must equal the oracle's and the GPU's exactly.  The tracker samples with
scipy.ndimage.map_coordinates: true bilinear weights, nothing rounded, the image mirrored about
its edge pixels (reflect-101) and the derivatives zero outside the level.  I is scaled by 32 and
the sums by 2^-20 as in cv2, so min_eig_threshold means what it means there.  The bounds rule,
the eigenvalue test and the three ways an iteration ends are those of include/onepose_hip.h."""
import numpy as np
from scipy import ndimage

REASONS = ("eps", "oscillation", "cap", "oob_pre", "oob_loop", "eig", "no_iter")
EPS, OSC, CAP, OOB_PRE, OOB_LOOP, EIG, NO_ITER = range(7)


def pyr_down(img):
    v = ndimage.correlate1d(img.astype(np.int64), [1, 4, 6, 4, 1], axis=1, mode="mirror")[:, ::2]
    v = ndimage.correlate1d(v, [1, 4, 6, 4, 1], axis=0, mode="mirror")[::2]
    return ((v + 128) // 256).astype(np.uint8)


def scharr(img):
    """(dx, dy), int64 [h, w] each."""
    v = img.astype(np.int64)
    smooth, diff = [3, 10, 3], [-1, 0, 1]
    dx = ndimage.correlate1d(ndimage.correlate1d(v, smooth, axis=0, mode="mirror"), diff, axis=1,
                             mode="mirror")
    dy = ndimage.correlate1d(ndimage.correlate1d(v, diff, axis=0, mode="mirror"), smooth, axis=1,
                             mode="mirror")
    return dx, dy


def pyramid(img, win, max_level):
    """[(image uint8, dx int64, dy int64)] per level; a level is added while both of its sides
    exceed the window."""
    levels = [np.ascontiguousarray(img, dtype=np.uint8)]
    while len(levels) <= max_level:
        nxt = pyr_down(levels[-1])
        if min(nxt.shape) <= win:
            break
        levels.append(nxt)
    return [(lv,) + scharr(lv) for lv in levels]


def _window(arr, x, y, grid, mode):
    """arr sampled bilinearly at (x + j, y + i) over the window grid."""
    return ndimage.map_coordinates(arr, [grid[0] + y, grid[1] + x], order=1, mode=mode, cval=0.0)


def track(prev_pyr, next_pyr, pts, win, max_count=10, epsilon=0.03, min_eig=1e-4):
    """-> positions [n, 2] float64, status [n] uint8, reason [n] (how level 0 ended)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    half = (win - 1) / 2
    grid = np.mgrid[0:win, 0:win].astype(np.float64)
    flt_eps = float(np.finfo(np.float32).eps)
    scale = 2.0 ** -20
    prev = [(i.astype(np.float64), dx.astype(np.float64), dy.astype(np.float64))
            for i, dx, dy in prev_pyr]
    nxt = [lv[0].astype(np.float64) for lv in next_pyr]
    out = np.zeros_like(pts)
    status = np.ones(len(pts), np.uint8)
    reason = np.full(len(pts), -1, np.int64)

    def outside(x, y, rows, cols):
        fx, fy = np.floor(x), np.floor(y)
        return not (-win <= fx < cols and -win <= fy < rows)

    for n, (px, py) in enumerate(pts):
        guess = None
        for l in range(len(prev) - 1, -1, -1):
            img, gx, gy = prev[l]
            rows, cols = img.shape
            x, y = px / 2 ** l - half, py / 2 ** l - half
            guess = np.array([px, py]) / 2 ** l if guess is None else guess * 2
            if outside(x, y, rows, cols):
                if l == 0:
                    status[n], reason[n] = 0, OOB_PRE
                continue
            I = 32.0 * _window(img, x, y, grid, "mirror")
            Ix = _window(gx, x, y, grid, "grid-constant")
            Iy = _window(gy, x, y, grid, "grid-constant")
            a11, a12, a22 = (Ix * Ix).sum() * scale, (Ix * Iy).sum() * scale, (Iy * Iy).sum() * scale
            det = a11 * a22 - a12 * a12
            lam = (a11 + a22 - np.sqrt((a11 - a22) ** 2 + 4 * a12 * a12)) / (2 * win * win)
            if lam < min_eig or det < flt_eps:
                if l == 0:
                    status[n], reason[n] = 0, EIG
                continue
            q = guess - half
            last = np.zeros(2)
            end = CAP if max_count > 0 else NO_ITER
            for j in range(max_count):
                if outside(q[0], q[1], rows, cols):
                    if l == 0:
                        status[n] = 0
                    end = OOB_LOOP
                    break
                dI = 32.0 * _window(nxt[l], q[0], q[1], grid, "mirror") - I
                b1, b2 = (dI * Ix).sum() * scale, (dI * Iy).sum() * scale
                step = np.array([a12 * b2 - a22 * b1, a12 * b1 - a11 * b2]) / det
                q = q + step
                guess = q + half
                if step @ step <= epsilon * epsilon:
                    end = EPS
                    break
                if j > 0 and (np.abs(step + last) < 0.01).all():
                    guess = guess - step / 2
                    end = OSC
                    break
                last = step
            if l == 0:
                reason[n] = end
        out[n] = guess
    return out, status, reason

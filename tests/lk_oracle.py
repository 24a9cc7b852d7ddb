"""The pyramidal Lucas-Kanade contract of include/onepose_hip.h restated in numpy: integer
pyramids and derivatives, float32 steps one by one (numpy never fuses a multiply and an add), the
window sums as exact integers.  Vectorised over the window; one Python loop over points, levels
and iterations.  The GPU tests compare bits with this; tests/golden/lk.npz and lk_edges.npz pin
it, and tests/lk_model.py (float64, no fixed point, no code shared) is held against it."""
import numpy as np

F = np.float32
(R_EPS, R_OSC, R_CAP, R_OOB_PRE, R_OOB_LOOP, R_EIG, R_NO_ITER, R_HOSTILE) = range(8)
REASONS = ("eps", "oscillation", "cap", "oob_pre", "oob_loop", "eig", "no_iter", "hostile")
FLT_EPSILON = F(np.finfo(np.float32).eps)


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 4, 6, 4, 1], dtype=np.int32)
    src = img.astype(np.int32)
    xs = reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    hor = (src[:, xs] * k).sum(-1)                       # [h, ow]
    ys = reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)
    ver = (hor[ys] * k[None, :, None]).sum(1)            # [oh, ow]
    return ((ver + 128) >> 8).astype(np.uint8)


def scharr(img):
    """int16 [h, w, 2]: (dx, dy)."""
    h, w = img.shape
    s = img.astype(np.int32)
    up, down = s[reflect101(np.arange(h) - 1, h)], s[reflect101(np.arange(h) + 1, h)]
    t0 = (up + down) * 3 + s * 10
    t1 = down - up
    xl, xr = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    dx = t0[:, xr] - t0[:, xl]
    dy = (t1[:, xr] + t1[:, xl]) * 3 + t1 * 10
    return np.stack([dx, dy], -1).astype(np.int16)


def level_shapes(h, w, win, max_level):
    shapes = [(h, w)]
    while len(shapes) <= max_level:
        h, w = (h + 1) // 2, (w + 1) // 2
        if h <= win or w <= win:
            break
        shapes.append((h, w))
    return shapes


def build_pyramid(img, win, max_level, with_deriv=True):
    """[(image uint8, derivative int16 or None)] per level."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    out = []
    for _ in level_shapes(*img.shape, win, max_level):
        out.append((img, scharr(img) if with_deriv else None))
        img = pyr_down(img)
    return out


def _weights(a, b):
    one, W = F(1), F(16384)
    w00 = int(np.rint((one - a) * (one - b) * W))
    w01 = int(np.rint(a * (one - b) * W))
    w10 = int(np.rint((one - a) * b * W))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _tap(pad, off, ix, iy, win, wts):
    """The 4-tap integer sum over the win x win window at (ix, iy) of an array padded by off."""
    y0, x0 = iy + off, ix + off
    p = pad[y0:y0 + win + 1, x0:x0 + win + 1].astype(np.int64)
    return (p[:-1, :-1] * wts[0] + p[:-1, 1:] * wts[1] + p[1:, :-1] * wts[2] + p[1:, 1:] * wts[3])


def _out(fx, fy, win, cols, rows):
    return not (fx >= F(-win) and fx < F(cols) and fy >= F(-win) and fy < F(rows))


def eps_squared(epsilon):
    e = min(max(float(F(epsilon)), 0.0), 10.0)
    return F(e * e)


def exact_sum(v):
    """The window sum as a Python int (the terms are int64 and far from its limits)."""
    return int(v.sum())


def wrapped_int32_sum(v):
    """What a 32-bit accumulator would hold: every term fits int32, the sum wraps.  Not the
    contract; tests pass it as ``window_sum`` to show which scenes tell the two apart."""
    return int(v.astype(np.int32).sum(dtype=np.int32))


def track(prev_pyr, next_pyr, pts, win, max_count=10, epsilon=0.03, min_eig=1e-4, eig_out=None,
          trace=None, window_sum=exact_sum, stats=None):
    """-> next_pts [n, 2] float32, status [n] uint8, reason [n] int (how level 0 ended).
    ``eig_out`` (a dict) receives {point index: minEig at level 0} of the points that reach the
    eigenvalue test there.  ``trace`` (a list) receives (point, level, reason) for every level a
    point visits, from the top down; a hostile point visits none.  ``stats`` (a dict) receives
    under "max_ix2" the largest window sum of Ix^2 or Iy^2 met, as an exact integer."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    n, levels = len(pts), len(prev_pyr)
    max_count = min(max(int(max_count), 0), 100)
    eps2, min_eig = eps_squared(epsilon), F(min_eig)
    half = F(win - 1) * F(0.5)
    pimg = [np.pad(i, win, mode="reflect") for i, _ in prev_pyr]
    nimg = [np.pad(i, win, mode="reflect") for i, _ in next_pyr]
    pder = [np.pad(d, ((win, win), (win, win), (0, 0))) for _, d in prev_pyr]
    out = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    reason = np.full(n, -1, np.int64)
    note = trace.append if trace is not None else (lambda t: None)
    with np.errstate(all="ignore"):
        for i in range(n):
            px, py = pts[i]
            if not (np.abs(px) < F(2 ** 30) and np.abs(py) < F(2 ** 30)):
                out[i], status[i], reason[i] = pts[i], 0, R_HOSTILE
                continue
            ox = oy = F(0)
            for l in range(levels - 1, -1, -1):
                rows, cols = prev_pyr[l][0].shape
                sc = F(1) / F(1 << l)
                qx, qy = px * sc, py * sc
                if l == levels - 1:
                    ox, oy = qx, qy
                else:
                    ox, oy = ox * F(2), oy * F(2)
                qx, qy = qx - half, qy - half
                fx, fy = np.floor(qx), np.floor(qy)
                if _out(fx, fy, win, cols, rows):
                    if l == 0:
                        status[i], reason[i] = 0, R_OOB_PRE
                    note((i, l, R_OOB_PRE))
                    continue
                ix, iy = int(fx), int(fy)
                wts = _weights(qx - fx, qy - fy)
                I = (_tap(pimg[l], win, ix, iy, win, wts) + 256) >> 9
                Ix = (_tap(pder[l][..., 0], win, ix, iy, win, wts) + 8192) >> 14
                Iy = (_tap(pder[l][..., 1], win, ix, iy, win, wts) + 8192) >> 14
                scale = F(2.0 ** -20)
                A11 = F(window_sum(Ix * Ix)) * scale
                A12 = F(window_sum(Ix * Iy)) * scale
                A22 = F(window_sum(Iy * Iy)) * scale
                if stats is not None:
                    stats["max_ix2"] = max(stats.get("max_ix2", 0), int((Ix * Ix).sum()),
                                           int((Iy * Iy).sum()))
                D = A11 * A22 - A12 * A12
                dif = A11 - A22
                m = (A22 + A11 - np.sqrt(dif * dif + F(4) * A12 * A12)) / F(2 * win * win)
                if eig_out is not None and l == 0:
                    eig_out[i] = m
                if m < min_eig or D < FLT_EPSILON:
                    if l == 0:
                        status[i], reason[i] = 0, R_EIG
                    note((i, l, R_EIG))
                    continue
                Dinv = F(1) / D
                nx, ny = ox - half, oy - half
                pdx = pdy = F(0)
                end = R_CAP if max_count > 0 else R_NO_ITER
                for j in range(max_count):
                    fx, fy = np.floor(nx), np.floor(ny)
                    if _out(fx, fy, win, cols, rows):
                        if l == 0:
                            status[i] = 0
                        end = R_OOB_LOOP
                        break
                    wts = _weights(nx - fx, ny - fy)
                    diff = ((_tap(nimg[l], win, int(fx), int(fy), win, wts) + 256) >> 9) - I
                    b1 = F(window_sum(diff * Ix)) * scale
                    b2 = F(window_sum(diff * Iy)) * scale
                    dx = (A12 * b2 - A22 * b1) * Dinv
                    dy = (A12 * b1 - A11 * b2) * Dinv
                    nx, ny = nx + dx, ny + dy
                    ox, oy = nx + half, ny + half
                    if dx * dx + dy * dy <= eps2:
                        end = R_EPS
                        break
                    if j > 0 and np.abs(dx + pdx) < F(0.01) and np.abs(dy + pdy) < F(0.01):
                        ox, oy = ox - dx * F(0.5), oy - dy * F(0.5)
                        end = R_OSC
                        break
                    pdx, pdy = dx, dy
                if l == 0:
                    reason[i] = end
                note((i, l, end))
            out[i] = (ox, oy)
    return out, status, reason


def calc_optical_flow_pyr_lk(prev_img, next_img, pts, win=15, max_level=2, max_count=10,
                             epsilon=0.03, min_eig=1e-4):
    p = build_pyramid(prev_img, win, max_level)
    q = build_pyramid(next_img, win, max_level, with_deriv=False)
    return track(p, q, pts, win, max_count, epsilon, min_eig)

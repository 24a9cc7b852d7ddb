"""The two device entry points of the sparse reconstruction, restated in plain loops from the
header's text (include/onepose_hip.h, "Sparse reconstruction").  Shares no code with the package.

``components``: the label of a node is the smallest id of its component.
``triangulate``: one track, every floating-point step a Python float operation in the header's
order.  ``solver`` picks how the DLT's null vector is taken: 'jacobi' is the contract (the cyclic
Jacobi of onepose_triangulate); 'eigh' of A^T A and 'svd' of A are numpy's, and the generator
sizes the tolerance by their deviation.  ``variant`` breaks one rule on purpose for
tests/test_sfm_model_host.py.
"""
import math

import numpy as np

MAX_TRACK = 256


def components(edges, n_nodes):
    label = list(range(n_nodes))
    changed = True
    while changed:   # plain label propagation to a fixed point
        changed = False
        for u, v in edges:
            if not (0 <= u < n_nodes and 0 <= v < n_nodes):
                continue
            lo = min(label[u], label[v])
            if label[u] != lo or label[v] != lo:
                label[u] = label[v] = lo
                changed = True
    return np.asarray(label, dtype=np.int32)


def tracks_from_labels(labels, n_feats_per_image):
    """The CSR of the header: components of >= 2 features by label, observations by feature id."""
    offsets = [0]
    for c in n_feats_per_image:
        offsets.append(offsets[-1] + int(c))
    groups = {}
    for node, lab in enumerate(labels):
        groups.setdefault(int(lab), []).append(node)
    start, img, feat = [0], [], []
    for lab in sorted(groups):
        if len(groups[lab]) < 2:
            continue
        for node in groups[lab]:
            k = max(i for i in range(len(offsets) - 1) if offsets[i] <= node)
            img.append(k)
            feat.append(node - offsets[k])
        start.append(len(img))
    return (np.asarray(start, np.int32), np.asarray(img, np.int32), np.asarray(feat, np.int32))


def jacobi_smallest(M):
    """The eigenvector of the smallest eigenvalue of a symmetric 4 x 4 matrix: cyclic Jacobi, at
    most 24 sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); an off-diagonal entry at or below
    1e-20 sqrt(|M_pp M_qq|) is set to zero and skipped."""
    M = [[float(v) for v in row] for row in M]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(24):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                apq = M[p][q]
                if abs(apq) <= 1e-20 * math.sqrt(abs(M[p][p] * M[q][q])) or apq == 0.0:
                    M[p][q] = M[q][p] = 0.0
                    continue
                rotated = True
                theta = (M[q][q] - M[p][p]) / (2.0 * apq)
                tt = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cs = 1.0 / math.sqrt(tt * tt + 1.0)
                sn = tt * cs
                for k in range(4):
                    mkp, mkq = M[k][p], M[k][q]
                    M[k][p] = cs * mkp - sn * mkq
                    M[k][q] = sn * mkp + cs * mkq
                for k in range(4):
                    mpk, mqk = M[p][k], M[q][k]
                    M[p][k] = cs * mpk - sn * mqk
                    M[q][k] = sn * mpk + cs * mqk
                M[p][q] = M[q][p] = 0.0
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = cs * vkp - sn * vkq
                    V[k][q] = sn * vkp + cs * vkq
        if not rotated:
            break
    best = 0
    for j in range(1, 4):
        if M[j][j] < M[best][best]:
            best = j
    return [V[k][best] for k in range(4)]


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _project(Rt, K, X, uv):
    Rt, K, X = [[float(v) for v in r] for r in Rt], [float(v) for v in K], [float(v) for v in X]
    p = [((Rt[r][0] * X[0] + Rt[r][1] * X[1]) + Rt[r][2] * X[2]) + Rt[r][3] for r in range(3)]
    ru = (K[0] * _div(p[0], p[2]) + K[2]) - float(uv[0])
    rv = (K[1] * _div(p[1], p[2]) + K[3]) - float(uv[1])
    return p, ru, rv


def _error(Rt, K, X, uv, depth=True):
    p, ru, rv = _project(Rt, K, X, uv)
    e = math.sqrt(ru * ru + rv * rv) if math.isfinite(ru * ru + rv * rv) else float(ru * ru + rv * rv)
    if math.isnan(e) or math.isnan(p[2]):
        return float("nan")
    return e if p[2] > 0 or not depth else float("inf")


def _note(margins, value):
    if margins is not None and math.isfinite(value):
        margins.append(abs(value))


def check_csr(track_start, obs_image, n_images, variant=None):
    """The check that runs before anything is read through the CSR -> (status, index): status 1
    when track_start is not 0 = s[0] <= s[1] <= ... <= s[n_tracks] = n_obs, else 2 when an image
    id lies outside [0, n_images), else 0; index is the smallest offending index (0 when clean).
    ``variant`` breaks one rule on purpose for tests/test_sfm_model_host.py."""
    s, img = [int(v) for v in track_start], [int(v) for v in obs_image]
    n_tracks, n_obs = len(s) - 1, len(img)
    starts, images = [], []
    for t in range(n_tracks + 1):
        bad = s[t] < 0 or s[t] > n_obs
        if t == 0 and s[t] != 0:
            bad = True
        if t == n_tracks and s[t] != n_obs:
            bad = True
        if t > 0 and s[t] < s[t - 1]:
            bad = True
        if bad:
            starts.append(t)
    for o in range(n_obs):
        if img[o] < 0 or img[o] >= n_images:
            images.append(o)
    pick = max if variant == "first offender found" else min   # found scanning from the end
    order = [(1, starts), (2, images)]
    if variant == "image ids before starts":
        order.reverse()
    for status, found in order:
        if found:
            return status, pick(found)
    return 0, 0


def triangulate(Rt, K4, img, uv, max_reproj, min_angle_deg, solver="jacobi", variant=None,
                margins=None, ties=None):
    """-> (reason, X [3] or None, err or None, keep [len] bool).  ``margins`` collects the
    distance of every decision from its threshold (px or degrees) and of every tie-break from a
    tie; ``ties`` collects the position pairs (stays, leaves) of the duplicate rule whose errors
    are equal."""
    Rt, K4 = np.asarray(Rt, np.float64), np.asarray(K4, np.float64)
    img, uv = [int(i) for i in img], np.asarray(uv, np.float64).reshape(-1, 2)
    L = len(img)
    keep = np.zeros(L, dtype=bool)
    if L < 2 or L > MAX_TRACK:
        return 3, None, None, keep
    rows = []
    with np.errstate(all="ignore"):
        for p in range(L):
            R, K = Rt[img[p]], K4[img[p]]
            xn, yn = (uv[p, 0] - K[2]) / K[0], (uv[p, 1] - K[3]) / K[1]
            rows.append(([float(xn * R[2][j] - R[0][j]) for j in range(4)],
                         [float(yn * R[2][j] - R[1][j]) for j in range(4)]))
    S = [True] * L
    order = range(L - 1, -1, -1) if variant == "sums in reverse order" else range(L)

    def solve():
        if solver == "svd":
            A = np.array([r for p in range(L) if S[p] for r in rows[p]])
            if not np.isfinite(A).all():
                return None
            h = np.linalg.svd(A)[2][-1]
        else:
            M = np.zeros((4, 4))
            for p in order:
                if S[p]:
                    a, b = rows[p]
                    for i in range(4):
                        for j in range(4):
                            M[i, j] = M[i, j] + (a[i] * a[j] + b[i] * b[j])
            if solver == "jacobi":
                h = np.array(jacobi_smallest(M))
            elif not np.isfinite(M).all():
                return None
            else:
                h = np.linalg.eigh(M)[1][:, 0]
        with np.errstate(all="ignore"):
            X = h[:3] / h[3]
        return X if np.isfinite(X).all() else None

    def errors(X):
        return [_error(Rt[img[p]], K4[img[p]], X, uv[p], variant != "depth not tested")
                if S[p] else None for p in range(L)]

    # 1, 2
    while True:
        X = solve()
        if X is None:
            return 4, None, None, keep
        e = errors(X)
        if any(v is not None and math.isnan(v) for v in e):
            return 4, None, None, keep
        worst = None
        for p in range(L):
            if S[p]:
                _note(margins, e[p] - max_reproj)
                if variant == "worst among the first 64 positions" and p >= 64:
                    continue
                if worst is None or e[p] > e[worst]:
                    worst = p
        if worst is None or not e[worst] > max_reproj or variant == "no drop-worst loop":
            break
        for p in range(L):
            if S[p] and p != worst and e[p] > max_reproj:
                _note(margins, e[p] - e[worst])
        S[worst] = False
        if sum(S) < 2:
            return 1, None, None, keep
    if variant == "no drop-worst loop":
        for p in range(L):
            if S[p] and e[p] > max_reproj:
                S[p] = False
        if sum(S) < 2:
            return 1, None, None, keep
    # 3
    if variant != "no duplicate rule":
        best = {}
        for p in range(L):
            if S[p]:
                q = best.get(img[p])
                if q is not None:
                    _note(margins, e[p] - e[q])
                    if ties is not None and e[p] == e[q]:
                        ties.append((q, p))
                if q is None or e[p] < e[q] or (
                        variant == "duplicate ties to the highest position" and e[p] == e[q]):
                    best[img[p]] = p
        for p in range(L):
            if S[p] and best[img[p]] != p:
                S[p] = False
        if sum(S) < 2:
            return 1, None, None, keep
    # 4
    for _ in range(0 if variant == "no refinement" else 5):
        H, g, cost = [[0.0] * 3 for _ in range(3)], [0.0] * 3, 0.0
        for p in order:
            if not S[p]:
                continue
            R, K = [[float(v) for v in r] for r in Rt[img[p]]], [float(v) for v in K4[img[p]]]
            pc, ru, rv = _project(R, K, X, uv[p])
            iz = _div(1.0, pc[2])
            xz, yz, fu, fv = pc[0] * iz, pc[1] * iz, K[0] * iz, K[1] * iz
            Ju = [fu * (R[0][k] - xz * R[2][k]) for k in range(3)]
            Jv = [fv * (R[1][k] - yz * R[2][k]) for k in range(3)]
            for i in range(3):
                for j in range(i, 3):
                    H[i][j] = H[i][j] + (Ju[i] * Ju[j] + Jv[i] * Jv[j])
                g[i] = g[i] + (Ju[i] * ru + Jv[i] * rv)
            cost = cost + (ru * ru + rv * rv)
        if not H[0][0] > 0.0:
            break
        l00 = math.sqrt(H[0][0])
        l10, l20 = H[0][1] / l00, H[0][2] / l00
        d11 = H[1][1] - l10 * l10
        if not d11 > 0.0:
            break
        l11 = math.sqrt(d11)
        l21 = (H[1][2] - l20 * l10) / l11
        d22 = (H[2][2] - l20 * l20) - l21 * l21
        if not d22 > 0.0:
            break
        l22 = math.sqrt(d22)
        y0 = -g[0] / l00
        y1 = (-g[1] - l10 * y0) / l11
        y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
        d2 = y2 / l22
        d1 = (y1 - l21 * d2) / l11
        d0 = ((y0 - l10 * d1) - l20 * d2) / l00
        d = np.array([d0, d1, d2])
        cand = 0.0
        for p in order:
            if S[p]:
                _, ru, rv = _project(Rt[img[p]], K4[img[p]], X + d, uv[p])
                cand = cand + (ru * ru + rv * rv)
        if not cand < cost:
            break
        X = X + d
    # 5
    e = errors(X)
    if any(v is not None and math.isnan(v) for v in e):
        return 4, None, None, keep
    for p in range(L):
        if S[p]:
            _note(margins, e[p] - max_reproj)
            if not e[p] <= max_reproj and variant != "no final check":
                S[p] = False
    if sum(S) < 2:
        return 1, None, None, keep
    rays = {}
    for p in range(L):
        if S[p]:
            R = Rt[img[p]]
            if variant == "angle between image rays":
                d = R[:, :3].T @ np.array([(uv[p, 0] - K4[img[p]][2]) / K4[img[p]][0],
                                           (uv[p, 1] - K4[img[p]][3]) / K4[img[p]][1], 1.0])
            else:
                d = np.array([-((float(R[0][k]) * float(R[0][3]) + float(R[1][k]) * float(R[1][3]))
                                + float(R[2][k]) * float(R[2][3])) - float(X[k]) for k in range(3)])
            rays[p] = d / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    cmin = 2.0
    pos = sorted(rays)
    for i, p in enumerate(pos):
        for q in pos[i + 1:]:
            c = float((rays[p][0] * rays[q][0] + rays[p][1] * rays[q][1]) + rays[p][2] * rays[q][2])
            if math.isnan(c):
                return 4, None, None, keep
            cmin = min(cmin, c)
    angle = math.degrees(math.acos(min(max(cmin, -1.0), 1.0)))
    _note(margins, angle - min_angle_deg)
    if angle < min_angle_deg:
        return 2, None, None, keep
    err = 0.0
    for p in order:
        if S[p]:
            err = err + e[p]
    return 0, X, err / sum(S), np.asarray(S, dtype=bool)


def triangulate_all(Rt, K4, track_start, obs_image, obs_xy, max_reproj, min_angle_deg, **kw):
    T = len(track_start) - 1
    out = {"xyz": np.full((T, 3), np.nan), "err": np.full(T, np.nan),
           "reason": np.zeros(T, np.int32), "n_kept": np.zeros(T, np.int32),
           "obs_keep": np.zeros(len(obs_image), bool)}
    for t in range(T):
        a, b = int(track_start[t]), int(track_start[t + 1])
        why, X, err, keep = triangulate(Rt, K4, obs_image[a:b], obs_xy[a:b], max_reproj,
                                        min_angle_deg, **kw)
        out["reason"][t] = why
        if why == 0:
            out["xyz"][t], out["err"][t], out["n_kept"][t] = X, err, keep.sum()
            out["obs_keep"][a:b] = keep
    return out

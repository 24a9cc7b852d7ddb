"""The object builder's contract (include/onepose_hip.h, "Object builder") restated in numpy, one
IEEE operation per step in the order the header writes them.  Neighbours are kept as sparse lists
(a row of distances at a time), never as the reference's dense n x n matrix.  The GPU tests ask
the kernels for these bits; tests/test_object_builder_host.py pins this file to the reference's
recorded outputs."""
import numpy as np


def filter_points(xyz, track_len, min_track, corners):
    """-> (xyz_out float32 [m, 3], index int32 [m]) in input order."""
    p = np.asarray(xyz, dtype=np.float64).astype(np.float32)
    keep = np.ones(p.shape[0], dtype=bool)
    if track_len is not None:
        keep &= np.asarray(track_len) >= min_track
    if corners is not None:
        c = np.asarray(corners, dtype=np.float64).astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            q = p - c[4]
            for other in (5, 0, 7):
                v = c[other] - c[4]
                m = (q[:, 0] * v[0] + q[:, 1] * v[1]) + q[:, 2] * v[2]
                vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                keep &= (np.float32(0) < m) & (m < vv)
    index = np.nonzero(keep)[0].astype(np.int32)
    return p[index], index


def box_margin(xyz, corners):
    """min over points and axes of min(|m|, |m - v.v|), in float64 on the float32 inputs."""
    p = np.asarray(xyz, dtype=np.float64).astype(np.float32).astype(np.float64)
    c = np.asarray(corners, dtype=np.float64).astype(np.float32).astype(np.float64)
    q = p - c[4]
    out = np.inf
    for other in (5, 0, 7):
        v = c[other] - c[4]
        m = q @ v
        out = min(out, np.abs(m).min(), np.abs(m - v @ v).min())
    return float(out)


def radius_neighbours(x, thr):
    """-> (row_start int64 [n + 1], cols int32 [total]): row j = ascending i with i == j or
    sqrt((dx dx + dy dy) + dz dz) < thr, float64 on the widened values."""
    xd = np.asarray(x).astype(np.float64)
    n = xd.shape[0]
    rows = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            d = xd - xd[j]
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            hit = np.sqrt(s) < thr
            hit[j] = True
            rows.append(np.nonzero(hit)[0].astype(np.int32))
    row_start = np.zeros(n + 1, dtype=np.int64)
    row_start[1:] = np.cumsum([len(r) for r in rows])
    return row_start, np.concatenate(rows) if rows else np.zeros(0, np.int32)


def merge_greedy(x, row_start, cols):
    """-> (cluster_of int32 [n], member_start int32 [m + 1], members int32, mean float64 [m, 3]).
    The mean is summed one member at a time in the dtype of x, divided by the count in that dtype,
    then widened."""
    x = np.asarray(x)
    T = x.dtype.type
    n = x.shape[0]
    recorded = np.zeros(n, dtype=bool)
    cluster_of = np.full(n, -1, dtype=np.int32)
    member_start, members, mean = [0], [], []
    for j in range(n):
        nb = cols[row_start[j]:row_start[j + 1]]
        if recorded[nb].any():
            continue
        s = [T(x[nb[0], a]) for a in range(3)]
        for i in nb[1:]:
            s = [T(s[a] + x[i, a]) for a in range(3)]
        mean.append([np.float64(T(s[a] / T(len(nb)))) for a in range(3)])
        recorded[nb] = True
        cluster_of[nb] = len(mean) - 1
        members.extend(int(i) for i in nb)
        member_start.append(len(members))
    return (cluster_of, np.asarray(member_start, dtype=np.int32),
            np.asarray(members, dtype=np.int32), np.asarray(mean, dtype=np.float64).reshape(-1, 3))


def merge(x, ids, thr):
    """filter_points.merge's return value through the two steps above."""
    rs, cols = radius_neighbours(x, thr)
    _, ms, mem, mean = merge_greedy(x, rs, cols)
    ids = np.asarray(ids)
    return mean, {c: ids[mem[ms[c]:ms[c + 1]]] for c in range(len(ms) - 1)}


def lift(bank, block_offset, block_cols, obs_block, obs_feat, seg_len, dim):
    """-> (seg_start int32 [n3 + 1], collected float64 [dim, S], mean64 [dim, n3], mean32)."""
    S, n3 = len(obs_block), len(seg_len)
    collected = np.empty((dim, S), dtype=np.float64)
    ch = np.arange(dim, dtype=np.int64)
    for o in range(S):
        b, f = int(obs_block[o]), int(obs_feat[o])
        collected[:, o] = bank[int(block_offset[b]) + ch * int(block_cols[b]) + f]
    seg_start = np.zeros(n3 + 1, dtype=np.int32)
    seg_start[1:] = np.cumsum(seg_len)
    mean64 = np.empty((dim, n3), dtype=np.float64)
    for p in range(n3):
        s = collected[:, seg_start[p]].copy()
        for o in range(seg_start[p] + 1, seg_start[p + 1]):
            s = s + collected[:, o]
        mean64[:, p] = s / np.float64(seg_len[p])
    return seg_start, collected, mean64, mean64.astype(np.float32)


def gather_leaves(collected, cols):
    """-> float32 [dim, len(cols)]; cols == S is the dustbin column of ones."""
    dim, S = collected.shape
    cols = np.asarray(cols, dtype=np.int64)
    src = np.concatenate([collected.astype(np.float32), np.ones((dim, 1), np.float32)], axis=1)
    return src[:, cols]

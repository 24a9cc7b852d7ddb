"""The object builder's cases, shared by tests/golden/make_golden_object_builder.py (which writes
the fixture model with the reference's writer and records the reference's outputs) and the tests
(which regenerate the inputs from the seeds and compare digests).  The second half holds the edge
cases of tests/golden/make_golden_object_builder_edges.py: long clusters, wide-exponent lifting
banks past the first 1024-wide chunk, filter keep patterns, hand-built neighbour lists, threshold
and special-value clouds, and the wrong variants the host tests show them to separate."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_DIR = os.path.join(GOLDEN, "object_builder_model")
DIM = 256
THR = 1e-3
THR32 = float(np.float32(1e-3))   # a threshold that float32 coordinates can hit exactly
MAX_KP3D = 40
N_IMAGES = 10
IMG_LISTS = [f"seq/color/{k}.png" for k in range(N_IMAGES)]
MODEL_SEED, FEATURE_SEED = 2024, 77
MARGIN = 1e-6


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _rotation(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def box_corners(seed=MODEL_SEED):
    """8 x 3 corners; the filter reads corner 4 and its three edges to corners 5, 0 and 7."""
    rs = np.random.RandomState(seed + 1)
    R, centre, half = _rotation(rs), np.array([0.02, -0.01, 0.03]), np.array([0.08, 0.05, 0.06])
    signs = {4: (-1, -1, -1), 5: (1, -1, -1), 0: (-1, 1, -1), 7: (-1, -1, 1),
             1: (1, 1, -1), 6: (1, -1, 1), 3: (-1, 1, 1), 2: (1, 1, 1)}
    c = np.stack([centre + R @ (np.array(signs[k]) * half) for k in range(8)])
    return c, R, centre, half


def planted(rs, centre_fn, step=7e-4):
    """Groups of rows, each in the order its points must be met: (name, [offsets])."""
    e = np.array([1.0, 0.0, 0.0])
    groups = []
    for _ in range(4):
        d = rs.randn(3)
        groups.append(("dup", [np.zeros(3), 3e-4 * d / np.linalg.norm(d)]))
    groups.append(("triple", [np.zeros(3), 2e-4 * e, np.array([1e-4, 1.5e-4, 0.0])]))
    groups.append(("quad", [np.zeros(3), 2e-4 * e, np.array([0.0, 2e-4, 0.0]),
                            np.array([0.0, 0.0, 2e-4])]))
    groups.append(("chain_end", [np.zeros(3), step * e, 2 * step * e]))      # a b c: c is lost
    groups.append(("chain_mid", [step * e, np.zeros(3), 2 * step * e]))      # b a c: all three
    out = []
    for name, offs in groups:
        c = centre_fn()
        out.append((name, [c + o for o in offs]))
    return out


def margin_ok(p, corners):
    import object_builder_oracle as O
    return O.box_margin(np.asarray(p).reshape(-1, 3), corners) >= MARGIN


def model_spec(seed=MODEL_SEED):
    """The synthetic SfM model: 'ids' ascending, 'xyz' float64, per point its 'tracks' (image
    index, feature index), per image 'point3D_ids' and 'xys', 'groups' name -> row indices, and
    'file_order' (the order the points are written in)."""
    rs = np.random.RandomState(seed)
    corners, R, centre, half = box_corners(seed)

    def inside():
        while True:
            p = centre + R @ (rs.uniform(-0.9, 0.9, 3) * half)
            if margin_ok(p, corners):
                return p

    def outside():
        while True:
            u = rs.uniform(-0.9, 0.9, 3)
            u[rs.randint(3)] = rs.choice([-1, 1]) * rs.uniform(1.1, 1.6)
            p = centre + R @ (u * half)
            if margin_ok(p, corners):
                return p
    items = [("in", [inside()]) for _ in range(70)] + [("out", [outside()]) for _ in range(12)]
    while True:
        pl = planted(rs, inside)
        if all(margin_ok(np.stack(g), corners) for _, g in pl):
            break
    items += pl
    order = rs.permutation(len(items))
    xyz, groups, long_rows = [], {}, []
    for k in order:
        name, pts = items[k]
        rows = list(range(len(xyz), len(xyz) + len(pts)))
        xyz.extend(pts)
        if name not in ("in", "out"):
            groups.setdefault(name, []).append(rows)
            long_rows.extend(rows)
    xyz = np.stack(xyz)
    P = xyz.shape[0]
    ids = np.sort(rs.choice(np.arange(1, 6000), size=P, replace=False)).astype(np.int64)
    tlen = rs.randint(2, 9, size=P)
    tlen[long_rows] = 8
    per_image = [[] for _ in range(N_IMAGES)]   # (row) per observation
    for r in range(P):
        for k in rs.choice(N_IMAGES, size=tlen[r], replace=False):
            per_image[k].append(r)
    twice = groups["triple"][0][0]
    per_image[[k for k in range(N_IMAGES) if twice in per_image[k]][0]].append(twice)
    tracks = [[] for _ in range(P)]
    p3d, xys = [], []
    for k in range(N_IMAGES):
        n_k = len(per_image[k]) + 20
        slots = rs.permutation(n_k)[:len(per_image[k])]
        a = np.full(n_k, -1, dtype=np.int64)
        for r, s in zip(per_image[k], slots):
            a[s] = ids[r]
            tracks[r].append((k, int(s)))
        p3d.append(a)
        xys.append(rs.uniform(0, 480, size=(n_k, 2)))
    return {"ids": ids, "xyz": xyz, "tracks": tracks, "point3D_ids": p3d, "xys": xys,
            "groups": groups, "file_order": rs.permutation(P), "corners": corners}


def features(counts, seed=FEATURE_SEED, dim=DIM):
    """The per-image features mapping for images of ``counts[k]`` keypoints."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, n in zip(IMG_LISTS, counts):
        d = rs.randn(dim, n).astype(np.float32)
        d /= np.linalg.norm(d, axis=0, keepdims=True)
        out[name] = {"keypoints": rs.uniform(0, 480, size=(n, 2)).astype(np.float32),
                     "descriptors": d, "scores": rs.uniform(0.01, 1, size=n).astype(np.float32)}
    return out


def features_sha(f):
    return sha(*[f[n][k] for n in IMG_LISTS for k in ("keypoints", "descriptors", "scores")])


# ------------------------------------------------------------------ stand-alone merge cases
MERGE_CASES = {"f64": (np.float64, THR, 260, 11), "f32": (np.float32, THR, 200, 12),
               "f32e": (np.float32, THR32, 64, 13)}


def merge_case(name):
    """-> (xyz of the case's dtype [n, 3], ids int64 [n], thr, groups: name -> lists of rows)."""
    dtype, thr, n_single, seed = MERGE_CASES[name]
    rs = np.random.RandomState(seed)
    items = [("single", [rs.uniform(1.0, 2.0, 3)]) for _ in range(n_single)]
    items += planted(rs, lambda: rs.uniform(1.0, 2.0, 3), step=7e-4)
    # pairs whose distance is the threshold or a neighbour of it: one coordinate is 0 in the
    # first point and d in the second, so the difference is d itself
    if dtype == np.float64:
        ds = [np.nextafter(thr, 0.0), thr, np.nextafter(thr, 1.0)]
    elif thr == THR32:
        ds = [thr] * 2
    else:
        ds = []   # float32 coordinates cannot come within an ulp of the double 1e-3
    k = 0
    for d in ds:
        for axis in range(2):
            p = np.array([3.0 + k, 5.0, 7.0])
            p[axis] = 0.0
            q = p.copy()
            q[axis] = d
            items.append(("edge", [p, q]))
            k += 1
    order = rs.permutation(len(items))
    xyz, groups = [], {}
    for o in order:
        nm, pts = items[o]
        rows = list(range(len(xyz), len(xyz) + len(pts)))
        xyz.extend(pts)
        if nm != "single":
            groups.setdefault(nm, []).append(rows)
    xyz = np.stack(xyz).astype(dtype)
    ids = rs.permutation(np.arange(100, 100 + 3 * len(xyz), 3))[:len(xyz)].astype(np.int64)
    return xyz, ids, thr, groups


def flatten_clusters(ret_idxs):
    """{new: old ids} -> (lengths int64 [m], concatenated ids int64)."""
    lens = np.asarray([len(v) for v in ret_idxs.values()], dtype=np.int64)
    flat = (np.concatenate([np.asarray(v, dtype=np.int64) for v in ret_idxs.values()])
            if len(lens) else np.zeros(0, np.int64))
    assert list(ret_idxs.keys()) == list(range(len(lens)))
    return lens, flat


# ------------------------------------------------------------------ the edge cases
# (tests/golden/make_golden_object_builder_edges.py records the reference's outputs for them in
# tests/golden/object_builder_edges.npz)
LONG_SIZES = (63, 64, 65, 128, 129, 200)
LONG_RADIUS = 4e-4          # every pair of a ball of this radius is below THR
# a table of their own: MERGE_CASES is what make_golden_object_builder.py writes into
# object_builder.npz and what the first suite's tests look up there, and that file stays as it is
LONG_MERGE_CASES = {"long64": (np.float64, THR, 300, 21), "long32": (np.float32, THR, 300, 22)}


def _ball(rs, k, radius):
    d = rs.randn(k, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True) * (radius * rs.uniform(0.05, 1.0, (k, 1)))


def long_merge_case(name):
    """merge_case's singles and planted groups, plus clusters of LONG_SIZES distinct members each
    inside a ball of LONG_RADIUS (members scattered over the rows, group "L<size>"), plus group
    "skip": 65 members in consecutive rows and then a point e that is near the last member and
    far from the first, so the last member's row has 66 entries, is skipped, and e is lost.
    -> (xyz, ids, thr, groups) as merge_case."""
    dtype, thr, n_single, seed = LONG_MERGE_CASES[name]
    rs = np.random.RandomState(seed)
    items = [("single", [rs.uniform(1.0, 2.0, 3)]) for _ in range(n_single)]
    items += planted(rs, lambda: rs.uniform(1.0, 2.0, 3), step=7e-4)
    for size in LONG_SIZES:
        c = rs.uniform(1.0, 2.0, 3)
        items += [(f"L{size}", [q]) for q in c + _ball(rs, size, LONG_RADIUS)]
    c, e = rs.uniform(1.0, 2.0, 3), np.array([1.0, 0.0, 0.0])
    body = c + _ball(rs, 63, 0.5 * LONG_RADIUS)
    items.append(("skip", [c - 3.9e-4 * e] + list(body) + [c + 3.9e-4 * e, c + 1.0e-3 * e]))
    order = rs.permutation(len(items))
    xyz, groups = [], {}
    for o in order:
        nm, pts = items[o]
        rows = list(range(len(xyz), len(xyz) + len(pts)))
        xyz.extend(pts)
        if nm != "single":
            groups.setdefault(nm, []).append(rows)
    xyz = np.stack(xyz).astype(dtype)
    ids = rs.permutation(np.arange(100, 100 + 3 * len(xyz), 3))[:len(xyz)].astype(np.int64)
    return xyz, ids, thr, groups


def long_rows(groups):
    """name -> the ascending rows of each long cluster ("skip": without the lost point)."""
    out = {f"L{s}": sorted(r for g in groups[f"L{s}"] for r in g) for s in LONG_SIZES}
    out["skip"] = groups["skip"][0][:65]
    return out


def mean_in_order(x, rows, chunk=None):
    """The cluster position of x[rows] summed in the given order in x's dtype; with ``chunk`` as
    partial sums of that many members, themselves summed in order (a WRONG variant)."""
    T = x.dtype.type
    if chunk is None:
        parts = [rows]
    else:
        parts = [rows[k:k + chunk] for k in range(0, len(rows), chunk)]
    sums = []
    for part in parts:
        s = x[part[0]].copy()
        for i in part[1:]:
            s = s + x[i]
        sums.append(s)
    s = sums[0]
    for t in sums[1:]:
        s = s + t
    return (s / T(len(rows))).astype(np.float64)


def cloud_points(n, dtype):
    """n points with natural near pairs (a dense corner) and, from 64 on, planted duplicates,
    clusters and both chains."""
    rs = np.random.RandomState(900 + n)
    items = []
    if n >= 64:
        items = planted(rs, lambda: rs.uniform(0.2, 1.0, 3))
    elif n == 2:
        items = [("dup", [np.full(3, 0.5), np.array([0.5, 0.5003, 0.5])])]
    left = n - sum(len(p) for _, p in items)
    dense = left // 8 if n >= 257 else 0
    side = 0.0125 * (dense / 512.0) ** (1 / 3) if dense else 0.0
    items += [("s", [rs.uniform(0.0, side, 3)]) for _ in range(dense)]
    items += [("s", [rs.uniform(0.2, 1.0, 3)]) for _ in range(left - dense)]
    x = np.concatenate([np.stack(items[k][1]) for k in rs.permutation(len(items))]).astype(dtype)
    assert x.shape == (n, 3)
    return x


# ---- lifting
def lift_inputs_old(dim):
    """The first suite's lifting case: n3 = 11, 869 observations, 5 blocks, a randn bank."""
    rs = np.random.RandomState(70 + dim)
    ncols = np.array([300, 257, 64, 411, 90], dtype=np.int32)     # block 2 is used by nobody
    off = np.concatenate([[0], np.cumsum(ncols[:-1].astype(np.int64) * dim)]).astype(np.int64)
    bank = rs.randn(int((ncols.astype(np.int64) * dim).sum())).astype(np.float32)
    seg = np.array([1, 2, 63, 64, 65, 519, 1, 7, 8, 9, 130], dtype=np.int32)
    S = int(seg.sum())
    blk = rs.choice([0, 1, 3, 4], size=S).astype(np.int32)
    feat = (rs.randint(0, 1 << 30, size=S) % ncols[blk]).astype(np.int32)
    return bank, off, ncols, blk, feat, seg


LIFT_N3 = (1023, 1024, 1025, 2049, 2500)
LIFT_BLOCKS, LIFT_UNUSED = 1500, 9
# (n3, dim) that the GPU tests run; the generator records the reference's mean for each, and for
# LIFT_REF_DIMS at n3 = 2500
LIFT_GPU = [(n3, d) for n3 in LIFT_N3 for d in (256, 3)] + [(1025, d) for d in (1, 2, 5, 1024)]
LIFT_REF_DIMS = (256, 128, 5, 3, 2, 1)
LIFT_ALL = sorted(set(LIFT_GPU) | {(2500, d) for d in LIFT_REF_DIMS})


def lift_structure(n3):
    """(block_cols, obs_block, obs_feat, seg_len): segments of 1..11 observations, one of 519 at
    point 3, one of 1300 at point 5 (it straddles observation 1024) and one of 65 as the last;
    1500 blocks of 1..39 columns, LIFT_UNUSED of them used by nobody."""
    rs = np.random.RandomState(5000 + n3)
    ncols = rs.randint(1, 40, size=LIFT_BLOCKS).astype(np.int32)
    unused = rs.choice(LIFT_BLOCKS, LIFT_UNUSED, replace=False)
    seg = rs.randint(1, 12, size=n3).astype(np.int32)
    seg[3], seg[5], seg[-1] = 519, 1300, 65
    S = int(seg.sum())
    used = np.setdiff1d(np.arange(LIFT_BLOCKS), unused)
    blk = rs.choice(used, size=S).astype(np.int32)
    feat = (rs.randint(0, 1 << 30, size=S) % ncols[blk]).astype(np.int32)
    start = int(seg[:5].sum())
    assert start < 1024 < start + 1300 and not np.isin(unused, blk).any()
    return ncols, blk, feat, seg


def lift_inputs(n3, dim, wide=True):
    """-> (bank, block_offset, block_cols, obs_block, obs_feat, seg_len).  ``wide``: the bank is
    randn * 2^randint(-30, 31), so a float64 sum of it depends on its order; otherwise plain
    randn, whose float64 sums are exact in any order."""
    ncols, blk, feat, seg = lift_structure(n3)
    total = int(ncols.astype(np.int64).sum()) * dim
    rs = np.random.RandomState(6000 + dim)
    bank = rs.randn(total)
    if wide:
        bank = bank * 2.0 ** rs.randint(-30, 31, size=total)
    off = np.concatenate([[0], np.cumsum(ncols[:-1].astype(np.int64) * dim)]).astype(np.int64)
    return bank.astype(np.float32), off, ncols, blk, feat, seg


def lift_blocks(bank, off, ncols, dim):
    """The bank as lift_descriptors' per-image [dim, n_i] list."""
    return [bank[int(o):int(o) + dim * int(c)].reshape(dim, int(c)) for o, c in zip(off, ncols)]


def segment_means(collected, seg, how):
    """WRONG variants of the descriptor mean on collected [dim, S]: 'reversed' sums each segment
    from its last observation, 'pairwise' lets numpy sum the contiguous row."""
    dim, n3 = collected.shape[0], len(seg)
    start = np.concatenate([[0], np.cumsum(seg)])
    out = np.empty((dim, n3))
    for p in range(n3):
        blk = collected[:, start[p]:start[p + 1]]
        if how == "pairwise":
            out[:, p] = np.sum(np.ascontiguousarray(blk), axis=1) / np.float64(seg[p])
        else:
            s = blk[:, -1].copy()
            for o in range(blk.shape[1] - 2, -1, -1):
                s = s + blk[:, o]
            out[:, p] = s / np.float64(seg[p])
    return out


# ---- filter
FILTER_N = (1023, 1024, 1025, 2047, 2048, 2049, 3073)
FILTER_PATTERNS = ("all", "none", "first", "last", "hole", "alternate")


def filter_pattern(n, name):
    """Track lengths (kept: 5, dropped: 1, min_track 3) that keep the named points."""
    i = np.arange(n)
    keep = {"all": i >= 0, "none": i < 0, "first": i % 1024 == 0,
            "last": (i % 1024 == 1023) | (i == n - 1), "hole": i // 1024 != 1,
            "alternate": i % 2 == 0}[name]
    return np.where(keep, 5, 1).astype(np.int32)


# ---- hand-built CSRs for the merge pass (n = 130: two groups of 64 rows and a tail of 2)
CSR_N = 130
CSR_CASES = ("lanes", "consecutive", "group_multi", "all_alone", "seen_at_100", "row_order",
             "asym_ab", "asym_ba", "not_self")


def csr_case(name, dtype):
    """-> (x [130, 3] distinct, row_start int64 [131], cols int32).  Rows not named below hold
    their own point alone."""
    n = CSR_N
    x = np.random.RandomState(300).uniform(1.0, 2.0, (n, 3)).astype(dtype)
    rows = {j: [j] for j in range(n)}
    if name == "lanes":             # not alone at lanes 0, 63, 64, 127, 128, 129
        for a, b in ((0, 5), (63, 70), (64, 90), (100, 127), (128, 129)):
            rows[a] = rows[b] = [a, b]
    elif name == "consecutive":     # row 11 is skipped because of row 10
        rows[10] = rows[11] = [10, 11]
        rows[12] = rows[77] = [12, 77]
    elif name == "group_multi":     # rows 64..127 all not alone, rows 0..63 all alone
        for a in range(64, 128, 2):
            rows[a] = rows[a + 1] = [a, a + 1]
    elif name == "seen_at_100":     # row 1: 130 entries, the only recorded one (0) at entry 100
        r = list(range(1, n))
        rows[1] = r[:100] + [0] + r[100:]
    elif name == "row_order":       # row 0: points 0..128 in an order that is not ascending
        rows[0] = np.random.RandomState(301).permutation(129).tolist()
    elif name == "asym_ab":         # row 20 = {20, 40}, row 40 = {40}: 40 must not start a cluster
        rows[20] = [20, 40]
    elif name == "asym_ba":         # row 20 = {20}, row 40 = {40, 20}: 40 is skipped and lost
        rows[40] = [40, 20]
    elif name == "not_self":        # rows that do not name their own point
        rows[30] = [31]
        rows[50] = [51, 52]
        rows[127] = [128]
    else:
        assert name == "all_alone"
    lens = [len(rows[j]) for j in range(n)]
    rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return x, rs, np.concatenate([rows[j] for j in range(n)]).astype(np.int32)


# ---- neighbour search: thresholds, special values, separating pairs
def small_cloud():
    """200 float64 points in [0.2, 1]^3 with the planted groups (threshold 1e-3)."""
    return cloud_points(200, np.float64)


def threshold_cases():
    """name -> (x, thr): the cloud and the threshold scaled together across ob_bound's limits."""
    base = small_cloud()
    out = {}
    for nm, thr in (("f64_1e-150", 1e-150), ("f64_1e144", 1e144), ("f64_1e-140", 1e-140),
                    ("f64_above_1e-140", float(np.nextafter(1e-140, 1.0))), ("f64_1e140", 1e140)):
        out[nm] = (base * (thr / THR), thr)
    for nm, thr in (("f32_1e-30", 1e-30), ("f32_1e30", 1e30)):
        out[nm] = ((base * (thr / THR)).astype(np.float32), thr)
    return out


def sq_separator():
    """A float64 pair at THR32 whose squared distance is one ulp below THR32 * THR32 while its
    root rounds to THR32: `s < thr * thr` calls it a neighbour, `sqrt(s) < thr` does not.  (At
    thr = 1e-3 no such s exists: there the two tests agree on every double.)"""
    thr = THR32
    rs = np.random.RandomState(1)
    dx = rs.uniform(0.3, 0.9, 400) * thr
    dy = np.sqrt(thr * thr - dx * dx)
    dy = (dy.view(np.int64) + rs.randint(-4, 5, 400)).view(np.float64)
    s = (dx * dx + dy * dy) + 0.0
    k = np.nonzero((np.sqrt(s) < thr) != (s < thr * thr))[0][0]
    return np.array([[0.0, 0.0, 9.0], [dx[k], dy[k], 9.0]])


def f32_separator():
    """A float32 pair that float32 distance arithmetic and the contract's float64 arithmetic
    place on different sides of 1e-3."""
    rs = np.random.RandomState(2)
    dx = (rs.uniform(0.3, 0.9, 400) * THR).astype(np.float32)
    dy = np.sqrt(THR ** 2 - dx.astype(np.float64) ** 2).astype(np.float32)
    dy = (dy.view(np.int32) + rs.randint(-3, 4, 400).astype(np.int32)).view(np.float32)
    xd, yd = dx.astype(np.float64), dy.astype(np.float64)
    want = np.sqrt((xd * xd + yd * yd) + 0.0) < THR
    got = np.sqrt((dx * dx + dy * dy) + np.float32(0)).astype(np.float64) < THR
    k = np.nonzero(want != got)[0][0]
    return np.array([[0.0, 0.0, 11.0], [dx[k], dy[k], 11.0]], dtype=np.float32)


def special_cloud(dtype):
    """(x, thr = 1e-3): 60 ordinary points, then a NaN coordinate, two points at +inf in one
    coordinate (inf - inf is NaN: not neighbours), a planted close pair, the float32 separator
    and, in float64, two coordinates of 1e200 whose squared distance overflows."""
    rs = np.random.RandomState(310)
    p = [rs.uniform(0.2, 1.0, (60, 3)), [[0.5, np.nan, 0.5]], [[np.inf, 0.3, 0.3]],
         [[np.inf, 0.3, 0.3002]], [[0.4, 0.4, 0.4], [0.4, 0.4003, 0.4]],
         f32_separator().astype(np.float64)]
    if dtype == np.float64:
        p.append([[1e200, 1.0, 1.0], [2e200, 1.0, 1.0]])
    return np.concatenate([np.asarray(a, dtype=np.float64) for a in p]).astype(dtype), THR


def underflow_case():
    """(x float64, thr = 1e-160): a pair 1e-170 apart, whose squares underflow to zero, and
    points 1e-150 and 1 away."""
    return np.array([[0.0, 0.0, 0.0], [1e-170, 0.0, 0.0], [1e-150, 0.0, 0.0],
                     [1.0, 1.0, 1.0], [0.0, 1e-170, 1e-170]]), 1e-160


def pruned_neighbours(x, thr):
    """O.radius_neighbours' CSR without the n x n walk: sort on x, candidates with
    |dx| <= thr (1 + 1e-9) (sqrt(s) >= |dx| up to rounding far below 1e-9), then the oracle's
    per-pair expression.  Points whose x is not finite are tested against everyone."""
    xd = np.asarray(x).astype(np.float64)
    n = xd.shape[0]
    fin = np.nonzero(np.isfinite(xd[:, 0]))[0]
    odd = np.nonzero(~np.isfinite(xd[:, 0]))[0]
    order = fin[np.argsort(xd[fin, 0], kind="stable")]
    xs = xd[order, 0]
    w = thr * (1 + 1e-9)
    pi, pj = [order], [order]                # i == j always counts
    k = 1
    while k < len(order):
        near = np.nonzero(xs[k:] - xs[:-k] <= w)[0]
        if near.size == 0:
            break
        pi.append(order[near])
        pj.append(order[near + k])
        k += 1
    a, b = np.concatenate(pi), np.concatenate(pj)
    if len(odd):
        every = np.arange(n)
        a = np.concatenate([a] + [np.full(n, o) for o in odd])
        b = np.concatenate([b] + [every for _ in odd])
    with np.errstate(invalid="ignore", over="ignore"):
        d = xd[a] - xd[b]
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        hit = (np.sqrt(s) < thr) | (a == b)
    a, b = a[hit], b[hit]
    key = np.unique(np.concatenate([a * n + b, b * n + a]))      # both directions, ascending
    jj, ii = key // n, key % n
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(jj, minlength=n), out=row_start[1:])
    return row_start, ii.astype(np.int32)


BIG_N = 65536


def big_cloud():
    """65536 float32 points, uniform in [0, 1]^3, with 24 planted pairs (one of them rows 0 and
    40000) and a triple at rows 1, 65534 and 65535.  -> (x, pairs [(a, b)], triple)."""
    rs = np.random.RandomState(65536)
    x = rs.uniform(0.0, 1.0, (BIG_N, 3))
    pairs = [(0, 40000)] + [tuple(int(v) for v in rs.choice(np.arange(2, BIG_N - 2), 2, replace=False))
                            for _ in range(23)]
    for a, b in pairs:
        d = rs.randn(3)
        x[b] = x[a] + 3e-4 * d / np.linalg.norm(d)
    triple = (1, BIG_N - 2, BIG_N - 1)
    x[triple[1]] = x[1] + np.array([2e-4, 0.0, 0.0])
    x[triple[2]] = x[1] + np.array([1e-4, 1.5e-4, 0.0])
    return x.astype(np.float32), pairs, triple


# ---- an in-memory SfM model at scale
CHAIN_IMAGES = [f"seq/color/{k}.png" for k in range(12)]
CHAIN_TKL = 3


def chain_model(seed=4100, n_points=3000, dim=DIM):
    """-> (points, images, corners, descriptors): the dicts read_points3d_binary and
    read_images_binary return, for 3000 points (a tenth of them 3e-4 from an earlier one) seen
    in 2..6 of 12 images, and per image a wide-exponent [dim, n_i] descriptor block."""
    rs = np.random.RandomState(seed)
    corners, R, centre, half = box_corners()
    xyz = centre + (rs.uniform(-1.15, 1.15, (n_points, 3)) * half) @ R.T
    twin = rs.choice(np.arange(1, n_points), n_points // 10, replace=False)
    d = rs.randn(len(twin), 3)
    xyz[twin] = xyz[twin - 1] + 3e-4 * d / np.linalg.norm(d, axis=1, keepdims=True)
    ids = np.sort(rs.choice(np.arange(1, 40000), size=n_points, replace=False)).astype(np.int64)
    tlen = rs.randint(2, 7, size=n_points).astype(np.int64)
    n_img = len(CHAIN_IMAGES)
    per_image = [[] for _ in range(n_img)]
    for r in range(n_points):
        for k in rs.choice(n_img, size=tlen[r], replace=False):
            per_image[k].append(r)
    p3d, desc = [], []
    for k in range(n_img):
        n_k = len(per_image[k]) + 30
        a = np.full(n_k, -1, dtype=np.int64)
        a[rs.permutation(n_k)[:len(per_image[k])]] = ids[per_image[k]]
        p3d.append(a)
        desc.append((rs.randn(dim, n_k) * 2.0 ** rs.randint(-30, 31, (dim, n_k))).astype(np.float32))
    points = {"ids": ids, "xyz": xyz, "track_len": tlen, "file_order": rs.permutation(n_points)}
    images = {"image_ids": np.arange(1, n_img + 1, dtype=np.int32), "names": list(CHAIN_IMAGES),
              "point3D_ids": p3d}
    return points, images, corners, desc

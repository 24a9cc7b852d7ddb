"""The object builder's cases, shared by tests/golden/make_golden_object_builder.py (which writes
the fixture model with the reference's writer and records the reference's outputs) and the tests
(which regenerate the inputs from the seeds and compare digests)."""
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

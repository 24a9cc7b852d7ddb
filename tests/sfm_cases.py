"""Seeded inputs of the sparse-reconstruction tests, shared by tests/golden/make_golden_sfm.py,
tests/golden/make_golden_sfm_edges.py and the test files so that all see the same bytes (the
generators record a hash)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_REPROJ, MIN_ANGLE = 4.0, 1.5
F, C = 600.0, 256.0   # K of a 512 x 512 crop


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


# ---- graphs ---------------------------------------------------------------------------------
def path_graph(n, order, seed=0):
    """A path through n nodes whose ids along the path are sorted, reversed, zig-zag or random."""
    ids = np.arange(n)
    if order == "reversed":
        ids = ids[::-1].copy()
    elif order == "zigzag":
        ids = np.stack([np.arange((n + 1) // 2), n - 1 - np.arange((n + 1) // 2)], 1).reshape(-1)[:n]
    elif order == "random":
        ids = np.random.default_rng(seed).permutation(n)
    return np.stack([ids[:-1], ids[1:]], axis=1).astype(np.int32)


def graph_cases():
    """name -> (edges int32 [E, 2], n_nodes)."""
    cases = {f"empty{n}": (np.zeros((0, 2), np.int32), n) for n in (1, 2, 63, 64, 65, 257, 1025)}
    for n in (300, 1025):
        for order in ("sorted", "reversed", "zigzag", "random"):
            cases[f"path{n}_{order}"] = (path_graph(n, order, seed=n), n)
    even, odd = np.arange(0, 40, 2), np.arange(1, 40, 2)
    cases["interleaved"] = (np.concatenate([np.stack([even[:-1], even[1:]], 1)[::-1],
                                            np.stack([odd[1:], odd[:-1]], 1)]).astype(np.int32), 40)
    loops = np.array([[3, 3], [5, 5], [3, 5], [9, 9], [0, 0]], np.int32)
    cases["self_loops"] = (loops, 12)
    dup = path_graph(70, "random", seed=7)
    cases["duplicates"] = (np.concatenate([dup, dup[::-1], dup[:, ::-1]]), 70)
    cases["block_edge"] = (path_graph(258, "random", seed=8), 300)   # 257 edges: 256 + 1
    oor = path_graph(100, "random", seed=9)
    bad = np.array([[-1, 4], [4, 100], [2**31 - 1, 0], [-2**31, -2**31], [50, -7]], np.int32)
    cases["out_of_range"] = (np.concatenate([oor[:50], bad, oor[50:]]), 100)
    cases.update(large_graph_cases())
    return cases


LARGE_GRAPHS = ("star2000_hub_last", "star2000_hub0", "complete40", "grid64_shuffled",
                "sparse65537", "two_paths500_joined")
SPARSE_NODES, SPARSE_EDGES = 65537, 60000


def large_graph_cases():
    """Graphs with a hub, a dense graph, more nodes than a few blocks: name -> (edges, n_nodes).
    star2000_hub_last / _hub0: 2000 leaves around the highest / the lowest id (every edge of one
    launch hooks the same root, or every root hooks node 0); complete40: every ordered pair;
    grid64_shuffled: a 64 x 64 grid under a permutation of the ids; sparse65537: 60 000 random
    edges over 65 537 nodes (a giant component, thousands of small ones, isolated nodes);
    two_paths500_joined: two random-order paths whose joining edge is the last of the list."""
    cases = {}
    leaves = np.arange(2000)
    cases["star2000_hub_last"] = (np.stack([leaves, np.full(2000, 2000)], 1).astype(np.int32), 2001)
    cases["star2000_hub0"] = (np.stack([np.zeros(2000, np.int64), leaves + 1], 1).astype(np.int32),
                              2001)
    u, v = np.nonzero(~np.eye(40, dtype=bool))
    cases["complete40"] = (np.stack([u, v], 1).astype(np.int32), 40)
    ids = np.random.default_rng(64).permutation(64 * 64).reshape(64, 64)
    cases["grid64_shuffled"] = (np.concatenate(
        [np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1),
         np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1)]).astype(np.int32), 64 * 64)
    cases["sparse65537"] = (np.random.default_rng(65537).integers(
        0, SPARSE_NODES, (SPARSE_EDGES, 2)).astype(np.int32), SPARSE_NODES)
    a, b = path_graph(500, "random", seed=500), path_graph(500, "random", seed=501) + 500
    cases["two_paths500_joined"] = (np.concatenate(
        [a, b, np.array([[a[-1, 1], b[0, 0]]], np.int32)]).astype(np.int32), 1000)
    return cases


OUT_OF_RANGE_COUNT = 5


# ---- cameras and tracks ---------------------------------------------------------------------
def look_at(centre, target=(0.0, 0.0, 0.0)):
    """World-to-camera [3, 4] of a camera at `centre` looking at `target` (z forward)."""
    c, t = np.asarray(centre, float), np.asarray(target, float)
    z = (t - c) / np.linalg.norm(t - c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ c)[:, None]], axis=1)


def project(Rt, K4, X):
    p = Rt[:, :3] @ X + Rt[:, 3]
    return np.array([K4[0] * p[0] / p[2] + K4[2], K4[1] * p[1] / p[2] + K4[3]])


def ring_cameras(m, seed):
    """m cameras 0.45 .. 0.6 m from the origin on a band of +-35 degrees elevation."""
    rng = np.random.default_rng(seed)
    az = 2 * np.pi * (np.arange(m) + rng.uniform(-0.2, 0.2, m)) / m
    el = np.deg2rad(rng.uniform(-35, 35, m))
    r = rng.uniform(0.45, 0.6, m)
    cs = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1)
    Rt = np.stack([look_at(c) for c in cs])
    K4 = np.stack([F + rng.uniform(-20, 20, m), F + rng.uniform(-20, 20, m),
                   C + rng.uniform(-5, 5, m), C + rng.uniform(-5, 5, m)], 1)
    return Rt, K4


TRI_CAMERAS = 260
ANGLE_RAYS_SHIFT = -3.5
TRI_NAMES = ("len2", "len3", "len17", "len63", "len64", "len65", "len130", "len256",
             "one_outlier", "several_outliers", "two_in_one_image", "behind_one_camera",
             "angle_below", "angle_above", "wrong_match", "len1", "len257", "nan_pixel",
             "angle_rays")
TRI_REFINED = ("len2", "len3", "len17", "len63", "len64", "len65", "len130", "len256",
               "one_outlier", "several_outliers", "two_in_one_image", "behind_one_camera",
               "angle_above")


def tri_problem(seed=4100):
    """All triangulation cases as one CSR: -> dict(Rt, K4, track_start, obs_image, obs_xy),
    names in TRI_NAMES order.  Cameras 0..259 lie on the band; 260 looks away from the object
    (the point is behind it); 261..263 sit 1.4 and 1.6 degrees apart as seen from the origin; 264
    sits 1.2 degrees from 261 and 265 is 261 again under another id (angle_rays: the third pixel
    is 3.5 px off, so its image ray open past 1.5 degrees while the angle at X stays below)."""
    rng = np.random.default_rng(seed)
    Rt, K4 = ring_cameras(TRI_CAMERAS, seed)
    away = look_at((0.5, 0.0, 0.0), target=(1.0, 0.0, 0.05))
    base = np.array([0.5, 0.0, 0.0])

    def turned(deg):
        a = np.deg2rad(deg)
        return look_at((0.5 * np.cos(a), 0.5 * np.sin(a), 0.0))
    Rt = np.concatenate([Rt, away[None], look_at(base)[None], turned(1.4)[None], turned(1.6)[None],
                         turned(1.2)[None], look_at(base)[None]])
    K4 = np.concatenate([K4, np.tile([[F, F, C, C]], (6, 1))])
    start, img, xy = [0], [], []

    def track(cams, X, noise=0.5, shift=None):
        for k, c in enumerate(cams):
            uv = project(Rt[c], K4[c], X) + noise * rng.standard_normal(2)
            if shift is not None and k in shift:
                uv = uv + shift[k]
            img.append(c)
            xy.append(uv)
        start.append(len(img))

    def point():
        return rng.uniform(-0.1, 0.1, 3)
    for n in (2, 3, 17, 63, 64, 65, 130, 256):
        cams = rng.permutation(TRI_CAMERAS)[:n]
        if n == 2:
            cams = np.array([10, 70])   # a wide baseline
        track(cams, point())
    track(rng.permutation(TRI_CAMERAS)[:17], point(), shift={5: np.array([60.0, -45.0])})
    track(rng.permutation(TRI_CAMERAS)[:20], point(),
          shift={1: np.array([90.0, 10.0]), 7: np.array([-30.0, 55.0]),
                 12: np.array([25.0, 25.0]), 19: np.array([-70.0, -70.0])})
    cams = rng.permutation(TRI_CAMERAS)[:6]
    track(np.concatenate([cams, cams[2:3]]), point(), shift={6: np.array([2.0, -1.5])})
    track(np.concatenate([rng.permutation(TRI_CAMERAS)[:5], [260]]), point())
    track([261, 262], np.zeros(3), noise=0.0)
    track([261, 263], np.zeros(3), noise=0.0)
    track([10, 70], point(), shift={1: np.array([0.0, 120.0])})
    track([3], point())
    track(np.arange(257), point())
    track(rng.permutation(TRI_CAMERAS)[:9], point(), shift={4: np.array([np.nan, 0.0])})
    track([261, 264, 265], np.zeros(3), noise=0.0, shift={2: np.array([ANGLE_RAYS_SHIFT, 0.0])})
    assert len(start) - 1 == len(TRI_NAMES)
    return {"Rt": Rt, "K4": K4, "track_start": np.asarray(start, np.int32),
            "obs_image": np.asarray(img, np.int32), "obs_xy": np.asarray(xy, np.float64)}


def tri_sha(p):
    return sha(*[p[k] for k in sorted(p)])


# ---- the edge cases of the triangulation ------------------------------------------------------
EDGE_NAMES = ("drop_past_64", "dup_past_64", "dup_exact_tie", "empty_mid", "behind_two",
              "final_check_drop", "noise_free", "mostly_unrelated", "same_centre", "same_ray",
              "parallel_rays", "empty_last")
EDGE_KEPT = ("drop_past_64", "dup_past_64", "dup_exact_tie", "behind_two", "final_check_drop",
             "noise_free")   # reason 0 by construction, compared in bits
EDGE_DEGENERATE = ("same_centre", "same_ray", "parallel_rays")   # the Jacobi oracle's decisions only
EDGE_DROPS = {"drop_past_64": (3, 64, 67, 130, 199), "behind_two": (1, 70)}
EDGE_TIES = ((2, 6), (3, 67), (10, 70))   # dup_exact_tie: (the original, its byte copy)
EDGE_DUPS = ((5, 69), (10, 100, 139))   # dup_past_64: positions that share an image
FINAL_CHECK_SEED = 370   # make_golden_sfm_edges.py --search: the widest margin below 600
EDGE_AWAY, EDGE_SAME_CENTRE, EDGE_COPY_OF, EDGE_COPY = (260, 261), (262, 263), 7, 264
EDGE_PARALLEL = (265, 266)
UNRELATED_SEED = 19   # of 40 tried: two observations survive 62 drops, the widest margin


def final_check_track(seed, Rt, K4):
    """4 observations of one point, 0.5 px noise, one shifted by 3.6 .. 4.6 px in a random
    direction -> (cams, uv [4, 2]).  Seeded on its own: the search for a seed at which the shifted
    observation passes at the DLT point and fails at the refined one changes nothing else."""
    rng = np.random.default_rng(seed)
    cams = rng.permutation(TRI_CAMERAS)[:4]
    X = rng.uniform(-0.1, 0.1, 3)
    uv = np.stack([project(Rt[c], K4[c], X) for c in cams]) + 0.5 * rng.standard_normal((4, 2))
    a = rng.uniform(0, 2 * np.pi)
    uv[rng.integers(0, 4)] += rng.uniform(3.6, 4.6) * np.array([np.cos(a), np.sin(a)])
    return cams, uv


def edge_problem(seed=4300, final_check_seed=None, unrelated_seed=None):
    """A second CSR beside tri_problem(), tracks in EDGE_NAMES order.  Cameras 0..259 are
    tri_problem()'s band; 260 and 261 look away from the object (every point is behind them); 262
    and 263 share a centre and differ in orientation; 264 is camera 7 again under another id; 265
    and 266 have R = I and centres 0.1 m apart, and parallel_rays gives both their principal
    point: the rows' third entries are exact zeros, the Jacobi's vector is (0, 0, 1, 0) and
    X = h[0:3] / h[3] is (NaN, NaN, inf)."""
    rng = np.random.default_rng(seed)
    Rt, K4 = ring_cameras(TRI_CAMERAS, 4100)
    centre = (0.0, -0.5, 0.1)
    extra = [look_at((0.5, 0.0, 0.0), target=(1.0, 0.0, 0.05)),
             look_at((0.0, 0.5, 0.1), target=(0.05, 1.0, 0.1)),
             look_at(centre), look_at(centre, target=(0.06, 0.0, 0.03)), Rt[EDGE_COPY_OF],
             np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1),
             np.concatenate([np.eye(3), [[0.1], [0.0], [0.5]]], 1)]
    Rt = np.concatenate([Rt, np.stack(extra)])
    K4 = np.concatenate([K4, np.tile([[F, F, C, C]], (4, 1)), K4[EDGE_COPY_OF][None],
                         np.tile([[F, F, C, C]], (2, 1))])
    start, img, xy = [0], [], []

    def track(cams, X, noise=0.5, shift=None):
        for k, c in enumerate(cams):
            uv = project(Rt[c], K4[c], X) + noise * rng.standard_normal(2)
            if shift is not None and k in shift:
                uv = uv + shift[k]
            img.append(int(c))
            xy.append(uv)
        start.append(len(img))

    def point():
        return rng.uniform(-0.1, 0.1, 3)

    def gross(lo=30.0, hi=110.0):
        a = rng.uniform(0, 2 * np.pi)
        return rng.uniform(lo, hi) * np.array([np.cos(a), np.sin(a)])
    # drop_past_64
    track(rng.permutation(TRI_CAMERAS)[:200], point(),
          shift={p: gross() for p in EDGE_DROPS["drop_past_64"]})
    # dup_past_64: 5 and 69 fall in one lane, 10, 100 and 139 in three
    cams = rng.permutation(TRI_CAMERAS)[:140]
    for first, *rest in EDGE_DUPS:
        cams[rest] = cams[first]
    track(cams, point())
    # dup_exact_tie: byte copies, image id and pixel
    base = len(img)
    track(rng.permutation(TRI_CAMERAS)[:80], point())
    for src, dst in EDGE_TIES:
        img[base + dst], xy[base + dst] = img[base + src], xy[base + src].copy()
    start.append(len(img))   # empty_mid
    # behind_two: the projection formula gives a pixel with a small residual at a negative depth
    cams = rng.permutation(TRI_CAMERAS)[:80]
    cams[list(EDGE_DROPS["behind_two"])] = EDGE_AWAY
    track(cams, point())
    # final_check_drop
    cams, uv = final_check_track(FINAL_CHECK_SEED if final_check_seed is None else final_check_seed,
                                 Rt, K4)
    img.extend(int(c) for c in cams)
    xy.extend(uv)
    start.append(len(img))
    # noise_free
    track(rng.permutation(TRI_CAMERAS)[:9], point(), noise=0.0)
    # mostly_unrelated: positions 2..63 are uniform random pixels
    base = len(img)
    track(rng.permutation(TRI_CAMERAS)[:64], point())
    unrelated = np.random.default_rng(UNRELATED_SEED if unrelated_seed is None else unrelated_seed)
    for p in range(2, 64):
        xy[base + p] = unrelated.uniform(10.0, 502.0, 2)
    track(EDGE_SAME_CENTRE, point(), noise=0.0)
    uv = project(Rt[EDGE_COPY_OF], K4[EDGE_COPY_OF], point())   # same_ray
    img.extend([EDGE_COPY_OF, EDGE_COPY])
    xy.extend([uv, uv.copy()])
    start.append(len(img))
    img.extend(EDGE_PARALLEL)   # parallel_rays
    xy.extend([np.array([C, C]), np.array([C, C])])
    start.append(len(img))
    start.append(len(img))   # empty_last: start == n_obs
    assert len(start) - 1 == len(EDGE_NAMES)
    return {"Rt": Rt, "K4": K4, "track_start": np.asarray(start, np.int32),
            "obs_image": np.asarray(img, np.int32), "obs_xy": np.asarray(xy, np.float64)}


BIG_TRACKS = 3000


def big_csr(seed=4400):
    """3000 tracks of 0, 2 or 3 observations (about one in fifty empty) over the band's cameras,
    0.5 px noise: more tracks than two strides of the CSR check and more observations than four."""
    rng = np.random.default_rng(seed)
    Rt, K4 = ring_cameras(TRI_CAMERAS, 4100)
    start, img, xy = [0], [], []
    for t in range(BIG_TRACKS):
        n = 0 if rng.random() < 0.02 else int(rng.integers(2, 4))
        X = rng.uniform(-0.1, 0.1, 3)
        for c in rng.permutation(TRI_CAMERAS)[:n]:
            img.append(int(c))
            xy.append(project(Rt[c], K4[c], X) + 0.5 * rng.standard_normal(2))
        start.append(len(img))
    p = {"Rt": Rt, "K4": K4, "track_start": np.asarray(start, np.int32),
         "obs_image": np.asarray(img, np.int32), "obs_xy": np.asarray(xy, np.float64)}
    assert len(img) > 4600 and (np.diff(p["track_start"]) == 0).sum() > 20
    return p


def malformed_csrs(p):
    """name -> (track_start, obs_image, the (status, index) the header's sentence gives): one
    offender in the last slot of the check's first stride, in the first of its second, in its
    last trip; two offenders in different trips; both kinds at once."""
    T, n_img = len(p["track_start"]) - 1, len(p["Rt"])
    out = {}

    def case(name, starts=(), images=(), want=None):
        ts, img = p["track_start"].copy(), p["obs_image"].copy()
        for t in starts:
            ts[t] = ts[t - 1] - 1   # below its predecessor; its successor stays above it
        for k, o in enumerate(images):
            img[o] = n_img if k % 2 == 0 else -1
        out[name] = (ts, img, want)
    case("start_1023", starts=(1023,), want=(1, 1023))
    case("start_1024", starts=(1024,), want=(1, 1024))
    case("start_last_track", starts=(T - 1,), want=(1, T - 1))
    case("starts_1500_2600", starts=(1500, 2600), want=(1, 1500))
    case("image_4095", images=(4095,), want=(2, 4095))
    case("images_4500_1030", images=(4500, 1030), want=(2, 1030))
    case("start_2000_image_5", starts=(2000,), images=(5,), want=(1, 2000))
    ts = p["track_start"].copy()
    ts[T] -= 1   # the end entry: the loop's last index, t == n_tracks
    out["end_entry"] = (ts, p["obs_image"].copy(), (1, T))
    return out


# ---- the chain's scene ----------------------------------------------------------------------
SCENE_POINTS, SCENE_DIM = 200, 64


def scene(seed=4200):
    """12 cameras on two rings around 200 points in a +-0.1 m box; per view every visible point
    becomes a feature (0.5 px noise, unit descriptor of the point plus per-view noise) and 10 %
    more features are distractors.  -> (features, img_lists, poses [12, 4, 4], Ks [12, 3, 3],
    points [200, 3], point_of_feature: name -> int array, -1 for a distractor)."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.1, 0.1, (SCENE_POINTS, 3))
    base = rng.standard_normal((SCENE_POINTS, SCENE_DIM))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    poses, Ks, names, feats, owner = [], [], [], {}, {}
    for k in range(12):
        ring, j = divmod(k, 6)
        az = 2 * np.pi * (j + 0.5 * ring) / 6
        el = np.deg2rad(20.0 if ring == 0 else 50.0)
        c = 0.5 * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
        T = np.eye(4)
        T[:3] = look_at(c)
        K = np.array([[F, 0, C], [0, F, C], [0, 0, 1.0]])
        name = f"scene/color/{k}.png"
        uv = np.stack([project(T[:3], (F, F, C, C), X) for X in pts]) + 0.5 * rng.standard_normal(
            (SCENE_POINTS, 2)) - 0.5   # the extractor's convention: COLMAP's pixel minus 0.5
        n_dis = SCENE_POINTS // 10
        dis_uv = rng.uniform(20, 490, (n_dis, 2))
        dis_d = rng.standard_normal((n_dis, SCENE_DIM))
        d = base + 0.05 * rng.standard_normal(base.shape)
        d = np.concatenate([d, dis_d])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        perm = rng.permutation(SCENE_POINTS + n_dis)
        own = np.concatenate([np.arange(SCENE_POINTS), np.full(n_dis, -1)])[perm]
        feats[name] = {"keypoints": np.concatenate([uv, dis_uv])[perm].astype(np.float32),
                       "descriptors": np.ascontiguousarray(d[perm].T.astype(np.float32)),
                       "scores": rng.uniform(0.1, 1.0, len(perm)).astype(np.float32),
                       "image_size": np.array([512, 512])}
        owner[name] = own
        poses.append(T)
        Ks.append(K)
        names.append(name)
    return feats, names, np.stack(poses), np.stack(Ks), pts, owner


SCENE_BOX = np.array([[x, y, z] for x, y, z in
                      [(-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1),
                       (-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)]], dtype=np.float64) * 0.15

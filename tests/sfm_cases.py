"""Seeded inputs of the sparse-reconstruction tests, shared by tests/golden/make_golden_sfm.py
and the test files so that both see the same bytes (the generator records a hash)."""
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

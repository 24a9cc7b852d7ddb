"""Seeded inputs of the two-view verification tests, shared by tests/golden/make_golden_two_view.py
and the test files so that all see the same bytes (the generator records a hash).

A scene: two posed views (the cameras of sfm_cases: f = 600, c = 256, 512 x 512) of points in a
+-0.1 m box, pixels in COLMAP's convention as float32.  Inliers carry bounded noise (uniform
within +-0.7 px per coordinate); an outlier's second point is redrawn uniformly in the image until
both its distance to the true epipolar line of the first point and the first point's distance to
the true epipolar line of the second are at least 12 px.  Every scene carries its true F and its
true inlier set."""
import numpy as np

from sfm_cases import C, F, look_at, sha   # noqa: F401  (sha re-exported)

NOISE, OUTLIER_MIN_DIST = 0.7, 12.0
DEFAULTS = dict(max_error=4.0, confidence=0.999, max_trials=10000, min_num_inliers=15,
                min_inlier_ratio=0.25, refine_iters=2)
K = np.array([[F, 0, C], [0, F, C], [0, 0, 1.0]])


def fundamental(T0, K0, T1, K1):
    """K1^-T [t]x R K0^-1 of the relative pose x1 = R x0 + t (world-to-camera T0, T1)."""
    R = T1[:3, :3] @ T0[:3, :3].T
    t = T1[:3, 3] - R @ T0[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.linalg.inv(K1).T @ tx @ R @ np.linalg.inv(K0)


def line_dist(Fm, p0, p1):
    """(distance of p1 to the line F p0, distance of p0 to the line F^T p1), per row."""
    h0 = np.concatenate([p0, np.ones((len(p0), 1))], 1)
    h1 = np.concatenate([p1, np.ones((len(p1), 1))], 1)
    l1, l0 = h0 @ Fm.T, h1 @ Fm
    e = np.abs((h1 * l1).sum(1))
    return e / np.hypot(l1[:, 0], l1[:, 1]), e / np.hypot(l0[:, 0], l0[:, 1])


def _project(T, X):
    p = X @ T[:3, :3].T + T[:3, 3]
    return np.stack([F * p[:, 0] / p[:, 2] + C, F * p[:, 1] / p[:, 2] + C], 1)


def cameras(rng, kind):
    az0, az1 = rng.uniform(0, 2 * np.pi), 0.0
    az1 = az0 + np.deg2rad(rng.uniform(20, 40))
    el = np.deg2rad(rng.uniform(15, 40, 2))
    c0 = 0.5 * np.array([np.cos(el[0]) * np.cos(az0), np.cos(el[0]) * np.sin(az0), np.sin(el[0])])
    c1 = 0.55 * np.array([np.cos(el[1]) * np.cos(az1), np.cos(el[1]) * np.sin(az1), np.sin(el[1])])
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3] = look_at(c0)
    if kind == "rotation":   # the same centre, the view turned by 8 degrees
        T1[:3] = look_at(c0, target=(0.07 * np.cos(az0 + 1.5), 0.07 * np.sin(az0 + 1.5), 0.0))
    else:
        T1[:3] = look_at(c1)
    return T0, T1


def scene(n, outlier_share, seed, kind="box"):
    """-> dict(pts0, pts1 float32 [n, 2], F_true [3, 3] (None for a pure rotation), inlier bool
    [n], T0, T1).  kind: "box", "planar" (the points on the plane z = 0) or "rotation"."""
    rng = np.random.default_rng(seed)
    T0, T1 = cameras(rng, kind)
    X = rng.uniform(-0.1, 0.1, (n, 3))
    if kind == "planar":
        X[:, 2] = 0.0
    p0 = _project(T0, X) + rng.uniform(-NOISE, NOISE, (n, 2))
    p1 = _project(T1, X) + rng.uniform(-NOISE, NOISE, (n, 2))
    Ft = None if kind == "rotation" else fundamental(T0, K, T1, K)
    inlier = np.ones(n, bool)
    n_out = int(round(outlier_share * n))
    out = rng.permutation(n)[:n_out]
    inlier[out] = False
    for i in out:
        while True:
            q = rng.uniform(10, 502, 2)
            if Ft is None:
                if np.hypot(*(q - p1[i])) >= 4 * OUTLIER_MIN_DIST:
                    break
                continue
            d1, d0 = line_dist(Ft, p0[i:i + 1], q[None])
            if min(d1[0], d0[0]) >= OUTLIER_MIN_DIST:
                break
        p1[i] = q
    p0, p1 = p0.astype(np.float32), p1.astype(np.float32)
    return {"pts0": p0, "pts1": p1, "F_true": Ft, "inlier": inlier, "T0": T0, "T1": T1}


# ---- the known-answer scenes of the host tests --------------------------------------------------
HOST_SCENES = [(n, share, 5000 + 10 * k + j) for k, n in enumerate((40, 130, 300))
               for j, share in enumerate((0.0, 0.3, 0.5))]


# ---- the GPU batch ------------------------------------------------------------------------------
COUNTS = (0, 7, 8, 14, 15, 16, 63, 64, 65, 257, 1000, "max")
SPECIALS = ("unrelated", "doubled", "planar", "rotation", "identical", "nonfinite")
CLAMP_POINTS = 80


def special(name, seed=7000):
    """-> (pts0, pts1, count as passed to the library, or None for len(pts0))."""
    rng = np.random.default_rng(seed + SPECIALS.index(name))
    if name == "unrelated":
        return (rng.uniform(10, 502, (100, 2)).astype(np.float32),
                rng.uniform(10, 502, (100, 2)).astype(np.float32), None)
    if name == "doubled":   # every match present twice
        s = scene(60, 0.2, seed + 50)
        return np.repeat(s["pts0"], 2, 0), np.repeat(s["pts1"], 2, 0), None
    if name in ("planar", "rotation"):
        s = scene(150, 0.2, seed + 60, kind=name)
        return s["pts0"], s["pts1"], None
    if name == "identical":   # the normalisation divides by a zero mean distance
        return (np.tile(np.float32([[100.5, 200.25]]), (64, 1)),
                np.tile(np.float32([[300.75, 50.5]]), (64, 1)), None)
    if name == "nonfinite":
        s = scene(120, 0.1, seed + 70)
        p0, p1 = s["pts0"].copy(), s["pts1"].copy()
        p0[3, 0], p1[17, 1], p0[40, 1], p1[41, 0] = np.nan, np.inf, -np.inf, 1e30
        p0[77], p1[90] = (np.nan, np.nan), (1e30, -1e30)
        return p0, p1, None
    raise KeyError(name)


def gpu_batches(max_points):
    """The GPU test's calls: name -> dict(options, max_points, names, pts0 / pts1 float32
    [B, max_points, 2] zero past a pair's points, counts int32 [B] as passed, n [B] the clamped
    counts).
    "main": every count at 0 and 30 % outliers and four of the special pairs, default options;
    "capped": the counts at 60 % outliers with max_trials = 300 (the loop ends at its cap), and
    the two special pairs whose loop never shortens (unrelated points, identical points);
    "small": counts 8 and 14 with min_num_inliers = 8 (and max_trials = 300), which the default
    would not run;
    "clamp": one scene of CLAMP_POINTS matches under max_points = CLAMP_POINTS with the counts
    10^9 (clamped to max_points), -5 (clamped to 0) and CLAMP_POINTS."""
    def count(c):
        return max_points if c == "max" else c
    plan = {"main": (dict(DEFAULTS), [], max_points),
            "capped": (dict(DEFAULTS, max_trials=300), [], max_points),
            "small": (dict(DEFAULTS, min_num_inliers=8, max_trials=300), [], 16),
            "clamp": (dict(DEFAULTS), [], CLAMP_POINTS)}
    for k, c in enumerate(COUNTS):
        for j, share in enumerate((0.0, 0.3)):
            s = scene(count(c), share, 6000 + 10 * k + j)
            plan["main"][1].append((f"n{c}_out{int(share * 100)}", s["pts0"], s["pts1"], None))
        s = scene(count(c), 0.6, 6000 + 10 * k + 2)
        plan["capped"][1].append((f"n{c}_out60", s["pts0"], s["pts1"], None))
    for name in SPECIALS:
        plan["capped" if name in ("unrelated", "identical") else "main"][1].append(
            (name, *special(name)))
    for c in (8, 14):
        s = scene(c, 0.0, 6500 + c)
        plan["small"][1].append((f"n{c}_min8", s["pts0"], s["pts1"], None))
    s = scene(CLAMP_POINTS, 0.1, 6600)
    for name, cnt in (("over_count", 10 ** 9), ("negative_count", -5), ("exact_count", None)):
        plan["clamp"][1].append((name, s["pts0"], s["pts1"], cnt))
    out = {}
    for key, (options, pairs, max_points) in plan.items():
        B = len(pairs)
        p0 = np.zeros((B, max_points, 2), np.float32)
        p1 = np.zeros((B, max_points, 2), np.float32)
        counts = np.zeros(B, np.int32)
        for b, (_, a0, a1, cnt) in enumerate(pairs):
            p0[b, :len(a0)], p1[b, :len(a1)] = a0, a1
            counts[b] = len(a0) if cnt is None else min(cnt, 2 ** 31 - 1)
        out[key] = {"options": options, "max_points": max_points, "names": [p[0] for p in pairs], "pts0": p0, "pts1": p1,
                    "counts": counts, "n": np.clip(counts, 0, max_points).astype(np.int32)}
    return out


# ---- the options and the given-F edges ----------------------------------------------------------
REFINE_ITERS = (0, 1, 2, 5)
REFINE_SCENES = ((65, 0.3, 8118), (40, 0.0, 8109), (130, 0.3, 8100), (65, 0.3, 8101))
TIGHT = dict(max_error=0.7, max_trials=300)   # the noise is +-0.7 px: matches sit at the threshold
LDS_MAX_POINTS = {8: (8, 5, 7), 9: (9, 4, 8), 15: (15, 6, 11), 17: (17, 7, 12), 33: (33, 3, 20)}


def _pack(options, max_points, pairs, F_in=None):
    B = len(pairs)
    p0 = np.zeros((B, max_points, 2), np.float32)
    p1 = np.zeros((B, max_points, 2), np.float32)
    counts = np.zeros(B, np.int32)
    for b, (_, a0, a1) in enumerate(pairs):
        p0[b, :len(a0)], p1[b, :len(a1)], counts[b] = a0, a1, len(a0)
    out = {"options": options, "max_points": max_points, "names": [p[0] for p in pairs],
           "pts0": p0, "pts1": p1, "counts": counts, "n": counts.copy()}
    if F_in is not None:
        out["F_in"] = np.ascontiguousarray(F_in, np.float64).reshape(B, 9)
    return out


def option_sha(call):
    """The hash a call is recorded under: its points, counts, given F and options."""
    arrays = [call["pts0"], call["pts1"], call["counts"]] + ([call["F_in"]] if "F_in" in call else [])
    return sha(*arrays, np.array(sorted(call["options"].items()), dtype="U32"))


def option_calls():
    """The "options" family: small calls, each with its own options -> name -> the dict of
    gpu_batches() (plus F_in [B, 9] for the given-geometry call).
    refine{k}, tight_refine{k}: refine_iters = 0, 1, 2, 5 on one batch, at the defaults and with
      max_error = 0.7 px, where refits move the mask and one is not kept;
    max_error{e}: 0, 0.5, 1 and 16 px with max_trials = 300;
    confidence{c}: 0.5 and 0.999999 on a clean pair (the loop ends inside its first round of 64)
      and on pairs with 30 % outliers (several rounds at 0.999999);
    ratio{r}: min_inlier_ratio 0.8, 1.0 and -1 on 30 % outliers and on a clean pair;
    points{P}: max_points = 8, 9, 15, 17, 33 (the flags start at byte 16 P of the dynamic LDS, whose
      size 17 P is rounded up to 16) with three pairs of unequal counts, one below
      min_num_inliers = 8;
    given: F_in with a NaN entry, an inf entry, all zeros, each also on a pair below
      min_num_inliers, and a true F."""
    def pairs(specs):
        return [(f"n{n}_out{int(100 * share)}_s{seed}", s["pts0"], s["pts1"])
                for n, share, seed in specs for s in [scene(n, share, seed)]]
    calls = {}
    refine = pairs(REFINE_SCENES)
    P = max(len(p[1]) for p in refine)
    for k in REFINE_ITERS:
        calls[f"refine{k}"] = _pack(dict(DEFAULTS, refine_iters=k), P, refine)
        calls[f"tight_refine{k}"] = _pack(dict(DEFAULTS, refine_iters=k, **TIGHT), P, refine)
    mixed = pairs(((40, 0.0, 8200), (65, 0.3, 8201), (130, 0.3, 8202), (100, 0.5, 8203)))
    for e in (0.0, 0.5, 1.0, 16.0):
        calls[f"max_error{e:g}"] = _pack(dict(DEFAULTS, max_error=e, max_trials=300), 130, mixed)
    for c in (0.5, 0.999999):
        calls[f"confidence{c:g}"] = _pack(dict(DEFAULTS, confidence=c), 130, mixed[:3])
    for r in (0.8, 1.0, -1.0):
        calls[f"ratio{r:g}"] = _pack(dict(DEFAULTS, min_inlier_ratio=r), 130, mixed[:3])
    for P, counts in LDS_MAX_POINTS.items():
        calls[f"points{P}"] = _pack(dict(DEFAULTS, min_num_inliers=8, max_trials=300), P,
                                    pairs([(c, 0.0, 8301 + 10 * P + j) for j, c in enumerate(counts)]))
    s, few = scene(40, 0.1, 8400), scene(10, 0.0, 8401)
    bad = []
    for k, value in ((4, np.nan), (7, np.inf), (None, 0.0)):
        Fb = s["F_true"].reshape(9).copy()
        if k is None:
            Fb[:] = value
        else:
            Fb[k] = value
        bad.append(Fb)
    given = ([(f"{name}_n40", s["pts0"], s["pts1"]) for name in ("nan", "inf", "zero")]
             + [(f"{name}_n10", few["pts0"], few["pts1"]) for name in ("nan", "inf", "zero", "true")]
             + [("true_n40", s["pts0"], s["pts1"])])
    calls["given"] = _pack(dict(DEFAULTS), 40, given,
                           F_in=bad + bad + [few["F_true"].reshape(9), s["F_true"].reshape(9)])
    return calls


# ---- the chain with wrong matches ---------------------------------------------------------------
class OracleNN:
    """NearestNeighbour's forward dict from tests/nn_oracle.py (numpy), for the host chain."""

    def __call__(self, data):
        import nn_oracle
        import torch
        r = nn_oracle.forward(data["descriptors0"].numpy(), data["descriptors1"].numpy(), 0.8, 0.7)
        return {k: torch.from_numpy(np.asarray(r[k])) for k in
                ("matches0", "matches1", "matching_scores0", "matching_scores1")}


class Redirecting:
    """A matcher wrapped so that a share of each pair's valid matches0 (rounded, seeded per call)
    points at a uniformly random feature of the other image.  matches1 and the scores stay."""

    def __init__(self, matcher, share, seed=4300):
        self.matcher, self.share, self.seed, self.calls = matcher, share, seed, 0

    def __call__(self, data):
        import torch
        pred = dict(self.matcher(data))
        rng = np.random.default_rng(self.seed + self.calls)
        self.calls += 1
        m0 = pred["matches0"].clone()
        valid = np.nonzero(m0[0].cpu().numpy() > -1)[0]
        n1 = data["keypoints1"].shape[1]
        hit = rng.permutation(valid)[:int(round(self.share * len(valid)))]
        if len(hit):
            m0[0, torch.from_numpy(hit).to(m0.device)] = torch.from_numpy(
                rng.integers(0, n1, len(hit))).to(m0.device, m0.dtype)
        pred["matches0"] = m0
        return pred


def points_within_1mm(model, pts, owner):
    """How many scene points the model holds within 1 mm of the ground truth, counted as
    tests/test_sfm_host.py counts them (a track all of whose features belong to one point)."""
    found = {}
    for k, tr_img in enumerate(model["track_image_ids"]):
        owners = {int(owner[model["names"][i - 1]][f]) for i, f in
                  zip(tr_img, model["track_point2D_idxs"][k])}
        if len(owners) == 1 and -1 not in owners:
            (o,) = owners
            found[o] = min(found.get(o, np.inf), np.linalg.norm(model["xyz"][k] - pts[o]))
    return sum(d <= 1e-3 for d in found.values())

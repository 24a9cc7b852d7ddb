"""The optical-flow scenes shared by tests/golden/make_golden_lk.py (which records the oracle's
results on them) and the tests (which regenerate the inputs from the seed and compare digests).

A scene: a sum of 12 cosines with |frequency| <= 0.35 rad/px scaled into 0..255 and rounded; the
second image is the same field shifted, plus uniform integer noise in [-6, 6]; one flat rectangle
(constant 90) in a corner of both; 300 points uniform in [-3, w + 3] x [-3, h + 3], the first of
them replaced by (-20, 5), which lies outside the image by more than a window.

EDGE_CASES (tests/golden/lk_edges.npz, make_golden_lk_edges.py) are a second set: every window
path, 0/255 images whose window sums pass 2^31, two warps with an analytic displacement, tight
criteria.  MODEL_SCENES are those on which tests/lk_model.py, a float64 model, is compared with
the oracle."""
import hashlib
import os

import numpy as np

import lk_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_POINTS = 300
COUNTS = (0, 1, 63, 64, 65, 300)

# name -> h, w, shift (x, y), win, max_level, max_count, seed
CASES = {
    "base": dict(h=120, w=160, shift=(3.3, -2.6), win=15, max_level=2, max_count=10, seed=11),
    "odd": dict(h=75, w=97, shift=(1.25, 0.75), win=7, max_level=3, max_count=10, seed=12),
    "far": dict(h=120, w=160, shift=(9.4, 6.2), win=15, max_level=2, max_count=10, seed=13),
    "win21": dict(h=120, w=160, shift=(14.0, -11.0), win=21, max_level=2, max_count=10, seed=14),
    "one_level": dict(h=30, w=40, shift=(1.5, -1.0), win=15, max_level=2, max_count=10, seed=15),
    "level0": dict(h=120, w=160, shift=(1.6, 1.1), win=15, max_level=0, max_count=10, seed=16),
    "count1": dict(h=120, w=160, shift=(3.3, -2.6), win=15, max_level=2, max_count=1, seed=17),
    "count0": dict(h=120, w=160, shift=(3.3, -2.6), win=15, max_level=2, max_count=0, seed=18),
}
EPSILON, MIN_EIG = 0.03, 1e-4


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cosine_field(h, w, seed):
    """A callable (x, y) -> the field in 0..255 (float64, not rounded)."""
    rng = np.random.default_rng(seed)
    # six long waves, which survive to the top level and carry the large shifts, and six short
    mag = np.concatenate([rng.uniform(0.03, 0.12, 6), rng.uniform(0.12, 0.35, 6)])
    ang = rng.uniform(0, 2 * np.pi, 12)
    fx, fy = mag * np.cos(ang), mag * np.sin(ang)
    ph = rng.uniform(0, 2 * np.pi, 12)
    amp = rng.uniform(0.5, 1.0, 12)

    def f(x, y):
        v = sum(a * np.cos(u * x + v_ * y + p) for a, u, v_, p in zip(amp, fx, fy, ph))
        return 127.5 + 127.5 * v / amp.sum()
    return f


def image_pair(h, w, shift, seed, noise=6, flat=True):
    """(first image, second image) uint8: the second shows the first moved by +shift."""
    f = cosine_field(h, w, seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.rint(f(x, y))
    b = np.rint(f(x - shift[0], y - shift[1]))
    if noise:
        b = b + np.random.default_rng(seed + 1000).integers(-noise, noise + 1, size=(h, w))
    a, b = np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8)
    if flat:
        fh, fw = max(h // 4, 8), max(w // 4, 8)
        a[:fh, :fw] = 90
        b[:fh, :fw] = 90
    return a, b


def scene(name):
    """dict(prev, next, pts, win, max_level, max_count) of a case (of either dict)."""
    if name in EDGE_CASES:
        return edge_scene(name)
    c = CASES[name]
    a, b = image_pair(c["h"], c["w"], c["shift"], c["seed"])
    rng = np.random.default_rng(c["seed"] + 2000)
    pts = np.stack([rng.uniform(-3, c["w"] + 3, N_POINTS), rng.uniform(-3, c["h"] + 3, N_POINTS)],
                   1).astype(np.float32)
    pts[0] = (-20.0, 5.0)
    return dict(prev=a, next=b, pts=pts, win=c["win"], max_level=c["max_level"],
                max_count=c["max_count"])


def scene_sha(s):
    return sha(s["prev"], s["next"], s["pts"])


_ORACLE = {}


def oracle(name):
    """The oracle's (next_pts, status, reason, pyramids) of a case, computed once per process."""
    if name not in _ORACLE:
        s = scene(name)
        p = lk_oracle.build_pyramid(s["prev"], s["win"], s["max_level"])
        q = lk_oracle.build_pyramid(s["next"], s["win"], s["max_level"])
        trace, stats = [], {}
        out, st, why = lk_oracle.track(p, q, s["pts"], s["win"], s["max_count"],
                                       s.get("epsilon", EPSILON), MIN_EIG, trace=trace, stats=stats)
        for arr in (out, st, why):
            arr.setflags(write=False)
        _ORACLE[name] = (out, st, why, p, q)
        _TRACE[name] = (trace_counts(trace, st, why), stats.get("max_ix2", 0))
    return _ORACLE[name]


# ---- edge scenes (tests/golden/lk_edges.npz) --------------------------------------------------
# A second dict, so that the ids and digests of CASES do not move.  120 points per scene, drawn
# like scene()'s; points 1..12 are then rounded to whole pixels (weights exactly 2^14, 0, 0, 0:
# on a 0/255 image the window then holds the unblended +-4080 of a straight edge).
#
# kind "cosine": image_pair plus a patch of stripes() in the bottom right corner of both images
#   (a quarter of each side).  Its period is 4 px, so level 1 holds a period of 2 px there, on
#   which the Scharr central differences vanish, and level 2 a constant: a point in the patch is
#   rejected by the eigenvalue test above level 0 and tracks at level 0.  Placed by hand for
#   that class of the per-level trace; the random points find it.
# kind "noise": block_noise, the second image an integer np.roll of the first.
# kind "stripes", "quilt": stripes and quilt, rolled likewise.
# kind "warp": warp_pair, no noise, no patches; the analytic displacement is warp_truth(name, pts).
N_EDGE_POINTS = 120
EDGE_CASES = {}
for _w in (3, 5, 9, 17, 23, 31):
    EDGE_CASES[f"noise_w{_w}"] = dict(kind="noise", h=96, w=112, cell=3, roll=(1, -1), win=_w,
                                      max_level=2, max_count=10, seed=40 + _w)
    EDGE_CASES[f"cosine_w{_w}"] = dict(kind="cosine", h=96, w=112, shift=(1.25, 0.75), win=_w,
                                       max_level=2, max_count=10, seed=80 + _w)
EDGE_CASES.update({
    "odd_w23": dict(kind="cosine", h=75, w=97, shift=(2.4, -1.7), win=23, max_level=2,
                    max_count=10, seed=120),
    "noise_w15": dict(kind="noise", h=96, w=112, cell=3, roll=(-1, 2), win=15, max_level=2,
                      max_count=10, seed=121),
    "stripes_w31": dict(kind="stripes", h=96, w=112, roll=(1, 0), win=31, max_level=2,
                        max_count=10, seed=122),
    # block noise at window 15 stays below 2^31 (1.6e9), where a 32-bit sum is still right; 129
    # window pixels of |Ix| = 4080 among the 225 are beyond it, and a quilt has such windows
    "quilt_w15": dict(kind="quilt", h=96, w=112, tile=20, roll=(1, 1), win=15, max_level=2,
                      max_count=10, seed=126),
    "warp_a": dict(kind="warp", h=160, w=200, angle=3.0, scale=1.03, shift=(2.2, -1.4), win=15,
                   max_level=2, max_count=10, seed=123),
    "warp_b": dict(kind="warp", h=160, w=200, angle=-5.0, scale=0.97, shift=(-3.1, 2.7), win=15,
                   max_level=2, max_count=10, seed=124),
    # the cap is out of reach for most points, so eps or an oscillation ends them after many
    # iterations per level
    "tight": dict(kind="cosine", h=96, w=112, shift=(2.6, 1.9), win=15, max_level=2, max_count=30,
                  epsilon=1e-3, seed=125),
})
del _w
# the saturated scenes: the largest window sum of Ix^2 or Iy^2 must exceed this
SATURATED = {"noise_w15": 2 ** 30, "noise_w31": 2 ** 31, "stripes_w31": 2 ** 31,
             "quilt_w15": 2 ** 31}
WARPS = ("warp_a", "warp_b")


def block_noise(h, w, cell, seed):
    """uint8 [h, w]: cell x cell blocks, each 0 or 255."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(-(-h // cell), -(-w // cell)), dtype=np.uint8)
    return (np.kron(bits, np.ones((cell, cell), np.uint8))[:h, :w] * 255).astype(np.uint8)


def stripes(h, w):
    """uint8 [h, w]: horizontal 2-px 0/255 stripes XOR vertical ones."""
    y, x = np.mgrid[0:h, 0:w]
    return ((((y >> 1) ^ (x >> 1)) & 1) * 255).astype(np.uint8)


def quilt(h, w, tile):
    """uint8 [h, w]: tile x tile squares of 2-px 0/255 stripes, vertical and horizontal in turn.
    Inside a square of vertical stripes every pixel has |Ix| = 4080 and Iy = 0."""
    y, x = np.mgrid[0:h, 0:w]
    vertical = ((y // tile + x // tile) & 1) == 0
    return (np.where(vertical, (x >> 1) & 1, (y >> 1) & 1) * 255).astype(np.uint8)


def _affine(h, w, angle, scale, t):
    """A [2, 2], c, t of p -> c + A (p - c) + t about the image centre; angle in degrees."""
    r = np.deg2rad(angle)
    A = scale * np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]])
    return A, np.array([(w - 1) / 2, (h - 1) / 2]), np.asarray(t, dtype=np.float64)


def warp_pair(h, w, seed, angle, scale, t):
    """(first, second, displacement): the cosine field, and the same field seen through the
    affine map; displacement(pts [n, 2]) is where each point of the first image went, minus
    where it was, in float64."""
    f = cosine_field(h, w, seed)
    A, c, t = _affine(h, w, angle, scale, t)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    back = np.linalg.inv(A)
    u, v = x - c[0] - t[0], y - c[1] - t[1]
    a = np.rint(f(x, y))
    b = np.rint(f(c[0] + back[0, 0] * u + back[0, 1] * v, c[1] + back[1, 0] * u + back[1, 1] * v))

    def displacement(pts):
        p = np.asarray(pts, dtype=np.float64)
        return (p - c) @ A.T + c + t - p
    return (np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8),
            displacement)


def _edge_images(c):
    if c["kind"] == "cosine":
        a, b = image_pair(c["h"], c["w"], c["shift"], c["seed"])
        ch, cw = c["h"] // 4, c["w"] // 4
        a[-ch:, -cw:] = b[-ch:, -cw:] = stripes(ch, cw)
        return a, b
    if c["kind"] == "warp":
        return warp_pair(c["h"], c["w"], c["seed"], c["angle"], c["scale"], c["shift"])[:2]
    a = {"noise": lambda: block_noise(c["h"], c["w"], c["cell"], c["seed"]),
         "stripes": lambda: stripes(c["h"], c["w"]),
         "quilt": lambda: quilt(c["h"], c["w"], c["tile"])}[c["kind"]]()
    return a, np.ascontiguousarray(np.roll(a, (c["roll"][1], c["roll"][0]), axis=(0, 1)))


def edge_scene(name):
    """dict(prev, next, pts, win, max_level, max_count, epsilon) of an edge case."""
    c = EDGE_CASES[name]
    a, b = _edge_images(c)
    rng = np.random.default_rng(c["seed"] + 2000)
    pts = np.stack([rng.uniform(-3, c["w"] + 3, N_EDGE_POINTS),
                    rng.uniform(-3, c["h"] + 3, N_EDGE_POINTS)], 1).astype(np.float32)
    pts[0] = (-20.0, 5.0)
    pts[1:13] = np.rint(pts[1:13])
    return dict(prev=a, next=b, pts=pts, win=c["win"], max_level=c["max_level"],
                max_count=c["max_count"], epsilon=c.get("epsilon", EPSILON))


def warp_truth(name, pts):
    c = EDGE_CASES[name]
    return warp_pair(c["h"], c["w"], c["seed"], c["angle"], c["scale"], c["shift"])[2](pts)


MAX_LEVELS = 6
_TRACE = {}


def trace_counts(trace, status, reason):
    """int64 [3, MAX_LEVELS, reasons]: how often each level ended with each reason, over all
    points ([0]), over those whose final status is 1 ([1]) and over those that the bounds check
    before the loop refused at level 0 ([2])."""
    n = np.zeros((3, MAX_LEVELS, len(lk_oracle.REASONS)), np.int64)
    for i, l, r in trace:
        n[0, l, r] += 1
        n[1, l, r] += int(status[i])
        n[2, l, r] += int(reason[i] == lk_oracle.R_OOB_PRE)
    return n


def oracle_trace(name):
    """(trace_counts, the largest window sum of Ix^2 or Iy^2) of a case of either dict."""
    oracle(name)
    return _TRACE[name]


def check_coverage(rec):
    """What CASES and EDGE_CASES together have to cover.  rec: name -> dict(levels, status,
    reason, trace, max_ix2), live from the oracle (the generator) or read back from
    tests/golden/lk_edges.npz (the host test)."""
    R = lk_oracle
    cases = {**CASES, **EDGE_CASES}
    assert set(rec) == set(cases)
    # lk_track_kernel<1|4|8|16> serves windows 3..7, 9..15, 17..21, 23..31: each at both ends
    assert {3, 7, 9, 15, 17, 21, 23, 31} <= {c["win"] for c in cases.values()}
    for name in EDGE_CASES:
        st = rec[name]["status"]
        assert len(st) == N_EDGE_POINTS and 2 * int(st.sum()) >= len(st), (name, int(st.sum()))
    assert rec["noise_w31"]["levels"] == rec["odd_w23"]["levels"] == 2
    assert rec["warp_a"]["levels"] == rec["warp_b"]["levels"] == rec["tight"]["levels"] == 3
    ran = [R.R_EPS, R.R_OSC, R.R_CAP, R.R_OOB_LOOP]   # level endings of a point that iterated
    for name, above in SATURATED.items():
        assert rec[name]["max_ix2"] > above, (name, rec[name]["max_ix2"])
        assert rec[name]["trace"][0, 0, ran].sum() > 0, f"{name}: no point passes the eigenvalue test"
    for name in CASES:   # the scenes from before this set cannot tell a 32-bit sum from a 64-bit one
        assert rec[name]["max_ix2"] < 2 ** 30, name
    # the tight criteria: the cap ends next to nothing, an oscillation a good share
    t = rec["tight"]["trace"][0, 0]
    assert 10 * t[R.R_CAP] <= N_EDGE_POINTS <= 6 * t[R.R_OSC], t
    # what happens above level 0 to a point that ends with status 1
    kept = sum(r["trace"][1, 1:] for r in rec.values()).sum(0)
    assert kept[R.R_EIG] > 0, "no kept point was rejected by the eigenvalue test above level 0"
    assert kept[R.R_OSC] > 0, "no kept point stopped on an oscillation above level 0"
    # A point that leaves the image inside the loop above level 0 cannot end with status 1: with
    # floor(n) < -win or >= cols at level l, the start 2 n + half at level l - 1 is outside too,
    # so every level below either refuses it before the loop, rejects it, or breaks at j = 0 (or
    # never iterates, with max_count 0), and at level 0 each of those clears the status.  The
    # event itself must occur, and this consequence of the contract with it.
    everyone = sum(r["trace"][0, 1:] for r in rec.values()).sum(0)
    assert everyone[R.R_OOB_LOOP] > 0 and kept[R.R_OOB_LOOP] == 0, (everyone, kept)
    # (-20, 5) with window 15 and three levels: inside at level 2 (-12 >= -15), where it
    # iterates; refused before the loop at levels 1 and 0
    for name in ("base", "noise_w15", "tight"):
        pre = rec[name]["trace"][2]
        assert rec[name]["reason"][0] == R.R_OOB_PRE and pre[0, R.R_OOB_PRE] >= 1, name
        assert pre[2, [R.R_EPS, R.R_OSC, R.R_CAP]].sum() >= 1 and pre[1, R.R_OOB_PRE] >= 1, name


# ---- the float64 model's scenes ---------------------------------------------------------------
# The four translation scenes of CASES that have three or more levels, and both warps.  In "win21"
# the shift (14, -11) is beyond what a 30 x 40 top level carries with a 21-px window, and a
# quarter of the points end at the iteration cap (compared set 73% of the points); "win21_half"
# is the same scene with half the shift, where the compared set is large enough (97%).  "win21"
# itself stays in for status equality and the bar.
MODEL_ONLY = {"win21_half": dict(CASES["win21"], shift=(7.0, -5.5))}
MODEL_SCENES = ("base", "odd", "far", "win21", "win21_half") + WARPS
COMPARED_SHARE = 0.9   # of a scene's points, on every model scene but "win21"
# The bar on |oracle - model| over the compared set, in pixels.  Measured on the CPU, oracle
# against model (tests/golden/make_golden_lk_edges.py prints it): base 0.00266, odd 0.01183, far
# 0.00292, win21 0.00568, win21_half 0.00210, warp_a 0.00643, warp_b 0.00683.  Four times the
# largest (the two sides may stop one iteration apart near the threshold) is 0.047, above
# epsilon = 0.03, the stopping rule's own resolution, which is therefore the bar.
MODEL_BAR = 0.03


def grid_points(h, w, win, target=130):
    """About ``target`` points on a grid that stays more than a window from every border, each
    0.37 px off the pixel centres."""
    m = win + 1
    step = max(int(np.sqrt((h - 2 * m) * (w - 2 * m) / target)), 1)
    ys, xs = np.mgrid[m:h - m:step, m:w - m:step]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32) + np.float32(0.37)


_MODEL = {}


def model_pair(name):
    """On the images of a scene and grid_points: the oracle's and the float64 model's
    (positions, status, reason), and the points.  Computed once per process."""
    if name not in _MODEL:
        import lk_model
        if name in MODEL_ONLY:
            c = MODEL_ONLY[name]
            a, b = image_pair(c["h"], c["w"], c["shift"], c["seed"])
            s = dict(prev=a, next=b, win=c["win"], max_level=c["max_level"],
                     max_count=c["max_count"])
        else:
            s = scene(name)
        pts = grid_points(*s["prev"].shape, s["win"])
        p = lk_oracle.build_pyramid(s["prev"], s["win"], s["max_level"])
        q = lk_oracle.build_pyramid(s["next"], s["win"], s["max_level"], with_deriv=False)
        o = lk_oracle.track(p, q, pts, s["win"], s["max_count"], EPSILON, MIN_EIG)
        mp = lk_model.pyramid(s["prev"], s["win"], s["max_level"])
        mq = lk_model.pyramid(s["next"], s["win"], s["max_level"])
        m = lk_model.track(mp, mq, pts, s["win"], s["max_count"], EPSILON, MIN_EIG)
        for arr in o + m + (pts,):
            arr.setflags(write=False)
        _MODEL[name] = (o, m, pts)
    return _MODEL[name]


def compared_set(name):
    """The points on which oracle and model are held to the bar: both end level 0 by the epsilon
    rule (elsewhere the last step is not small, and two trajectories a rounding apart need not
    end together).  grid_points keeps all of them more than a window from every border."""
    o, m, _ = model_pair(name)
    return (o[2] == lk_oracle.R_EPS) & (m[2] == 0)


def interior(name, margin=26):
    """Of grid_points: those more than 25 px from every border, as in
    test_known_shift_is_recovered; the warps are compared with the truth there."""
    _, _, pts = model_pair(name)
    c = EDGE_CASES[name]
    return ((pts >= margin) & (pts <= np.array([c["w"], c["h"]]) - margin)).all(1)

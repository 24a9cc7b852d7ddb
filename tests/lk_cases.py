"""The optical-flow scenes shared by tests/golden/make_golden_lk.py (which records the oracle's
results on them) and the tests (which regenerate the inputs from the seed and compare digests).

A scene: a sum of 12 cosines with |frequency| <= 0.35 rad/px scaled into 0..255 and rounded; the
second image is the same field shifted, plus uniform integer noise in [-6, 6]; one flat rectangle
(constant 90) in a corner of both; 300 points uniform in [-3, w + 3] x [-3, h + 3], the first of
them replaced by (-20, 5), which lies outside the image by more than a window."""
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
    """dict(prev, next, pts, win, max_level, max_count) of a case."""
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
        out, st, why = lk_oracle.track(p, q, s["pts"], s["win"], s["max_count"], EPSILON, MIN_EIG)
        for arr in (out, st, why):
            arr.setflags(write=False)
        _ORACLE[name] = (out, st, why, p, q)
    return _ORACLE[name]

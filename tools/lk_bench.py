#!/usr/bin/env python
"""Time the tracker's optical flow (onepose_lk_build_pyramid, onepose_lk_track), a first
measurement with nothing tuned, at the crop size the detector leaves on the GPU:

    512 x 512, win 15, max_level 2: the pyramid build with and without derivatives, and the
    track call at n = 256, 1024 and 4096 points; each for one frame and for B = 8 next frames
    against a shared keyframe pyramid and shared points.

Warm-up, then the median (and min, max) of `--replays` replays of a captured graph, each between
two events.  There is no baseline: cv2 is not available, and an eager PyTorch Lucas-Kanade would
be a second implementation, not a yardstick.  No ratio and no target is claimed.  Points per
second is derived from the median; launches per call are the library's (header).  The scene is
tests/lk_cases.py's cosine field shifted by (3.3, -2.6) px with noise, points uniform in the
image.

    python tools/lk_bench.py --out profiles/lk/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import lk_cases  # noqa: E402
from onepose_amd import _lib  # noqa: E402

H = W = 512
WIN, MAX_LEVEL, MAX_COUNT, EPSILON, MIN_EIG = 15, 2, 10, 0.03, 1e-4
POINTS = (256, 1024, 4096)


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def graph_ms(run, dev, replays):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return median_ms(graph.replay, replays)


def entry(t, **extra):
    return {"graph_ms_median": t[0], "graph_ms_min_max": t[1:], **extra}


def bench(lib, dev, B, replays):
    a, b = lk_cases.image_pair(H, W, (3.3, -2.6), 7)
    nexts = np.stack([np.roll(b, k, axis=1) if k else b for k in range(B)])
    img_a = torch.from_numpy(a).to(dev)
    img_b = torch.from_numpy(nexts).to(dev)
    nbytes = lib.onepose_lk_pyramid_bytes(H, W, WIN, MAX_LEVEL)
    kf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nx = torch.empty(B, nbytes, dtype=torch.uint8, device=dev)

    def build(img, batch, deriv, blob):
        _lib.check(lib.onepose_lk_build_pyramid(img.data_ptr(), H * W, batch, H, W, WIN, MAX_LEVEL,
                                                deriv, blob.data_ptr(), _lib.stream_ptr(dev)))

    build(img_a, 1, 1, kf)
    res = {"batch": B, "pyramid_bytes": int(nbytes),
           "levels": int(lib.onepose_lk_levels(H, W, WIN, MAX_LEVEL)),
           "build_with_deriv": entry(graph_ms(lambda: build(img_b, B, 1, nx), dev, replays),
                                     launches=2),
           "build_without_deriv": entry(graph_ms(lambda: build(img_b, B, 0, nx), dev, replays),
                                        launches=2)}
    rng = np.random.default_rng(5)
    for n in POINTS:
        pts = torch.from_numpy(rng.uniform(0, W, (n, 2)).astype(np.float32)).to(dev)
        counts = torch.full((B,), n, dtype=torch.int32, device=dev)
        out = torch.empty(B, n, 2, dtype=torch.float32, device=dev)
        st = torch.empty(B, n, dtype=torch.uint8, device=dev)

        def track():
            _lib.check(lib.onepose_lk_track(kf.data_ptr(), 0, nx.data_ptr(), pts.data_ptr(), 0,
                                            counts.data_ptr(), B, n, H, W, WIN, MAX_LEVEL,
                                            MAX_COUNT, EPSILON, MIN_EIG, out.data_ptr(),
                                            st.data_ptr(), _lib.stream_ptr(dev)))

        t = graph_ms(track, dev, replays)
        res[f"track_{n}"] = entry(t, launches=1, points=B * n,
                                  points_per_second_derived=B * n / (t[0] * 1e-3),
                                  status_1=int(st.sum().item()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lk/bench.json")
    ap.add_argument("--replays", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lk_bench needs a ROCm GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(dev), "replays": a.replays, "h": H, "w": W,
           "win": WIN, "max_level": MAX_LEVEL, "max_count": MAX_COUNT, "epsilon": EPSILON}
    for B in (1, 8):
        res[f"batch_{B}"] = bench(lib, dev, B, a.replays)
        print(json.dumps(res[f"batch_{B}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

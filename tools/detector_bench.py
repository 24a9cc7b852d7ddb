#!/usr/bin/env python
"""Time the 2D object detector's entry points (onepose_amd.detector), a first measurement:

    onepose_detect_stage at 15 views x 1024 and x 4096 matches (60 % inliers, sigma 0.5 px),
    onepose_crop_resize from 1440 x 1920 to 512 x 512.

Each is captured in a graph; after a warm-up the median of >= 50 replays, each between two
events, is reported.  No time is a pass/fail bar: the stage is latency-bound (15 workgroups).

    python tools/detector_bench.py --out profiles/detector/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from onepose_amd import detector  # noqa: E402

VIEWS = 15


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


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
        out = run()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return median_ms(graph.replay, replays), out


def stage_inputs(n, dev, seed=0):
    """15 views with n keypoints each, all matched: 60 % under a similarity with sigma 0.5 px
    noise, 40 % gross outliers."""
    rs = np.random.RandomState(seed)
    kpts1 = rs.uniform(0, 1900, (n, 2)).astype(np.float32)
    m = np.stack([rs.permutation(n) for _ in range(VIEWS)]).astype(np.int64)
    k0 = np.zeros((VIEWS, n, 2), np.float32)
    for b in range(VIEWS):
        ang, s = np.deg2rad(rs.uniform(-40, 40)), rs.uniform(0.4, 0.9)
        R = s * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        t = rs.uniform(50, 300, 2)
        k0[b] = (kpts1[m[b]] - t) @ np.linalg.inv(R).T + 0.5 * rs.standard_normal((n, 2))
        out = rs.permutation(n)[:int(0.4 * n)]
        k0[b, out] = rs.uniform(0, 640, (len(out), 2))
    hw = np.tile(np.array([[480, 640]], np.int32), (VIEWS, 1))
    return tuple(torch.from_numpy(a).to(dev) for a in (m, k0, kpts1, hw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "replays": a.replays, "detect_stage": {}}
    for n in (1024, 4096):
        m, k0, k1, hw = stage_inputs(n, dev)
        ms, res = graph_ms(lambda: detector.detect_stage(m, None, k0, k1, hw, (1440, 1920)), dev,
                           a.replays)
        entry = {"views": VIEWS, "matches": n, "graph_ms_median": ms,
                 "iters_per_view": res["iters"].cpu().tolist(),
                 "inliers_per_view": res["n_inliers"].cpu().tolist()}
        out["detect_stage"][f"views15_x{n}"] = entry
        print(json.dumps({f"detect_stage_15x{n}": entry}))
    img = torch.randint(0, 256, (1440, 1920), dtype=torch.uint8, device=dev)
    box = torch.tensor([400, 300, 1200, 1000], dtype=torch.int32, device=dev)
    K = torch.tensor([[1500.0, 0, 960], [0, 1500.0, 720], [0, 0, 1]], dtype=torch.float64, device=dev)
    ms, _ = graph_ms(lambda: detector.crop_resize(img, box, K, 512), dev, a.replays)
    out["crop_resize"] = {"image": [1440, 1920], "bbox": box.cpu().tolist(), "crop_size": 512,
                          "graph_ms_median": ms}
    print(json.dumps({"crop_resize_1440x1920_to_512": out["crop_resize"]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

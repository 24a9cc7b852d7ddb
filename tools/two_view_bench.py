#!/usr/bin/env python
"""Time the two-view verification (onepose_amd.sfm.two_view_verify_device), a first measurement, at

    132 pairs x 128 matches and 1000 pairs x 1024 matches, two views of points in a +-0.1 m box,
    0.5 px noise, 20 % of the matches pointing at a random pixel,

in both modes: estimate (F-matrix RANSAC and two refits) and given F (the Sampson test alone).

HIP path: onepose_two_view_verify as a captured graph on preallocated buffers; warm-up, then the
median of >= 50 replays, each between two events.  The host path (the device=None formulation,
sfm._host_two_view) runs on the same inputs in the same process, wall clock.  No target was fixed
in advance; the JSON holds what was read.

    python tools/two_view_bench.py --out profiles/two_view/bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from onepose_amd import _lib, sfm  # noqa: E402

SIZES = [("pairs_132_matches_128", 132, 128), ("pairs_1000_matches_1024", 1000, 1024)]
OPTIONS = dict(max_error=4.0, confidence=0.999, max_trials=10000, min_num_inliers=15,
               min_inlier_ratio=0.25, refine_iters=2)
F, C, OUTLIERS = 600.0, 256.0, 0.2


def look_at(c):
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    T = np.eye(4)
    T[:3] = np.concatenate([R, (-R @ c)[:, None]], axis=1)
    return T


def make_inputs(B, n, seed):
    """-> (pts0, pts1 float32 [B, n, 2], counts int32 [B], F of the poses [B, 9])."""
    rng = np.random.default_rng(seed)
    K = np.array([[F, 0, C], [0, F, C], [0, 0, 1.0]])
    p0, p1, Fs = np.empty((B, n, 2), np.float32), np.empty((B, n, 2), np.float32), np.empty((B, 9))
    for b in range(B):
        az = rng.uniform(0, 2 * np.pi) + np.array([0.0, np.deg2rad(rng.uniform(20, 40))])
        el = np.deg2rad(rng.uniform(15, 40, 2))
        Ts = [look_at(0.5 * np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)]))
              for a, e in zip(az, el)]
        X = rng.uniform(-0.1, 0.1, (n, 3))
        uv = []
        for T in Ts:
            pc = X @ T[:3, :3].T + T[:3, 3]
            uv.append(np.stack([F * pc[:, 0] / pc[:, 2] + C, F * pc[:, 1] / pc[:, 2] + C], 1)
                      + 0.5 * rng.standard_normal((n, 2)))
        wrong = rng.random(n) < OUTLIERS
        uv[1][wrong] = rng.uniform(10, 502, (int(wrong.sum()), 2))
        p0[b], p1[b] = uv[0], uv[1]
        Fs[b] = sfm.fundamental_from_poses(Ts[0], K, Ts[1], K).reshape(9)
    return p0, p1, np.full(B, n, np.int32), Fs


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
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def bench_size(B, n, dev, replays):
    p0, p1, counts, Fs = make_inputs(B, n, B)
    d0, d1, dc, dF = (torch.from_numpy(a).to(dev) for a in (p0, p1, counts, Fs))
    out = {"pairs": B, "matches_per_pair": n, "outlier_share": OUTLIERS}
    for mode, F_host, F_dev in (("estimate", None, None), ("given_F", Fs, dF)):
        t = time.perf_counter()
        host = sfm._host_two_view(p0, p1, counts, F_host, **OPTIONS)
        host_ms = (time.perf_counter() - t) * 1e3
        got = [x.cpu().numpy() for x in sfm.two_view_verify_device(d0, d1, dc, F_in=F_dev, **OPTIONS)]
        equal = all(np.array_equal(g, h) for g, h in zip(got[1:], host[1:]))
        bufs = [torch.empty_like(x) for x in sfm.two_view_verify_device(d0, d1, dc, F_in=F_dev, **OPTIONS)]
        ws = torch.empty(256, dtype=torch.uint8, device=dev)

        def run():
            _lib.run("onepose_two_view_verify", pts0=d0, pts1=d1, counts=dc, max_points=n, batch=B,
                     F_in=F_dev, F=bufs[0], inlier_mask=bufs[1], n_inliers=bufs[2], iters=bufs[3],
                     status=bufs[4], workspace=ws, workspace_bytes=256,
                     stream=_lib.stream_ptr(dev), **OPTIONS)
        med, mn = graph_ms(run, dev, replays)
        out[mode] = {"hip_graph_ms_median": med, "hip_graph_ms_min": mn, "host_ms": host_ms,
                     "host_over_hip": host_ms / med,
                     "decisions_equal_to_host_path": bool(equal),
                     "F_bits_equal_to_host_path": bool(got[0].tobytes() == host[0].tobytes()),
                     "status_counts": {str(k): int((got[4] == k).sum()) for k in range(4)},
                     "iters_mean": float(got[3].mean()), "iters_max": int(got[3].max()),
                     "inlier_share_mean": float(got[2].mean() / n)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "replays": a.replays,
           "first_measurement_no_target": True, "options": OPTIONS, "sizes": {}}
    for name, B, n in SIZES:
        out["sizes"][name] = bench_size(B, n, dev, a.replays)
        print(json.dumps({name: out["sizes"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

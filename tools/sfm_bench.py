#!/usr/bin/env python
"""Time the two device stages of the sparse reconstruction (onepose_amd.sfm), a first
measurement, at

    100 images x 1000 features and 400 images x 2000 features, every scene point seen in 8
    images, about 10 matched pairs per image, 0.5 px noise and 0.5 % wrong matches.

HIP path: onepose_track_components (16 rounds, one call) and onepose_tracks_triangulate, each as
a captured graph on preallocated buffers; warm-up, then the median of >= 50 replays, each between
two events.  The host path (the device=None formulation: a union-find loop, the batched numpy
triangulation) runs on the same inputs in the same process, wall clock.  No target was fixed in
advance; the JSON holds what was read.

    python tools/sfm_bench.py --out profiles/sfm/bench.json
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

SIZES = [("images_100_features_1000", 100, 1000), ("images_400_features_2000", 400, 2000)]
VIEWS, F, C = 8, 600.0, 256.0


def look_at(c):
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R, (-R @ c)[:, None]], axis=1)


def make_inputs(m, f, seed):
    """-> (Rt [m, 3, 4], K4 [m, 4], counts [m], keypoints + 0.5 [sum counts, 2], edges [E, 2])."""
    rng = np.random.default_rng(seed)
    az, el = rng.uniform(0, 2 * np.pi, m), np.deg2rad(rng.uniform(-40, 40, m))
    cs = 0.5 * np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    Rt = np.stack([look_at(c) for c in cs])
    K4 = np.tile([[F, F, C, C]], (m, 1))
    n_pts = m * f // VIEWS
    pts = rng.uniform(-0.1, 0.1, (n_pts, 3))
    # point k is seen by a window of 24 neighbouring cameras, 8 of them
    views = (np.sort(np.argsort(rng.random((n_pts, 24)), axis=1)[:, :VIEWS], axis=1)
             + rng.integers(0, m, n_pts)[:, None]) % m
    img = views.reshape(-1)
    order = np.argsort(img, kind="stable")
    counts = np.bincount(img, minlength=m)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    node = np.empty(len(img), dtype=np.int64)
    node[order] = np.arange(len(img))          # the global feature id of (point, view)
    node = node.reshape(n_pts, VIEWS)
    X = np.repeat(pts, VIEWS, axis=0)[order]
    pc = np.einsum("kij,kj->ki", Rt[img[order], :, :3], X) + Rt[img[order], :, 3]
    xy = np.stack([F * pc[:, 0] / pc[:, 2] + C, F * pc[:, 1] / pc[:, 2] + C], 1)
    xy += 0.5 * rng.standard_normal(xy.shape)
    edges = np.concatenate([np.stack([node[:, :-1], node[:, 1:]], -1).reshape(-1, 2),
                            np.stack([node[:, :-2], node[:, 2:]], -1).reshape(-1, 2)])
    wrong = rng.random(len(edges)) < 0.005
    edges[wrong, 1] = rng.integers(0, len(img), int(wrong.sum()))
    edges = edges[rng.permutation(len(edges))].astype(np.int32)
    return Rt, K4, counts, xy, edges, offsets


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


def host_ms(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), out


def bench_size(m, f, dev, replays, host_reps):
    lib = _lib.load()
    Rt, K4, counts, xy, edges, offsets = make_inputs(m, f, m)
    n_nodes = int(counts.sum())
    h_cc_ms, h_labels = host_ms(lambda: sfm._host_components(edges, n_nodes), host_reps)
    tracks = sfm.build_tracks(counts, edges, device=dev)
    ts, oi, of = tracks["track_start"], tracks["obs_image"], tracks["obs_feat"]
    obs_xy = xy[offsets[oi] + of]
    h_tri_ms, h_tri = host_ms(lambda: sfm.triangulate_tracks(Rt, K4, ts, oi, obs_xy), host_reps)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    E = up(edges)
    parent = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)

    def s_cc():
        _lib.check(lib.onepose_track_components(E.data_ptr(), len(edges), n_nodes, sfm.CC_ROUNDS, 1,
                                                parent.data_ptr(), status.data_ptr(),
                                                _lib.stream_ptr(dev)), "track_components")
    dRt, dK4, dts, doi, dxy = (up(a) for a in (Rt, K4, ts, oi, obs_xy))
    holder = {}

    def s_tri():
        holder["out"] = sfm.tracks_triangulate_device(dRt, dK4, dts, doi, dxy, sfm.MAX_REPROJ,
                                                      sfm.MIN_ANGLE_DEG)
    s_cc()
    s_tri()
    torch.cuda.synchronize()
    st = status.tolist()
    xyz, err, reason, n_kept, keep, tstat = (t.cpu().numpy() for t in holder["out"])
    equal = (np.array_equal(parent.cpu().numpy(), h_labels) and tstat[0] == 0
             and np.array_equal(reason, h_tri["reason"]) and np.array_equal(keep.astype(bool),
                                                                            h_tri["obs_keep"])
             and np.array_equal(xyz, h_tri["xyz"], equal_nan=True)
             and np.array_equal(err, h_tri["err"], equal_nan=True))
    # the triangulation allocates its outputs; for the graph they are allocated once, outside
    outs = [torch.empty_like(t) for t in holder["out"]]

    def s_tri_graph():
        _lib.check(lib.onepose_tracks_triangulate(
            dRt.data_ptr(), dK4.data_ptr(), m, dts.data_ptr(), doi.data_ptr(), dxy.data_ptr(),
            len(ts) - 1, len(oi), sfm.MAX_REPROJ, sfm.MIN_ANGLE_DEG, *(t.data_ptr() for t in outs),
            _lib.stream_ptr(dev)), "tracks_triangulate")
    cc_med, cc_min = graph_ms(s_cc, dev, replays)
    tri_med, tri_min = graph_ms(s_tri_graph, dev, replays)
    lens = np.diff(ts)
    return {"images": m, "features_per_image": f, "nodes": n_nodes, "edges": int(len(edges)),
            "tracks": int(len(lens)), "observations": int(len(oi)),
            "track_length_mean": float(lens.mean()), "track_length_max": int(lens.max()),
            "tracks_kept": int((reason == 0).sum()),
            "reasons": {str(k): int((reason == k).sum()) for k in range(5)},
            "components_rounds_that_joined": st[1], "components_open_edges": st[0],
            "equal_to_host_path": bool(equal),
            "components": {"hip_graph_ms_median": cc_med, "hip_graph_ms_min": cc_min,
                           "host_ms_median": h_cc_ms, "host_over_hip": h_cc_ms / cc_med},
            "triangulation": {"hip_graph_ms_median": tri_med, "hip_graph_ms_min": tri_min,
                              "host_ms_median": h_tri_ms, "host_over_hip": h_tri_ms / tri_med}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--host", type=int, default=1, help="timed host calls per stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "replays": a.replays, "host_calls": a.host,
           "first_measurement_no_target": True, "sizes": {}}
    for name, m, f in SIZES:
        out["sizes"][name] = bench_size(m, f, dev, a.replays, a.host)
        print(json.dumps({name: out["sizes"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

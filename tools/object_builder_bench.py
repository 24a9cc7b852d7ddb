#!/usr/bin/env python
"""Time the object builder (onepose_amd.object_builder: SfM filter, radius neighbours, greedy
merge, descriptor lifting, leaf gather) stage by stage and as one chain, a first measurement, at

    2500 points (the reference's max_num_kp3d) and 16384 points (config 3), about 10
    observations per point, dim 256, 8 leaves.

HIP path: every stage and the whole chain as a captured graph on preallocated buffers; warm-up,
then the median of >= 50 replays, each between two events.  The numpy path (the device=None
formulation of the same functions, neighbour lists instead of the reference's n x n matrix) runs
on the same inputs in the same process, wall clock, the median of `--host` calls.  The lifting
kernel's traffic is computed from the shapes: the gathered fp32 values, the observation lists,
the fp64 collected array and both means; bytes over time is reported next to it.

    python tools/object_builder_bench.py --out profiles/object_builder/bench.json
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

from onepose_amd import _lib, data_utils, object_builder as ob  # noqa: E402

DIM, LEAVES, THR, IMAGES = 256, 8, 1e-3, 200
SIZES = [("points_2500", 2500), ("points_16384", 16384)]


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
        run()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return median_ms(graph.replay, replays)


def host_ms(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), out


def make_inputs(n, seed):
    """n model points in a unit box (about one in eight fails a filter), spaced so that a few
    percent of the kept ones have a neighbour within the threshold."""
    rs = np.random.RandomState(seed)
    side = (n * n * 4.19e-9 / (0.03 * n)) ** (1 / 3)      # ~0.03 n near pairs
    corners = side * np.array([[0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1],
                               [0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], dtype=np.float64)
    xyz = rs.uniform(-0.02 * side, 1.02 * side, size=(n, 3))
    return xyz, rs.randint(3, 40, size=n).astype(np.int32), corners


def make_observations(n3, seed):
    rs = np.random.RandomState(seed)
    idxs = rs.randint(6, 15, size=n3).astype(np.int64)       # about 10 per point
    S = int(idxs.sum())
    per = -(-S // IMAGES) + 16
    desc = [rs.standard_normal((DIM, per)).astype(np.float32) for _ in range(IMAGES)]
    return desc, rs.randint(0, IMAGES, size=S).astype(np.int32), \
        rs.randint(0, per, size=S).astype(np.int32), idxs


def bench_size(n, dev, replays, host_reps):
    lib, st = _lib.load(), lambda: _lib.stream_ptr(dev)
    xyz, tl, corners = make_inputs(n, n)
    min_track = 4

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def i32(k):
        return torch.empty(k, dtype=torch.int32, device=dev)
    # ---- numpy path, and the sizes the device buffers need
    f_ms, (hx, hidx) = host_ms(lambda: ob.filter_3d({"ids": np.arange(n), "xyz": xyz, "track_len": tl},
                                                     min_track, corners), host_reps)
    hx = hx.numpy()
    nb_ms, (hrs, hcols) = host_ms(lambda: ob._host_neighbours(hx, THR), host_reps)
    g_ms, hm = host_ms(lambda: ob._host_greedy(hx, hrs, hcols), host_reps)
    m, total, n3 = len(hx), int(hrs[-1]), len(hm[1]) - 1
    desc, oi, of, idxs = make_observations(n3, n + 1)
    S = len(oi)
    l_ms, (hcol, h64, h32) = host_ms(lambda: ob.lift_descriptors(desc, oi, of, idxs), host_reps)
    np.random.seed(0)
    leaf_cols = data_utils.leaf_indices(idxs, LEAVES, S)
    lv_ms, hleaves = host_ms(lambda: np.concatenate(
        [hcol.astype(np.float32), np.ones((DIM, 1), np.float32)], axis=1)[:, leaf_cols], host_reps)

    # ---- device buffers
    X, T, B = up(xyz), up(tl), up(corners)
    fx, fi, fc = torch.empty(n, 3, dtype=torch.float32, device=dev), i32(n), i32(1)
    rs_, cols, ninfo = i32(m + 1), i32(total), torch.empty(2, dtype=torch.int64, device=dev)
    cof, ms, mem, minfo = i32(m), i32(m + 1), i32(m), i32(2)
    mean = torch.empty(m, 3, dtype=torch.float64, device=dev)
    ncols = np.asarray([d.shape[1] for d in desc], dtype=np.int64)
    bank = up(np.concatenate([d.reshape(-1) for d in desc]))
    off = up(np.concatenate([[0], np.cumsum(ncols[:-1] * DIM)]).astype(np.int64))
    NC, OI, OF, SEG = up(ncols.astype(np.int32)), up(oi), up(of), up(idxs.astype(np.int32))
    ss, linfo = i32(n3 + 1), i32(2)
    col = torch.empty(DIM, S, dtype=torch.float64, device=dev)
    m64 = torch.empty(DIM, n3, dtype=torch.float64, device=dev)
    m32 = torch.empty(DIM, n3, dtype=torch.float32, device=dev)
    LC = up(leaf_cols)
    leaves = torch.empty(DIM, len(leaf_cols), dtype=torch.float32, device=dev)

    def s_filter():
        _lib.check(lib.onepose_filter_points(X.data_ptr(), T.data_ptr(), n, min_track, B.data_ptr(),
                                             fx.data_ptr(), fi.data_ptr(), fc.data_ptr(), st()), "filter")

    def s_neigh():
        _lib.check(lib.onepose_radius_neighbours(fx.data_ptr(), ob.OBJ_F32, m, THR, rs_.data_ptr(),
                                                 cols.data_ptr(), total, ninfo.data_ptr(), st()), "nb")

    def s_merge():
        _lib.check(lib.onepose_merge_greedy(fx.data_ptr(), ob.OBJ_F32, m, rs_.data_ptr(),
                                            cols.data_ptr(), cof.data_ptr(), ms.data_ptr(),
                                            mem.data_ptr(), mean.data_ptr(), minfo.data_ptr(), st()),
                   "merge")

    def s_lift():
        _lib.check(lib.onepose_lift_descriptors(bank.data_ptr(), bank.numel(), off.data_ptr(),
                                                NC.data_ptr(), IMAGES, OI.data_ptr(), OF.data_ptr(), S,
                                                SEG.data_ptr(), n3, DIM, ss.data_ptr(), col.data_ptr(),
                                                m64.data_ptr(), m32.data_ptr(), linfo.data_ptr(), st()),
                   "lift")

    def s_leaves():
        _lib.check(lib.onepose_gather_leaves(col.data_ptr(), S, DIM, LC.data_ptr(), len(leaf_cols),
                                             leaves.data_ptr(), st()), "leaves")
    stages = [("filter", s_filter, f_ms), ("radius_neighbours", s_neigh, nb_ms),
              ("merge_greedy", s_merge, g_ms), ("lift_descriptors", s_lift, l_ms),
              ("gather_leaves", s_leaves, lv_ms)]
    for _, fn, _ in stages:     # once eagerly: the later stages read the earlier ones' outputs
        fn()
    torch.cuda.synchronize()
    equal = (int(fc.item()) == m and np.array_equal(fx[:m].cpu().numpy(), hx)
             and ninfo.tolist() == [total, 0] and np.array_equal(cols.cpu().numpy(), hcols)
             and minfo.tolist() == [n3, 0] and np.array_equal(mean[:n3].cpu().numpy(), hm[3])
             and linfo.tolist() == [0, 0] and np.array_equal(col.cpu().numpy(), hcol)
             and np.array_equal(m64.cpu().numpy(), h64) and np.array_equal(m32.cpu().numpy(), h32)
             and np.array_equal(leaves.cpu().numpy(), hleaves))
    res = {"points": n, "kept_by_filter": m, "neighbour_pairs": total, "merged_points": n3,
           "observations": S, "dim": DIM, "leaves": LEAVES, "bits_equal_numpy_path": bool(equal),
           "stages": {}}
    for name, fn, h in stages:
        g = graph_ms(fn, dev, replays)
        res["stages"][name] = {"hip_graph_ms_median": g, "numpy_ms_median": h,
                               "numpy_over_hip": h / g}
    chain = graph_ms(lambda: [fn() for _, fn, _ in stages], dev, replays)
    host_chain = sum(h for _, _, h in stages)
    res["chain"] = {"hip_graph_ms_median": chain, "numpy_ms_sum_of_stage_medians": host_chain,
                    "numpy_over_hip": host_chain / chain}
    lift_bytes = 4 * DIM * S + 8 * S + 8 * DIM * S + 12 * DIM * n3 + 8 * n3
    t = res["stages"]["lift_descriptors"]["hip_graph_ms_median"] * 1e-3
    res["lift_bytes_moved"] = lift_bytes
    res["lift_gbytes_per_s"] = lift_bytes / t / 1e9
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--host", type=int, default=3, help="timed numpy calls per stage")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "replays": a.replays, "numpy_calls": a.host,
           "dist_threshold": THR, "first_measurement_no_target": True, "sizes": {}}
    for name, n in SIZES:
        out["sizes"][name] = bench_size(n, dev, a.replays, a.host)
        print(json.dumps({name: out["sizes"][name]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

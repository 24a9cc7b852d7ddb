#!/usr/bin/env python
"""Time the NearestNeighbour matcher (onepose_amd.nn_matcher, ratio 0.8, mutual check on) against
an eager PyTorch-ROCm evaluation of the reference's formula, a first measurement, on

    pairs 1024 x 1024, 2048 x 2048, 4096 x 4096 and B = 10 keyframes x 2048 against one shared
    query of 2048 (d = 256).

HIP path: warm-up, then the median of >= 50 replays of a captured graph of onepose_nn_match,
each between two events.  The similarity launch is timed the same way on its own
(onepose_nn_similarity_top2: launch 1 alone); the merge and mutual launches are reported as the
difference of the two medians, a derived number (the profile hook's kinds are a closed list, so
these launches are not bracketed one by one).  Eager path, same process: einsum, two topk(2), the
masks and the gather written below, and the einsum alone; warm-up, then the median of `--eager`
calls.  mfma_peak_fraction = 2 B d n0 n1 FLOP over the similarity launch's time, against the
157.3 TFLOP/s fp32 MFMA peak.  Partial and matrix bytes are computed from the shapes.

    python tools/nn_bench.py --out profiles/nn/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from onepose_amd import _lib, nn_matcher, synthetic  # noqa: E402

RATIO, D = 0.8, 256
PEAK_FP32_MFMA = 157.3e12
SHAPES = [("pair_1024", 1, 1024, 1024), ("pair_2048", 1, 2048, 2048),
          ("pair_4096", 1, 4096, 4096), ("keyframes_b10_2048_shared_query", 10, 2048, 2048)]


# ------------------------------------------------------------------ eager formulation
def eager_find_nn(sim, ratio):
    val, ind = sim.topk(2, dim=-1)
    dist = 2 * (1 - val)
    ok = dist[..., 0] <= (ratio ** 2) * dist[..., 1]
    return (torch.where(ok, ind[..., 0], ind.new_tensor(-1)),
            torch.where(ok, (val[..., 0] + 1) / 2, val.new_tensor(0)))


def eager_forward(d0, d1, ratio):
    sim = torch.einsum("bdn,bdm->bnm", d0, d1)
    m0, s0 = eager_find_nn(sim, ratio)
    m1, s1 = eager_find_nn(sim.transpose(1, 2), ratio)
    loop = torch.gather(m1, -1, torch.where(m0 > -1, m0, m0.new_tensor(0)))
    keep = (m0 > -1) & (loop == torch.arange(m0.shape[-1], device=m0.device))
    return torch.where(keep, m0, m0.new_tensor(-1)), m1, s0, s1


# ------------------------------------------------------------------ timing
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


def bench_shape(name, B, n0, n1, dev, replays, eager_reps):
    x = synthetic.make_nn_inputs(n0, n1, 0, batch=B, shared1=B > 1)
    d0 = torch.from_numpy(x["descriptors0"]).to(dev)
    d1 = torch.from_numpy(x["descriptors1"]).to(dev)                    # [1, d, n1] when shared
    lib = _lib.load()
    ws = torch.empty(lib.onepose_nn_match_workspace_bytes(B, n0, n1), dtype=torch.uint8, device=dev)
    bs1 = 0 if B > 1 else D * n1

    def sim_only():
        _lib.check(lib.onepose_nn_similarity_top2(d0.data_ptr(), D * n0, d1.data_ptr(), bs1,
                                                  _lib.DT_F32, B, D, n0, n1, ws.data_ptr(),
                                                  ws.numel(), _lib.stream_ptr(dev)), "nn_sim")

    full_ms, out = graph_ms(lambda: nn_matcher.nearest_neighbour_match(d0, d1, RATIO, None, True,
                                                                      workspace=ws), dev, replays)
    sim_ms, _ = graph_ms(sim_only, dev, replays)
    e1 = d1.expand(B, -1, -1)
    for _ in range(3):
        ref = eager_forward(d0, e1, RATIO)
        torch.einsum("bdn,bdm->bnm", d0, e1)
    torch.cuda.synchronize()
    eager_ms = median_ms(lambda: eager_forward(d0, e1, RATIO), eager_reps)
    einsum_ms = median_ms(lambda: torch.einsum("bdn,bdm->bnm", d0, e1), eager_reps)
    flop = 2.0 * B * D * n0 * n1
    differ = int((out[0] != ref[0]).sum() + (out[1] != ref[1]).sum())
    return {
        "batch": B, "n0": n0, "n1": n1, "d": D, "side1_shared": B > 1,
        "hip_graph_ms_median": full_ms, "eager_ms_median": eager_ms,
        "eager_over_hip": eager_ms / full_ms,
        "similarity_launch_ms_median": sim_ms,
        "merge_and_mutual_ms_derived": full_ms - sim_ms,
        "eager_einsum_ms_median": einsum_ms,
        "similarity_slower_than_eager_einsum": bool(sim_ms > einsum_ms),
        "similarity_tflops": flop / (sim_ms * 1e-3) / 1e12,
        "mfma_peak_fraction": flop / (sim_ms * 1e-3) / PEAK_FP32_MFMA,
        "partials_bytes": ws.numel(), "sim_matrix_bytes": 4 * B * n0 * n1,
        "matched_rows": int((out[0] > -1).sum()),
        "indices_differing_from_eager": differ,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--eager", type=int, default=20, help="timed eager calls per shape")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "replays": a.replays,
           "eager_calls": a.eager, "ratio_threshold": RATIO, "do_mutual_check": True,
           "peak_fp32_mfma_tflops": PEAK_FP32_MFMA / 1e12, "shapes": {}}
    for name, B, n0, n1 in SHAPES:
        out["shapes"][name] = bench_shape(name, B, n0, n1, dev, a.replays, a.eager)
        print(json.dumps({name: out["shapes"][name]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

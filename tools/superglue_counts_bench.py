#!/usr/bin/env python
"""Time the variable-count SuperGlue entry (onepose_superglue_match_counts) against the uniform
one, in tools/superglue_bench.py's style: warm-up, then the median of >= 50 replays of a
captured graph, each between two events, at 100 Sinkhorn iterations.

    detector shape      15 views with counts spread evenly over 700..1024 against one shared
                        1024-point query: ONE counts call against the 15 single-pair calls of
                        the uniform entry (all 15 in one graph), both times, their ratio and the
                        padded / real token ratio
    counts overhead     B = 15 at 1024 x 1024 uniform: the counts entry with NULL counts, with
                        counts all 1024, and the uniform entry
    match_pairs         200 pairs drawn from 40 images with 300..2048 keypoints, end to end (wall
                        clock, uploads and downloads included) at batch_size 8 and 16 against
                        batch_size=None

Nothing here is tuned (max_pad_ratio is match_pairs' default).

    python tools/superglue_counts_bench.py --out profiles/superglue/counts_bench.json
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

from onepose_amd import sfm, superglue, synthetic  # noqa: E402

ITERS = 100


def graph_ms(fn, dev, replays):
    """Median (and min, max) of `replays` replays of fn captured in a graph."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(3):
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
    return {"ms_median": float(np.median(times)), "ms_min": float(min(times)),
            "ms_max": float(max(times)), "replays": replays}


def dev_inputs(n0, n1, B, shared, dev, seed=9):
    data = synthetic.make_superglue_inputs(n0, n1, seed=seed, batch=B, shared1=shared)
    d = {}
    for k, v in data.items():
        t = torch.as_tensor(v).to(dev)
        d[k] = t.expand(B, *t.shape[1:]) if t.shape[0] != B else t
    return d


def bench_detector(model, dev, replays):
    B, n = 15, 1024
    counts = [int(round(c)) for c in np.linspace(700, 1024, B)]
    d = dev_inputs(n, n, B, True, dev)
    padded = dict(d)
    for k in ("keypoints0", "scores0", "descriptors0"):
        padded[k] = d[k].clone()
    for b, c in enumerate(counts):                       # zeros past each view's count
        padded["keypoints0"][b, c:] = 0
        padded["scores0"][b, c:] = 0
        padded["descriptors0"][b, :, c:] = 0
    padded["counts0"] = torch.tensor(counts, dtype=torch.int32, device=dev)
    singles = []
    for b, c in enumerate(counts):
        s = {"keypoints0": d["keypoints0"][b:b + 1, :c].contiguous(),
             "scores0": d["scores0"][b:b + 1, :c].contiguous(),
             "descriptors0": d["descriptors0"][b:b + 1, :, :c].contiguous(),
             "keypoints1": d["keypoints1"][:1], "scores1": d["scores1"][:1],
             "descriptors1": d["descriptors1"][:1], "image0": d["image0"][:1],
             "image1": d["image1"][:1]}
        singles.append(s)
    with torch.no_grad():
        one = model(padded)
        per = [model(s) for s in singles]
        torch.cuda.synchronize()
        same = all(bool((one["matches0"][b, :c] == per[b]["matches0"][0]).all().item())
                   for b, c in enumerate(counts))
        t_one = graph_ms(lambda: model(padded), dev, replays)
        t_per = graph_ms(lambda: [model(s) for s in singles], dev, replays)
    real = sum(counts) + B * n
    res = {"views": B, "counts0": counts, "n1": n, "iters": ITERS,
           "one_counts_call": t_one, "fifteen_single_pair_calls": t_per,
           "ratio_single_over_one": t_per["ms_median"] / t_one["ms_median"],
           "padded_over_real_tokens": B * (n + n) / real,
           "indices_equal_single_pair_calls": same}
    print(json.dumps({"detector_shape": res}))
    return res


def bench_overhead(model, dev, replays):
    B, n = 15, 1024
    d = dev_inputs(n, n, B, False, dev)
    hw = torch.tensor([[512, 512]] * B, dtype=torch.int32, device=dev)
    null = {**d, "image_hw0": hw}                         # the counts entry, NULL counts
    full = {**d, "counts0": torch.full((B,), n, dtype=torch.int32, device=dev),
            "counts1": torch.full((B,), n, dtype=torch.int32, device=dev)}
    with torch.no_grad():
        a, b, c = model(d), model(null), model(full)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k])) for k in a)
        res = {"batch": B, "n0": n, "n1": n, "iters": ITERS,
               "uniform_entry": graph_ms(lambda: model(d), dev, replays),
               "counts_entry_null_counts": graph_ms(lambda: model(null), dev, replays),
               "counts_entry_counts_all_1024": graph_ms(lambda: model(full), dev, replays),
               "bits_equal": same}
    print(json.dumps({"counts_path_overhead": res}))
    return res


def bench_match_pairs(model, dev):
    rs = np.random.RandomState(17)
    names = [f"obj/color/{i}.png" for i in range(40)]
    feats = {}
    for i, name in enumerate(names):
        n = int(rs.randint(300, 2049))
        d = synthetic.make_superglue_inputs(n, 8, seed=100 + i)
        feats[name] = {"keypoints": d["keypoints0"][0], "scores": d["scores0"][0],
                       "descriptors": d["descriptors0"][0], "image_size": np.array([512, 512])}
    all_pairs = [(names[i], names[j]) for i in range(40) for j in range(i + 1, 40)]
    pairs = [all_pairs[i] for i in rs.permutation(len(all_pairs))[:200]]
    res = {"pairs": len(pairs), "images": 40, "iters": ITERS}
    ref = None
    for bs in (None, 8, 16):
        sfm.match_pairs(feats, pairs[:4], model, device=dev, batch_size=bs)     # warm up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sfm.match_pairs(feats, pairs, model, device=dev, batch_size=bs)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        key = "per_pair" if bs is None else f"batch_size_{bs}"
        res[key] = {"wall_s": t}
        if bs is None:
            ref = out
        else:
            counts = [(len(feats[a]["scores"]), len(feats[b]["scores"])) for a, b in pairs]
            groups = sfm.plan_match_batches(counts, bs)
            res[key]["matcher_calls"] = len(groups)
            res[key]["speedup_vs_per_pair"] = res["per_pair"]["wall_s"] / t
            res[key]["pairs_with_equal_matches0"] = sum(
                bool(np.array_equal(out[p]["matches0"], ref[p]["matches0"])) for p in ref)
    print(json.dumps({"match_pairs": res}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=["detector", "overhead", "match_pairs"])
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    model = superglue.from_state_dict(synthetic.superglue_state_dict(11),
                                      {"sinkhorn_iterations": ITERS}).to(dev)
    out = {"device": torch.cuda.get_device_name(dev)}
    if a.only in (None, "detector"):
        out["detector_shape"] = bench_detector(model, dev, a.replays)
    if a.only in (None, "overhead"):
        out["counts_path_overhead"] = bench_overhead(model, dev, a.replays)
    if a.only in (None, "match_pairs"):
        out["match_pairs"] = bench_match_pairs(model, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the SuperGlue forward (onepose_amd.superglue) against an eager PyTorch-ROCm
formulation of the same forward, on three shapes:

    pair 1024 x 1024, pair 2048 x 2048 (100 Sinkhorn iterations), and the detector's workload:
    B = 15 at 1024 x 1024 with image 1 shared by the batch.

HIP path: warm-up, then >= 50 replays of one captured graph, each between two events; the median
is reported.  Eager path: the reference's formulas (einsum, softmax, logsumexp) written below,
warm-up and the median of a few calls in the same process.  One more eager HIP forward runs
under the event profile hook for the per-kind split; the Sinkhorn stage's achieved bytes/s is
2 * iters * B * (n0+1)(n1+1) * 4 bytes over its time.  The Sinkhorn entry point is also timed on its
own (a captured graph of 100 iterations) at 1024, 2048, 4096 and 8192 points a side.

    python tools/superglue_bench.py --out profiles/superglue/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from onepose_amd import _lib, superglue, synthetic  # noqa: E402

ITERS = 100
SHAPES = [("pair_1024", 1, 1024, 1024, False), ("pair_2048", 1, 2048, 2048, False),
          ("detector_b15_1024", 15, 1024, 1024, True)]


# ------------------------------------------------------------------ eager formulation
def _mlp(sd, prefix, x, n):
    for j in range(n):
        x = torch.einsum("oc,bcn->bon", sd[f"{prefix}.{3 * j}.weight"][:, :, 0], x) \
            + sd[f"{prefix}.{3 * j}.bias"][None, :, None]
        if j < n - 1:
            p = f"{prefix}.{3 * j + 1}"
            x = (x - sd[p + ".running_mean"][None, :, None]) / torch.sqrt(
                sd[p + ".running_var"][None, :, None] + 1e-5)
            x = torch.relu(x * sd[p + ".weight"][None, :, None] + sd[p + ".bias"][None, :, None])
    return x


def _conv(sd, name, x):
    return torch.einsum("oc,bcn->bon", sd[name + ".weight"][:, :, 0], x) + sd[name + ".bias"][None, :, None]


def _propagate(sd, p, x, src):
    B = x.shape[0]
    q, k, v = (_conv(sd, f"{p}.attn.proj.{j}", t).view(B, 64, 4, -1)
               for j, t in enumerate((x, src, src)))
    prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / 8.0, dim=-1)
    msg = torch.einsum("bhnm,bdhm->bdhn", prob, v).contiguous().view(B, 256, -1)
    return _mlp(sd, f"{p}.mlp", torch.cat([x, _conv(sd, f"{p}.attn.merge", msg)], dim=1), 2)


def eager_forward(sd, data, iters, thr):
    def encode(i):
        kp, im = data[f"keypoints{i}"], data[f"image{i}"]
        h, w = im.shape[-2:]
        size = kp.new_tensor([[w, h]])
        kn = (kp - (size / 2)[:, None, :]) / (size.max(1, keepdim=True).values * 0.7)[:, None, :]
        x = torch.cat([kn.transpose(1, 2), data[f"scores{i}"].unsqueeze(1)], dim=1)
        return data[f"descriptors{i}"] + _mlp(sd, "kenc.encoder", x, 5)

    d0, d1 = encode(0), encode(1)
    for i in range(18):
        p = f"gnn.layers.{i}"
        s0, s1 = (d1, d0) if i % 2 else (d0, d1)
        d0, d1 = d0 + _propagate(sd, p, d0, s0), d1 + _propagate(sd, p, d1, s1)
    m0, m1 = _conv(sd, "final_proj", d0), _conv(sd, "final_proj", d1)
    S = torch.einsum("bdn,bdm->bnm", m0, m1) / 16.0
    b, m, n = S.shape
    a = sd["bin_score"]
    Z = torch.cat([torch.cat([S, a.expand(b, m, 1)], -1), a.expand(b, 1, n + 1)], 1)
    ms, ns = S.new_tensor(float(m)), S.new_tensor(float(n))
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])[None].expand(b, -1)
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])[None].expand(b, -1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    Z = Z + u.unsqueeze(2) + v.unsqueeze(1) - norm
    max0, max1 = Z[:, :-1, :-1].max(2), Z[:, :-1, :-1].max(1)
    i0, i1 = max0.indices, max1.indices
    ar0 = torch.arange(m, device=S.device)[None]
    ar1 = torch.arange(n, device=S.device)[None]
    mutual0, mutual1 = ar0 == i1.gather(1, i0), ar1 == i0.gather(1, i1)
    sc0 = torch.where(mutual0, max0.values.exp(), S.new_tensor(0))
    sc1 = torch.where(mutual1, sc0.gather(1, i1), S.new_tensor(0))
    valid0 = mutual0 & (sc0 > thr)
    valid1 = mutual1 & valid0.gather(1, i1)
    return {"matches0": torch.where(valid0, i0, i0.new_tensor(-1)),
            "matches1": torch.where(valid1, i1, i1.new_tensor(-1)),
            "matching_scores0": sc0, "matching_scores1": sc1}


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
    return float(np.median(times)), times


def kind_split(lib, fn, cap=4096):
    names = {}
    for k in range(64):
        n = lib.onepose_profile_kind_name(k)
        if n:
            names[k] = n.decode()
    _lib.check(lib.onepose_profile_begin((1 << 64) - 1, cap), "profile_begin")
    fn()
    kinds, ms, cnt = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(1, np.int32)
    _lib.check(lib.onepose_profile_end(kinds.ctypes.data, ms.ctypes.data, cap, cnt.ctypes.data),
               "profile_end")
    out = {}
    for k, t in zip(kinds[:int(cnt[0])], ms[:int(cnt[0])]):
        e = out.setdefault(names[int(k)], {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += float(t)
    return out


def bench_shape(name, B, n0, n1, shared, sd_np, dev, replays, eager_reps):
    lib = _lib.load()
    data = synthetic.make_superglue_inputs(n0, n1, seed=9, batch=B, shared1=shared)
    d = {}
    for k, v in data.items():
        t = torch.as_tensor(v).to(dev)
        d[k] = t.expand(B, *t.shape[1:]) if t.shape[0] != B else t
    model = superglue.from_state_dict(sd_np, {"sinkhorn_iterations": ITERS}).to(dev)
    sd = {k: v.to(dev) for k, v in model.state_dict().items()}
    with torch.no_grad():
        hip = model(d)
        ref = eager_forward(sd, d, ITERS, 0.2)
        torch.cuda.synchronize()
        same = bool((hip["matches0"] == ref["matches0"]).all().item())
        dscore = float((hip["matching_scores0"] - ref["matching_scores0"]).abs().max().item())
        split = kind_split(lib, lambda: model(d))
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                model(d)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            model(d)
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        hip_ms, hip_times = median_ms(graph.replay, replays)
        for _ in range(2):
            eager_forward(sd, d, ITERS, 0.2)
        torch.cuda.synchronize()
        eager_ms, _ = median_ms(lambda: eager_forward(sd, d, ITERS, 0.2), eager_reps)
    sk_ms = split.get("sg_sinkhorn", {}).get("ms", 0.0)
    sk_bytes = 2.0 * ITERS * B * (n0 + 1) * (n1 + 1) * 4
    res = {"shape": {"batch": B, "n0": n0, "n1": n1, "side1_shared": shared, "iters": ITERS},
           "hip_graph_ms_median": hip_ms, "hip_replays": replays,
           "hip_graph_ms_min": float(min(hip_times)), "hip_graph_ms_max": float(max(hip_times)),
           "eager_torch_ms_median": eager_ms, "eager_reps": eager_reps,
           "speedup_vs_eager": eager_ms / hip_ms,
           "indices_equal_eager": same, "max_score_diff_vs_eager": dscore,
           "per_kind_eager_launches": split,
           "sinkhorn_ms": sk_ms, "sinkhorn_bytes": sk_bytes,
           "sinkhorn_GBps": sk_bytes / (sk_ms * 1e-3) / 1e9 if sk_ms > 0 else None}
    print(json.dumps({name: {k: v for k, v in res.items() if k != "per_kind_eager_launches"}}))
    return res


def bench_sinkhorn_alone(m, n, dev, replays):
    """onepose_log_optimal_transport on an m x n matrix, 100 iterations in one captured graph."""
    lib = _lib.load()
    S = torch.randn(1, m, n, device=dev) * 10
    out = torch.empty(1, m + 1, n + 1, device=dev)
    nbytes = lib.onepose_log_optimal_transport_workspace_bytes(1, m, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run():
        _lib.check(lib.onepose_log_optimal_transport(S.data_ptr(), m * n, 1, m, n, 1.0, ITERS,
                                                     out.data_ptr(), ws.data_ptr(), nbytes,
                                                     _lib.stream_ptr(dev)), "log_optimal_transport")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ms, _ = median_ms(graph.replay, replays)
    nbytes_moved = 2.0 * ITERS * (m + 1) * (n + 1) * 4
    res = {"m": m, "n": n, "iters": ITERS, "graph_ms_median": ms,
           "GBps": nbytes_moved / (ms * 1e-3) / 1e9}
    print(json.dumps({f"sinkhorn_alone_{m}x{n}": res}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--eager-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape name")
    a = ap.parse_args()
    assert a.replays >= 50, "at least 50 graph replays"
    dev = torch.device("cuda", 0)
    sd_np = synthetic.superglue_state_dict(11)
    out = {"device": torch.cuda.get_device_name(dev), "shapes": {}}
    for name, B, n0, n1, shared in SHAPES:
        if a.only and a.only != name:
            continue
        out["shapes"][name] = bench_shape(name, B, n0, n1, shared, sd_np, dev, a.replays,
                                          a.eager_reps)
    if not a.only:
        out["sinkhorn_alone"] = [bench_sinkhorn_alone(m, m, dev, a.replays)
                                 for m in (1024, 2048, 4096, 8192)]
    out["hip_faster_on_all"] = all(s["speedup_vs_eager"] > 1 for s in out["shapes"].values())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"hip_faster_on_all": out["hip_faster_on_all"]}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the tracker back end (onepose_ba_solve, onepose_ba_linearize, onepose_triangulate), a first
measurement, against the same Levenberg-Marquardt written in eager PyTorch-ROCm float64
(index_add_, linalg.cholesky), in the same process, on

    11 cameras x 500 observations each, 21 cameras x 1000 each (600 / 1200 points), the
    linearisation alone at both shapes, and triangulation of 1000 pairs.

HIP path: warm-up, then the median of 50 replays of a captured graph, each between two events.
The solve moves its variables, so the graph of the solve begins with two device copies that put
the initial variables back; they are inside the timed window.  Eager path: the same algorithm
(tests/ba_oracle.py) on torch tensors, its index lists prepared once outside the timed window as
the HIP path's index is, its accept / reject decision read on the host as eager code does;
warm-up, then the median of `--eager` calls.  No target is set for these numbers.

    python tools/ba_bench.py --out profiles/ba/bench.json
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

import ba_oracle as O  # noqa: E402
from onepose_amd import _lib, synthetic, tracker  # noqa: E402

# (cameras) x (observations per camera), with enough points for distinct (camera, point) pairs
SHAPES = [("window_11x500", dict(n_cams=11, n_points=600, n_obs=11 * 500)),
          ("window_21x1000", dict(n_cams=21, n_points=1200, n_obs=21 * 1000))]


# ------------------------------------------------------------------ eager formulation
def _skew(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1),
                        torch.stack([v[:, 2], z, -v[:, 0]], 1),
                        torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def eager_linearize(points, cams, feats, pt, cam, jac=True):
    X, w, t = points[pt], cams[cam, :3], cams[cam, 3:6]
    th2 = (w * w).sum(1)
    th = torch.sqrt(th2)
    c, s = torch.cos(th), torch.sin(th)
    a, b = s / th, (1.0 - c) / th2
    wx, wd = torch.linalg.cross(w, X), (w * X).sum(1)
    p = X * c[:, None] + wx * a[:, None] + w * (b * wd)[:, None] + t
    f = feats[:, 2]
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = torch.stack([f * xp + feats[:, 3] - feats[:, 0], f * yp + feats[:, 4] - feats[:, 1]], 1)
    if not jac:
        return r
    eye = torch.eye(3, dtype=X.dtype, device=X.device)[None]
    ca, ab = (c - a) / th2, (a - 2.0 * b) / th2
    ww = w[:, :, None] * w[:, None, :]
    R = c[:, None, None] * eye + a[:, None, None] * _skew(w) + b[:, None, None] * ww
    M = (-a[:, None, None] * (X[:, :, None] * w[:, None, :])
         + ca[:, None, None] * (wx[:, :, None] * w[:, None, :]) - a[:, None, None] * _skew(X)
         + b[:, None, None] * (w[:, :, None] * X[:, None, :] + wd[:, None, None] * eye)
         + (ab * wd)[:, None, None] * ww)
    iz = 1.0 / p[:, 2]
    D = torch.zeros(len(X), 2, 3, dtype=X.dtype, device=X.device)
    D[:, 0, 0] = D[:, 1, 1] = f * iz
    D[:, 0, 2] = -f * xp * iz
    D[:, 1, 2] = -f * yp * iz
    return r, torch.cat([D @ M, D], 2), D @ R


def eager_solve(points, cams, feats, pt, cam, lists, iters=5, radius=1e4):
    """The header's algorithm with the rotation's theta > 0 branch only (the bench scene has no
    zero rotation).  lists = (active cams, active points, slot per observation x 2, pair lists)."""
    act_c, act_p, ac, ap, pn, pm = lists
    A, Pa = len(act_c), len(act_p)
    f64 = dict(dtype=torch.float64, device=points.device)
    cur = 0.5 * (eager_linearize(points, cams, feats, pt, cam, jac=False) ** 2).sum().item()
    factor, succ = 2.0, 0
    i6, i3 = torch.arange(6, device=points.device), torch.arange(3, device=points.device)
    for _ in range(iters):
        r, Jc, Jp = eager_linearize(points, cams, feats, pt, cam)
        mu = 1.0 / radius
        JcT, JpT = Jc.transpose(1, 2), Jp.transpose(1, 2)
        U = torch.zeros(A, 6, 6, **f64).index_add_(0, ac, JcT @ Jc)
        V = torch.zeros(Pa, 3, 3, **f64).index_add_(0, ap, JpT @ Jp)
        gc = torch.zeros(A, 6, **f64).index_add_(0, ac, (JcT @ r[:, :, None])[:, :, 0])
        gp = torch.zeros(Pa, 3, **f64).index_add_(0, ap, (JpT @ r[:, :, None])[:, :, 0])
        W = JcT @ Jp
        U[:, i6, i6] += mu * U[:, i6, i6].clamp(1e-6, 1e32)
        V[:, i3, i3] += mu * V[:, i3, i3].clamp(1e-6, 1e32)
        Vinv = torch.linalg.inv(V)
        T = W @ Vinv[ap]
        S4 = torch.zeros(A * A, 6, 6, **f64)
        S4[torch.arange(A, device=points.device) * (A + 1)] = U
        S4.index_add_(0, ac[pn] * A + ac[pm], -(T[pn] @ W[pm].transpose(1, 2)))
        rhs = (-gc).index_add_(0, ac, (T @ gp[ap][:, :, None])[:, :, 0])
        S = S4.view(A, A, 6, 6).permute(0, 2, 1, 3).reshape(6 * A, 6 * A)
        L, bad = torch.linalg.cholesky_ex(S)
        accept = False
        if bad.item() == 0:
            dc = torch.cholesky_solve(rhs.reshape(-1, 1), L).reshape(A, 6)
            bb = (-gp).index_add_(0, ap, -(W.transpose(1, 2) @ dc[ac][:, :, None])[:, :, 0])
            dp = (Vinv @ bb[:, :, None])[:, :, 0]
            cams_n, points_n = cams.clone(), points.clone()
            cams_n[act_c] += dc
            points_n[act_p] += dp
            cand = 0.5 * (eager_linearize(points_n, cams_n, feats, pt, cam, jac=False) ** 2).sum()
            Jd = (Jc @ dc[ac][:, :, None] + Jp @ dp[ap][:, :, None])[:, :, 0]
            md = -(Jd * (r + 0.5 * Jd)).sum()
            cand, md = cand.item(), md.item()
            rho = (cur - cand) / md if md != 0 else float("nan")
            accept = np.isfinite(cand) and md > 0 and rho > 1e-3
        if accept:
            points.copy_(points_n)
            cams.copy_(cams_n)
            cur = cand
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            factor, succ = 2.0, succ + 1
        else:
            radius /= factor
            factor *= 2.0
    return cur


def eager_lists(prob, dev):
    pt, cam = prob["ptIdx"], prob["camIdx"]
    act_c, ac = np.unique(cam, return_inverse=True)
    act_p, ap = np.unique(pt, return_inverse=True)
    order = np.argsort(ap, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(ap))])
    pn = np.repeat(np.arange(len(ap)), (start[1:] - start[:-1])[ap])
    pm = order[np.concatenate([np.arange(start[q], start[q + 1]) for q in ap])]
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                 for x in (act_c, act_p, ac, ap, pn, pm))


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


def bench_solve(lib, dev, kw, replays, eager_calls):
    prob = synthetic.make_ba_problem(1, **kw)
    N, C, P = kw["n_obs"], kw["n_cams"], kw["n_points"]
    buf, A, Pa = tracker.build_index(prob["ptIdx"], prob["camIdx"], C, P)
    t = {k: torch.from_numpy(v).to(dev) for k, v in prob.items()}
    p0, c0 = t["points"].clone(), t["cam_pose"].clone()
    ix = torch.from_numpy(buf).to(dev)
    ws = torch.empty(lib.onepose_ba_workspace_bytes(N, A, Pa), dtype=torch.uint8, device=dev)
    info = torch.zeros(O.INFO_DOUBLES, dtype=torch.float64, device=dev)
    r, Jc, Jp = (torch.empty(N * k, dtype=torch.float64, device=dev) for k in (2, 12, 6))
    cost = torch.empty(1, dtype=torch.float64, device=dev)

    def solve():
        t["points"].copy_(p0)
        t["cam_pose"].copy_(c0)
        _lib.check(lib.onepose_ba_solve(
            t["points"].data_ptr(), t["cam_pose"].data_ptr(), t["features"].data_ptr(),
            t["ptIdx"].data_ptr(), t["camIdx"].data_ptr(), ix.data_ptr(), N, C, P, A, Pa, 5, 5,
            1e4, info.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))

    def linearize():
        _lib.check(lib.onepose_ba_linearize(
            p0.data_ptr(), c0.data_ptr(), t["features"].data_ptr(), t["ptIdx"].data_ptr(),
            t["camIdx"].data_ptr(), N, C, P, r.data_ptr(), Jc.data_ptr(), Jp.data_ptr(),
            cost.data_ptr(), _lib.stream_ptr(dev)))

    hip = graph_ms(solve, dev, replays)
    h = info.cpu().numpy()
    lin = graph_ms(linearize, dev, replays)
    lists = eager_lists(prob, dev)

    def eager():
        t["points"].copy_(p0)
        t["cam_pose"].copy_(c0)
        return eager_solve(t["points"], t["cam_pose"], t["features"], t["ptIdx"], t["camIdx"],
                           lists)

    for _ in range(3):
        final = eager()
    eg = median_ms(eager, eager_calls)
    elin = median_ms(lambda: eager_linearize(p0, c0, t["features"], t["ptIdx"], t["camIdx"]),
                     eager_calls)
    return {
        "n_obs": N, "n_cams": C, "n_points": P, "iterations": int(h[1]), "accepted": int(h[2]),
        "cost_initial": float(h[3]), "cost_final": float(h[4]), "eager_cost_final": float(final),
        "hip_graph_ms_median": hip[0], "hip_graph_ms_min_max": hip[1:],
        "eager_ms_median": eg[0], "eager_ms_min_max": eg[1:], "eager_over_hip": eg[0] / hip[0],
        "linearize_hip_graph_ms_median": lin[0], "linearize_eager_ms_median": elin[0],
        "workspace_bytes": int(ws.numel()), "index_bytes": int(ix.numel()),
    }


def bench_triangulate(lib, dev, n, replays):
    d = synthetic.make_triangulation_inputs(n, 3)
    P1 = torch.from_numpy(d["K1"] @ np.linalg.inv(d["Tcw1"])[:3]).to(dev)
    P2 = torch.from_numpy(d["K2"] @ np.linalg.inv(d["Tcw2"])[:3]).to(dev)
    a, b = torch.from_numpy(d["kpt2d_1"]).to(dev), torch.from_numpy(d["kpt2d_2"]).to(dev)
    out = {}

    def run():
        out.update(tracker.triangulate_points(P1, P2, a, b))

    tri = graph_ms(run, dev, replays)

    def eager():
        A = torch.stack([a[:, :1] * P1[2] - P1[0], a[:, 1:] * P1[2] - P1[1],
                         b[:, :1] * P2[2] - P2[0], b[:, 1:] * P2[2] - P2[1]], 1)
        h = torch.linalg.svd(A)[2][:, 3, :]
        return h[:, :3] / h[:, 3:]

    for _ in range(3):
        eager()
    eg = median_ms(eager, 20)
    return {"pairs": n, "hip_graph_ms_median": tri[0], "hip_graph_ms_min_max": tri[1:],
            "eager_svd_ms_median": eg[0], "kept": int(out["keep"].sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ba/bench.json")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--eager", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ba_bench needs a ROCm GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_name(dev), "replays": a.replays, "eager_calls": a.eager,
           "max_iters": 5, "initial_radius": 1e4, "shapes": {}}
    for name, kw in SHAPES:
        res["shapes"][name] = bench_solve(lib, dev, kw, a.replays, a.eager)
        print(name, json.dumps(res["shapes"][name]), flush=True)
    res["triangulate_1000"] = bench_triangulate(lib, dev, 1000, a.replays)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["triangulate_1000"]))


if __name__ == "__main__":
    main()

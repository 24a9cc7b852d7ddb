#!/usr/bin/env python
"""Time global bundle adjustment (onepose_gba_begin + onepose_gba_step), a first measurement,
against the same algorithm written in eager PyTorch-ROCm float64 (index_add_, batched small
solves, its decisions read on the host as eager code does), in the same process, and once
against the package's numpy host path, on

    100 cameras x 5 000 points x 10 views and 300 x 20 000 x 10 (tests/gba_cases.ring_problem:
    0.5 px noise, poses off by 0.5 degrees and 5 mm, points by 3 mm, gauge fixed).

HIP path: warm-up, then the median of `--replays` replays of a captured graph of begin + 50
steps at the Python layer's defaults (pcg_max_iters 100, pcg_tol 1e-6, function_tolerance 1e-6),
each between two events.  The solve moves its variables, so the graph begins with two device
copies that put the initial variables back; they are inside the timed window.  Recorded with it:
outer and CG iterations, the final costs of the three paths, a sweep of pcg_tol over 1e-1, 1e-3,
1e-6 and 1e-10, and the cost of the idle tail: the solve that stops after k iterations inside the
50-step graph against the same solve captured with k steps.  No target is set for these numbers
and nothing is tuned from them.

    python tools/gba_bench.py --out profiles/gba/bench.json
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import gba_cases as G  # noqa: E402
from onepose_amd import _lib, global_ba, tracker  # noqa: E402

SHAPES = [("c100_p5000_v10", dict(seed=7100, m=100, npts=5000, views=10)),
          ("c300_p20000_v10", dict(seed=7200, m=300, npts=20000, views=10))]
DEFAULTS = dict(max_iters=50, pcg_max_iters=100, pcg_tol=1e-6, function_tolerance=1e-6,
                radius=1e4)


# ------------------------------------------------------------------ eager formulation
def _skew(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], 1),
                        torch.stack([v[:, 2], z, -v[:, 0]], 1),
                        torch.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def eager_linearize(points, cams, K4, xy, pt, cam, fixbits=None, jac=True):
    """The cost function's theta > 0 branch (the bench scene has no zero rotation)."""
    X, w, t = points[pt], cams[cam, :3], cams[cam, 3:6]
    k = K4[cam]
    th2 = (w * w).sum(1)
    th = torch.sqrt(th2)
    c, s = torch.cos(th), torch.sin(th)
    a, b = s / th, (1.0 - c) / th2
    wx, wd = torch.linalg.cross(w, X), (w * X).sum(1)
    p = X * c[:, None] + wx * a[:, None] + w * (b * wd)[:, None] + t
    xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    r = torch.stack([k[:, 0] * xp + k[:, 2] - xy[:, 0], k[:, 1] * yp + k[:, 3] - xy[:, 1]], 1)
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
    D[:, 0, 0] = k[:, 0] * iz
    D[:, 0, 2] = -k[:, 0] * xp * iz
    D[:, 1, 1] = k[:, 1] * iz
    D[:, 1, 2] = -k[:, 1] * yp * iz
    Jc = torch.cat([D @ M, D], 2)
    if fixbits is not None:
        Jc = torch.where(fixbits[cam][:, None, :], torch.zeros_like(Jc), Jc)
    return r, Jc, D @ R


def eager_solve(points, cams, K4, xy, pt, cam, lists, fixbits, max_iters, pcg_max_iters, pcg_tol,
                function_tolerance, radius):
    """The header's algorithm on torch tensors (3 x 3 and 6 x 6 blocks through
    torch.linalg.cholesky / cholesky_solve) -> (final cost, outer iterations, CG iterations)."""
    act_c, act_p, ac, ap = lists
    A, Pa = len(act_c), len(act_p)
    f64 = dict(dtype=torch.float64, device=points.device)
    fix = fixbits[act_c]
    cur = 0.5 * (eager_linearize(points, cams, K4, xy, pt, cam, jac=False) ** 2).sum().item()
    factor, it, cg_total, lin = 2.0, 0, 0, None
    i6, i3 = torch.arange(6, device=points.device), torch.arange(3, device=points.device)
    while it < max_iters:
        if lin is None:
            lin = eager_linearize(points, cams, K4, xy, pt, cam, fixbits)
        r, Jc, Jp = lin
        mu = 1.0 / radius
        JcT, JpT = Jc.transpose(1, 2), Jp.transpose(1, 2)
        U = torch.zeros(A, 6, 6, **f64).index_add_(0, ac, JcT @ Jc)
        V = torch.zeros(Pa, 3, 3, **f64).index_add_(0, ap, JpT @ Jp)
        gc = torch.zeros(A, 6, **f64).index_add_(0, ac, (JcT @ r[:, :, None])[:, :, 0])
        gp = torch.zeros(Pa, 3, **f64).index_add_(0, ap, (JpT @ r[:, :, None])[:, :, 0])
        U[:, i6, i6] += mu * U[:, i6, i6].clamp(1e-6, 1e32)
        V[:, i3, i3] += mu * V[:, i3, i3].clamp(1e-6, 1e32)
        U[:, i6, i6] = torch.where(fix, torch.ones_like(U[:, i6, i6]), U[:, i6, i6])
        Lv = torch.linalg.cholesky(V)
        Y = torch.linalg.solve_triangular(Lv[ap], (JcT @ Jp).transpose(1, 2), upper=False)
        zp = torch.linalg.solve_triangular(Lv, gp[:, :, None], upper=False)
        Mb = U - torch.zeros(A, 6, 6, **f64).index_add_(0, ac, Y.transpose(1, 2) @ Y)
        C = torch.linalg.cholesky(Mb)
        rhs = (-gc).index_add_(0, ac, (Y.transpose(1, 2) @ zp[ap])[:, :, 0])

        def S(v):
            s = torch.zeros(Pa, 3, **f64).index_add_(0, ap, (JpT @ (Jc @ v[ac][:, :, None]))[:, :, 0])
            y = torch.cholesky_solve(s[:, :, None], Lv)
            acc = torch.zeros(A, 6, **f64).index_add_(0, ac, (JcT @ (Jp @ y[ap]))[:, :, 0])
            return (U @ v[:, :, None])[:, :, 0] - acc

        x = torch.zeros(A, 6, **f64)
        res = rhs.clone()
        z = torch.cholesky_solve(res[:, :, None], C)[:, :, 0]
        p = z.clone()
        rz0 = rz = (res * z).sum().item()
        k = 0
        while rz0 > 0 and np.isfinite(rz0):
            Sp = S(p)
            pSp = (p * Sp).sum().item()
            if not np.isfinite(pSp) or pSp <= 0:
                break
            k += 1
            alpha = rz / pSp
            x += alpha * p
            res -= alpha * Sp
            z = torch.cholesky_solve(res[:, :, None], C)[:, :, 0]
            rzn = (res * z).sum().item()
            p = z + (rzn / rz) * p
            rz = rzn
            if not np.isfinite(rz) or np.sqrt(rz / rz0) <= pcg_tol or k >= pcg_max_iters:
                break
        cg_total += k
        s = torch.zeros(Pa, 3, **f64).index_add_(0, ap, (JpT @ (Jc @ x[ac][:, :, None]))[:, :, 0])
        dp = torch.cholesky_solve((-gp - s)[:, :, None], Lv)[:, :, 0]
        cams_n, points_n = cams.clone(), points.clone()
        cams_n[act_c] += x
        points_n[act_p] += dp
        cand = 0.5 * (eager_linearize(points_n, cams_n, K4, xy, pt, cam, jac=False) ** 2).sum()
        Jd = (Jc @ x[ac][:, :, None] + Jp @ dp[ap][:, :, None])[:, :, 0]
        md = -(Jd * (r + 0.5 * Jd)).sum()
        cand, md = cand.item(), md.item()
        rho = (cur - cand) / md if md != 0 else float("nan")
        it += 1
        if np.isfinite(cand) and md > 0 and rho > 1e-3:
            converged = function_tolerance > 0 and abs(cur - cand) / cur <= function_tolerance
            points.copy_(points_n)
            cams.copy_(cams_n)
            cur, lin, factor = cand, None, 2.0
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e16)
            if converged:
                break
        else:
            radius /= factor
            factor *= 2.0
        if radius < 1e-32:
            break
    return cur, it, cg_total


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
        run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    t0 = time.perf_counter()
    with torch.cuda.graph(graph):
        run()
    capture_s = time.perf_counter() - t0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    return median_ms(graph.replay, replays), capture_s


def bench_shape(dev, kw, replays, eager_calls, sweep):
    prob = G.ring_problem(big_cam=False, lone_cam=False, idle=False, **kw)
    N, C, P = len(prob["ptIdx"]), len(prob["cam_pose"]), len(prob["points"])
    buf, A, Pa = tracker.build_index(prob["ptIdx"], prob["camIdx"], C, P)
    t = {k: torch.from_numpy(np.ascontiguousarray(prob[k])).to(dev) for k in G.KEYS}
    p0, c0 = t["points"].clone(), t["cam_pose"].clone()
    ix = torch.from_numpy(buf).to(dev)
    need = _lib.call("onepose_gba_workspace_bytes", n_obs=N, n_active_cams=A, n_active_points=Pa)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rows = DEFAULTS["max_iters"]
    info = torch.zeros(8 + 8 * rows, dtype=torch.float64, device=dev)
    common = dict(points=t["points"], cam_pose=t["cam_pose"], cam_K4=t["K4"], obs_xy=t["xy"],
                  ptIdx=t["ptIdx"], camIdx=t["camIdx"], cam_fixed=t["fixed"], index=ix, n_obs=N,
                  n_cams=C, n_points=P, n_active_cams=A, n_active_points=Pa, info=info,
                  info_rows=rows, workspace=ws, workspace_bytes=need)

    def solver(n_steps, pcg_tol):
        def run():
            t["points"].copy_(p0)
            t["cam_pose"].copy_(c0)
            s = _lib.stream_ptr(dev)
            _lib.run("onepose_gba_begin", initial_radius=DEFAULTS["radius"], stream=s, **common)
            _lib.run("onepose_gba_step", n_steps=n_steps, pcg_max_iters=DEFAULTS["pcg_max_iters"],
                     pcg_tol=pcg_tol, function_tolerance=DEFAULTS["function_tolerance"],
                     stream=s, **common)
        return run

    def head():
        h = info.cpu().numpy()
        return {"status": int(h[0]), "iterations": int(h[1]), "accepted": int(h[2]),
                "cost_initial": float(h[3]), "cost_final": float(h[4]),
                "cg_iterations": int(h[6])}

    out = {"n_obs": N, "n_cams": C, "n_points": P, "workspace_bytes": int(need),
           "index_bytes": int(ix.numel())}
    (med, lo, hi), cap = graph_ms(solver(DEFAULTS["max_iters"], DEFAULTS["pcg_tol"]), dev, replays)
    out["hip"] = dict(head(), graph_ms_median=med, graph_ms_min_max=[lo, hi], capture_s=cap)
    k = out["hip"]["iterations"]
    (med_k, lo_k, hi_k), _ = graph_ms(solver(k, DEFAULTS["pcg_tol"]), dev, replays)
    same = head()["cost_final"] == out["hip"]["cost_final"]
    out["idle_tail"] = {"steps_run": k, "graph_50_steps_ms": med, "graph_k_steps_ms": med_k,
                        "graph_k_steps_ms_min_max": [lo_k, hi_k], "same_bits": bool(same)}
    out["pcg_tol_sweep"] = {}
    for tol in sweep:
        (m, a, b), _ = graph_ms(solver(DEFAULTS["max_iters"], tol), dev, max(5, replays // 5))
        out["pcg_tol_sweep"][f"{tol:g}"] = dict(head(), graph_ms_median=m)
    # eager PyTorch, the same algorithm
    act_c, ac = (torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                 for x in np.unique(prob["camIdx"], return_inverse=True))
    act_p, ap = (torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                 for x in np.unique(prob["ptIdx"], return_inverse=True))
    fixbits = torch.from_numpy(global_ba.fixed_bits(prob["fixed"], C)).to(dev)
    res = {}

    def eager():
        t["points"].copy_(p0)
        t["cam_pose"].copy_(c0)
        res["v"] = eager_solve(t["points"], t["cam_pose"], t["K4"], t["xy"], t["ptIdx"],
                               t["camIdx"], (act_c, act_p, ac, ap), fixbits,
                               DEFAULTS["max_iters"], DEFAULTS["pcg_max_iters"],
                               DEFAULTS["pcg_tol"], DEFAULTS["function_tolerance"],
                               DEFAULTS["radius"])
    eager()
    eg = median_ms(eager, eager_calls)
    out["eager"] = {"ms_median": eg[0], "ms_min_max": eg[1:], "cost_final": res["v"][0],
                    "iterations": res["v"][1], "cg_iterations": res["v"][2]}
    out["eager_over_hip"] = eg[0] / med
    # the numpy host path, once
    t0 = time.perf_counter()
    _, _, hinfo = global_ba._host_solve(prob["points"], prob["cam_pose"], prob["K4"], prob["xy"],
                                        prob["ptIdx"], prob["camIdx"], prob["fixed"],
                                        DEFAULTS["max_iters"], DEFAULTS["function_tolerance"],
                                        DEFAULTS["pcg_tol"], DEFAULTS["pcg_max_iters"],
                                        DEFAULTS["radius"])
    out["host"] = {"seconds_once": time.perf_counter() - t0, "cost_final": float(hinfo[4]),
                   "iterations": int(hinfo[1]), "cg_iterations": int(hinfo[6])}
    ref = out["hip"]["cost_final"]
    out["same_cost"] = {"eager_rel": abs(out["eager"]["cost_final"] - ref) / ref,
                        "host_rel": abs(out["host"]["cost_final"] - ref) / ref}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gba/bench.json")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--eager", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(n for n, _ in SHAPES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gba_bench needs a ROCm GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    _lib.load()
    res = {"device": torch.cuda.get_device_name(dev), "replays": a.replays,
           "eager_calls": a.eager, "settings": DEFAULTS, "shapes": {}}
    for name, kw in SHAPES:
        if name not in a.shapes.split(","):
            continue
        res["shapes"][name] = bench_shape(dev, kw, a.replays, a.eager, (1e-1, 1e-3, 1e-6, 1e-10))
        print(name, json.dumps(res["shapes"][name]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

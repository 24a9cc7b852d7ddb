"""Records tests/golden/lk_edges.npz: per edge case of tests/lk_cases.py what lk.npz holds per
case (digest of the inputs, the numpy oracle's next_pts, status, end reasons and level count, the
digest of every pyramid level and derivative image), and for the cases of both dicts the per-level
trace counts and the largest window sum.  No image is stored.  Asserts what the two sets have to
cover (lk_cases.check_coverage) and prints the figures of the float64 model (tests/lk_model.py)
against the oracle, from which the bar in tests/test_lk_host.py was set.

    python tests/golden/make_golden_lk_edges.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lk_cases   # noqa: E402
import lk_oracle   # noqa: E402


def histogram(row):
    return {lk_oracle.REASONS[r]: int(c) for r, c in enumerate(row) if c}


def main():
    out, rec = {}, {}
    for name in list(lk_cases.CASES) + list(lk_cases.EDGE_CASES):
        s = lk_cases.scene(name)
        nxt, status, why, p, q = lk_cases.oracle(name)
        trace, max_ix2 = lk_cases.oracle_trace(name)
        rec[name] = dict(levels=len(p), status=status, reason=why, trace=trace, max_ix2=max_ix2)
        out[f"{name}_trace"] = trace.astype(np.int32)
        out[f"{name}_max_ix2"] = np.int64(max_ix2)
        if name in lk_cases.EDGE_CASES:
            out[f"{name}_sha"] = lk_cases.scene_sha(s)
            out[f"{name}_next_pts"] = nxt
            out[f"{name}_status"] = status
            out[f"{name}_reason"] = why.astype(np.int8)
            out[f"{name}_levels"] = len(p)
            out[f"{name}_pyr_sha"] = np.array([[lk_cases.sha(img), lk_cases.sha(der)]
                                               for pyr in (p, q) for img, der in pyr])
        print(f"{name}: win {s['win']}, {len(p)} level(s), status 1 on {int(status.sum())} of "
              f"{len(status)}, level 0 {histogram(trace[0, 0])}, above {histogram(trace[0, 1:].sum(0))}"
              f", above on kept points {histogram(trace[1, 1:].sum(0))}, largest window sum "
              f"{max_ix2:.3e} = {max_ix2 / 2 ** 31:.2f} x 2^31")
    lk_cases.check_coverage(rec)
    for name in lk_cases.MODEL_SCENES:
        o, m, pts = lk_cases.model_pair(name)
        cs = lk_cases.compared_set(name)
        d = np.abs(o[0] - m[0]).max(1)
        assert np.array_equal(o[1], m[1]), name
        assert name == "win21" or cs.mean() >= lk_cases.COMPARED_SHARE, (name, cs.mean())
        line = (f"model {name}: {len(pts)} points, status equal, compared set {int(cs.sum())} "
                f"({100 * cs.mean():.1f}%), max |oracle - model| there {d[cs].max():.5f} px, median "
                f"{np.median(d[cs]):.5f} px")
        if name in lk_cases.WARPS:
            inside = lk_cases.interior(name)
            truth = pts + lk_cases.warp_truth(name, pts)
            em, eo = (np.abs(x[0] - truth).max(1)[inside].max() for x in (m, o))
            line += (f"; against the analytic displacement on {int(inside.sum())} interior points: "
                     f"model {em:.4f} px, oracle {eo:.4f} px")
        print(line)
    path = os.path.join(HERE, "lk_edges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

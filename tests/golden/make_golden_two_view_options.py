"""Records tests/golden/two_view_options.npz: the plain-loop oracle (tests/two_view_oracle.py) on
the "options" family of tests/two_view_cases.option_calls(): refine_iters, max_error, confidence,
min_inlier_ratio, the max_points that move the inlier flags' LDS offset, and the given-F edges
(a NaN, an inf, all zeros, a pair below min_num_inliers).  The fields are two_view.npz's.
Stand-alone: the inputs come from seeds, the expectations from the oracle as it is.

    python tests/golden/make_golden_two_view_options.py

The F tolerance is measured as make_golden_two_view.py measures it: the oracle again with
numpy.linalg.eigh in place of both Jacobi eigen-solves; on the pairs where both runs give the
same mask, the largest entry-wise deviation of the normalised F is `f_dev`, and the tolerance is
16 x that with a floor of 1e-12.

What the calls are for is asserted here and recorded (`refine_pairs`): a pair whose F differs
between refine_iters 0 and 1, one whose F differs between 1 and 2, and one whose F at 2 equals its
F at 5 bit for bit because the refit after the second is not kept (its inlier count is smaller),
which ends the refits.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import two_view_cases as C   # noqa: E402
import two_view_oracle as O   # noqa: E402

OUT = os.path.join(HERE, "two_view_options.npz")


def run_call(call, variant=None):
    """The oracle on every pair of a call -> dict of arrays shaped like the library's outputs."""
    B, P = call["pts0"].shape[:2]
    out = {"F": np.zeros((B, 9)), "mask": np.zeros((B, P), np.uint8),
           "n_inliers": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32),
           "status": np.zeros(B, np.int32)}
    for b in range(B):
        n = int(call["n"][b])
        r = O.verify(call["pts0"][b, :n], call["pts1"][b, :n],
                     F_in=call["F_in"][b] if "F_in" in call else None, variant=variant,
                     **call["options"])
        out["F"][b] = r["F"]
        out["mask"][b, :n] = r["mask"]
        out["n_inliers"][b], out["iters"][b], out["status"][b] = r["n_inliers"], r["iters"], r["status"]
    return out


def next_refit_count(call, b, out):
    """The inlier count of the refit that would follow the returned model of pair b."""
    n = int(call["n"][b])
    Q = tuple(a.astype(np.float64) for a in (call["pts0"][b, :n, 0], call["pts0"][b, :n, 1],
                                             call["pts1"][b, :n, 0], call["pts1"][b, :n, 1]))
    P = tuple(a.tolist() for a in Q)
    F = O.solve(P, [i for i in range(n) if out["mask"][b, i]])
    return int(O.inliers(F, Q, call["options"]["max_error"] ** 2).sum())


def same_F(a, b, pair):
    return a["F"][pair].tobytes() == b["F"][pair].tobytes()


def record():
    calls = C.option_calls()
    rec, got, devs, same, models = {"calls": np.array(list(calls))}, {}, [], 0, 0
    for key, call in calls.items():
        got[key] = out = run_call(call)
        rec[f"{key}_sha"] = C.option_sha(call)
        rec[f"{key}_names"] = np.array(call["names"])
        for k, v in out.items():
            rec[f"{key}_{k}"] = v
        alt = None if "F_in" in call else run_call(call, variant="eigh")
        for b, name in enumerate(call["names"]):
            note = ""
            if alt is not None and out["status"][b] in (0, 3):
                models += 1
                agree = alt["status"][b] == out["status"][b] and np.array_equal(alt["mask"][b], out["mask"][b])
                if agree:
                    same += 1
                    devs.append(float(np.abs(O.normalised(out["F"][b]) - O.normalised(alt["F"][b])).max()))
                note = f"; eigh variant: {'same' if agree else 'another'} mask"
            print(f"{key}/{name}: status {out['status'][b]}, {out['n_inliers'][b]} of "
                  f"{call['n'][b]} inliers, {out['iters'][b]} iterations{note}")
    assert same >= 0.75 * models, f"eigh variant agrees on {same} of {models} pairs: choose other seeds"
    rec["f_dev"] = np.float64(max(devs))
    rec["f_tol"] = np.float64(max(16.0 * max(devs), 1e-12))
    rec["f_same"], rec["f_models"] = np.int32(same), np.int32(models)
    print(f"eigh variant: same mask on {same} of {models} pairs with a model, largest F deviation "
          f"{max(devs):.3e}, tolerance {rec['f_tol']:.3e}")

    # ---- what the calls are for ----
    r = {k: got[f"tight_refine{k}"] for k in C.REFINE_ITERS}
    call = calls["tight_refine2"]
    B = len(call["names"])
    d01 = [b for b in range(B) if not same_F(r[0], r[1], b)]
    d12 = [b for b in range(B) if not same_F(r[1], r[2], b)]
    ended = [b for b in range(B) if same_F(r[2], r[5], b)
             and next_refit_count(call, b, r[5]) < r[5]["n_inliers"][b]]
    assert d01 and d12 and ended, (d01, d12, ended)
    # of those, the pair on which the "refits_never_stop" variant gives another F at 5 refits
    never = [b for b in ended if O.verify(
        call["pts0"][b, :call["n"][b]], call["pts1"][b, :call["n"][b]], variant="refits_never_stop",
        **calls["tight_refine5"]["options"])["F"].tobytes() != r[5]["F"][b].tobytes()]
    assert never, "no pair separates the refits_never_stop variant: choose other seeds"
    rec["refine_pairs"] = np.array([d01[0], d12[0], never[0]], np.int32)
    print(f"refits_never_stop differs at refine_iters = 5 on pairs {never} of {ended}")
    print(f"tight_refine: F at 0 and 1 differ on pairs {d01}, at 1 and 2 on {d12}; F at 2 equals F "
          f"at 5 with the next refit not kept on {ended} "
          f"({[(next_refit_count(call, b, r[5]), int(r[5]['n_inliers'][b])) for b in ended]})")
    plain = {k: got[f"refine{k}"] for k in C.REFINE_ITERS}
    assert any(not same_F(plain[0], plain[1], b) for b in range(B))
    e0 = got["max_error0"]
    assert (e0["status"] == 2).all() and (e0["iters"] == 300).all() and not e0["F"].any()
    tight = np.concatenate([got["max_error0.5"]["status"], got["max_error1"]["status"]])
    assert (tight == 3).any() and (tight == 0).any(), tight
    assert (got["max_error16"]["status"] == 0).all()
    lo, hi = got["confidence0.5"]["iters"], got["confidence0.999999"]["iters"]
    assert lo[0] < 64 and hi[0] < 64 and (hi[1:] > 128).all() and (lo[1:] < hi[1:]).all(), (lo, hi)
    default = run_call(dict(calls["confidence0.5"], options=dict(C.DEFAULTS)))["iters"]
    assert (default[1:] != lo[1:]).all() and (default[1:] != hi[1:]).all(), (default, lo, hi)
    print(f"confidence: iterations {lo.tolist()} at 0.5, {default.tolist()} at the default, "
          f"{hi.tolist()} at 0.999999")
    for key, want in (("ratio0.8", [0, 3, 3]), ("ratio1", [0, 3, 3]), ("ratio-1", [0, 0, 0])):
        assert got[key]["status"].tolist() == want, (key, got[key]["status"])
        assert got[key]["F"].tobytes() == got["ratio-1"]["F"].tobytes()   # reported as for status 0
        assert np.array_equal(got[key]["mask"], got["ratio-1"]["mask"])
    for P, counts in C.LDS_MAX_POINTS.items():
        st = got[f"points{P}"]["status"]
        assert st.tolist() == [1 if c < 8 else 0 for c in counts], (P, st)
    g, call = got["given"], calls["given"]
    assert g["status"].tolist() == [3, 3, 3, 1, 1, 1, 1, 0] and not g["iters"].any()
    assert not g["mask"][:7].any() and g["F"].tobytes() == call["F_in"].tobytes()
    return rec


if __name__ == "__main__":
    rec = record()
    np.savez_compressed(OUT, **rec)
    print("wrote", os.path.relpath(OUT), os.path.getsize(OUT), "bytes")

"""Records tests/golden/two_view.npz: the plain-loop oracle (tests/two_view_oracle.py) on the GPU
test's batches (tests/two_view_cases.gpu_batches), so that the GPU test does not run the oracle;
tests/test_two_view_host.py checks that the file equals the oracle run afresh.

Also measured here, as DESIGN.md 8k quotes: the F tolerance.  The oracle is run a second time
with numpy.linalg.eigh in place of both of its Jacobi eigen-solves; on the pairs where both runs
give the same mask (at least three quarters of the pairs with a model, or the seeds are to be
changed) the largest entry-wise deviation between the two F, each scaled to unit Frobenius norm
with its largest entry positive, is `f_dev`; the tolerance is 16 x that with a floor of 1e-12.

    python tests/golden/make_golden_two_view.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import two_view_cases as C   # noqa: E402
import two_view_oracle as O   # noqa: E402


def run_batch(batch, variant=None, F_in=None):
    """The oracle on every pair of a batch -> dict of arrays shaped like the library's outputs."""
    B, P = batch["pts0"].shape[:2]
    out = {"F": np.zeros((B, 9)), "mask": np.zeros((B, P), np.uint8),
           "n_inliers": np.zeros(B, np.int32), "iters": np.zeros(B, np.int32),
           "status": np.zeros(B, np.int32)}
    for b in range(B):
        n = int(batch["n"][b])
        r = O.verify(batch["pts0"][b, :n], batch["pts1"][b, :n],
                     F_in=None if F_in is None else F_in[b], variant=variant, **batch["options"])
        out["F"][b] = r["F"]
        out["mask"][b, :n] = r["mask"]
        out["n_inliers"][b], out["iters"][b], out["status"][b] = r["n_inliers"], r["iters"], r["status"]
    return out


def record(max_points):
    batches = C.gpu_batches(max_points)
    rec = {"max_points": np.int32(max_points)}
    devs, same, models = [], 0, 0
    for key, batch in batches.items():
        got = run_batch(batch)
        alt = run_batch(batch, variant="eigh")
        given = run_batch(batch, F_in=got["F"])
        rec[f"{key}_sha"] = C.sha(batch["pts0"], batch["pts1"], batch["counts"])
        rec[f"{key}_names"] = np.array(batch["names"])
        for k, v in got.items():
            rec[f"{key}_{k}"] = v
        rec[f"{key}_given_mask"] = given["mask"]
        rec[f"{key}_given_status"] = given["status"]
        for b, name in enumerate(batch["names"]):
            if got["status"][b] in (1, 2):
                continue
            models += 1
            if alt["status"][b] == got["status"][b] and np.array_equal(alt["mask"][b], got["mask"][b]):
                same += 1
                devs.append(float(np.abs(O.normalised(got["F"][b]) - O.normalised(alt["F"][b])).max()))
            print(f"{key}/{name}: status {got['status'][b]}, {got['n_inliers'][b]} of "
                  f"{batch['n'][b]} inliers, {got['iters'][b]} iterations; eigh variant: "
                  f"{'same mask' if devs and alt['status'][b] == got['status'][b] and np.array_equal(alt['mask'][b], got['mask'][b]) else 'another mask'}")
    assert same >= 0.75 * models, f"eigh variant agrees on {same} of {models} pairs: choose other seeds"
    rec["f_dev"] = np.float64(max(devs))
    rec["f_tol"] = np.float64(max(16.0 * max(devs), 1e-12))
    rec["f_same"], rec["f_models"] = np.int32(same), np.int32(models)
    print(f"eigh variant: same mask on {same} of {models} pairs with a model, largest F deviation "
          f"{max(devs):.3e}, tolerance {rec['f_tol']:.3e}")
    return rec


if __name__ == "__main__":
    from onepose_amd import _lib
    _lib.load()
    rec = record(int(_lib.call("onepose_two_view_max_points")))
    np.savez_compressed(os.path.join(HERE, "two_view.npz"), **rec)

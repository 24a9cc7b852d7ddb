"""Records tests/golden/lk.npz: per case of tests/lk_cases.py the digest of the inputs, the
numpy oracle's next_pts, status, end reasons and level count, and the digest of every pyramid
level and derivative image of both images.  Asserts what the set has to cover.

    python tests/golden/make_golden_lk.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lk_cases   # noqa: E402
import lk_oracle   # noqa: E402


def main():
    out = {}
    seen = np.zeros(len(lk_oracle.REASONS), dtype=np.int64)
    for name in lk_cases.CASES:
        s = lk_cases.scene(name)
        nxt, status, why, p, q = lk_cases.oracle(name)
        out[f"{name}_sha"] = lk_cases.scene_sha(s)
        out[f"{name}_next_pts"] = nxt
        out[f"{name}_status"] = status
        out[f"{name}_reason"] = why.astype(np.int8)
        out[f"{name}_levels"] = len(p)
        out[f"{name}_pyr_sha"] = np.array([[lk_cases.sha(img), lk_cases.sha(der)]
                                           for pyr in (p, q) for img, der in pyr])
        seen += np.bincount(why, minlength=len(seen))
        assert 2 * int(status.sum()) >= len(status), (name, int(status.sum()))
        print(f"{name}: {len(p)} level(s), status 1 on {int(status.sum())} of {len(status)}, "
              f"reasons {dict(zip(lk_oracle.REASONS, np.bincount(why, minlength=len(seen))))}")
    for r in (lk_oracle.R_EPS, lk_oracle.R_OSC, lk_oracle.R_CAP, lk_oracle.R_OOB_PRE,
              lk_oracle.R_OOB_LOOP, lk_oracle.R_EIG):
        assert seen[r] > 0, f"no point ends with reason {lk_oracle.REASONS[r]}"
    path = os.path.join(HERE, "lk.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Generate the object builder's second fixture by running the REFERENCE itself.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_object_builder_edges.py

What is imported from the reference (read-only, nothing copied), through
make_golden_object_builder.import_reference():
  * src.sfm.postprocess.filter_points.merge
  * src.sfm.postprocess.feature_process.mean_descriptors

Written: tests/golden/object_builder_edges.npz, arrays and digests only:
  * merge_<name>_{sha, points, lens, ids} for the long-cluster cases (C.LONG_MERGE_CASES): the
    reference's merge output on clusters of 63 .. 200 distinct members;
  * lift_<n3>_<dim>_{in_sha, ref_sha} for C.LIFT_ALL: digests of the regenerated inputs and of the
    reference's mean_descriptors on the collected array of each wide-exponent lifting case;
  * blind_* / wide_*: how many points a reversed and a pairwise (np.sum) mean change on the old
    randn banks (none) and on the wide bank (most);
  * lift_2500_1_oracle_sha: the sequential mean at dim 1, which the reference does NOT give.

The generator fails unless
  * O.merge equals the reference's merge on every bit of the long cases;
  * in the float32 long case the mean in reversed member order differs from the reference for every
    long cluster, and the mean by 64-wide partial sums differs for every long cluster of more
    than 65 members (up to 65 the partial sums ARE the sequential sum: the second partial has at
    most one addend);
  * the 66-entry row of the "skip" group exists and its extra point is lost;
  * O.lift's mean64 has the reference's digest at every dim >= 2, and not at dim 1 (numpy sums a
    contiguous [k, 1] block pairwise);
  * on the wide bank at dim 256 the reversed and the pairwise mean each differ from the oracle on
    at least a quarter of the points, and on the randn banks on none.
The file is written with fixed zip timestamps, so two runs give identical bytes.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_object_builder import C, O, import_reference  # noqa: E402


def long_merge_fixture(fp_mod, name, out):
    xyz, ids, thr, groups = C.long_merge_case(name)
    pts, ret = fp_mod.merge(xyz, ids, dist_threshold=thr)
    lens, flat = C.flatten_clusters(ret)
    opts, oret = O.merge(xyz, ids, thr)
    olens, oflat = C.flatten_clusters(oret)
    assert np.array_equal(olens, lens) and np.array_equal(oflat, flat), f"{name}: clusters differ"
    assert opts.dtype == pts.dtype and opts.tobytes() == pts.tobytes(), f"{name}: means differ"
    # every long cluster came out whole, in ascending member order
    start = np.concatenate([[0], np.cumsum(lens)])
    first = {int(flat[start[c]]): c for c in range(len(lens))}
    rows = C.long_rows(groups)
    for key, r in rows.items():
        c = first[int(ids[r[0]])]
        assert np.array_equal(flat[start[c]:start[c + 1]], ids[r]), f"{name}: {key} is not whole"
        assert len(np.unique(xyz[r], axis=0)) == len(r), f"{name}: {key} has equal members"
        ref = pts[c]
        assert C.mean_in_order(xyz, r).tobytes() == ref.tobytes()
        if xyz.dtype == np.float32:
            assert (C.mean_in_order(xyz, r[::-1]) != ref).any(), f"{name}: {key} reversed is blind"
            if len(r) > 65:
                assert (C.mean_in_order(xyz, r, 64) != ref).any(), f"{name}: {key} partial is blind"
    assert sorted(len(r) for r in rows.values()) == sorted(C.LONG_SIZES + (65,))
    lost = groups["skip"][0][65]
    assert ids[lost] not in set(flat.tolist()), f"{name}: the point behind the 66-entry row is kept"
    rs, _ = O.radius_neighbours(xyz, thr)
    last = groups["skip"][0][64]
    assert rs[last + 1] - rs[last] == 66
    out[f"merge_{name}_sha"] = C.sha(xyz, ids)
    out[f"merge_{name}_points"] = pts
    out[f"merge_{name}_lens"] = lens
    out[f"merge_{name}_ids"] = flat
    print(f"merge {name}: {len(xyz)} points -> {len(lens)} clusters, largest {int(lens.max())}")


def changed_points(a, b):
    return int((a != b).any(axis=0).sum())


def lifting_fixture(fproc, out):
    for n3, dim in C.LIFT_ALL:
        args = C.lift_inputs(n3, dim)
        seg = args[5]
        _, collected, mean64, _ = O.lift(*args, dim)
        ref = fproc.mean_descriptors(np.ascontiguousarray(collected.T), seg.astype(np.int64))
        assert ref.dtype == np.float64 and ref.shape == (n3, dim)
        ref_sha, oracle_sha = C.sha(np.ascontiguousarray(ref.T)), C.sha(mean64)
        if dim >= 2:
            assert ref_sha == oracle_sha, f"lift {n3} x {dim}: the oracle is not the reference"
        else:
            assert ref_sha != oracle_sha, f"lift {n3} x 1: the reference sums sequentially after all"
            out[f"lift_{n3}_{dim}_oracle_sha"] = oracle_sha
        out[f"lift_{n3}_{dim}_in_sha"] = C.sha(*args)
        out[f"lift_{n3}_{dim}_ref_sha"] = ref_sha
        if (n3, dim) == (2500, 256):
            rev = changed_points(C.segment_means(collected, seg, "reversed"), mean64)
            pw = changed_points(C.segment_means(collected, seg, "pairwise"), mean64)
            assert rev >= n3 // 4 and pw >= n3 // 4, (rev, pw)
            out["wide_reversed_changed"], out["wide_pairwise_changed"] = np.int64(rev), np.int64(pw)
            print(f"wide bank, 2500 x 256: reversed changes {rev} points, pairwise {pw}")
    # the old inputs were blind: the first suite's case, and the new structure on a randn bank
    blind = []
    for args, dim in ((C.lift_inputs_old(256), 256), (C.lift_inputs(2500, 256, wide=False), 256)):
        _, collected, mean64, _ = O.lift(*args, dim)
        ref = fproc.mean_descriptors(np.ascontiguousarray(collected.T), args[5].astype(np.int64))
        assert np.ascontiguousarray(ref.T).tobytes() == mean64.tobytes()
        for how in ("reversed", "pairwise"):
            blind.append(changed_points(C.segment_means(collected, args[5], how), mean64))
    assert blind == [0, 0, 0, 0], blind
    out["blind_old_case_changed"] = np.asarray(blind[:2], dtype=np.int64)
    out["blind_randn_2500_changed"] = np.asarray(blind[2:], dtype=np.int64)
    print("randn banks: reversed and pairwise change no point")


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps and key order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)),
                       buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main():
    fpts, _, fproc, _ = import_reference()
    out = {}
    for name in C.LONG_MERGE_CASES:
        long_merge_fixture(fpts, name, out)
    lifting_fixture(fproc, out)
    path = os.path.join(HERE, "object_builder_edges.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    assert size < 100_000, size
    print("object_builder_edges.npz", size, "bytes")


if __name__ == "__main__":
    main()

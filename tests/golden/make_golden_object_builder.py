"""Generate the object builder's fixtures by running the REFERENCE itself.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_object_builder.py

What is imported from the reference (read-only, nothing copied):
  * src.utils.colmap.read_write_model        (write_model, read_model, the record types)
  * src.sfm.postprocess.filter_tkl           (get_tkl)
  * src.sfm.postprocess.filter_points        (filter_by_track_length, filter_by_3d_box,
                                              filter_3d, merge)
  * src.sfm.postprocess.feature_process      (id_mapping, count_features, gather_3d_ann,
                                              mean_descriptors, mean_scores, save_3d_anno)
Their unrelated top-level imports (cv2, h5py, matplotlib) are satisfied by empty placeholder
modules for the duration of the import.

Written: tests/golden/object_builder_model/{points3D,images,cameras}.bin and
box3d_corners.txt (a small synthetic model, through the reference's write_model: data), and
tests/golden/object_builder.npz with the reference's output of every stage plus digests of the
inputs, which tests/object_builder_cases.py regenerates from seeds.

The generator fails unless the fixtures hold what the tests are there to see: a cluster of >= 3
points, a chain seeded at its end that loses a point, a chain seeded at its middle that loses
none, >= 4 pairs whose distance as the reference computes it is the threshold or one of its two
float64 neighbours, a box margin of >= 1e-6 for every point and axis, and >= 2 points of exactly
the chosen track length.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)

import object_builder_cases as C  # noqa: E402
import object_builder_oracle as O  # noqa: E402


def import_reference():
    added = []
    for name in ("cv2", "h5py", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            added.append(name)
    if "matplotlib" in added:
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    try:
        from src.sfm.postprocess import feature_process, filter_points, filter_tkl
        from src.utils.colmap import read_write_model
    finally:
        for name in added:
            del sys.modules[name]
    return filter_points, filter_tkl, feature_process, read_write_model


def write_fixture_model(rw, spec):
    os.makedirs(C.MODEL_DIR, exist_ok=True)
    cameras = {1: rw.Camera(id=1, model="PINHOLE", width=640, height=480,
                            params=np.array([500.0, 500.0, 320.0, 240.0]))}
    images = {}
    for k, name in enumerate(C.IMG_LISTS):
        images[k + 1] = rw.Image(id=k + 1, qvec=np.array([1.0, 0.0, 0.0, 0.0]),
                                 tvec=np.array([0.0, 0.0, 0.5 + 0.01 * k]), camera_id=1, name=name,
                                 xys=spec["xys"][k], point3D_ids=spec["point3D_ids"][k])
    points = {}
    for r in spec["file_order"]:
        tr = spec["tracks"][r]
        points[int(spec["ids"][r])] = rw.Point3D(
            id=int(spec["ids"][r]), xyz=spec["xyz"][r], rgb=np.array([128, 128, 128]), error=0.5,
            image_ids=np.array([k + 1 for k, _ in tr]), point2D_idxs=np.array([s for _, s in tr]))
    rw.write_model(cameras, images, points, C.MODEL_DIR, ext=".bin")
    np.savetxt(os.path.join(C.MODEL_DIR, "box3d_corners.txt"), spec["corners"])


def merge_fixture(fp_mod, name, out):
    from scipy.spatial.distance import pdist, squareform
    xyz, ids, thr, groups = C.merge_case(name)
    pts, ret = fp_mod.merge(xyz, ids, dist_threshold=thr)
    lens, flat = C.flatten_clusters(ret)
    kept = set(flat.tolist())
    assert lens.max() >= 3, "no cluster of >= 3 points"
    a, b, c = groups["chain_end"][0]
    assert ids[a] in kept and ids[b] in kept and ids[c] not in kept, "the end-seeded chain keeps c"
    assert all(ids[r] in kept for r in groups["chain_mid"][0]), "the middle-seeded chain lost one"
    d = squareform(pdist(xyz, "euclidean"))
    near = {np.nextafter(thr, 0.0), thr, np.nextafter(thr, 1.0)}
    edge = [(p, q) for p, q in groups.get("edge", []) if d[p, q] in near]
    assert len(edge) >= 4 or "edge" not in groups, f"{name}: {len(edge)} threshold-edge pairs"
    out[f"merge_{name}_sha"] = C.sha(xyz, ids)
    out[f"merge_{name}_points"] = pts
    out[f"merge_{name}_lens"] = lens
    out[f"merge_{name}_ids"] = flat
    out[f"merge_{name}_edge_below"] = np.asarray([bool(d[p, q] < thr) for p, q in edge])
    out[f"merge_{name}_edge_pairs"] = np.asarray(edge, dtype=np.int64).reshape(-1, 2)
    # the restated oracle must already agree before anything is committed
    opts, oret = O.merge(xyz, ids, thr)
    olens, oflat = C.flatten_clusters(oret)
    assert np.array_equal(olens, lens) and np.array_equal(oflat, flat)
    assert opts.tobytes() == pts.tobytes()
    print(f"merge {name}: {len(xyz)} points -> {len(lens)} clusters, {len(xyz) - len(flat)} dropped,"
          f" {len(edge)} edge pairs ({int(out[f'merge_{name}_edge_below'].sum())} below)")


def main():
    fpts, ftkl, fproc, rw = import_reference()
    spec = C.model_spec()
    write_fixture_model(rw, spec)
    out = {}
    box_path = os.path.join(C.MODEL_DIR, "box3d_corners.txt")
    corners = np.loadtxt(box_path)
    out["box_margin"] = np.float64(O.box_margin(spec["xyz"], corners))
    assert out["box_margin"] >= C.MARGIN, out["box_margin"]

    # run.py:220-249 stage by stage
    tkl, count_list = ftkl.get_tkl(C.MODEL_DIR, thres=C.MAX_KP3D, show=False)
    assert int(np.sum(np.asarray(count_list) == tkl)) >= 2, "fewer than 2 points of the chosen length"
    out["tkl"] = np.asarray(tkl)
    out["points_count_list"] = np.asarray(count_list)
    _, images, points3D = rw.read_model(C.MODEL_DIR, ext=".bin")
    x_tl, i_tl = fpts.filter_by_track_length(points3D, tkl)
    out["tl_xyzs"], out["tl_idxs"] = x_tl, i_tl
    x_box, i_box = fpts.filter_by_3d_box(x_tl, i_tl, box_path)
    out["box_xyzs"], out["box_idxs"] = x_box.numpy(), np.asarray(i_box)
    x3, i3 = fpts.filter_3d(C.MODEL_DIR, tkl, box_path)
    assert np.array_equal(x3.numpy(), out["box_xyzs"]) and np.array_equal(i3, out["box_idxs"])
    assert 0 < len(i_box) < len(i_tl) < len(points3D)
    m_xyz, m_idx = fpts.merge(x3, i3, dist_threshold=C.THR)
    out["merge_points"] = m_xyz
    out["merge_lens"], out["merge_ids"] = C.flatten_clusters(m_idx)
    assert out["merge_lens"].max() >= 3

    counts = [len(v) for v in spec["point3D_ids"]]
    feats = C.features(counts)
    out["feature_counts"] = np.asarray(counts)
    out["features_sha"] = C.features_sha(feats)
    mapping = fproc.id_mapping(m_idx)
    dim, pos, feat, score, image, _ = fproc.count_features(C.IMG_LISTS, feats, images, mapping)
    f_xyz, f_desc, f_score, idxs = fproc.gather_3d_ann(pos, feat, score, image, m_xyz, m_idx, dim)
    avg_d, avg_s = fproc.mean_descriptors(f_desc, idxs), fproc.mean_scores(f_score, idxs)
    with tempfile.TemporaryDirectory() as tmp:
        fproc.save_3d_anno(f_xyz, avg_d, avg_s, os.path.join(tmp, "anno_3d_average.npz"))
        fproc.save_3d_anno(f_xyz, f_desc, f_score, os.path.join(tmp, "anno_3d_collect.npz"))
        np.save(os.path.join(tmp, "idxs.npy"), idxs)
        for f in ("anno_3d_average", "anno_3d_collect"):
            z = np.load(os.path.join(tmp, f + ".npz"))
            for k in z.files:
                out[f"{f}_{k}"] = z[k]
        out["idxs"] = np.load(os.path.join(tmp, "idxs.npy"))
    # the collected descriptors are float32 values in a float64 array: stored as float32 (exact)
    # with the digest and dtype of the array the reference wrote
    cd = out.pop("anno_3d_collect_descriptors3d")
    assert np.array_equal(cd.astype(np.float32).astype(np.float64), cd)
    out["anno_3d_collect_descriptors3d_f32"] = cd.astype(np.float32)
    out["anno_3d_collect_descriptors3d_dtype"] = str(cd.dtype)
    out["anno_3d_collect_descriptors3d_sha"] = C.sha(cd)
    assert int(idxs.max()) > 8 > int(idxs.min()), "leaves need points of fewer and more than 8"
    print(f"model: {len(points3D)} points, tkl {tkl}, {len(i_tl)} by track, {len(i_box)} in the box,"
          f" {len(out['merge_lens'])} merged, {int(idxs.sum())} observations, margin"
          f" {float(out['box_margin']):.3g}")

    for name in C.MERGE_CASES:
        merge_fixture(fpts, name, out)
    np.savez_compressed(os.path.join(HERE, "object_builder.npz"), **out)
    total = sum(os.path.getsize(os.path.join(C.MODEL_DIR, f)) for f in os.listdir(C.MODEL_DIR))
    print("object_builder.npz", os.path.getsize(os.path.join(HERE, "object_builder.npz")),
          "bytes; model", total, "bytes")


if __name__ == "__main__":
    main()

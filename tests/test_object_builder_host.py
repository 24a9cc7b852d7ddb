"""The object builder without a GPU: the COLMAP readers against the fixture model, and the numpy
oracle (tests/object_builder_oracle.py) and the device=None path of every
onepose_amd.object_builder function against the outputs the reference itself produced on that
model (tests/golden/object_builder.npz, written by make_golden_object_builder.py): dtype, shape
and every bit.  Then the checks the C entry points make before anything is launched."""
import os
import struct

import numpy as np
import pytest
import torch

import object_builder_cases as C
import object_builder_oracle as O
from conftest import golden
from onepose_amd import _lib, object_builder as ob


def same(a, ref):
    a, ref = np.asarray(a), np.asarray(ref)
    return a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes()


@pytest.fixture(scope="module")
def g():
    return golden("object_builder")


@pytest.fixture(scope="module")
def model():
    return (ob.read_points3d_binary(os.path.join(C.MODEL_DIR, "points3D.bin")),
            ob.read_images_binary(os.path.join(C.MODEL_DIR, "images.bin")))


@pytest.fixture(scope="module")
def feats(g):
    f = C.features(g["feature_counts"].tolist())
    assert C.features_sha(f) == str(g["features_sha"]), "synthetic features changed"
    return f


BOX = os.path.join(C.MODEL_DIR, "box3d_corners.txt")


def test_readers_recover_the_model(model):
    pts, imgs = model
    spec = C.model_spec()
    assert pts["ids"].dtype == np.int64 and np.array_equal(pts["ids"], spec["ids"])
    assert pts["xyz"].dtype == np.float64 and pts["xyz"].tobytes() == spec["xyz"].tobytes()
    assert np.array_equal(pts["track_len"], [len(t) for t in spec["tracks"]])
    # the file is not in id order; file_order says where each of its points went
    assert np.array_equal(pts["file_order"], spec["file_order"])
    assert not np.array_equal(spec["file_order"], np.arange(len(spec["ids"])))
    assert imgs["names"] == C.IMG_LISTS
    assert np.array_equal(imgs["image_ids"], np.arange(1, C.N_IMAGES + 1))
    for got, want in zip(imgs["point3D_ids"], spec["point3D_ids"]):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(np.loadtxt(BOX), spec["corners"])


def test_readers_refuse_a_truncated_file(tmp_path):
    for name, reader in (("points3D.bin", ob.read_points3d_binary),
                         ("images.bin", ob.read_images_binary)):
        raw = open(os.path.join(C.MODEL_DIR, name), "rb").read()
        p = tmp_path / name
        p.write_bytes(raw[:-5])
        with pytest.raises((ValueError, struct.error)):
            reader(str(p))


def test_get_tkl(g, model):
    tkl, counts = ob.get_tkl(model[0], C.MAX_KP3D)
    assert same(np.asarray(tkl), g["tkl"])
    assert isinstance(counts, list) and same(np.asarray(counts), g["points_count_list"])
    tkl2, _ = ob.get_tkl(C.MODEL_DIR, C.MAX_KP3D)          # a model directory, as the reference
    assert tkl2 == tkl
    tl = model[0]["track_len"]
    assert (tl == tkl).sum() >= 2
    # the quirk: points of exactly the chosen length survive, so more than thres may pass
    assert (tl > tkl).sum() <= C.MAX_KP3D < (tl >= tkl).sum()
    with pytest.raises(ValueError):
        ob.get_tkl(model[0], -1)


def test_filters(g, model):
    pts = model[0]
    tkl = int(g["tkl"])
    x, i = ob.filter_by_track_length(pts, tkl)
    assert same(x, g["tl_xyzs"]) and same(i, g["tl_idxs"])
    xb, ib = ob.filter_by_3d_box(x, i, BOX)
    assert isinstance(xb, torch.Tensor) and same(xb.numpy(), g["box_xyzs"]) and same(ib, g["box_idxs"])
    x3, i3 = ob.filter_3d(C.MODEL_DIR, tkl, np.loadtxt(BOX))     # corners as an array
    assert same(x3.numpy(), g["box_xyzs"]) and same(i3, g["box_idxs"])
    # the oracle's compaction, and the margin that makes the comparison with torch.matmul fair
    ox, oi = O.filter_points(pts["xyz"], pts["track_len"], tkl, np.loadtxt(BOX))
    assert same(ox, g["box_xyzs"]) and np.array_equal(pts["ids"][oi], g["box_idxs"])
    assert O.box_margin(pts["xyz"], np.loadtxt(BOX)) == float(g["box_margin"]) >= C.MARGIN


def test_box_faces_and_nan_are_outside():
    corners = np.array([[0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1],
                        [0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], dtype=np.float64)
    p = np.array([[0.5, 0.5, 0.5], [0.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.5, 0.0, 0.5],
                  [0.5, 0.5, 1.0], [np.nan, 0.5, 0.5], [0.25, 0.75, 0.125]])
    for fn in (lambda: ob.filter_by_3d_box(p, np.arange(7), corners)[1],
               lambda: O.filter_points(p, None, 0, corners)[1]):
        assert fn().tolist() == [0, 6]


@pytest.mark.parametrize("name", list(C.MERGE_CASES))
def test_merge_cases(g, name):
    xyz, ids, thr, groups = C.merge_case(name)
    assert C.sha(xyz, ids) == str(g[f"merge_{name}_sha"]), "synthetic inputs changed"
    for fn in (lambda: ob.merge(xyz, ids, thr), lambda: O.merge(xyz, ids, thr)):
        pts, ret = fn()
        lens, flat = C.flatten_clusters(ret)
        assert same(pts, g[f"merge_{name}_points"])
        assert same(lens, g[f"merge_{name}_lens"]) and same(flat, g[f"merge_{name}_ids"])
    # what the fixture was built to show, as the reference decided it
    kept = set(g[f"merge_{name}_ids"].tolist())
    a, b, c = groups["chain_end"][0]
    assert ids[a] in kept and ids[b] in kept and ids[c] not in kept
    assert all(ids[r] in kept for r in groups["chain_mid"][0])
    assert g[f"merge_{name}_lens"].max() >= 3
    cluster_of = {}
    pos = 0
    for cl, n in enumerate(g[f"merge_{name}_lens"]):
        for v in g[f"merge_{name}_ids"][pos:pos + n]:
            cluster_of[int(v)] = cl
        pos += n
    pairs, below = g[f"merge_{name}_edge_pairs"], g[f"merge_{name}_edge_below"]
    assert len(pairs) >= 4 or name == "f32"
    for (p, q), lt in zip(pairs, below):   # a pair at the threshold merges iff the reference says so
        merged = cluster_of.get(int(ids[p]), -1) == cluster_of.get(int(ids[q]), -2)
        assert merged == bool(lt)


def test_merge_in_the_flow_is_float32(g):
    x = torch.from_numpy(g["box_xyzs"])          # filter_by_3d_box hands over a float32 tensor
    for fn in (lambda: ob.merge(x, g["box_idxs"], C.THR),
               lambda: O.merge(g["box_xyzs"], g["box_idxs"], C.THR)):
        pts, ret = fn()
        lens, flat = C.flatten_clusters(ret)
        assert same(pts, g["merge_points"])
        assert same(lens, g["merge_lens"]) and same(flat, g["merge_ids"])
    assert all(v.dtype == np.int64 for v in ob.merge(x, g["box_idxs"], C.THR)[1].values())


def clusters(g):
    out, pos = {}, 0
    for c, n in enumerate(g["merge_lens"]):
        out[c] = g["merge_ids"][pos:pos + n]
        pos += n
    return out


def test_collect_order_and_lifting(g, model, feats):
    oi, of, idxs = ob.collect_observations(model[1], C.IMG_LISTS, clusters(g))
    assert same(idxs, g["idxs"])
    assert oi.dtype == np.int32 and of.dtype == np.int32
    desc = [feats[n]["descriptors"] for n in C.IMG_LISTS]
    want = g["anno_3d_collect_descriptors3d_f32"].astype(str(g["anno_3d_collect_descriptors3d_dtype"]))
    assert C.sha(want) == str(g["anno_3d_collect_descriptors3d_sha"])
    col, m64, m32 = ob.lift_descriptors(desc, oi, of, idxs)
    assert same(col, want) and same(m64, g["anno_3d_average_descriptors3d"])
    assert same(m32, g["anno_3d_average_descriptors3d"].astype(np.float32))
    # a point seen twice in one image contributes both features, in ascending feature order
    spec = C.model_spec()
    track = spec["tracks"][spec["groups"]["triple"][0][0]]
    (k,) = {k for k, _ in track if sum(1 for kk, _ in track if kk == k) == 2}
    slots = sorted(s for kk, s in track if kk == k)
    at = [o for o in range(len(oi)) if oi[o] == k and of[o] in slots]
    assert at == [at[0], at[0] + 1] and [int(of[o]) for o in at] == slots
    # the oracle's formulation of the kernel's inputs
    ncols = np.asarray([d.shape[1] for d in desc])
    off = np.concatenate([[0], np.cumsum(ncols[:-1] * C.DIM)])
    bank = np.concatenate([d.reshape(-1) for d in desc])
    ss, ocol, o64, o32 = O.lift(bank, off, ncols, oi, of, idxs, C.DIM)
    assert same(ocol, want) and same(o64, m64) and same(o32, m32)
    assert ss[-1] == len(oi)


def test_missing_observation_is_a_key_error(g, model):
    cl = clusters(g)
    with pytest.raises(KeyError):
        ob.collect_observations(model[1], C.IMG_LISTS[:1], cl)       # most points are not in image 0
    with pytest.raises(KeyError):
        ob.collect_observations(model[1], C.IMG_LISTS + ["seq/color/none.png"], cl)
    cl[len(cl)] = np.array([999999])                                # an id no image observes
    with pytest.raises(KeyError) as e:
        ob.collect_observations(model[1], C.IMG_LISTS, cl)
    assert e.value.args[0] == 999999


def test_written_files(g, model, feats, tmp_path):
    out = str(tmp_path / "anno")
    ob.build_annotations(C.MODEL_DIR, feats, C.IMG_LISTS, BOX, out, max_num_kp3d=C.MAX_KP3D,
                         dist_threshold=C.THR)
    assert sorted(os.listdir(out)) == ["anno_3d_average.npz", "anno_3d_collect.npz", "idxs.npy"]
    for f in ("anno_3d_average", "anno_3d_collect"):
        z = np.load(os.path.join(out, f + ".npz"))
        assert sorted(z.files) == ["descriptors3d", "keypoints3d", "scores3d"]
        for k in z.files:
            if f"{f}_{k}" in g.files:
                want = g[f"{f}_{k}"]
            else:
                want = g[f"{f}_{k}_f32"].astype(str(g[f"{f}_{k}_dtype"]))
                assert C.sha(want) == str(g[f"{f}_{k}_sha"])
            assert same(z[k], want), (f, k)
    assert same(np.load(os.path.join(out, "idxs.npy")), g["idxs"])


def test_python_side_argument_checks(feats):
    with pytest.raises(ValueError):
        ob.merge(np.zeros((3, 3)), np.arange(3), dist_threshold=0.0)
    with pytest.raises(ValueError):
        ob.merge(np.zeros((3, 3)), np.arange(2))
    with pytest.raises(ValueError):
        ob.filter_by_3d_box(np.zeros((2, 3)), np.arange(2), np.zeros((7, 3)))
    with pytest.raises(ValueError):
        ob.merge(np.zeros((3, 3)), np.arange(3), device="cpu")
    d = [feats[C.IMG_LISTS[0]]["descriptors"]]
    with pytest.raises(ValueError):     # a 3D point without observations
        ob.lift_descriptors(d, np.zeros(2, np.int32), np.zeros(2, np.int32), np.array([2, 0]))
    with pytest.raises(ValueError):
        ob.lift_descriptors(d, np.zeros(2, np.int32), np.zeros(2, np.int32), np.array([3]))
    with pytest.raises(ValueError):
        ob.lift_descriptors(d, np.zeros(1, np.int32), np.array([d[0].shape[1]], np.int32), np.array([1]))
    assert ob.merge(np.zeros((0, 3)), np.zeros(0, np.int64))[1] == {}


def test_entry_points_refuse_on_the_host():
    """Every check the header lists as made before a launch: status ONEPOSE_ERR_INVALID, and no
    pointer is touched (the non-null ones below point nowhere)."""
    lib = _lib.load()
    assert lib.onepose_objbuild_version() == 1
    P = 0x1000   # never dereferenced on a refused call
    bad = [
        lib.onepose_filter_points(P, P, 0, 1, P, P, P, P, None),
        lib.onepose_filter_points(P, P, (1 << 24) + 1, 1, P, P, P, P, None),
        lib.onepose_filter_points(None, P, 4, 1, P, P, P, P, None),
        lib.onepose_filter_points(P, None, 4, 1, None, P, P, None, None),
        lib.onepose_radius_neighbours(P, 2, 4, 1e-3, P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 0, 0, 1e-3, P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 0, 65537, 1e-3, P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, 0.0, P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, float("nan"), P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, float("inf"), P, P, 16, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, 1e-3, P, P, -1, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, 1e-3, P, P, 1 << 31, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, 1e-3, P, None, 16, P, None),
        lib.onepose_radius_neighbours(P, 1, 4, 1e-3, None, P, 16, P, None),
        lib.onepose_merge_greedy(P, 3, 4, P, P, P, P, P, P, P, None),
        lib.onepose_merge_greedy(P, 0, 65537, P, P, P, P, P, P, P, None),
        lib.onepose_merge_greedy(P, 0, 4, P, None, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 1, P, P, 4, P, 2, 1025, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 1, P, P, 4, P, 2, 0, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 1, P, P, 0, P, 1, 8, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 1, P, P, 4, P, 5, 8, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 0, P, P, 4, P, 2, 8, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 0, P, P, 1, P, P, 4, P, 2, 8, P, P, P, P, P, None),
        lib.onepose_lift_descriptors(P, 100, P, P, 1, P, P, 4, None, 2, 8, P, P, P, P, P, None),
        lib.onepose_gather_leaves(P, 4, 1025, P, 8, P, None),
        lib.onepose_gather_leaves(P, 0, 8, P, 8, P, None),
        lib.onepose_gather_leaves(P, 4, 8, P, 0, P, None),
        lib.onepose_gather_leaves(P, 4, 8, None, 8, P, None),
    ]
    assert bad == [1] * len(bad), bad     # ONEPOSE_ERR_INVALID
    assert b"gather_leaves" in lib.onepose_last_error()

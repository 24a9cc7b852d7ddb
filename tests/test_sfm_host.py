"""The host stages of onepose_amd.sfm against what the reference recorded
(tests/golden/make_golden_sfm.py), and the host formulation of the two device stages against
tests/sfm_oracle.py.  No GPU."""
import os

import numpy as np
import pytest
import torch

import sfm_cases as C
import sfm_oracle as O
from conftest import golden
from onepose_amd import object_builder, sfm


# ---- pairs ------------------------------------------------------------------------------------
PAIRS = golden("sfm_pairs")
SAME_NUMPY = str(PAIRS["numpy_version"]).split(".")[0] == np.__version__.split(".")[0]


@pytest.mark.parametrize("name", [str(n) for n in PAIRS["cases"]])
def test_pairs_equal_the_reference(name):
    """dist bit for bit, dR to 1e-9 degrees (its einsum's bits depend on BLAS; every dR is
    >= dR_margin from 10), the pair list equal.  The chosen set depends on numpy's partition
    order, so the list is compared only under the numpy major version that recorded it."""
    poses, seq = PAIRS[f"{name}_poses"], PAIRS[f"{name}_seq"]
    dist, dR = sfm.get_pairwise_distances(poses)
    assert dist.tobytes() == PAIRS[f"{name}_dist"].tobytes()
    assert np.abs(dR - PAIRS[f"{name}_dR"]).max() <= 1e-9
    assert float(PAIRS["dR_margin"]) >= 1e-6
    if not SAME_NUMPY:
        pytest.skip(f"pair order recorded under numpy {PAIRS['numpy_version']}, this is "
                    f"{np.__version__}: argpartition's order is not comparable")
    names = [f"s/color/{i}.png" for i in range(len(poses))]
    pairs = sfm.covis_from_pose(names, poses, int(PAIRS[f"{name}_num_matched"]), max_rotation=3,
                                seq_ids=[f"seq{s}" for s in seq])
    got = np.array([[names.index(a), names.index(b)] for a, b in pairs], np.int32).reshape(-1, 2)
    assert np.array_equal(got, PAIRS[f"{name}_pairs"])
    assert len(got) > 0


def test_pair_fixtures_cover_the_branches():
    branches = {str(PAIRS[f"{n}_branch"]) for n in PAIRS["cases"]}
    assert branches == {"try", "except"}
    dR = PAIRS["all_fail_dR"]
    off = ~np.eye(len(dR), dtype=bool)
    assert (~((dR > 10) & off).any(1)).sum() == 1   # an image all of whose candidates fail
    dist = PAIRS["duplicates_dist"]
    assert any(len(r) != len(np.unique(r)) for r in dist)


def test_sequences_default_to_the_pose_files_grandparent(tmp_path):
    poses = PAIRS["three_seqs_poses"]
    seq = PAIRS["three_seqs_seq"]
    files = []
    for i, P in enumerate(poses):
        d = tmp_path / f"seq{seq[i]}" / "poses_ba"
        d.mkdir(parents=True, exist_ok=True)
        np.savetxt(d / f"{i}.txt", P, fmt="%.18e")
        files.append(str(d / f"{i}.txt"))
    names = [f"{i}.png" for i in range(len(poses))]
    a = sfm.covis_from_pose(names, files, 12)
    b = sfm.covis_from_pose(names, poses, 12, seq_ids=[f"seq{s}" for s in seq])
    assert a == b and len(a) > 0
    # three sequences whose 2k is out of range: the reference's fallback asks for a kth beyond the
    # sequence and raises
    with pytest.raises(ValueError):
        sfm.covis_from_pose(names, poses, 90, seq_ids=[f"seq{s}" for s in seq])


def test_write_pairs(tmp_path):
    sfm.write_pairs(tmp_path / "p.txt", [("a/0.png", "a/1.png"), ("a/1.png", "a/2.png")])
    assert (tmp_path / "p.txt").read_text() == "a/0.png a/1.png\na/1.png a/2.png"


# ---- match export / import --------------------------------------------------------------------
class StubMatcher:
    def __init__(self):
        self.calls = []

    def __call__(self, data):
        self.calls.append({k: tuple(v.shape) for k, v in data.items()})
        n0, n1 = data["keypoints0"].shape[1], data["keypoints1"].shape[1]
        assert data["descriptors0"].dtype == torch.float32 and data["scores1"].dtype == torch.float32
        m0 = (torch.arange(n0) * 7 % (n1 + 1)) - 1
        m1 = (torch.arange(n1) * 3 % (n0 + 1)) - 1
        return {"matches0": m0[None], "matches1": m1[None],
                "matching_scores0": (torch.arange(n0) / 1000.0 + 1 / 3)[None],
                "matching_scores1": (torch.arange(n1) / 1000.0)[None]}


def _features(counts, sizes):
    rng = np.random.default_rng(0)
    return {f"o/c/{k}.png": {"keypoints": rng.uniform(0, 100, (n, 2)).astype(np.float32),
                             "descriptors": rng.standard_normal((8, n)).astype(np.float32),
                             "scores": rng.random(n).astype(np.float32),
                             "image_size": np.array(sizes[k])} for k, n in enumerate(counts)}


def test_match_pairs_follows_the_reference_loop():
    feats = _features([5, 9, 4], [(640, 480), (512, 384), (320, 200)])
    n = list(feats)
    m = StubMatcher()
    pairs = [(n[0], n[1]), (n[1], n[0]), (n[0], n[1]), (n[2], n[1]), (n[1], n[2]), (n[0], n[2])]
    out = sfm.match_pairs(feats, pairs, m)
    assert list(out) == [sfm.names_to_pair(n[0], n[1]), sfm.names_to_pair(n[2], n[1]),
                         sfm.names_to_pair(n[0], n[2])]
    assert sfm.names_to_pair("a/b/0.png", "a/b/1.png") == "a-b-0.png_a-b-1.png"
    assert len(m.calls) == 3   # a pair seen before, and its reverse, are skipped
    first = m.calls[0]
    assert first["image0"] == (1, 1, 480, 640) and first["image1"] == (1, 1, 384, 512)   # [::-1]
    assert first["keypoints0"] == (1, 5, 2) and first["descriptors1"] == (1, 8, 9)
    assert set(first) == {k + s for k in ("keypoints", "descriptors", "scores", "image_size")
                          for s in "01"} | {"image0", "image1"}
    g = out[sfm.names_to_pair(n[0], n[1])]
    assert g["matches0"].dtype == np.int16 and g["matches1"].dtype == np.int16
    assert g["matching_scores0"].dtype == np.float16 and g["matching_scores1"].dtype == np.float16
    assert np.array_equal(g["matches0"], (np.arange(5) * 7 % 10 - 1).astype(np.int16))
    assert np.array_equal(g["matching_scores0"], (np.arange(5, dtype=np.float32) / np.float32(1000)
                                                  + np.float32(1 / 3)).astype(np.float16))


MATCHES = golden("sfm_matches")


def _match_inputs():
    names = [str(n) for n in MATCHES["names"]]
    pairs = [(names[a], names[b]) for a, b in MATCHES["pairs"]]
    stub = {str(k): {"matches0": MATCHES[f"m0_{k}"], "matching_scores0": MATCHES[f"s0_{k}"]}
            for k in MATCHES["stub_keys"]}
    offsets = np.concatenate([[0], np.cumsum(MATCHES["counts"])])
    return (pairs, stub, {n: i + 1 for i, n in enumerate(names)},
            {n: int(o) for n, o in zip(names, offsets)})


@pytest.mark.parametrize("label,score", [("none", None), ("half", 0.5), ("zero", 0)])
def test_import_matches_equals_the_reference_arithmetic(label, score):
    pairs, stub, image_ids, offsets = _match_inputs()
    edges = sfm.import_matches(pairs, stub, image_ids, score, offsets=offsets)
    assert edges.dtype == np.int32 and np.array_equal(edges, MATCHES[f"edges_{label}"])
    assert len(MATCHES["edges_half"]) < len(MATCHES["edges_none"])


def test_import_matches_missing_pair():
    pairs, stub, image_ids, offsets = _match_inputs()
    del stub[next(iter(stub))]
    with pytest.raises(ValueError, match="Could not find pair"):
        sfm.import_matches(pairs, stub, image_ids, offsets=offsets)


# ---- the model files ----------------------------------------------------------------------------
MODEL = golden("sfm_model")


def _model_from_fixture():
    g = MODEL
    m = len(g["names"])
    kp_off = np.concatenate([[0], np.cumsum(g["n_kp"])])
    t_off = np.concatenate([[0], np.cumsum(g["t_len"])])
    ids = np.arange(1, m + 1, dtype=np.int32)
    n = len(g["xyz"])
    return {"camera_ids": ids, "camera_sizes": g["sizes"], "camera_params": g["params"],
            "image_ids": ids, "image_camera_ids": ids, "names": [str(s) for s in g["names"]],
            "qvec": g["qvec"], "tvec": g["tvec"],
            "xys": [g["xys"][kp_off[k]:kp_off[k + 1]] for k in range(m)],
            "point3D_ids": [g["p3d"][kp_off[k]:kp_off[k + 1]] for k in range(m)],
            "ids": np.arange(1, n + 1), "xyz": g["xyz"], "rgb": np.zeros((n, 3), np.uint8),
            "error": g["err"],
            "track_image_ids": [g["t_img"][t_off[k]:t_off[k + 1]] for k in range(n)],
            "track_point2D_idxs": [g["t_idx"][t_off[k]:t_off[k + 1]] for k in range(n)]}


def test_writer_is_byte_equal_to_the_reference(tmp_path):
    sfm.write_model_binary(_model_from_fixture(), tmp_path)
    for f in ("cameras.bin", "images.bin", "points3D.bin"):
        want = open(os.path.join(C.GOLDEN, "sfm_model", f), "rb").read()
        assert (tmp_path / f).read_bytes() == want, f
    pts = object_builder.read_points3d_binary(tmp_path / "points3D.bin")
    img = object_builder.read_images_binary(tmp_path / "images.bin")
    assert np.array_equal(pts["ids"], MODEL["read_point_ids"])
    assert np.array_equal(pts["xyz"], MODEL["read_xyz"])
    assert np.array_equal(pts["track_len"], MODEL["read_track_len"])
    assert np.array_equal(img["image_ids"], MODEL["read_image_ids"])
    assert img["names"] == [str(s) for s in MODEL["read_names"]]
    assert np.array_equal(np.concatenate(img["point3D_ids"]), MODEL["read_p3d"])


def test_rotmat2qvec():
    for R, q in zip(MODEL["rot"], MODEL["rot_qvec"]):
        got = sfm.rotmat2qvec(R)
        assert got[0] >= 0 and np.abs(got - q).max() <= 1e-12


def test_empty_model_sorts_by_integer_stem():
    names = ["o/color/10.png", "o/color/9.png", "o/color/100.png", "o/color/0.png"]
    poses = np.tile(np.eye(4), (4, 1, 1))
    poses[:, 0, 3] = [10, 9, 100, 0]
    Ks = np.tile(np.array([[500.0, 0, 250], [0, 510, 260], [0, 0, 1]]), (4, 1, 1))
    Ks[:, 0, 0] += [10, 9, 100, 0]
    m = sfm.empty_model(names, poses, Ks, [(640, 480)] * 4)
    assert m["names"] == [names[3], names[1], names[0], names[2]]
    assert np.array_equal(m["image_ids"], [1, 2, 3, 4]) and np.array_equal(m["camera_ids"], [1, 2, 3, 4])
    assert np.array_equal(m["tvec"][:, 0], [0, 9, 10, 100])
    assert np.array_equal(m["camera_params"][:, 0], [500, 509, 510, 600])
    assert np.array_equal(m["camera_params"][0], [500, 510, 250, 260])
    assert np.array_equal(m["camera_sizes"][0], [640, 480]) and len(m["ids"]) == 0


# ---- tracks and triangulation, host formulation -------------------------------------------------
@pytest.mark.parametrize("name", list(C.graph_cases()))
def test_host_tracks_equal_the_oracle(name):
    edges, n = C.graph_cases()[name]
    counts = [n // 3, n - n // 3 - n // 4, n // 4] if n >= 4 else [n]
    labels = O.components(edges.tolist(), n)
    want = O.tracks_from_labels(labels, counts)
    got = sfm.build_tracks(counts, edges, device=None)
    for a, b in zip(want, (got["track_start"], got["obs_image"], got["obs_feat"])):
        assert a.dtype == b.dtype and np.array_equal(a, b)


TRI = golden("sfm_tri")


def test_host_triangulation_equals_the_oracle():
    p = C.tri_problem()
    assert C.tri_sha(p) == str(TRI["sha"])
    assert float(TRI["margin"]) >= 1e-6
    out = sfm.triangulate_tracks(p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"])
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(out[k], TRI[k]), k
    kept = TRI["reason"] == 0
    assert np.array_equal(np.isnan(out["xyz"][:, 0]), ~kept)
    dev = np.maximum(np.abs(out["xyz"] - TRI["xyz"]).max(1), np.abs(out["err"] - TRI["err"]))
    assert (dev[kept] <= TRI["tol"][kept]).all(), dev[kept] / TRI["tol"][kept]
    want = dict(len1=3, len257=3, nan_pixel=4, wrong_match=1, angle_below=2, angle_above=0,
                one_outlier=0, several_outliers=0)
    for name, why in want.items():
        assert out["reason"][C.TRI_NAMES.index(name)] == why, name
    lens = np.diff(p["track_start"])
    drop = {n: int(lens[i] - out["n_kept"][i]) for i, n in enumerate(C.TRI_NAMES)}
    assert (drop["one_outlier"], drop["several_outliers"], drop["two_in_one_image"],
            drop["behind_one_camera"]) == (1, 4, 1, 1)


def test_host_triangulation_refuses_a_malformed_csr():
    p = C.tri_problem()
    bad = p["track_start"].copy()
    bad[3] = bad[4] + 1
    with pytest.raises(sfm._lib.OnePoseError, match="monotone"):
        sfm.triangulate_tracks(p["Rt"], p["K4"], bad, p["obs_image"], p["obs_xy"])
    img = p["obs_image"].copy()
    img[5] = len(p["Rt"])
    with pytest.raises(sfm._lib.OnePoseError, match="image id"):
        sfm.triangulate_tracks(p["Rt"], p["K4"], p["track_start"], img, p["obs_xy"])


# ---- the edge fixture and the CSR larger than one stride of the check ---------------------------
EDGES = golden("sfm_tri_edges")
KEYS = ("xyz", "err", "reason", "n_kept", "obs_keep")


def _generator():
    import sys
    if C.GOLDEN not in sys.path:
        sys.path.insert(0, C.GOLDEN)
    import make_golden_sfm_edges as G
    return G


def _same(out, prefix, keys=KEYS):
    """Decisions equal, xyz and err equal in bits on the kept tracks and NaN on the others."""
    kept = EDGES[f"{prefix}_reason"] == 0
    for k in keys:
        want = EDGES[f"{prefix}_{k}"]
        assert out[k].dtype == want.dtype, k
        if k in ("xyz", "err"):
            assert out[k][kept].tobytes() == want[kept].tobytes(), (prefix, k)
            assert np.isnan(out[k][~kept]).all(), (prefix, k)
        else:
            assert np.array_equal(out[k], want), (prefix, k)


def test_the_edge_fixture_equals_the_oracle_run_afresh():
    G = _generator()
    p = C.edge_problem()
    assert C.tri_sha(p) == str(EDGES["edge_sha"])
    assert int(EDGES["edge_final_check_seed"]) == C.FINAL_CHECK_SEED
    assert float(EDGES["edge_margin"]) >= 1e-6
    out, margins, ties = G.run(p)
    _same(out, "edge")
    t = C.EDGE_NAMES.index("dup_exact_tie")
    assert sorted(ties[t]) == sorted(C.EDGE_TIES) and not any(ties[:t] + ties[t + 1:])
    assert sorted(margins[t])[:4][:3] == [0.0] * 3 and sorted(margins[t])[3] >= 1e-6
    rest = [m for k, ms in enumerate(margins) for m in ms if k != t or m != 0.0]
    assert min(rest) == float(EDGES["edge_margin"])
    _same(G.run(p, max_reproj=np.inf)[0], "inf")
    assert np.array_equal(G.run(p, max_reproj=0.0)[0]["reason"], EDGES["zero_reason"])
    kept = EDGES["edge_reason"] == 0
    assert np.isfinite(EDGES["edge_tol"][kept]).all() and np.isfinite(EDGES["edge_ls_dist"][kept]).all()


def test_the_big_csr_fixture_equals_the_oracle_run_afresh():
    p = C.big_csr()
    assert C.tri_sha(p) == str(EDGES["big_sha"]) and float(EDGES["big_margin"]) >= 1e-6
    _same(_generator().run(p)[0], "big")
    assert O.check_csr(p["track_start"], p["obs_image"], len(p["Rt"])) == (0, 0)
    for name, (ts, img, want) in C.malformed_csrs(p).items():
        assert O.check_csr(ts, img, len(p["Rt"])) == want, name
        with pytest.raises(sfm._lib.OnePoseError, match="monotone" if want[0] == 1 else "image id"):
            sfm.triangulate_tracks(p["Rt"], p["K4"], ts, img, p["obs_xy"])


def test_host_triangulation_equals_the_edge_fixtures():
    """sfm.triangulate_tracks(device=None) on both new problems and at both thresholds: the
    oracle's decisions, and its xyz and err bit for bit."""
    p = C.edge_problem()
    args = (p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"])
    _same(sfm.triangulate_tracks(*args), "edge")
    _same(sfm.triangulate_tracks(*args, max_reproj=np.inf), "inf")
    assert np.array_equal(sfm.triangulate_tracks(*args, max_reproj=0.0)["reason"], EDGES["zero_reason"])
    b = C.big_csr()
    _same(sfm.triangulate_tracks(b["Rt"], b["K4"], b["track_start"], b["obs_image"], b["obs_xy"]), "big")


REFUSALS = [   # (entry point, the arguments changed, the header's message)
    ("tri", dict(n_tracks=0), "tracks_triangulate: n_tracks=0 outside 1..2^24"),
    ("tri", dict(n_obs=0), "tracks_triangulate: n_obs=0 outside 1..2^28"),
    ("tri", dict(n_images=0), "tracks_triangulate: n_images=0"),
    ("tri", dict(max_reproj=float("nan")), "tracks_triangulate: NaN threshold"),
    ("tri", dict(min_angle_deg=float("nan")), "tracks_triangulate: NaN threshold"),
    ("tri", dict(obs_keep=None), "tracks_triangulate: null pointer"),
    ("tri", dict(status=None), "tracks_triangulate: null pointer"),
    ("cc", dict(n_nodes=0), "track_components: n_nodes=0 outside 1..2^30"),
    ("cc", dict(rounds=65), "track_components: rounds=65 outside 0..64"),
    ("cc", dict(n_edges=-1), "track_components: n_edges=-1 outside 0..2^30"),
    ("cc", dict(parent=None), "track_components: null pointer"),
]


@pytest.mark.parametrize("entry,change,text", REFUSALS,
                         ids=[f"{e}-{'-'.join(c)}" for e, c, _ in REFUSALS])
def test_host_refusals_launch_nothing(entry, change, text):
    """Every pointer is a value that is never dereferenced: the call is refused on the host
    before a launch, with code 1 (ONEPOSE_ERR_INVALID) and the message of the check."""
    lib = sfm._lib.load()
    p = 0x1000
    if entry == "tri":
        a = dict(Rt=p, K4=p, n_images=3, track_start=p, obs_image=p, obs_xy=p, n_tracks=2, n_obs=5,
                 max_reproj=4.0, min_angle_deg=1.5, xyz=p, err=p, reason=p, n_kept=p, obs_keep=p,
                 status=p, stream=None)
        a.update(change)
        rc = lib.onepose_tracks_triangulate(*a.values())
    else:
        a = dict(edges=p, n_edges=4, n_nodes=8, rounds=2, init=1, parent=p, status=p, stream=None)
        a.update(change)
        rc = lib.onepose_track_components(*a.values())
    assert rc == 1 and lib.onepose_last_error().decode() == text


# ---- the chain on the host ----------------------------------------------------------------------
class OracleNN:
    """NearestNeighbour's forward dict from tests/nn_oracle.py (numpy), for the host chain."""

    def __init__(self, ratio=0.8, distance=0.7):
        self.ratio, self.distance = ratio, distance

    def __call__(self, data):
        import nn_oracle
        r = nn_oracle.forward(data["descriptors0"].numpy(), data["descriptors1"].numpy(),
                              self.ratio, self.distance)
        return {k: torch.from_numpy(np.asarray(r[k])) for k in
                ("matches0", "matches1", "matching_scores0", "matching_scores1")}


@pytest.fixture(scope="module")
def host_chain(tmp_path_factory):
    feats, names, poses, Ks, pts, owner = C.scene()
    out = tmp_path_factory.mktemp("sfm") / "model"
    model = sfm.reconstruct(feats, names, poses, Ks, OracleNN(), covis_num=10, out_dir=str(out),
                            device=None)
    return feats, names, pts, owner, model, str(out)


def test_host_chain_recovers_the_scene(host_chain):
    """The scene's own condition: the host chain keeps >= 90 % of the 200 points, each within
    1 mm of its ground truth."""
    feats, names, pts, owner, model, _ = host_chain
    found = {}
    for k, tr_img in enumerate(model["track_image_ids"]):
        owners = {int(owner[model["names"][i - 1]][f]) for i, f in
                  zip(tr_img, model["track_point2D_idxs"][k])}
        if len(owners) == 1 and -1 not in owners:
            (o,) = owners
            d = np.linalg.norm(model["xyz"][k] - pts[o])
            found[o] = min(found.get(o, np.inf), d)
    good = sum(d <= 1e-3 for d in found.values())
    print(f"{len(model['ids'])} points kept, {good} of {C.SCENE_POINTS} scene points within 1 mm, "
          f"{len(model['pairs'])} pairs")
    assert good >= 0.9 * C.SCENE_POINTS
    assert np.array_equal(model["ids"], np.arange(1, len(model["ids"]) + 1))
    # point3D_ids: -1 except on the final observations of kept tracks
    marked = sum(int((p != -1).sum()) for p in model["point3D_ids"])
    assert marked == int(model["track_len"].sum()) == sum(len(t) for t in model["track_image_ids"])
    for k in (0, len(model["ids"]) - 1):
        for i, f in zip(model["track_image_ids"][k], model["track_point2D_idxs"][k]):
            assert model["point3D_ids"][i - 1][f] == model["ids"][k]


def test_object_builder_runs_on_the_mapping_and_on_the_files(host_chain):
    feats, names, pts, owner, model, out = host_chain
    a = object_builder.build_object(model, feats, names, C.SCENE_BOX, device=None)
    b = object_builder.build_object(out, feats, names, C.SCENE_BOX, device=None)
    assert a["keypoints3d"].shape[0] >= 0.9 * C.SCENE_POINTS
    for k in ("keypoints3d", "idxs", "collected", "mean64", "mean32", "scores"):
        assert np.array_equal(a[k], b[k]), k
    pts3 = object_builder.read_points3d_binary(os.path.join(out, "points3D.bin"))
    assert np.array_equal(pts3["xyz"], model["xyz"]) and np.array_equal(pts3["track_len"],
                                                                         model["track_len"])

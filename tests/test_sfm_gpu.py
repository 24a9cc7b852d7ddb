"""The sparse-reconstruction kernels on the GPU: onepose_track_components against the plain-loop
oracle (labels equal), onepose_tracks_triangulate against the oracle's recorded results
(tests/golden/make_golden_sfm.py: decisions equal, xyz and err within 16 x the eigh-vs-svd
deviation of the oracle with a floor of 1e-12, and no farther from scipy's least_squares minimum
than the oracle is), and the chain against its host formulation."""
import numpy as np
import pytest
import torch

import sfm_cases as C
import sfm_oracle as O
from ba_cases import Guarded
from conftest import golden
from onepose_amd import _lib, nn_matcher, object_builder, sfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- components -------------------------------------------------------------------------------
def components(lib, device, edges, n_nodes, rounds, init=1, parent=None):
    e = Guarded(device, data=edges if len(edges) else np.zeros((1, 2), np.int32))
    par = parent or Guarded(device, nbytes=4 * n_nodes, dtype=torch.int32)
    status = Guarded(device, nbytes=16, dtype=torch.int32)
    _lib.check(lib.onepose_track_components(e.ptr if len(edges) else None, len(edges), n_nodes,
                                            rounds, init, par.ptr, status.ptr,
                                            _lib.stream_ptr(device)), "track_components")
    torch.cuda.synchronize(device)
    assert e.intact() and par.intact() and status.intact(), "guard words overwritten"
    return par, status.numpy()


GRAPHS = C.graph_cases()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_components_equal_the_oracle(name, lib, device):
    edges, n = GRAPHS[name]
    par, status = components(lib, device, edges, n, 16)
    print(f"{name}: {status[1]} rounds joined something, {status[0]} edges open")
    assert status[0] == 0
    assert status[2] == (C.OUT_OF_RANGE_COUNT if name == "out_of_range" else 0)
    assert np.array_equal(par.numpy(), O.components(edges.tolist(), n))
    if not len(edges):
        assert status[1] == 0


@pytest.mark.parametrize("name", ["path1025_random", "path300_zigzag", "interleaved"])
def test_one_round_per_call_continues_to_the_same_labels(name, lib, device):
    edges, n = GRAPHS[name]
    want = O.components(edges.tolist(), n)
    par, status = components(lib, device, edges, n, 1)
    calls = 1
    while status[0] != 0:
        assert calls < 64
        par, status = components(lib, device, edges, n, 1, init=0, parent=par)
        calls += 1
    print(f"{name}: converged after {calls} calls of one round")
    assert np.array_equal(par.numpy(), want)
    if name == "path1025_random":
        assert calls > 2   # the first call alone must not have been enough


def test_components_replay_in_a_graph(lib, device):
    edges, n = GRAPHS["path1025_random"]
    eager, _ = components(lib, device, edges, n, 16)
    e = torch.from_numpy(edges).to(device)
    par = torch.empty(n, dtype=torch.int32, device=device)
    status = torch.empty(4, dtype=torch.int32, device=device)
    stream = torch.cuda.Stream(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            _lib.check(lib.onepose_track_components(e.data_ptr(), len(edges), n, 16, 1,
                                                    par.data_ptr(), status.data_ptr(),
                                                    _lib.stream_ptr(device)), "track_components")
    for _ in range(2):
        par.fill_(-7)
        graph.replay()
        torch.cuda.synchronize(device)
        assert np.array_equal(par.cpu().numpy(), eager.numpy()) and int(status[0]) == 0


def test_wrapper_and_build_tracks_equal_the_host(device):
    for name in ("path1025_random", "duplicates", "out_of_range", "empty65", "star2000_hub_last",
                 "grid64_shuffled", "sparse65537"):
        edges, n = GRAPHS[name]
        counts = [n // 3, n - n // 3 - n // 4, n // 4]
        a = sfm.build_tracks(counts, edges, device=device)
        b = sfm.build_tracks(counts, edges, device=None)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)


# ---- triangulation ----------------------------------------------------------------------------
TRI = golden("sfm_tri")


def triangulate(lib, device, p, max_reproj=C.MAX_REPROJ, min_angle=C.MIN_ANGLE):
    T, n_obs = len(p["track_start"]) - 1, len(p["obs_image"])
    g = [Guarded(device, data=p[k]) for k in ("Rt", "K4", "track_start", "obs_image", "obs_xy")]
    xyz, err = Guarded(device, nbytes=24 * T), Guarded(device, nbytes=8 * T)
    reason, kept = (Guarded(device, nbytes=4 * T, dtype=torch.int32) for _ in range(2))
    keep = Guarded(device, nbytes=n_obs, dtype=torch.uint8)
    status = Guarded(device, nbytes=8, dtype=torch.int32)
    _lib.check(lib.onepose_tracks_triangulate(
        g[0].ptr, g[1].ptr, len(p["Rt"]), g[2].ptr, g[3].ptr, g[4].ptr, T, n_obs, max_reproj,
        min_angle, xyz.ptr, err.ptr, reason.ptr, kept.ptr, keep.ptr, status.ptr,
        _lib.stream_ptr(device)), "tracks_triangulate")
    torch.cuda.synchronize(device)
    for x in (*g, xyz, err, reason, kept, keep, status):
        assert x.intact(), "guard words overwritten"
    return {"xyz": xyz.numpy((T, 3)), "err": err.numpy(), "reason": reason.numpy(),
            "n_kept": kept.numpy(), "obs_keep": keep.numpy().astype(bool),
            "status": status.numpy()}


@pytest.fixture(scope="module")
def tri_out(lib, device):
    p = C.tri_problem()
    assert C.tri_sha(p) == str(TRI["sha"])
    return p, triangulate(lib, device, p)


def test_triangulation_decisions_equal_the_oracle(tri_out):
    p, out = tri_out
    assert float(TRI["margin"]) >= 1e-6 and out["status"][0] == 0
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(out[k], TRI[k]), (k, out[k], TRI[k])
    lost = TRI["reason"] != 0
    assert np.isnan(out["xyz"][lost]).all() and np.isnan(out["err"][lost]).all()
    got = {n: int(out["reason"][i]) for i, n in enumerate(C.TRI_NAMES)}
    assert (got["len1"], got["len257"], got["nan_pixel"], got["wrong_match"], got["angle_below"],
            got["angle_above"], got["angle_rays"]) == (3, 3, 4, 1, 2, 0, 2)


@pytest.mark.parametrize("name", [n for n in C.TRI_NAMES if n in C.TRI_REFINED])
def test_triangulation_within_the_recorded_tolerance(name, tri_out):
    p, out = tri_out
    t = C.TRI_NAMES.index(name)
    tol = float(TRI["tol"][t])
    dev = max(np.abs(out["xyz"][t] - TRI["xyz"][t]).max(), abs(out["err"][t] - TRI["err"][t]))
    ls = np.abs(out["xyz"][t] - TRI["ls_xyz"][t]).max()
    bits = out["xyz"][t].tobytes() == TRI["xyz"][t].tobytes() and out["err"][t] == TRI["err"][t]
    print(f"{name}: deviation {dev:.2e} (tol {tol:.1e}), {ls:.2e} from the least_squares minimum "
          f"(the oracle: {float(TRI['ls_dist'][t]):.2e}), bits equal: {bits}")
    assert out["reason"][t] == 0
    assert dev <= tol
    assert ls <= float(TRI["ls_dist"][t]) + tol
    assert bits   # a fixed order in every sum and no contraction: the oracle's very numbers


def test_two_calls_are_bit_equal(lib, device, tri_out):
    p, out = tri_out
    again = triangulate(lib, device, p)
    for k in out:
        assert np.array_equal(out[k], again[k], equal_nan=True), k


def test_thresholds_are_arguments(lib, device, tri_out):
    p, out = tri_out
    loose = triangulate(lib, device, p, max_reproj=1e9, min_angle=0.0)
    t = C.TRI_NAMES.index("angle_below")
    assert loose["reason"][t] == 0 and out["reason"][t] == 2
    t = C.TRI_NAMES.index("one_outlier")
    assert loose["n_kept"][t] == 17 and out["n_kept"][t] == 16
    none = triangulate(lib, device, p, max_reproj=-1.0)
    assert set(none["reason"].tolist()) <= {1, 3, 4}


@pytest.mark.parametrize("what", ["decreasing", "first", "last", "image"])
def test_a_malformed_csr_sets_status_and_writes_nothing(what, lib, device):
    p = dict(C.tri_problem())
    ts, img = p["track_start"].copy(), p["obs_image"].copy()
    if what == "decreasing":
        ts[5] = ts[6] + 3
        want = (1, 6)
    elif what == "first":
        ts[0] = 1
        want = (1, 0)
    elif what == "last":
        ts[-1] += 1
        want = (1, len(ts) - 1)
    else:
        img[40] = len(p["Rt"])
        img[77] = -1
        want = (2, 40)
    p["track_start"], p["obs_image"] = ts, img
    out = triangulate(lib, device, p)
    assert tuple(out["status"]) == want
    # Guarded fills with 0xA5: every output byte is still that
    assert (out["reason"].view(np.uint8) == 0xA5).all() and (out["n_kept"].view(np.uint8) == 0xA5).all()
    assert (out["xyz"].view(np.uint8) == 0xA5).all() and (out["err"].view(np.uint8) == 0xA5).all()
    assert (out["obs_keep"].view(np.uint8) != 0).all()
    with pytest.raises(_lib.OnePoseError):
        sfm.triangulate_tracks(p["Rt"], p["K4"], ts, img, p["obs_xy"], device=device)


def test_python_layer_equals_the_host_path(device, tri_out):
    p, out = tri_out
    a = sfm.triangulate_tracks(p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"],
                               device=device)
    b = sfm.triangulate_tracks(p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"])
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], out[k], equal_nan=True), k
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(a[k], b[k]), k


# ---- the chain --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains(device, tmp_path_factory):
    feats, names, poses, Ks, pts, owner = C.scene()
    nn = nn_matcher.NearestNeighbour({"ratio_threshold": 0.8, "distance_threshold": 0.7})
    out = tmp_path_factory.mktemp("sfm") / "model"
    gpu = sfm.reconstruct(feats, names, poses, Ks, nn, covis_num=10, out_dir=str(out),
                          device=device)
    host = sfm.reconstruct(feats, names, poses, Ks, nn, covis_num=10, device=None,
                           match_device=device)
    return feats, names, pts, gpu, host, str(out)


def test_chain_equals_its_host_formulation(chains):
    feats, names, pts, gpu, host, _ = chains
    for k in ("track_start", "obs_image", "obs_feat"):
        assert np.array_equal(gpu["tracks"][k], host["tracks"][k]), k
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(gpu["triangulation"][k], host["triangulation"][k]), k
    assert len(gpu["ids"]) >= 0.9 * C.SCENE_POINTS
    # the tolerance of the triangulation tests, worked out for these tracks: 16 x the oracle's
    # eigh-vs-svd deviation, floor 1e-12
    tr, K4 = gpu["tracks"], gpu["camera_params"]
    kept = np.nonzero(gpu["triangulation"]["reason"] == 0)[0]
    order = sorted(range(len(names)), key=lambda i: int(names[i].split("/")[-1].split(".")[0]))
    Rt = C.scene()[2][order][:, :3, :4]
    xy = np.concatenate([np.asarray(feats[n]["keypoints"], np.float64) for n in gpu["names"]]) + 0.5
    off = np.concatenate([[0], np.cumsum([len(feats[n]["keypoints"]) for n in gpu["names"]])])
    worst = 0.0
    for t in kept[:: max(1, len(kept) // 40)]:   # 40 tracks spread over the model
        a, b = tr["track_start"][t], tr["track_start"][t + 1]
        img, uv = tr["obs_image"][a:b], xy[off[tr["obs_image"][a:b]] + tr["obs_feat"][a:b]]
        e = O.triangulate(Rt, K4, img, uv, 4.0, 1.5, solver="eigh")
        s = O.triangulate(Rt, K4, img, uv, 4.0, 1.5, solver="svd")
        tol = max(16 * np.abs(e[1] - s[1]).max(), 1e-12)
        dev = np.abs(gpu["triangulation"]["xyz"][t] - host["triangulation"]["xyz"][t]).max()
        worst = max(worst, dev / tol)
        assert dev <= tol, (t, dev, tol)
    print(f"{len(kept)} points kept; largest deviation / tolerance over the sampled tracks: {worst:.3g}")
    assert np.array_equal(gpu["xyz"], host["xyz"])   # the same operations in the same order


def test_object_builder_on_the_mapping_and_on_the_directory(chains, device):
    feats, names, pts, gpu, host, out = chains
    a = object_builder.build_object(gpu, feats, names, C.SCENE_BOX, device=device)
    b = object_builder.build_object(out, feats, names, C.SCENE_BOX, device=device)
    assert a["keypoints3d"].shape[0] >= 0.9 * C.SCENE_POINTS
    for k in ("keypoints3d", "idxs", "scores"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("collected", "mean64", "mean32"):
        assert torch.equal(a[k], b[k]), k

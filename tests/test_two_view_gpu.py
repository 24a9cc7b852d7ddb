"""onepose_two_view_verify on the GPU against the plain-loop oracle's recorded results
(tests/golden/make_golden_two_view.py): status, inlier mask, inlier count and iterations equal; F,
scaled to unit Frobenius norm with its largest entry positive, within the recorded tolerance (16 x
the oracle's Jacobi-vs-eigh deviation, floor 1e-12); the given-F mode; determinism, another
stream, a captured graph; the refusals; and the chain against its host formulation."""
import numpy as np
import pytest
import torch

import sfm_cases
import two_view_cases as C
import two_view_oracle as O
from ba_cases import Guarded
from conftest import golden
from onepose_amd import _lib, nn_matcher, sfm

pytestmark = pytest.mark.gpu

GOLD = golden("two_view")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def batches(lib):
    P = int(lib.onepose_two_view_max_points())
    assert P >= 4096 and P == int(GOLD["max_points"]), \
        "onepose_two_view_max_points() changed: record tests/golden/two_view.npz again"
    b = C.gpu_batches(P)
    for key, batch in b.items():
        assert C.sha(batch["pts0"], batch["pts1"], batch["counts"]) == str(GOLD[f"{key}_sha"]), key
    return b


def verify(device, batch, F_in=None, stream=None, **over):
    """One guarded call -> dict of numpy outputs."""
    B, P = batch["pts0"].shape[:2]
    opts = dict(batch["options"], **over)
    g = [Guarded(device, data=batch[k]) for k in ("pts0", "pts1", "counts")]
    fin = None if F_in is None else Guarded(device, data=np.ascontiguousarray(F_in, np.float64))
    F = Guarded(device, nbytes=72 * B)
    mask = Guarded(device, nbytes=B * P, dtype=torch.uint8)
    nin, iters, status = (Guarded(device, nbytes=4 * B, dtype=torch.int32) for _ in range(3))
    nbytes = _lib.call("onepose_two_view_workspace_bytes", batch=B, max_points=P)
    ws = Guarded(device, nbytes=nbytes, dtype=torch.uint8)
    rc = _lib.call("onepose_two_view_verify", pts0=g[0].ptr, pts1=g[1].ptr, counts=g[2].ptr,
                   max_points=P, batch=B, F_in=None if fin is None else fin.ptr,
                   max_error=opts["max_error"], confidence=opts["confidence"],
                   max_trials=opts["max_trials"], min_num_inliers=opts["min_num_inliers"],
                   min_inlier_ratio=opts["min_inlier_ratio"], refine_iters=opts["refine_iters"],
                   F=F.ptr, inlier_mask=mask.ptr, n_inliers=nin.ptr, iters=iters.ptr,
                   status=status.ptr, workspace=ws.ptr, workspace_bytes=nbytes,
                   stream=stream if stream is not None else _lib.stream_ptr(device))
    torch.cuda.synchronize(device)
    for x in (*g, F, mask, nin, iters, status, ws):
        assert x.intact(), "guard words overwritten"
    return {"rc": rc, "F": F.numpy((B, 9)), "mask": mask.numpy((B, P)), "n_inliers": nin.numpy(),
            "iters": iters.numpy(), "status": status.numpy()}


@pytest.fixture(scope="module")
def outs(device, batches):
    return {key: verify(device, batch) for key, batch in batches.items()}


@pytest.mark.parametrize("key", ["main", "capped", "small", "clamp"])
def test_estimate_equals_the_oracle(key, outs, batches):
    out, batch = outs[key], batches[key]
    assert out["rc"] == 0
    dev = np.abs(O.normalised(out["F"]) - O.normalised(GOLD[f"{key}_F"])).max(1)
    bits = sum(out["F"][b].tobytes() == GOLD[f"{key}_F"][b].tobytes() for b in range(len(dev)))
    print(f"{key}: largest F deviation {dev.max():.3e} (tolerance {float(GOLD['f_tol']):.1e}, "
          f"measured Jacobi-vs-eigh deviation {float(GOLD['f_dev']):.3e}); F bit-equal on {bits} "
          f"of {len(dev)} pairs")
    for k in ("status", "n_inliers", "iters"):
        assert np.array_equal(out[k], GOLD[f"{key}_{k}"]), (k, out[k], GOLD[f"{key}_{k}"])
    assert np.array_equal(out["mask"], GOLD[f"{key}_mask"])
    for b, n in enumerate(batch["n"]):
        assert not out["mask"][b, n:].any()   # zero past the count
    assert (dev <= float(GOLD["f_tol"])).all(), dev
    # the same operations in the same order: the kernel reproduces the oracle's F bit for bit
    assert bits == len(dev)
    none = np.isin(out["status"], (1, 2))
    assert not out["F"][none].any() and not out["n_inliers"][none].any()


# ---- the options and the given-F edges (tests/golden/make_golden_two_view_options.py) ------------
OPT = golden("two_view_options")
OPTION_CALLS = C.option_calls()


@pytest.mark.parametrize("key", list(OPTION_CALLS))
def test_option_calls_equal_the_oracle(key, device):
    """Every call of the "options" family as test_estimate_equals_the_oracle compares a batch:
    status, count, iterations and mask equal, F within the tolerance recorded with the family,
    F bit-equal; a given F comes back byte for byte, a NaN entry included."""
    call = OPTION_CALLS[key]
    assert C.option_sha(call) == str(OPT[f"{key}_sha"]), key
    out = verify(device, call, F_in=call.get("F_in"))
    want = {k: OPT[f"{key}_{k}"] for k in ("F", "mask", "n_inliers", "iters", "status")}
    assert out["rc"] == 0
    with np.errstate(invalid="ignore"):
        dev = np.abs(O.normalised(out["F"]) - O.normalised(want["F"])).max(1)
    finite = np.isfinite(want["F"]).all(1)
    bits = sum(out["F"][b].tobytes() == want["F"][b].tobytes() for b in range(len(dev)))
    print(f"{key}: status {out['status'].tolist()}, inliers {out['n_inliers'].tolist()}, iterations "
          f"{out['iters'].tolist()}; largest F deviation {dev[finite].max():.3e} (tolerance "
          f"{float(OPT['f_tol']):.1e}); F bit-equal on {bits} of {len(dev)} pairs")
    for k in ("status", "n_inliers", "iters"):
        assert np.array_equal(out[k], want[k]), (k, out[k], want[k])
    assert np.array_equal(out["mask"], want["mask"])
    for b, n in enumerate(call["n"]):
        assert not out["mask"][b, n:].any()   # zero past the count
    assert (dev[finite] <= float(OPT["f_tol"])).all(), dev
    assert bits == len(dev)
    if "F_in" in call:
        assert out["F"].tobytes() == call["F_in"].tobytes() and not out["iters"].any()
    else:
        none = np.isin(out["status"], (1, 2))
        assert not out["F"][none].any() and not out["n_inliers"][none].any()


def test_the_option_calls_hold_what_they_are_for(device):
    """Spot assertions, so that a fixture recorded again cannot change what a call is for."""
    def run(key):
        return verify(device, OPTION_CALLS[key], F_in=OPTION_CALLS[key].get("F_in"))
    r = {k: run(f"tight_refine{k}") for k in C.REFINE_ITERS}
    d01, d12, ended = (int(b) for b in OPT["refine_pairs"])
    assert r[0]["F"][d01].tobytes() != r[1]["F"][d01].tobytes()
    assert r[1]["F"][d12].tobytes() != r[2]["F"][d12].tobytes()
    assert r[2]["F"][ended].tobytes() == r[5]["F"][ended].tobytes()   # a refit not kept ends them
    zero = run("max_error0")
    assert (zero["status"] == 2).all() and (zero["iters"] == 300).all()
    tight = np.concatenate([run("max_error0.5")["status"], run("max_error1")["status"]])
    assert (tight == 3).any() and (tight == 0).any()
    lo, hi = run("confidence0.5")["iters"], run("confidence0.999999")["iters"]
    assert lo[0] < 64 and (hi[1:] > 128).all() and (lo[1:] < hi[1:]).all()
    assert run("ratio0.8")["status"].tolist() == run("ratio1")["status"].tolist() == [0, 3, 3]
    assert run("ratio-1")["status"].tolist() == [0, 0, 0]
    for P, counts in C.LDS_MAX_POINTS.items():
        assert run(f"points{P}")["status"].tolist() == [1 if c < 8 else 0 for c in counts]
    assert run("given")["status"].tolist() == [3, 3, 3, 1, 1, 1, 1, 0]


def test_the_batches_hold_what_they_are_for(outs, batches):
    main, capped = outs["main"], outs["capped"]
    name = {key: list(batches[key]["names"]) for key in batches}
    for c in (0, 7, 8, 14):   # fewer matches than min_num_inliers: nothing is run
        for share in (0, 30):
            b = name["main"].index(f"n{c}_out{share}")
            assert main["status"][b] == 1 and main["iters"][b] == 0
    for c in (63, 64, 65, 257, 1000, "max"):
        assert main["status"][name["main"].index(f"n{c}_out0")] == 0
        assert main["status"][name["main"].index(f"n{c}_out30")] == 0
        assert capped["iters"][name["capped"].index(f"n{c}_out60")] == 300   # the loop at its cap
    assert capped["status"][name["capped"].index("unrelated")] in (2, 3)
    assert capped["status"][name["capped"].index("identical")] == 2
    assert capped["iters"][name["capped"].index("identical")] == 300
    b = name["main"].index("nonfinite")
    assert main["status"][b] == 0 and not main["mask"][b, [3, 17, 40, 41, 77, 90]].any()
    b = name["main"].index("doubled")
    assert np.array_equal(main["mask"][b, 0:120:2], main["mask"][b, 1:120:2])
    assert outs["small"]["status"][name["small"].index("n14_min8")] == 0
    clamp = outs["clamp"]   # 10^9 -> max_points, -5 -> 0
    over, neg, exact = (name["clamp"].index(k) for k in ("over_count", "negative_count", "exact_count"))
    assert clamp["status"][neg] == 1 and not clamp["mask"][neg].any()
    for k in ("F", "mask", "n_inliers", "iters", "status"):
        assert np.array_equal(clamp[k][over], clamp[k][exact]), k


@pytest.mark.parametrize("key", ["main", "capped"])
def test_given_geometry_scores_like_the_oracle(key, device, outs, batches):
    """F_in: the oracle's F gives the oracle's scoring; the estimate's own F fed back in gives
    the estimate's mask; F comes back as given, iters 0."""
    batch = batches[key]
    a = verify(device, batch, F_in=GOLD[f"{key}_F"])
    assert a["rc"] == 0
    assert np.array_equal(a["mask"], GOLD[f"{key}_given_mask"])
    assert np.array_equal(a["status"], GOLD[f"{key}_given_status"])
    assert a["F"].tobytes() == GOLD[f"{key}_F"].tobytes() and not a["iters"].any()
    own = outs[key]
    b = verify(device, batch, F_in=own["F"])
    run = own["status"] != 1
    model = np.isin(own["status"], (0, 3))
    assert np.array_equal(b["mask"][model], own["mask"][model])
    assert np.array_equal(b["n_inliers"][model], own["n_inliers"][model])
    assert np.array_equal(b["status"][model], own["status"][model])
    assert not b["mask"][~model].any() and (b["status"][run & ~model] == 3).all()


def test_runs_and_streams_give_equal_bits(device, outs, batches):
    again = verify(device, batches["main"])
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        other = verify(device, batches["main"], stream=side.cuda_stream)
    for k in ("F", "mask", "n_inliers", "iters", "status"):
        assert again[k].tobytes() == outs["main"][k].tobytes(), k
        assert other[k].tobytes() == outs["main"][k].tobytes(), k


def test_graph_replay_equals_the_eager_call(device, outs, batches):
    batch = batches["capped"]
    t = [torch.from_numpy(batch[k]).to(device) for k in ("pts0", "pts1", "counts")]
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        sfm.two_view_verify_device(*t, **batch["options"])   # (the attribute call, outside capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = sfm.two_view_verify_device(*t, **batch["options"])
    for _ in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize(device)
        for o, k in zip(out, ("F", "mask", "n_inliers", "iters", "status")):
            assert o.cpu().numpy().tobytes() == outs["capped"][k].tobytes(), k


@pytest.mark.parametrize("change,text", [
    (dict(min_num_inliers=7), "min_num_inliers 7 below 8"),
    (dict(max_trials=0), "max_trials 0 below 1"),
    (dict(refine_iters=-1), "refine_iters -1"),
    (dict(confidence=1.0), "confidence"),
    (dict(max_error=float("nan")), "max_error"),
])
def test_refusals_leave_the_outputs_untouched(change, text, device, batches, lib):
    out = verify(device, batches["clamp"], **change)
    assert out["rc"] == 1 and text in lib.onepose_last_error().decode()
    for k in ("F", "mask", "n_inliers", "iters", "status"):   # Guarded fills with 0xA5
        assert (out[k].view(np.uint8) == 0xA5).all(), k


def test_max_points_is_checked_on_the_host(lib):
    P = lib.onepose_two_view_max_points()
    p = 0x1000   # never dereferenced: every call is refused before a launch
    def call(max_points, ws=p, wsb=1 << 20):
        return lib.onepose_two_view_verify(p, p, p, max_points, 1, None, 4.0, 0.999, 100, 15, 0.25,
                                           2, p, p, p, p, p, ws, wsb, None)
    assert call(P + 1) == 1 and b"onepose_two_view_max_points" in lib.onepose_last_error()
    assert call(0) == 1
    assert call(P, ws=None, wsb=0) == 4 and b"workspace" in lib.onepose_last_error()
    assert lib.onepose_twoview_version() == 1 and lib.onepose_abi_version() == 9


# ---- the Python layer and the chain ------------------------------------------------------------
def test_verify_matches_equals_its_host_path(device):
    feats, names, poses, Ks, pts, owner = sfm_cases.scene()
    pairs = sfm.covis_from_pose(names, poses, 10)[:24]
    matcher = C.Redirecting(nn_matcher.NearestNeighbour({"ratio_threshold": 0.8,
                                                        "distance_threshold": 0.7}), 0.05)
    matches = sfm.match_pairs(feats, pairs, matcher, device=device)
    for geometry in ("estimate", "poses"):
        kw = dict(geometry=geometry, poses=poses, Ks=Ks, img_lists=names)
        va, ra = sfm.verify_matches(pairs, matches, feats, device=device, **kw)
        vb, rb = sfm.verify_matches(pairs, matches, feats, device=None, **kw)
        assert list(va) == list(vb) == list(matches)
        for pair in va:
            for k in va[pair]:
                assert va[pair][k].dtype == vb[pair][k].dtype == matches[pair][k].dtype
                assert np.array_equal(va[pair][k], vb[pair][k]), (geometry, pair, k)
            for k in ("status", "n_matches", "n_inliers", "iters"):
                assert ra[pair][k] == rb[pair][k], (geometry, pair, k)
            dev = np.abs(O.normalised(ra[pair]["F"].reshape(9)) - O.normalised(rb[pair]["F"].reshape(9)))
            assert dev.max() <= float(GOLD["f_tol"])


@pytest.mark.parametrize("mode", ["poses", "estimate"])
def test_chain_equals_its_host_formulation(mode, device):
    """The chain on redirected matches with verification, on the GPU and on the host: the same
    tracks, the same kept set, the same xyz bits, and the scene's own bar."""
    feats, names, poses, Ks, pts, owner = sfm_cases.scene()
    nn = nn_matcher.NearestNeighbour({"ratio_threshold": 0.8, "distance_threshold": 0.7})
    gpu = sfm.reconstruct(feats, names, poses, Ks, C.Redirecting(nn, 0.02), covis_num=10,
                          device=device, verify=mode)
    host = sfm.reconstruct(feats, names, poses, Ks, C.Redirecting(nn, 0.02), covis_num=10,
                           device=None, match_device=device, verify=mode)
    for k in ("track_start", "obs_image", "obs_feat"):
        assert np.array_equal(gpu["tracks"][k], host["tracks"][k]), k
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(gpu["triangulation"][k], host["triangulation"][k]), k
    assert gpu["xyz"].tobytes() == host["xyz"].tobytes()
    for pair, r in gpu["two_view"].items():
        for k in ("status", "n_matches", "n_inliers", "iters"):
            assert r[k] == host["two_view"][pair][k], (pair, k)
    good = C.points_within_1mm(gpu, pts, owner)
    print(f"verify={mode}: {good} of {sfm_cases.SCENE_POINTS} scene points within 1 mm")
    assert good >= 0.9 * sfm_cases.SCENE_POINTS

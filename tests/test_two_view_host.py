"""Two-view verification on the host (no GPU): the oracle's known answers, the recorded results
against the oracle run afresh, the package's device=None path against the oracle, verify_matches'
bookkeeping, and the chain on sfm_cases.scene() with wrong matches.  Figures are printed
(pytest -s)."""
import os
import sys

import numpy as np
import pytest

import sfm_cases
import two_view_cases as C
import two_view_oracle as O
from conftest import GOLDEN, golden
from onepose_amd import _lib, sfm

GOLD = golden("two_view")


# ---- known answers ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_scenes():
    scenes = [C.scene(n, share, seed) for n, share, seed in C.HOST_SCENES]
    return scenes, [O.verify(s["pts0"], s["pts1"], **C.DEFAULTS) for s in scenes]


def test_the_oracle_finds_the_true_inliers(host_scenes):
    """0, 30 and 50 % outliers at 40, 130 and 300 matches: the mask is the true inlier set, no
    scene left out, and the clean points lie within 2 px of the returned F's epipolar lines (the
    noise is +-0.7 px per coordinate in both images)."""
    for (n, share, seed), s, r in zip(C.HOST_SCENES, *host_scenes):
        assert r["status"] == 0 and np.array_equal(r["mask"], s["inlier"]), (n, share)
        d1, d0 = C.line_dist(r["F"].reshape(3, 3), s["pts0"][s["inlier"]].astype(np.float64),
                             s["pts1"][s["inlier"]].astype(np.float64))
        print(f"n={n} outliers={share}: {r['iters']} iterations, largest epipolar distance of a "
              f"clean point {max(d1.max(), d0.max()):.2f} px")
        assert max(d1.max(), d0.max()) <= 2.0
        out = ~s["inlier"]
        if out.any():   # the outliers stay far from the estimated lines too
            o1, o0 = C.line_dist(r["F"].reshape(3, 3), s["pts0"][out].astype(np.float64),
                                 s["pts1"][out].astype(np.float64))
            assert np.minimum(o1, o0).min() > 4.0


def test_fundamental_from_poses():
    s = C.scene(50, 0.0, 5100)
    F = sfm.fundamental_from_poses(s["T0"], C.K, s["T1"], C.K)
    assert F.shape == (3, 3) and F.dtype == np.float64
    assert np.abs(O.normalised(F.reshape(9)) - O.normalised(s["F_true"].reshape(9))).max() <= 1e-12
    assert np.array_equal(F, sfm.fundamental_from_poses(s["T0"][:3], C.K, s["T1"][:3], C.K))
    d1, d0 = C.line_dist(F, s["pts0"].astype(np.float64), s["pts1"].astype(np.float64))
    assert max(d1.max(), d0.max()) <= 2.0   # x1^T F x0 = 0 up to the noise
    assert np.linalg.matrix_rank(F / np.abs(F).max(), tol=1e-9) == 2


# ---- the recorded results -----------------------------------------------------------------------
def _batches():
    return C.gpu_batches(int(GOLD["max_points"]))


def test_the_golden_file_equals_the_oracle_run_afresh():
    sys.path.insert(0, GOLDEN)
    import make_golden_two_view as G
    assert int(GOLD["max_points"]) == _lib.call("onepose_two_view_max_points") >= 4096
    for key, batch in _batches().items():
        assert C.sha(batch["pts0"], batch["pts1"], batch["counts"]) == str(GOLD[f"{key}_sha"]), key
        assert list(GOLD[f"{key}_names"]) == batch["names"]
        got = G.run_batch(batch)
        for k, v in got.items():
            assert v.dtype == GOLD[f"{key}_{k}"].dtype and v.tobytes() == GOLD[f"{key}_{k}"].tobytes(), (key, k)
    assert float(GOLD["f_tol"]) == max(16 * float(GOLD["f_dev"]), 1e-12)
    assert int(GOLD["f_same"]) >= 0.75 * int(GOLD["f_models"])


@pytest.mark.parametrize("key", ["main", "capped", "small", "clamp"])
def test_device_none_equals_the_oracle(key):
    """The package's host path (hypotheses solved in batches) makes the oracle's decisions on
    every recorded pair -- and, the operations being the same, gives its F bit for bit."""
    batch = _batches()[key]
    F, mask, nin, iters, status = sfm._host_two_view(batch["pts0"], batch["pts1"], batch["counts"],
                                                     None, **batch["options"])
    for k, v in (("status", status), ("n_inliers", nin), ("iters", iters), ("mask", mask)):
        assert v.dtype == GOLD[f"{key}_{k}"].dtype and np.array_equal(v, GOLD[f"{key}_{k}"]), k
    assert F.tobytes() == GOLD[f"{key}_F"].tobytes()
    F2, mask2, _, iters2, status2 = sfm._host_two_view(
        batch["pts0"], batch["pts1"], batch["counts"], GOLD[f"{key}_F"], **batch["options"])
    assert np.array_equal(mask2, GOLD[f"{key}_given_mask"]) and not iters2.any()
    assert np.array_equal(status2, GOLD[f"{key}_given_status"])
    assert F2.tobytes() == GOLD[f"{key}_F"].tobytes()


# ---- the options and the given-F edges ------------------------------------------------------------
OPT = golden("two_view_options")
OPTION_CALLS = C.option_calls()
FIELDS = ("F", "mask", "n_inliers", "iters", "status")


@pytest.mark.parametrize("key", list(OPTION_CALLS))
def test_the_option_fixture_equals_the_oracle_and_the_host_path(key):
    """two_view_options.npz against the oracle run afresh, and the package's host path against
    both: decisions equal and F bit for bit, a given F with a NaN entry included."""
    sys.path.insert(0, GOLDEN)
    import make_golden_two_view_options as G
    call = OPTION_CALLS[key]
    assert list(OPT["calls"]) == list(OPTION_CALLS)
    assert C.option_sha(call) == str(OPT[f"{key}_sha"]) and list(OPT[f"{key}_names"]) == call["names"]
    got = G.run_call(call)
    host = dict(zip(FIELDS, sfm._host_two_view(call["pts0"], call["pts1"], call["counts"],
                                               call.get("F_in"), **call["options"])))
    for k in FIELDS:
        want = OPT[f"{key}_{k}"]
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), (key, k)
        assert host[k].dtype == want.dtype and host[k].tobytes() == want.tobytes(), (key, k)
    if "F_in" in call:
        assert host["F"].tobytes() == call["F_in"].tobytes()
    assert float(OPT["f_tol"]) == max(16 * float(OPT["f_dev"]), 1e-12)
    assert int(OPT["f_same"]) >= 0.75 * int(OPT["f_models"])


def test_device_none_equals_the_oracle_on_the_known_answers(host_scenes):
    scenes, want = host_scenes
    P = max(len(s["pts0"]) for s in scenes)
    p0, p1 = np.zeros((len(scenes), P, 2), np.float32), np.zeros((len(scenes), P, 2), np.float32)
    for b, s in enumerate(scenes):
        p0[b, :len(s["pts0"])], p1[b, :len(s["pts1"])] = s["pts0"], s["pts1"]
    counts = np.array([len(s["pts0"]) for s in scenes], np.int32)
    F, mask, nin, iters, status = sfm._host_two_view(p0, p1, counts, None, **C.DEFAULTS)
    for b, r in enumerate(want):
        assert (status[b], nin[b], iters[b]) == (r["status"], r["n_inliers"], r["iters"])
        assert np.array_equal(mask[b, :counts[b]].astype(bool), r["mask"]) and not mask[b, counts[b]:].any()
        assert F[b].tobytes() == r["F"].tobytes()


# ---- verify_matches' bookkeeping ----------------------------------------------------------------
class StubPairs:
    """Three images; pair (0, 1) carries a scene's matches among unmatched features, pair (0, 2)
    has too few matches, pair (1, 2) unrelated points."""

    def __init__(self):
        s = C.scene(60, 0.25, 5200)
        rng = np.random.default_rng(5)
        self.scene = s
        n0, n1 = 90, 75
        self.i0 = np.sort(rng.permutation(n0)[:60])
        self.i1 = rng.permutation(n1)[:60]
        kp = [rng.uniform(10, 500, (n, 2)).astype(np.float32) for n in (n0, n1, 70)]
        kp[0][self.i0] = s["pts0"] - np.float32(0.5)
        kp[1][self.i1] = s["pts1"] - np.float32(0.5)
        self.names = [f"o/c/{k}.png" for k in range(3)]
        self.features = {n: {"keypoints": k, "image_size": np.array([512, 512])}
                         for n, k in zip(self.names, kp)}
        self.pairs = [(self.names[0], self.names[1]), (self.names[0], self.names[2]),
                      (self.names[1], self.names[2]), (self.names[1], self.names[0])]

        def group(n_a, n_b, ia, ib):
            m0, m1 = np.full(n_a, -1, np.int16), np.full(n_b, -1, np.int16)
            m0[ia], m1[ib] = ib, ia
            return {"matches0": m0, "matches1": m1,
                    "matching_scores0": rng.random(n_a).astype(np.float16),
                    "matching_scores1": rng.random(n_b).astype(np.float16)}
        few = np.arange(9)
        rnd = rng.permutation(70)[:40]
        self.matches = {
            sfm.names_to_pair(*self.pairs[0]): group(n0, n1, self.i0, self.i1),
            sfm.names_to_pair(*self.pairs[1]): group(n0, 70, few, few + 3),
            sfm.names_to_pair(*self.pairs[2]): group(n1, 70, np.arange(40), rnd)}


def test_verify_matches_bookkeeping():
    st = StubPairs()
    before = {p: {k: v.copy() for k, v in g.items()} for p, g in st.matches.items()}
    verified, report = sfm.verify_matches(st.pairs, st.matches, st.features, device=None)
    for p, g in st.matches.items():   # the input is untouched
        for k in g:
            assert np.array_equal(g[k], before[p][k]) and verified[p][k] is not g[k]
    assert list(verified) == list(st.matches) == list(report)
    for p in verified:   # keys, dtypes, shapes; scores untouched
        assert set(verified[p]) == set(st.matches[p])
        for k, v in verified[p].items():
            assert v.dtype == st.matches[p][k].dtype and v.shape == st.matches[p][k].shape
            if k.startswith("matching_scores"):
                assert np.array_equal(v, st.matches[p][k])
    p01, p02, p12 = list(st.matches)
    r = report[p01]
    assert set(r) == {"status", "n_matches", "n_inliers", "iters", "F"} and r["F"].shape == (3, 3)
    assert (r["status"], r["n_matches"], r["n_inliers"]) == (0, 60, int(st.scene["inlier"].sum()))
    want0 = st.matches[p01]["matches0"].copy()
    want0[st.i0[~st.scene["inlier"]]] = -1
    want1 = st.matches[p01]["matches1"].copy()
    want1[st.i1[~st.scene["inlier"]]] = -1
    assert np.array_equal(verified[p01]["matches0"], want0)
    assert np.array_equal(verified[p01]["matches1"], want1)
    assert report[p02]["status"] == 1 and report[p02]["n_matches"] == 9 and report[p02]["iters"] == 0
    assert report[p12]["status"] in (2, 3) and report[p12]["n_matches"] == 40
    for p in (p02, p12):   # a pair that is not verified loses every match
        assert (verified[p]["matches0"] == -1).all() and (verified[p]["matches1"] == -1).all()
    # the oracle on the packed points of the first pair
    o = O.verify(st.scene["pts0"], st.scene["pts1"], **C.DEFAULTS)
    assert (o["status"], o["n_inliers"], o["iters"]) == (r["status"], r["n_inliers"], r["iters"])
    assert r["F"].tobytes() == o["F"].tobytes()
    # the given geometry
    T = np.stack([st.scene["T0"], st.scene["T1"], st.scene["T1"]])
    Ks = np.stack([C.K] * 3)
    v2, r2 = sfm.verify_matches(st.pairs[:1], st.matches, st.features, geometry="poses", poses=T,
                                Ks=Ks, img_lists=st.names, device=None)
    assert list(r2) == [p01] and r2[p01]["iters"] == 0 and r2[p01]["status"] == 0
    assert np.array_equal(v2[p01]["matches0"], want0)
    assert np.array_equal(v2[p02]["matches0"], st.matches[p02]["matches0"])   # not in `pairs`: copied
    with pytest.raises(ValueError):
        sfm.verify_matches(st.pairs, st.matches, st.features, geometry="poses", device=None)
    with pytest.raises(ValueError):
        sfm.verify_matches(st.pairs, st.matches, st.features, geometry="homography", device=None)
    with pytest.raises(_lib.OnePoseError):
        sfm.verify_matches(st.pairs, st.matches, st.features, min_num_inliers=7, device=None)


def test_the_binding_reads_the_family_header():
    sig = _lib.FAMILY_SIGNATURES
    assert set(sig) == {"onepose_twoview_version", "onepose_two_view_max_points",
                        "onepose_two_view_workspace_bytes", "onepose_two_view_verify"}
    assert not set(sig) & set(_lib.SIGNATURES)
    names = [n for n, _ in sig["onepose_two_view_verify"][1]]
    assert names[:6] == ["pts0", "pts1", "counts", "max_points", "batch", "F_in"] and len(names) == 20
    lib = _lib.load()
    assert lib.onepose_twoview_version() == 1 and lib.onepose_abi_version() == 9
    assert _lib.call("onepose_two_view_workspace_bytes", batch=0, max_points=10) == 0
    assert _lib.call("onepose_two_view_workspace_bytes", batch=3, max_points=10) > 0
    header = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "onepose_two_view.h")).read()
    assert "NOT verified and is not claimed" in header


# ---- the chain ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains():
    feats, names, poses, Ks, pts, owner = sfm_cases.scene()
    out = {}
    for mode in (None, "poses", "estimate"):
        out[mode] = sfm.reconstruct(feats, names, poses, Ks, C.Redirecting(C.OracleNN(), 0.02),
                                    covis_num=10, device=None, verify=mode)
    return pts, owner, out


def test_wrong_matches_ruin_the_chain_and_verification_restores_it(chains):
    """2 % of every pair's matches redirected: without verification fewer than half of the 200
    points survive within 1 mm; with either geometry the chain meets its own bar of 90 %."""
    pts, owner, out = chains
    good = {mode: C.points_within_1mm(m, pts, owner) for mode, m in out.items()}
    print(f"scene points within 1 mm, of {sfm_cases.SCENE_POINTS}: {good}")
    assert good[None] < 0.5 * sfm_cases.SCENE_POINTS
    assert good["poses"] >= 0.9 * sfm_cases.SCENE_POINTS
    assert good["estimate"] >= 0.9 * sfm_cases.SCENE_POINTS
    assert "two_view" not in out[None]
    for mode in ("poses", "estimate"):
        rep = out[mode]["two_view"]
        assert len(rep) == len({frozenset(p) for p in out[mode]["pairs"]})
        assert all(r["status"] == 0 for r in rep.values())
        assert all((r["iters"] == 0) == (mode == "poses") for r in rep.values())


def test_verify_none_is_the_chain_as_it_was():
    feats, names, poses, Ks, pts, owner = sfm_cases.scene()
    a = sfm.reconstruct(feats, names, poses, Ks, C.OracleNN(), covis_num=10, device=None)
    b = sfm.reconstruct(feats, names, poses, Ks, C.OracleNN(), covis_num=10, device=None, verify=None)
    assert set(a) == set(b)
    for k in ("xyz", "error", "track_len", "ids"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("track_start", "obs_image", "obs_feat"):
        assert np.array_equal(a["tracks"][k], b["tracks"][k])
    for k in ("reason", "n_kept", "obs_keep"):
        assert np.array_equal(a["triangulation"][k], b["triangulation"][k])
    for x, y in zip(a["point3D_ids"], b["point3D_ids"]):
        assert np.array_equal(x, y)

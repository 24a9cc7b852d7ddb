"""NearestNeighbour matcher, host side (no GPU): the numpy oracle against the reference-generated
fixtures and on constructed ties, the library's version / workspace / argument checks (all before
any launch), and the module's CPU refusal and conf merge."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import nn_oracle as oracle
import parity
from onepose_amd import _lib, nn_matcher, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("nn_s", "nn_m", "nn_b3")
KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")
OK, INVALID, WORKSPACE = 0, 1, 4   # ONEPOSE_OK, ONEPOSE_ERR_INVALID, ONEPOSE_ERR_WORKSPACE


def load_case(name):
    """(fixture, configurations, inputs) regenerated from the fixture's seed, digest checked."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n0, n1, batch, shared1, d = (int(x) for x in g["shape"])
    data = synthetic.make_nn_inputs(n0, n1, int(g["input_seed"]), batch=batch,
                                    shared1=bool(shared1), d=d)
    h = hashlib.sha256()
    for k in sorted(data):
        h.update(np.ascontiguousarray(data[k]).tobytes())
    assert h.hexdigest() == str(g["inputs_sha"]), "synthetic inputs changed"
    return g, json.loads(str(g["configs"])), data


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_fixture(name):
    g, configs, data = load_case(name)
    assert len(configs) == 4
    for i, conf in enumerate(configs):
        out = oracle.from_conf(data["descriptors0"], data["descriptors1"], conf)
        assert oracle.well_separated(out)
        for b in range(out["matches0"].shape[0]):
            got = {k: out[k][b] for k in KEYS}
            ref = {k: g[f"c{i}_{k}"][b] for k in KEYS}
            assert parity.assert_pred_equal(got, ref, f"{name} c{i} [{b}]") == 0
            assert (ref["matches0"] > -1).mean() >= 0.15


def test_fixture_dtypes():
    g, _, _ = load_case("nn_s")
    assert g["c0_matches0"].dtype == np.int64 and g["c0_matches1"].dtype == np.int64
    assert g["c0_matching_scores0"].dtype == np.float32
    assert g["c0_matches0"].shape == (1, 65) and g["c0_matches1"].shape == (1, 33)


def test_oracle_ties_duplicated_columns():
    d = synthetic.make_nn_inputs(6, 5, 0, d=16)
    d0, d1 = d["descriptors0"].copy(), d["descriptors1"].copy()
    d1[:, :, 3] = d1[:, :, 1]                    # columns 1 and 3 of side 1 are bit-equal
    d0[:, :, 2] = d1[0, :, 1]                    # row 2's best is that column, twice
    out = oracle.forward(d0, d1, mutual=False)
    assert out["matches0"][0, 2] == 1            # the lowest index
    assert out["gap0"][0, 2] == 0.0              # the duplicate is its own runner-up
    assert out["matches1"][0, 1] == out["matches1"][0, 3]
    # with a ratio test the duplicated best fails it: dist_best <= r^2 dist_best only at <= 0
    r = oracle.forward(d0, d1, ratio=0.9, mutual=False)
    assert r["matches0"][0, 2] == -1 and r["matching_scores0"][0, 2] == 0


def test_oracle_all_equal_descriptors():
    v = np.full((1, 8, 1), np.float32(0.25))
    d0, d1 = np.repeat(v, 7, axis=2), np.repeat(v, 5, axis=2)
    out = oracle.forward(d0, d1)
    assert np.array_equal(out["matches1"][0], np.zeros(5, np.int64))
    assert np.array_equal(out["matches0"][0], np.array([0] + [-1] * 6))
    raw = oracle.forward(d0, d1, mutual=False)
    assert np.array_equal(raw["matches0"][0], np.zeros(7, np.int64))
    assert np.all(out["matching_scores0"] == out["matching_scores0"][0, 0])   # not zeroed


def test_oracle_zero_thresholds_are_none():
    d = synthetic.make_nn_inputs(20, 17, 1, d=32)
    a = oracle.forward(d["descriptors0"], d["descriptors1"], ratio=0, distance=0)
    b = oracle.forward(d["descriptors0"], d["descriptors1"], ratio=None, distance=None)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    c = oracle.forward(d["descriptors0"], d["descriptors1"], ratio=0.8, distance=0.7)
    assert (c["matches1"] > -1).sum() < (b["matches1"] > -1).sum()
    with pytest.raises(RuntimeError):
        oracle.forward(d["descriptors0"], d["descriptors1"][:, :, :1], ratio=0.8)


def test_versions(lib):
    assert lib.onepose_nn_version() == 1 == nn_matcher.NN_VERSION
    assert lib.onepose_abi_version() == 9


def test_workspace_bytes(lib):
    wb = lib.onepose_nn_match_workspace_bytes
    for bad in ((0, 5, 5), (1, 0, 5), (1, 5, 0), (1, 16385, 5), (1, 5, 16385), (-1, 5, 5)):
        assert wb(*bad) == 0, bad
    assert wb(1, 1, 1) > 0 and wb(1, 16384, 16384) > 0
    sizes = (1, 2, 63, 64, 65, 127, 128, 129, 300, 4096, 16384)
    for fixed in (1, 130):
        prev = [0, 0, 0]
        for s in sizes:
            cur = [wb(s, fixed, fixed), wb(2, s, fixed), wb(2, fixed, s)]
            assert all(c >= p and c > 0 for c, p in zip(cur, prev)), (s, cur, prev)
            prev = cur


def _match(lib, d0=256, d1=256, dtype=0, batch=1, d=256, n0=5, n1=6, ratio=0.0, dist=0.0, m0=256,
           m1=256, s0=256, s1=256, ws=256, ws_bytes=1 << 40, bs0=0, bs1=0):
    """onepose_nn_match with dummy (never dereferenced) pointers: every refusal below happens on
    the host before anything is launched."""
    return lib.onepose_nn_match(d0, bs0, d1, bs1, dtype, batch, d, n0, n1, ratio, dist, 1,
                                m0, m1, s0, s1, ws, ws_bytes, None)


def test_bad_arguments_are_refused_on_the_host(lib):
    err = lambda: lib.onepose_last_error().decode()
    for kw in ({"d0": None}, {"d1": None}, {"m0": None}, {"m1": None}, {"s0": None},
               {"s1": None}, {"ws": None}):
        assert _match(lib, **kw) == INVALID and "null" in err(), kw
    assert _match(lib, batch=0) == INVALID and "batch" in err()
    for kw in ({"n0": 0}, {"n1": 0}, {"n0": 16385}, {"n1": 16385}, {"n0": -3}):
        assert _match(lib, **kw) == INVALID and "n0" in err(), kw
    for dd in (0, 1025, -1):
        assert _match(lib, d=dd) == INVALID and "d =" in err()
    for dt in (2, -1):
        assert _match(lib, dtype=dt) == INVALID and "dtype" in err()
    assert _match(lib, bs0=-1) == INVALID and "stride" in err()
    assert _match(lib, n1=1, ratio=0.8) == INVALID and "ratio" in err()
    assert _match(lib, n0=1, ratio=0.8) == INVALID and "ratio" in err()
    assert _match(lib, ws_bytes=16) == WORKSPACE and "needed" in err()
    assert _match(lib, ws_bytes=lib.onepose_nn_match_workspace_bytes(1, 5, 6) - 1) == WORKSPACE


def test_refusals_come_in_the_documented_order(lib):
    """null pointers, batch, n0 / n1, d, dtype, strides, the ratio test's candidates, workspace:
    a call wrong in several ways reports the first."""
    err = lambda: lib.onepose_last_error().decode()
    wrong = dict(d0=None, batch=0, n0=0, d=0, dtype=7, bs0=-1, ratio=0.8, ws_bytes=0)
    for key, word in (("d0", "null"), ("batch", "batch"), ("n0", "n0"), ("d", "d ="),
                      ("dtype", "dtype"), ("bs0", "stride")):
        assert _match(lib, **wrong) == INVALID and word in err(), (key, err())
        del wrong[key]
    assert _match(lib, n1=1, **wrong) == INVALID and "ratio" in err()
    assert _match(lib, **wrong) == WORKSPACE
    # a threshold that is not > 0, or NaN, is no test: one candidate is then enough
    for r in (0.0, -1.0, float("nan")):
        assert _match(lib, n1=1, ratio=r, ws_bytes=0) == WORKSPACE


def test_similarity_entry_checks(lib):
    f = lib.onepose_nn_similarity_top2
    assert f(None, 0, 256, 0, 0, 1, 256, 5, 6, 256, 1 << 40, None) == INVALID
    assert f(256, 0, 256, 0, 0, 1, 256, 5, 6, 256, 16, None) == WORKSPACE


def test_cpu_forward_raises():
    d = synthetic.make_nn_inputs(8, 9, 0)
    m = nn_matcher.NearestNeighbour()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m({k: torch.as_tensor(v) for k, v in d.items()})
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        nn_matcher.nearest_neighbour_match(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def test_conf_merge():
    ref_default = {"match_threshold": None, "ratio_threshold": None, "distance_threshold": None,
                   "do_mutual_check": True}
    assert nn_matcher.NearestNeighbour.default_conf == ref_default
    assert nn_matcher.NearestNeighbour().conf == ref_default
    assert nn_matcher.NearestNeighbour({}).conf == ref_default
    conf = {"ratio_threshold": 0.8, "extra": 1}
    assert nn_matcher.NearestNeighbour(conf).conf == {**ref_default, **conf}

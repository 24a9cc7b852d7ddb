"""NearestNeighbour matcher on the GPU: the reference's fixtures end to end, ragged shapes, non-unit
descriptors, ties, shared sides, fp16, determinism / streams / graphs and buffer bounds, against
tests/nn_oracle.py.

Inputs are chosen on the CPU by a bounded seed search (at most 32 seeds) so that, in float64,
every row's and column's best-minus-second gap is >= 2e-5 x scale and every enabled decision is
>= 1e-3 x scale from its boundary (scale = max(1, largest |sim|); the fp32 similarity differs
from float64 by under 5e-7 x scale at d = 256).  Indices must then be equal everywhere, with no
exemption, and scores within parity.ATOL x scale.

d = 1 is the one shape where that gap cannot exist: a unit-norm scalar is +-1, every similarity
is exactly +-1 and most rows tie.  There both sides compute the similarity exactly (one product,
no sum), so the indices are pinned by the tie rule itself and the gap bound is not applied; the
ratio test (which a tie puts exactly on its boundary) is left off and the distance test stays.
"""
import functools

import numpy as np
import pytest
import torch

import nn_oracle as oracle
import parity
from onepose_amd import _lib, nn_matcher, synthetic
from test_nn_host import CASES, KEYS, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MAX_SEEDS = 32
# The kernel as built: 32 x 32 MFMA blocks, 64 x 64 partial blocks, 128 x 128 workgroup tiles, K
# staged 32 rows at a time in steps of 2.  Each has sizes one below, at and one above it; 257
# spans three workgroup tiles; d = 1, 31, 32, 33, 37 walk the K edges.
RAGGED = [(1, 1, 256), (1, 2, 256), (2, 1, 256), (2, 129, 256), (31, 32, 32), (32, 31, 33),
          (63, 65, 256), (64, 64, 256), (127, 128, 256), (129, 127, 256), (257, 130, 256),
          (130, 257, 128), (97, 66, 37), (33, 40, 1), (33, 40, 31)]


def gpu_match(d0, d1, ratio=None, distance=None, mutual=True):
    t0 = d0 if torch.is_tensor(d0) else torch.from_numpy(np.ascontiguousarray(d0)).to(DEV)
    t1 = d1 if torch.is_tensor(d1) else torch.from_numpy(np.ascontiguousarray(d1)).to(DEV)
    out = nn_matcher.nearest_neighbour_match(t0, t1, ratio, distance, mutual)
    torch.cuda.synchronize()
    return dict(zip(KEYS, (o.cpu().numpy() for o in out)))


def assert_equal_to_oracle(got, ref, what, scale=1.0):
    for b in range(ref["matches0"].shape[0]):
        n = parity.assert_pred_equal({k: got[k][b] for k in KEYS}, {k: ref[k][b] for k in KEYS},
                                     f"{what} [{b}]", atol=parity.ATOL * scale)
        assert n == 0


def assert_bit_equal(a, b, what):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{what}: {k}"


def search(make, ratio, distance, ties=False):
    """The first of MAX_SEEDS inputs make(seed) that meets the selection bounds under (ratio,
    distance); with `ties`, gaps of exactly equal similarities (< 1e-12) are allowed."""
    for seed in range(MAX_SEEDS):
        d0, d1 = make(seed)
        o = oracle.forward(d0, d1, ratio, distance)
        s = o["scale"]
        gaps = np.concatenate([o["gap0"].ravel(), o["gap1"].ravel()])
        if ties:
            gaps = gaps[gaps > 1e-12]
        slack = min(o["slack0"].min(), o["slack1"].min())
        if (gaps.size == 0 or gaps.min() >= 2e-5 * s) and slack >= 1e-3 * s:
            return d0, d1
    raise AssertionError("no seed meets the selection bounds")


@functools.lru_cache(maxsize=None)
def ragged_inputs(n0, n1, d):
    ratio = 0.8 if min(n0, n1) >= 2 and d > 1 else None

    def make(seed):
        x = synthetic.make_nn_inputs(n0, n1, 1000 + seed, d=d)
        return x["descriptors0"], x["descriptors1"]

    if d == 1:   # see the module docstring: exact similarities, ties by rule
        d0, d1 = make(0)
        o = oracle.forward(d0, d1, None, 0.7)
        assert min(o["slack0"].min(), o["slack1"].min()) >= 1e-3
        return d0, d1, None, 0.7
    d0, d1 = search(make, ratio, 0.7)
    return d0, d1, ratio, 0.7


# ---------------------------------------------------------------- 1. fixtures
@pytest.mark.parametrize("name", CASES)
def test_fixtures_end_to_end(name):
    g, configs, data = load_case(name)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in data.items()}
    t["keypoints0"] = torch.zeros(1, 3, 2, device=DEV)   # other keys are ignored
    for i, conf in enumerate(configs):
        out = nn_matcher.NearestNeighbour(conf)(t)
        assert set(out) == set(KEYS)
        for k in KEYS:
            assert out[k].device == t["descriptors0"].device
            assert out[k].dtype == (torch.int64 if k.startswith("matches") else torch.float32)
            assert tuple(out[k].shape) == g[f"c{i}_{k}"].shape
        got = {k: out[k].cpu().numpy() for k in KEYS}
        assert_equal_to_oracle(got, {k: g[f"c{i}_{k}"] for k in KEYS}, f"{name} c{i}")


# ---------------------------------------------------------------- 2. ragged shapes
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("n0,n1,d", RAGGED)
def test_ragged_shapes(n0, n1, d, mutual):
    d0, d1, ratio, distance = ragged_inputs(n0, n1, d)
    ref = oracle.forward(d0, d1, ratio, distance, mutual)
    assert_equal_to_oracle(gpu_match(d0, d1, ratio, distance, mutual), ref, f"{n0}x{n1}x{d}")
    ref = oracle.forward(d0, d1, None, None, mutual)
    assert_equal_to_oracle(gpu_match(d0, d1, None, None, mutual), ref, f"{n0}x{n1}x{d} plain")


def test_ratio_test_with_one_candidate_raises():
    d0, d1 = torch.zeros(1, 8, 4, device=DEV), torch.zeros(1, 8, 1, device=DEV)
    with pytest.raises(RuntimeError, match="ratio"):
        nn_matcher.nearest_neighbour_match(d0, d1, ratio=0.8)
    with pytest.raises(RuntimeError, match="ratio"):
        nn_matcher.NearestNeighbour({"ratio_threshold": 0.8})({"descriptors0": d1,
                                                              "descriptors1": d0})


# ---------------------------------------------------------------- 3. non-unit descriptors
def test_non_unit_descriptors():
    def make(seed):
        x = synthetic.make_nn_inputs(97, 66, 2000 + seed)
        return x["descriptors0"] * np.float32(3), x["descriptors1"] * np.float32(0.5)

    for ratio, distance in ((0.8, 0.7), (None, None)):
        d0, d1 = search(make, ratio, distance)
        ref = oracle.forward(d0, d1, ratio, distance)
        sims = oracle.similarities(d0, d1)
        assert sims.max() > 1.0 and 2 * (1 - sims.max()) < 0      # outside [-1, 1], dist < 0
        scale = 3 * 0.5          # the similarities' scale: |sim| <= 3 x 0.5 x (1 + rounding)
        assert ref["scale"] <= scale * (1 + 1e-5)
        assert_equal_to_oracle(gpu_match(d0, d1, ratio, distance), ref, "non-unit", scale=scale)


# ---------------------------------------------------------------- 4. ties
def test_duplicates_across_tiles():
    """Bit-equal columns of side 1 (3 = 70 = 129: another 64-block, another 128-tile) and of side
    0 (5 = 66 = 128); row 10 / column 20 have such a duplicated best.  The lowest index must win,
    which also needs the sum over d to run in the same order in every tile."""
    def make(seed):
        x = synthetic.make_nn_inputs(130, 130, 3000 + seed)
        d0, d1 = x["descriptors0"].copy(), x["descriptors1"].copy()
        d1[:, :, 70] = d1[:, :, 129] = d1[:, :, 3]
        d0[:, :, 66] = d0[:, :, 128] = d0[:, :, 5]
        d0[:, :, 10] = d1[:, :, 3]
        d1[:, :, 20] = d0[:, :, 5]
        return d0, d1

    d0, d1 = search(make, None, None, ties=True)
    for mutual in (True, False):
        ref = oracle.forward(d0, d1, mutual=mutual)
        got = gpu_match(d0, d1, mutual=mutual)
        assert_equal_to_oracle(got, ref, "duplicates")
        assert got["matches1"][0, 20] == 5
    assert ref["matches0"][0, 10] == 3 and got["matches0"][0, 10] == 3
    assert got["matches1"][0, 3] == got["matches1"][0, 70] == got["matches1"][0, 129]


def test_all_equal_descriptors():
    v = synthetic.make_nn_inputs(1, 1, 5)["descriptors0"]          # [1, 256, 1]
    d0, d1 = np.repeat(v, 130, axis=2), np.repeat(v, 130, axis=2)
    got = gpu_match(d0, d1)
    assert np.array_equal(got["matches1"][0], np.zeros(130, np.int64))
    assert np.array_equal(got["matches0"][0], np.array([0] + [-1] * 129))
    assert np.all(got["matching_scores0"] == got["matching_scores0"][0, 0])
    assert np.all(got["matching_scores0"] > 0)                     # not zeroed by the mutual check
    assert_equal_to_oracle(got, oracle.forward(d0, d1), "all equal")
    raw = gpu_match(d0, d1, mutual=False)
    assert np.array_equal(raw["matches0"][0], np.zeros(130, np.int64))


def test_all_negative_similarities_at_a_ragged_edge():
    """Zero-padded rows and columns have similarity 0, above every real one here."""
    def make(seed):
        rs = np.random.RandomState(4000 + seed)
        a = np.abs(rs.standard_normal((1, 256, 130)))
        b = np.abs(rs.standard_normal((1, 256, 67)))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        return (-a).astype(np.float32), b.astype(np.float32)

    d0, d1 = search(make, None, None)
    assert oracle.similarities(d0, d1).max() < 0
    for mutual in (True, False):
        ref = oracle.forward(d0, d1, mutual=mutual)
        assert (ref["matches1"] > -1).all()
        assert_equal_to_oracle(gpu_match(d0, d1, mutual=mutual), ref, "negative")


# ---------------------------------------------------------------- 5. shared side
def test_shared_side_equals_materialised_batch():
    x = synthetic.make_nn_inputs(130, 200, 7, batch=3, shared1=True)
    d0 = torch.from_numpy(x["descriptors0"]).to(DEV)
    d1 = torch.from_numpy(x["descriptors1"]).to(DEV)
    assert d1.shape[0] == 1
    full = gpu_match(d0, d1.expand(3, -1, -1).contiguous(), 0.8, 0.7)
    assert_bit_equal(gpu_match(d0, d1, 0.8, 0.7), full, "batch dimension 1")
    assert_bit_equal(gpu_match(d0, d1.expand(3, -1, -1), 0.8, 0.7), full, "stride 0")
    # side 0 shared: one set of 200 against three of 130
    full = gpu_match(d1.expand(3, -1, -1).contiguous(), d0, 0.8, 0.7)
    assert_bit_equal(gpu_match(d1, d0, 0.8, 0.7), full, "side 0 shared")
    assert full["matches0"].shape == (3, 200) and full["matches1"].shape == (3, 130)


# ---------------------------------------------------------------- 6. fp16
def test_fp16_equals_fp32_on_upcast_inputs():
    x = synthetic.make_nn_inputs(129, 67, 8, batch=2, d=37)
    h0 = torch.from_numpy(x["descriptors0"]).to(DEV).half()
    h1 = torch.from_numpy(x["descriptors1"]).to(DEV).half()
    for ratio, distance in ((0.8, 0.7), (None, None)):
        assert_bit_equal(gpu_match(h0, h1, ratio, distance),
                         gpu_match(h0.float(), h1.float(), ratio, distance), "fp16")


# ---------------------------------------------------------------- 7. determinism, reentrancy
def test_repeat_streams_and_graph():
    x = synthetic.make_nn_inputs(300, 257, 9)
    y = synthetic.make_nn_inputs(257, 300, 10)
    tx = [torch.from_numpy(x[k]).to(DEV) for k in ("descriptors0", "descriptors1")]
    ty = [torch.from_numpy(y[k]).to(DEV) for k in ("descriptors0", "descriptors1")]
    ex, ey = gpu_match(*tx, 0.8, 0.7), gpu_match(*ty, 0.8, 0.7)
    assert_bit_equal(gpu_match(*tx, 0.8, 0.7), ex, "second call")
    # two streams, a workspace each (the module keys its workspaces by stream)
    sa, sb = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    outs = []
    for s, t in ((sa, tx), (sb, ty), (sa, tx), (sb, ty)):
        with torch.cuda.stream(s):
            outs.append(nn_matcher.nearest_neighbour_match(*t, 0.8, 0.7))
    torch.cuda.synchronize()
    for o, e in zip(outs, (ex, ey, ex, ey)):
        assert_bit_equal(dict(zip(KEYS, (v.cpu().numpy() for v in o))), e, "streams")
    # a captured graph, replayed
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        nn_matcher.nearest_neighbour_match(*tx, 0.8, 0.7)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = nn_matcher.nearest_neighbour_match(*tx, 0.8, 0.7)
    for _ in range(3):
        for o in out:
            o.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert_bit_equal(dict(zip(KEYS, (v.cpu().numpy() for v in out))), ex, "graph replay")


# ---------------------------------------------------------------- 8. bounds
def test_outputs_fully_written_and_nothing_outside():
    B, n0, n1, d, PAD = 2, 129, 67, 37, 64
    x = synthetic.make_nn_inputs(n0, n1, 11, batch=B, d=d)
    d0 = torch.from_numpy(x["descriptors0"]).to(DEV)
    d1 = torch.from_numpy(x["descriptors1"]).to(DEV)
    lib = _lib.load()
    need = lib.onepose_nn_match_workspace_bytes(B, n0, n1)
    WPAD = PAD * 16                                    # 64 partial records on each side
    ws = torch.full((need + 2 * WPAD,), 0xA5, dtype=torch.uint8, device=DEV)
    m0 = torch.full((B * n0 + 2 * PAD,), -7, dtype=torch.int64, device=DEV)
    m1 = torch.full((B * n1 + 2 * PAD,), -7, dtype=torch.int64, device=DEV)
    s0 = torch.full((B * n0 + 2 * PAD,), -5.0, dtype=torch.float32, device=DEV)
    s1 = torch.full((B * n1 + 2 * PAD,), -5.0, dtype=torch.float32, device=DEV)
    rc = lib.onepose_nn_match(d0.data_ptr(), d * n0, d1.data_ptr(), d * n1, _lib.DT_F32, B, d, n0,
                              n1, 0.8, 0.7, 1, m0[PAD:].data_ptr(), m1[PAD:].data_ptr(),
                              s0[PAD:].data_ptr(), s1[PAD:].data_ptr(), ws[WPAD:].data_ptr(), need,
                              _lib.stream_ptr(DEV))
    _lib.check(rc, "onepose_nn_match")
    torch.cuda.synchronize()
    for t, fill in ((m0, -7), (m1, -7), (s0, -5.0), (s1, -5.0)):
        assert (t[:PAD] == fill).all() and (t[-PAD:] == fill).all()
        assert (t[PAD:-PAD] != fill).all()             # matches >= -1, scores >= 0: all written
    assert (ws[:WPAD] == 0xA5).all() and (ws[-WPAD:] == 0xA5).all()
    got = {"matches0": m0[PAD:-PAD].view(B, n0), "matches1": m1[PAD:-PAD].view(B, n1),
           "matching_scores0": s0[PAD:-PAD].view(B, n0), "matching_scores1": s1[PAD:-PAD].view(B, n1)}
    assert_bit_equal({k: v.cpu().numpy() for k, v in got.items()}, gpu_match(d0, d1, 0.8, 0.7),
                     "direct call")

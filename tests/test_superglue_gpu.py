"""SuperGlue matcher on the GPU: the forward against the reference-generated fixtures and the
float64 oracle, the two new kernels (softmax attention, log-domain optimal transport) alone at
edge shapes, determinism, stream reentrancy, graph capture and the shared-side batch stride.

Bounds that are not the project's index / score contract (tests/parity.py) are built from the
error an fp32 evaluation of the same formula on the CPU makes against the float64 oracle: two
fp32 evaluations in different summation orders are each within e of the truth, hence at most
2e apart, and a further factor 2 covers the exp / log implementations: GPU error <= 4 e_cpu.
"""
import os

import numpy as np
import pytest
import torch

import parity
import superglue_oracle as oracle
from onepose_amd import _lib, superglue, synthetic
from test_superglue_host import CASES, T_BIN_SCORE, load_case

pytestmark = pytest.mark.gpu
KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")


def to_dev(data, device, expand=True):
    """The data dict on the device; a side with batch dimension 1 is expanded (stride 0)."""
    B = max(v.shape[0] for v in data.values())
    out = {}
    for k, v in data.items():
        t = torch.as_tensor(v).to(device)
        if expand and t.shape[0] != B:
            t = t.expand(B, *t.shape[1:])
        out[k] = t
    return out


def model_for(sd, device, iters, thr=0.2):
    return superglue.from_state_dict(sd, {"sinkhorn_iterations": iters,
                                          "match_threshold": thr}).to(device)


def run(model, data, log_assignment=True):
    out = model(data, return_log_assignment=log_assignment)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = load_case(name)
    return _cache[name]


def oracle_m():
    """The oracle's forward of superglue_m's inputs with every intermediate (computed once)."""
    if "oracle_m" not in _cache:
        _, sd, data = case("superglue_m")
        _cache["oracle_m"] = oracle.forward(sd, data, iters=0, keep_states=True)
    return _cache["oracle_m"]


# ---------------------------------------------------------------- 1. fixtures, end to end
@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference_fixture(device, name):
    g, sd, data = case(name)
    thr = float(g["match_threshold"])
    out = run(model_for(sd, device, int(g["sinkhorn_iterations"]), thr), to_dev(data, device))
    assert out["matches0"].dtype == np.int64 and out["matching_scores0"].dtype == np.float32
    for b in range(g["matches0"].shape[0]):
        exempt = parity.assert_pred_equal({k: out[k][b] for k in KEYS}, {k: g[k][b] for k in KEYS},
                                          f"{name}[{b}]", thr=thr)
        assert exempt == 0
        got, ref = out["log_assignment"][b], g["log_assignment"][b]
        print(f"{name}[{b}] max |exp(Z) - ref| = "
              f"{np.abs(np.exp(got[:-1, :-1]) - np.exp(ref[:-1, :-1])).max():.3g}")
        parity.assert_scores_close(np.exp(got[:-1, :-1]), np.exp(ref[:-1, :-1]),
                                   f"{name}[{b}] exp(log_assignment)")


# ---------------------------------------------------------------- 2. attention alone
def gpu_mha(device, q, k, v):
    lib = _lib.load()
    tq, tk, tv = (torch.as_tensor(x).to(device).contiguous() for x in (q, k, v))
    B, n, m = tq.shape[0], tq.shape[1], tk.shape[1]
    out = torch.full_like(tq, float("nan"))
    _lib.check(lib.onepose_mha_softmax(tq.data_ptr(), n * 256, tk.data_ptr(), m * 256,
                                       tv.data_ptr(), m * 256, B, n, m, out.data_ptr(), n * 256,
                                       _lib.stream_ptr(device)), "mha_softmax")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def torch_mha(q, k, v):
    """The same formula in fp32 on the CPU (einsum, softmax)."""
    q, k, v = (torch.as_tensor(x).view(x.shape[0], 4, 64) for x in (q, k, v))
    p = torch.softmax(torch.einsum("nhd,mhd->hnm", q, k) / 8.0, dim=-1)
    return torch.einsum("hnm,mhd->nhd", p, v).reshape(q.shape[0], 256).numpy()


@pytest.mark.parametrize("n,m", [(1, 1), (1, 70), (63, 64), (65, 33), (300, 257)])
def test_mha_softmax_against_oracle(device, n, m):
    rs = np.random.RandomState(100 * n + m)
    q, k = rs.standard_normal((n, 256)), rs.standard_normal((m, 256))
    v = rs.standard_normal((m, 256)).astype(np.float32)
    # logits reach +-60: a missing max shift overflows, an unmasked key tail (weight exp(0 - max)
    # on zero-padded keys) shows
    peak = max(np.abs(q[:, h * 64:(h + 1) * 64] @ k[:, h * 64:(h + 1) * 64].T / 8.0).max()
               for h in range(4))
    q = (q * np.sqrt(60.0 / peak)).astype(np.float32)
    k = (k * np.sqrt(60.0 / peak)).astype(np.float32)
    want = oracle.mha_softmax(q, k, v)
    e_cpu = np.abs(torch_mha(q, k, v) - want).max()
    got = gpu_mha(device, q[None], k[None], v[None])[0]
    e_gpu = np.abs(got - want).max()
    print(f"mha {n}x{m}: gpu error {e_gpu:.3g}, cpu fp32 error {e_cpu:.3g}")
    assert np.isfinite(got).all()
    assert e_gpu <= 4 * e_cpu


def test_mha_softmax_batch_and_shared_keys(device):
    """Two samples, the second sample's rows independent of the first; k / v at stride 0."""
    rs = np.random.RandomState(7)
    q = rs.standard_normal((2, 37, 256)).astype(np.float32)
    k = rs.standard_normal((1, 70, 256)).astype(np.float32)
    v = rs.standard_normal((1, 70, 256)).astype(np.float32)
    lib = _lib.load()
    tq, tk, tv = (torch.as_tensor(x).to(device) for x in (q, k, v))
    out = torch.empty_like(tq)
    _lib.check(lib.onepose_mha_softmax(tq.data_ptr(), 37 * 256, tk.data_ptr(), 0, tv.data_ptr(), 0,
                                       2, 37, 70, out.data_ptr(), 37 * 256,
                                       _lib.stream_ptr(device)), "mha_softmax")
    torch.cuda.synchronize()
    for b in range(2):
        single = gpu_mha(device, q[b:b + 1], k, v)[0]
        assert np.array_equal(out[b].cpu().numpy(), single)


@pytest.mark.parametrize("batch,waves", [(33, 4), (22, 2)])
def test_mha_softmax_workgroup_variants(device, batch, waves):
    """The launch picks 4, 2 or 1 waves (32 queries each) per workgroup from the grid size; the
    waves of a workgroup only share the staged K / V tile, so every variant gives the bits of the
    one-wave launch a single sample gets.  n = 130 = 128 + 2: the last workgroup's waves are
    partly or wholly past the queries; m = 70 has a ragged second key tile.  (The fourth
    variant, four waves splitting the keys of one query block, is what 300 x 257 above runs.)"""
    n, m = 130, 70
    rs = np.random.RandomState(batch)
    q = rs.standard_normal((batch, n, 256)).astype(np.float32)
    k = rs.standard_normal((batch, m, 256)).astype(np.float32)
    v = rs.standard_normal((batch, m, 256)).astype(np.float32)
    got = gpu_mha(device, q, k, v)
    assert np.isfinite(got).all()
    e_gpu = e_cpu = 0.0
    for b in (0, 1, batch // 2, batch - 1):
        want = oracle.mha_softmax(q[b], k[b], v[b])
        e_gpu = max(e_gpu, np.abs(got[b] - want).max())
        e_cpu = max(e_cpu, np.abs(torch_mha(q[b], k[b], v[b]) - want).max())
        assert np.array_equal(got[b], gpu_mha(device, q[b:b + 1], k[b:b + 1], v[b:b + 1])[0])
    print(f"mha B={batch} ({waves} waves): gpu error {e_gpu:.3g}, cpu fp32 error {e_cpu:.3g}")
    assert e_gpu <= 4 * e_cpu


# ---------------------------------------------------------------- 3. optimal transport alone
def gpu_lot(device, scores, alpha, iters):
    lib = _lib.load()
    s = torch.as_tensor(np.ascontiguousarray(scores, dtype=np.float32)).to(device)
    B, m, n = s.shape
    out = torch.full((B, m + 1, n + 1), float("nan"), dtype=torch.float32, device=device)
    nbytes = lib.onepose_log_optimal_transport_workspace_bytes(B, m, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _lib.check(lib.onepose_log_optimal_transport(s.data_ptr(), m * n, B, m, n, float(alpha), iters,
                                                 out.data_ptr(), ws.data_ptr(), nbytes,
                                                 _lib.stream_ptr(device)), "log_optimal_transport")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def torch_lot(scores, alpha, iters):
    """superglue.py:181-210's formula in fp32 on the CPU (cat, logsumexp)."""
    S = torch.as_tensor(np.ascontiguousarray(scores, dtype=np.float32))
    m, n = S.shape
    a = torch.tensor(alpha, dtype=torch.float32)
    Z = torch.cat([torch.cat([S, a.expand(m, 1)], 1), a.expand(1, n + 1)], 0)
    ms, ns = torch.tensor(float(m)), torch.tensor(float(n))
    norm = -(ms + ns).log()
    log_mu = torch.cat([norm.expand(m), ns.log()[None] + norm])
    log_nu = torch.cat([norm.expand(n), ms.log()[None] + norm])
    u, v = torch.zeros(m + 1), torch.zeros(n + 1)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None, :], dim=1)
        v = log_nu - torch.logsumexp(Z + u[:, None], dim=0)
    return (Z + u[:, None] + v[None, :] - norm).numpy()


def lot_scores(m, n):
    """An m x n block of realistic scores: the oracle's score matrix of superglue_m (300 x 257),
    transposed when the block is wider than it."""
    S = oracle_m()["scores"][0]
    if n > S.shape[1]:
        S = S.T
    return np.ascontiguousarray(S[:m, :n]).astype(np.float32)


def lot_errors(Z, want):
    inner = np.abs(np.exp(Z[:-1, :-1]) - np.exp(want[:-1, :-1])).max()
    bins = max(np.abs(Z[-1, :] - want[-1, :]).max(), np.abs(Z[:, -1] - want[:, -1]).max())
    return inner, bins


def marginal_errors(Z, want, m, n):
    """Row / column sums of exp(Z + norm) against the oracle's (which are the marginals mu, nu up
    to the Sinkhorn residual that every evaluation shares)."""
    norm = -np.log(m + n)
    P, W = np.exp(np.float64(Z) + norm), np.exp(want + norm)
    return max(np.abs(P.sum(1) - W.sum(1)).max(), np.abs(P.sum(0) - W.sum(0)).max())


@pytest.mark.parametrize("m,n,iters,batch", [(1, 1, 1, 1), (1, 70, 20, 1), (65, 33, 20, 2),
                                             (257, 300, 100, 1), (64, 64, 0, 1)])
def test_log_optimal_transport_against_oracle(device, m, n, iters, batch):
    check_lot(device, m, n, iters, batch, 1.0)


@pytest.mark.parametrize("alpha", [2.3457, -1.5])
@pytest.mark.parametrize("m,n,iters", [(255, 33, 20), (256, 33, 20), (256, 64, 20)])
def test_log_optimal_transport_chunk_boundary(device, m, n, iters, alpha):
    """m + 1 = 256 rows are one column-pass chunk, 257 are three (128, 128 and the dustbin row
    alone); a trained-like and a negative dustbin score."""
    check_lot(device, m, n, iters, 1, alpha)


def check_lot(device, m, n, iters, batch, alpha):
    S = np.stack([lot_scores(m, n)] + [lot_scores(m + 3, n + 5)[3:, 5:] for _ in range(batch - 1)])
    got = gpu_lot(device, S, alpha, iters)
    assert np.isfinite(got).all()
    for b in range(batch):
        want = oracle.log_optimal_transport(S[b], alpha, iters)
        cpu = torch_lot(S[b], alpha, iters)
        (ei, eb), (ci, cb) = lot_errors(got[b], want), lot_errors(cpu, want)
        print(f"lot {m}x{n} it {iters} [{b}]: exp(Z) inner gpu {ei:.3g} cpu {ci:.3g}; "
              f"Z bins gpu {eb:.3g} cpu {cb:.3g}")
        assert ei <= 4 * ci and eb <= 4 * cb
        if iters == 100:
            mg, mc = marginal_errors(got[b], want, m, n), marginal_errors(cpu, want, m, n)
            mu_err = np.abs(np.exp(want[:-1] - np.log(m + n)).sum(1) - 1.0 / (m + n)).max()
            print(f"  marginals: gpu {mg:.3g} cpu {mc:.3g}; oracle residual {mu_err:.3g}")
            assert mg <= 4 * mc


# ---------------------------------------------------------------- 4. layer states
# trained-like weights, images 480 x 640 and 384 x 512, (n0, n1, input seed): below one encoder
# group, tile edges at 64 -+ 1, and 256 tokens against 40 (the seeds of the same shapes in
# test_superglue_edges_gpu.py)
RAGGED = ((7, 9, 0), (63, 65, 0), (256, 40, 0))


def test_final_descriptors_through_scores(device):
    """sinkhorn_iters = 0: log_assignment's inner block is S - norm, S = mdesc0 . mdesc1 / 16, the
    end of the encoder and all 18 layers and the final projection.  fp32 yardstick: the oracle's
    own formulas evaluated in float32 (numpy).  superglue_m's inputs, then the ragged shapes."""
    g, sd, data = case("superglue_m")
    check_scores_through_layers(device, "superglue_m", sd, data, oracle_m())
    tsd = synthetic.superglue_state_dict(11, affine_bn=True, bin_score=T_BIN_SCORE)
    for n0, n1, seed in RAGGED:
        data = synthetic.make_superglue_inputs(n0, n1, seed=seed, image_hw0=(480, 640),
                                               image_hw1=(384, 512))
        check_scores_through_layers(device, f"{n0}x{n1}", tsd, data,
                                    oracle.forward(tsd, data, iters=0, keep_states=True))


def check_scores_through_layers(device, what, sd, data, want):
    # (without Sinkhorn the fp32 matching scores exp(S - norm) overflow; they are not used)
    with oracle.precision(np.float32), np.errstate(over="ignore"):
        cpu = oracle.forward(sd, data, iters=0, keep_states=True)
    out = run(model_for(sd, device, 0), to_dev(data, device))
    n0, n1 = want["scores"].shape[1:]
    assert out["log_assignment"].shape == (1, n0 + 1, n1 + 1)
    norm = -np.log(n0 + n1)
    S = np.float64(out["log_assignment"][0][:-1, :-1]) + norm
    e_gpu = np.abs(S - want["scores"][0]).max()
    # (adding and removing norm in fp32 costs the GPU path up to an ulp of |S| + |norm| more than
    # the CPU's S, which never carried norm: put the CPU's S through the same round trip)
    cpu_S = np.float64(np.float32(cpu["scores"][0]) - np.float32(norm)) + norm
    e_cpu = np.abs(cpu_S - want["scores"][0]).max()
    print(f"{what} scores after 18 layers: gpu error {e_gpu:.3g}, cpu fp32 error {e_cpu:.3g}, "
          f"max |S| {np.abs(want['scores']).max():.3g}")
    assert e_gpu <= 4 * e_cpu
    # the dustbins carry bin_score - norm: the model's fp32 bin_score, the subtraction in float64,
    # rounded to fp32 once
    bins = np.float32(np.float64(np.float32(sd["bin_score"])) - norm)
    assert np.allclose(out["log_assignment"][0][-1, :], bins, rtol=0, atol=1e-6)
    assert np.allclose(out["log_assignment"][0][:, -1], bins, rtol=0, atol=1e-6)


# ---------------------------------------------------------------- 5. determinism, reentrancy
def test_same_call_twice_is_bit_identical(device):
    g, sd, data = case("superglue_m")
    model = model_for(sd, device, 30)
    d = to_dev(data, device)
    a, b = run(model, d), run(model, d)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_two_streams_equal_sequential(device):
    gs, sd, ds = case("superglue_s")
    gm, _, dm = case("superglue_m")
    model = model_for(sd, device, 25)
    d1, d2 = to_dev(ds, device), to_dev(dm, device)
    seq1, seq2 = run(model, d1), run(model, d2)
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        o1 = model(d1, return_log_assignment=True)
    with torch.cuda.stream(s2):
        o2 = model(d2, return_log_assignment=True)
    torch.cuda.synchronize()
    for k in seq1:
        assert np.array_equal(o1[k].cpu().numpy(), seq1[k]), k
        assert np.array_equal(o2[k].cpu().numpy(), seq2[k]), k


def test_graph_replay_equals_eager(device):
    g, sd, data = case("superglue_s")
    model = model_for(sd, device, 20)
    d = to_dev(data, device)
    eager = run(model, d)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # warm up on the capture stream: weights packed
        model(d)
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model(d, return_log_assignment=True)
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert np.array_equal(out[k].cpu().numpy(), eager[k]), k


# ---------------------------------------------------------------- 6. mid-size run
def test_midsize_against_oracle(device):
    sd = synthetic.superglue_state_dict(11)
    data = synthetic.make_superglue_inputs(1024, 1000, seed=5)
    want = oracle.forward(sd, data, iters=100, thr=0.2)
    assert (want["matches0"] > -1).mean() > 0.25
    out = run(model_for(sd, device, 100), to_dev(data, device))
    exempt = parity.assert_pred_equal({k: out[k][0] for k in KEYS}, {k: want[k][0] for k in KEYS},
                                      "1024x1000", thr=0.2)
    assert exempt == 0
    parity.assert_scores_close(np.exp(out["log_assignment"][0][:-1, :-1]),
                               np.exp(want["log_assignment"][0][:-1, :-1]),
                               "1024x1000 exp(log_assignment)")


# ---------------------------------------------------------------- 7. shared side
def test_shared_side_stride0_equals_materialised(device):
    g, sd, data = case("superglue_b3")
    model = model_for(sd, device, int(g["sinkhorn_iterations"]))
    shared = to_dev(data, device)                       # side 1 expanded: batch stride 0
    assert shared["descriptors1"].stride(0) == 0 and shared["descriptors1"].shape[0] == 3
    full = {k: v.contiguous() for k, v in shared.items()}
    assert full["descriptors1"].stride(0) != 0
    a, b = run(model, shared), run(model, full)
    for k in a:
        assert np.array_equal(a[k], b[k]), k

"""Variable-count SuperGlue batches on the GPU (include/onepose_superglue_counts.h): the counts
entries against their uniform siblings bit for bit, then each kernel path -- attention, Sinkhorn,
the whole forward -- against the float64 oracle evaluated per sample on the trimmed inputs, and
the contract's independence, empty-sample, clamping and graph clauses.

The yardsticks are tests/test_superglue_gpu.py's: parity.assert_pred_equal with 0 exempt rows,
parity.assert_scores_close on exp(log_assignment), and "GPU error <= 4 x the fp32 CPU
evaluation's error" for attention, Sinkhorn and the scores through 18 layers.  The
zero-exemption cap is a condition on the inputs: every case first asserts on the CPU that no
oracle matching score lies within MARGIN = 1e-4 of the threshold (above two paths' ATOL = 2e-5).

Which test holds which kernel path:
  attention  four waves splitting the keys (both sides >= 128, few workgroups): 130 x 130 B = 7
             and 300 x 257 B = 3; one wave per workgroup: 37 x 70 B = 2; four and two waves of
             32 queries each: 130 x 70 at B = 33 and B = 22 (attention alone)
  Sinkhorn   chunked column pass: maxima 300 x 257; single chunk: maxima 255 x 70
  input stage, mutual check, per-sample image sizes: the whole-forward tests
"""
import numpy as np
import pytest
import torch

import parity
import superglue_oracle as oracle
from onepose_amd import _lib, superglue, synthetic
from test_superglue_gpu import (KEYS, gpu_mha, lot_errors, lot_scores, marginal_errors, torch_lot,
                                torch_mha)
from test_superglue_host import load_case

pytestmark = pytest.mark.gpu
THR = 0.2
MARGIN = 1e-4
SIZES = ((480, 640), (384, 512), (512, 512))
# (counts_q / counts0, counts_k / counts1) of the attention shape sets, maxima first
KS4 = (130, 130, (1, 31, 32, 33, 64, 65, 130), (130, 1, 65, 129, 63, 128, 7))
NW_A = (37, 70, (37, 1), (64, 70))
NW_B = (300, 257, (300, 1, 256), (1, 257, 64))
# 130 x 70 at the batch sizes that make attn_launch pick four and two waves per workgroup
_CQ, _CK = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 130), (70, 1, 64, 65, 33, 7)
NW4 = (130, 70, tuple(_CQ[b % 11] for b in range(33)), tuple(_CK[b % 6] for b in range(33)))
NW2 = (130, 70, tuple(_CQ[b % 11] for b in range(22)), tuple(_CK[b % 6] for b in range(22)))
_cache = {}


def weights():
    if "sd" not in _cache:
        _cache["sd"] = synthetic.superglue_state_dict(11, affine_bn=True, bin_score=2.3457)
    return _cache["sd"]


def model_for(device, iters):
    key = ("model", str(device), iters)
    if key not in _cache:
        _cache[key] = superglue.from_state_dict(
            weights(), {"sinkhorn_iterations": iters, "match_threshold": THR}).to(device)
    return _cache[key]


def samples(n0, n1, counts0, counts1, seed):
    """Per sample the trimmed inputs (numpy, no batch axis) and its (h, w) pair."""
    out = []
    for b, (c0, c1) in enumerate(zip(counts0, counts1)):
        hw0, hw1 = SIZES[b % 3], SIZES[(b + 1) % 3]
        d = synthetic.make_superglue_inputs(max(c0, 1), max(c1, 1), seed=seed + b, image_hw0=hw0,
                                            image_hw1=hw1)
        s = {k: d[k][0] for k in d if not k.startswith("image")}
        for side, c in ((0, c0), (1, c1)):
            s[f"descriptors{side}"] = s[f"descriptors{side}"][:, :c]
            s[f"keypoints{side}"] = s[f"keypoints{side}"][:c]
            s[f"scores{side}"] = s[f"scores{side}"][:c]
        s["hw0"], s["hw1"] = hw0, hw1
        out.append(s)
    return out


def padded(smp, n0, n1, fill=0.0):
    """The samples stacked at the batch maxima; slots past a count hold `fill`."""
    B = len(smp)
    a = {"descriptors0": np.full((B, 256, n0), fill, np.float32),
         "descriptors1": np.full((B, 256, n1), fill, np.float32),
         "keypoints0": np.full((B, n0, 2), fill, np.float32),
         "keypoints1": np.full((B, n1, 2), fill, np.float32),
         "scores0": np.full((B, n0), fill, np.float32),
         "scores1": np.full((B, n1), fill, np.float32)}
    for b, s in enumerate(smp):
        for side in (0, 1):
            c = s[f"scores{side}"].shape[0]
            a[f"descriptors{side}"][b, :, :c] = s[f"descriptors{side}"]
            a[f"keypoints{side}"][b, :c] = s[f"keypoints{side}"]
            a[f"scores{side}"][b, :c] = s[f"scores{side}"]
    return a


def oracle_one(s, iters, **kw):
    return oracle.forward_one(weights(), s["descriptors0"], s["keypoints0"], s["scores0"],
                              s["descriptors1"], s["keypoints1"], s["scores1"], s["hw0"], s["hw1"],
                              iters, THR, **kw)


def assert_margin(want, what):
    """The zero-exemption precondition: no oracle matching score near the threshold."""
    for k in ("matching_scores0", "matching_scores1"):
        gap = np.abs(np.asarray(want[k]) - THR).min() if np.asarray(want[k]).size else 1.0
        assert gap > MARGIN, f"{what}: an oracle {k} lies {gap:.3g} from the threshold; pick a seed"


def i32(device, x):
    return None if x is None else torch.tensor(np.asarray(x), dtype=torch.int32, device=device)


def entry(device, arrs, n0, n1, iters, counts0=None, counts1=None, hw0=None, hw1=None,
          scalar_hw=((480, 640), (480, 640)), counts_entry=True, ws_fill=0, la_fill=float("nan")):
    """onepose_superglue_match_counts (or the uniform sibling) on numpy inputs; a side given with
    batch dimension 1 goes at batch stride 0.  Returns numpy outputs with log_assignment."""
    lib = _lib.load()
    w = model_for(device, iters).packed_weights(device)
    B = max(v.shape[0] for v in arrs.values())
    t = {k: torch.as_tensor(v).to(device).contiguous() for k, v in arrs.items()}
    bs = {k: (0 if v.shape[0] == 1 and B > 1 else v[0].numel()) for k, v in t.items()}
    nbytes = lib.onepose_superglue_workspace_bytes(B, n0, n1)
    ws = torch.full((nbytes,), ws_fill, dtype=torch.uint8, device=device)
    out = {"matches0": torch.full((B, n0), 7, dtype=torch.int64, device=device),
           "matches1": torch.full((B, n1), 7, dtype=torch.int64, device=device),
           "mscores0": torch.full((B, n0), float("nan"), device=device),
           "mscores1": torch.full((B, n1), float("nan"), device=device),
           "log_assignment": torch.full((B, n0 + 1, n1 + 1), la_fill, device=device)}
    extra = {}
    if counts_entry:
        extra = dict(counts0=i32(device, counts0), counts1=i32(device, counts1),
                     hw0=i32(device, hw0), hw1=i32(device, hw1))
    (h0, w0), (h1, w1) = scalar_hw
    _lib.run("onepose_superglue_match_counts" if counts_entry else "onepose_superglue_match",
             packed_weights=w, desc0=t["descriptors0"], desc0_bstride=bs["descriptors0"],
             kpts0=t["keypoints0"], kpts0_bstride=bs["keypoints0"], scores0=t["scores0"],
             scores0_bstride=bs["scores0"], desc1=t["descriptors1"],
             desc1_bstride=bs["descriptors1"], kpts1=t["keypoints1"],
             kpts1_bstride=bs["keypoints1"], scores1=t["scores1"], scores1_bstride=bs["scores1"],
             batch=B, n0=n0, n1=n1, h0=h0, w0=w0, h1=h1, w1=w1, sinkhorn_iters=iters,
             match_threshold=THR, precision=0, **out, workspace=ws, workspace_bytes=nbytes,
             stream=_lib.stream_ptr(device), **extra)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["matching_scores0"], res["matching_scores1"] = res.pop("mscores0"), res.pop("mscores1")
    return res


def run_counts(device, smp, n0, n1, iters, **kw):
    return entry(device, padded(smp, n0, n1, kw.pop("fill", 0.0)), n0, n1, iters,
                 counts0=[s["scores0"].shape[0] for s in smp],
                 counts1=[s["scores1"].shape[0] for s in smp],
                 hw0=[s["hw0"] for s in smp], hw1=[s["hw1"] for s in smp], **kw)


def same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what} {k}"


# ---------------------------------------------------------------- 1. uniform = the existing entry
def test_uniform_counts_equal_the_existing_entry_bit_for_bit(device):
    n0, n1, B = 70, 65, 3
    d = synthetic.make_superglue_inputs(n0, n1, seed=21, batch=B, image_hw0=(480, 640),
                                        image_hw1=(384, 512))
    arrs = {k: v for k, v in d.items() if not k.startswith("image")}
    hw = ((480, 640), (384, 512))
    ref = entry(device, arrs, n0, n1, 20, scalar_hw=hw, counts_entry=False)
    for c0, c1 in ((None, None), ([n0] * B, [n1] * B)):
        for h0, h1 in ((None, None), ([hw[0]] * B, [hw[1]] * B)):
            # (with the arrays given, the scalars are not read: pass other ones)
            got = entry(device, arrs, n0, n1, 20, counts0=c0, counts1=c1, hw0=h0, hw1=h1,
                        scalar_hw=hw if h0 is None else ((3, 5), (7, 2)))
            same(ref, got, f"counts {c0 is not None} hw {h0 is not None}")


def test_uniform_counts_equal_the_existing_entry_shared_side(device):
    g, sd, data = load_case("superglue_b3")
    n0, n1, B, _ = (int(x) for x in g["shape"])
    iters = int(g["sinkhorn_iterations"])
    _cache[("model", str(device), iters)] = superglue.from_state_dict(
        sd, {"sinkhorn_iterations": iters, "match_threshold": THR}).to(device)
    try:
        arrs = {k: v for k, v in data.items() if not k.startswith("image")}
        assert arrs["descriptors1"].shape[0] == 1 and B == 3
        hw = (tuple(data["image0"].shape[-2:]), tuple(data["image1"].shape[-2:]))
        ref = entry(device, arrs, n0, n1, iters, scalar_hw=hw, counts_entry=False)
        for c0 in (None, [n0] * B):
            for h0, h1 in ((None, None), ([hw[0]] * B, [hw[1]] * B)):
                got = entry(device, arrs, n0, n1, iters, counts0=c0, hw0=h0, hw1=h1, scalar_hw=hw)
                same(ref, got, f"shared side, counts {c0 is not None} hw {h0 is not None}")
    finally:
        del _cache[("model", str(device), iters)]


# ---------------------------------------------------------------- 2. attention alone
def gpu_mha_counts(device, q, k, v, cq, ck):
    tq, tk, tv = (torch.as_tensor(x).to(device).contiguous() for x in (q, k, v))
    B, n, m = tq.shape[0], tq.shape[1], tk.shape[1]
    out = torch.full_like(tq, float("nan"))
    _lib.run("onepose_mha_softmax_counts", q=tq, q_bstride=n * 256, k=tk, k_bstride=m * 256, v=tv,
             v_bstride=m * 256, batch=B, n=n, m=m, counts_q=i32(device, cq),
             counts_k=i32(device, ck), out=out, out_bstride=n * 256,
             stream=_lib.stream_ptr(device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def mha_case(n, m, cq, ck):
    B = len(cq)
    rs = np.random.RandomState(1000 * n + m)
    # slots past a count hold NaN: nothing may read them
    q = np.full((B, n, 256), np.nan, np.float32)
    k = np.full((B, m, 256), np.nan, np.float32)
    v = np.full((B, m, 256), np.nan, np.float32)
    per = []
    for b in range(B):
        qb, kb = rs.standard_normal((cq[b], 256)), rs.standard_normal((ck[b], 256))
        vb = rs.standard_normal((ck[b], 256)).astype(np.float32)
        peak = max(np.abs(qb[:, h * 64:(h + 1) * 64] @ kb[:, h * 64:(h + 1) * 64].T / 8.0).max()
                   for h in range(4))           # logits reach +-60, as in the uniform test
        qb = (qb * np.sqrt(60.0 / peak)).astype(np.float32)
        kb = (kb * np.sqrt(60.0 / peak)).astype(np.float32)
        q[b, :cq[b]], k[b, :ck[b]], v[b, :ck[b]] = qb, kb, vb
        per.append((qb, kb, vb))
    return q, k, v, per


@pytest.mark.parametrize("n,m,cq,ck", [KS4, NW_A, NW_B],
                         ids=["130x130_B7", "37x70_B2", "300x257_B3"])
def test_mha_softmax_counts_against_oracle(device, n, m, cq, ck):
    q, k, v, per = mha_case(n, m, cq, ck)
    got = gpu_mha_counts(device, q, k, v, cq, ck)
    for b, (qb, kb, vb) in enumerate(per):
        want = oracle.mha_softmax(qb, kb, vb)
        e_cpu = np.abs(torch_mha(qb, kb, vb) - want).max()
        e_gpu = np.abs(got[b, :cq[b]] - want).max()
        print(f"mha counts {n}x{m} [{b}] {cq[b]}x{ck[b]}: gpu error {e_gpu:.3g}, "
              f"cpu fp32 error {e_cpu:.3g}")
        assert np.isfinite(got[b, :cq[b]]).all()
        assert e_gpu <= 4 * e_cpu
        assert np.all(got[b, cq[b]:] == 0), f"sample {b}: rows past the count are not zero"


@pytest.mark.parametrize("n,m,cq,ck", [NW4, NW2], ids=["130x70_B33", "130x70_B22"])
def test_mha_softmax_counts_workgroup_variants(device, n, m, cq, ck):
    """Four and two waves of 32 queries per workgroup (tests/test_superglue_gpu.py's
    test_mha_softmax_workgroup_variants, with counts).  m = 70 < 128 never splits the keys, and
    the waves of a workgroup only share the staged K / V tile, so every sample must give the BITS
    of the uniform entry on its trimmed inputs alone.  The error bar is that test's: the largest
    error over the batch against four times the fp32 CPU evaluation's largest.  (Per sample the
    bar is too tight at these shapes: with logits at +-60 both evaluations err by 1.2e-5 to
    1.4e-5 on most samples, but on a 65 x 7 sample the CPU's one draw was 2.9e-6 against the
    GPU's 1.25e-5.)"""
    q, k, v, per = mha_case(n, m, cq, ck)
    got = gpu_mha_counts(device, q, k, v, cq, ck)
    e_gpu = e_cpu = 0.0
    for b, (qb, kb, vb) in enumerate(per):
        want = oracle.mha_softmax(qb, kb, vb)
        e_gpu = max(e_gpu, np.abs(got[b, :cq[b]] - want).max())
        e_cpu = max(e_cpu, np.abs(torch_mha(qb, kb, vb) - want).max())
        assert np.array_equal(got[b, :cq[b]], gpu_mha(device, qb[None], kb[None], vb[None])[0]), b
        assert np.all(got[b, cq[b]:] == 0), f"sample {b}: rows past the count are not zero"
    print(f"mha counts {n}x{m} B={len(cq)}: gpu error {e_gpu:.3g}, cpu fp32 error {e_cpu:.3g}")
    assert e_gpu <= 4 * e_cpu


# ---------------------------------------------------------------- 3. Sinkhorn alone
CHUNKED = (300, 257, ((300, 257), (255, 33), (256, 64), (127, 257), (128, 1), (1, 70)))
SINGLE = (255, 70, ((255, 70), (128, 1), (1, 70), (200, 33)))


def gpu_lot_counts(device, S, cm, cn, alpha, iters):
    lib = _lib.load()
    s = torch.as_tensor(S).to(device).contiguous()
    B, m, n = s.shape
    out = torch.full((B, m + 1, n + 1), float("nan"), dtype=torch.float32, device=device)
    nbytes = lib.onepose_log_optimal_transport_workspace_bytes(B, m, n)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
    _lib.run("onepose_log_optimal_transport_counts", scores=s, scores_bstride=m * n, batch=B, m=m,
             n=n, counts_m=i32(device, cm), counts_n=i32(device, cn), alpha=float(alpha),
             iters=iters, out=out, workspace=ws, workspace_bytes=nbytes,
             stream=_lib.stream_ptr(device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("M,N,dims,iters,alpha",
                         [CHUNKED + (20, 2.3457), CHUNKED + (20, -1.5), SINGLE + (20, 2.3457),
                          SINGLE + (20, -1.5), CHUNKED + (100, 2.3457)],
                         ids=["chunked_it20", "chunked_it20_neg", "single_it20", "single_it20_neg",
                              "chunked_it100"])
def test_log_optimal_transport_counts_against_oracle(device, M, N, dims, iters, alpha):
    S = np.full((len(dims), M, N), np.nan, np.float32)
    for b, (m, n) in enumerate(dims):
        S[b, :m, :n] = lot_scores(m, n)
    got = gpu_lot_counts(device, S, [d[0] for d in dims], [d[1] for d in dims], alpha, iters)
    for b, (m, n) in enumerate(dims):
        Z = got[b, :m + 1, :n + 1]
        assert np.isfinite(Z).all()
        want = oracle.log_optimal_transport(S[b, :m, :n], alpha, iters)
        cpu = torch_lot(S[b, :m, :n], alpha, iters)
        (ei, eb), (ci, cb) = lot_errors(Z, want), lot_errors(cpu, want)
        print(f"lot counts {M}x{N} [{b}] {m}x{n} it {iters}: exp(Z) inner gpu {ei:.3g} cpu "
              f"{ci:.3g}; Z bins gpu {eb:.3g} cpu {cb:.3g}")
        assert ei <= 4 * ci and eb <= 4 * cb
        if iters == 100:
            mg, mc = marginal_errors(Z, want, m, n), marginal_errors(cpu, want, m, n)
            print(f"  marginals: gpu {mg:.3g} cpu {mc:.3g}")
            assert mg <= 4 * mc
        outside = np.ones((M + 1, N + 1), bool)
        outside[:m + 1, :n + 1] = False
        assert np.isnan(got[b][outside]).all(), f"sample {b}: written outside its block"


# ---------------------------------------------------------------- 4. the whole forward
@pytest.mark.parametrize("n0,n1,c0,c1", [KS4, NW_A, NW_B], ids=["130x130_B7", "37x70_B2",
                                                                "300x257_B3"])
def test_forward_counts_scores_through_18_layers(device, n0, n1, c0, c1):
    """sinkhorn_iters = 0: the block's inner part is S - norm of the sample's own counts."""
    smp = samples(n0, n1, c0, c1, seed=300 + n0)
    out = run_counts(device, smp, n0, n1, 0)
    bin_f32 = np.float64(np.float32(weights()["bin_score"]))
    for b, s in enumerate(smp):
        want = oracle_one(s, 0, keep_states=True)
        with oracle.precision(np.float32), np.errstate(over="ignore"):
            cpu = oracle_one(s, 0, keep_states=True)
        norm = -np.log(c0[b] + c1[b])
        Z = out["log_assignment"][b, :c0[b] + 1, :c1[b] + 1]
        S = np.float64(Z[:-1, :-1]) + norm
        e_gpu = np.abs(S - want["scores"]).max()
        cpu_S = np.float64(np.float32(cpu["scores"]) - np.float32(norm)) + norm
        e_cpu = np.abs(cpu_S - want["scores"]).max()
        print(f"counts {n0}x{n1} [{b}] {c0[b]}x{c1[b]} scores after 18 layers: gpu error "
              f"{e_gpu:.3g}, cpu fp32 error {e_cpu:.3g}")
        assert e_gpu <= 4 * e_cpu
        bins = np.float32(bin_f32 - norm)
        assert np.allclose(Z[-1, :], bins, rtol=0, atol=1e-6)
        assert np.allclose(Z[:, -1], bins, rtol=0, atol=1e-6)


def check_against_oracle(out, smp, n0, n1, iters, what):
    for b, s in enumerate(smp):
        c0, c1 = s["scores0"].shape[0], s["scores1"].shape[0]
        want = oracle_one(s, iters)
        assert_margin(want, f"{what}[{b}]")
        got = {"matches0": out["matches0"][b, :c0], "matches1": out["matches1"][b, :c1],
               "matching_scores0": out["matching_scores0"][b, :c0],
               "matching_scores1": out["matching_scores1"][b, :c1]}
        exempt = parity.assert_pred_equal(got, {k: want[k] for k in KEYS}, f"{what}[{b}]", thr=THR)
        assert exempt == 0
        Z = out["log_assignment"][b, :c0 + 1, :c1 + 1]
        parity.assert_scores_close(np.exp(Z[:-1, :-1]), np.exp(want["log_assignment"][:-1, :-1]),
                                   f"{what}[{b}] exp(log_assignment)")
        assert np.all(out["matches0"][b, c0:] == -1) and np.all(out["matches1"][b, c1:] == -1)
        assert np.all(out["matching_scores0"][b, c0:] == 0)
        assert np.all(out["matching_scores1"][b, c1:] == 0)
        outside = np.ones((n0 + 1, n1 + 1), bool)
        outside[:c0 + 1, :c1 + 1] = False
        assert np.isnan(out["log_assignment"][b][outside]).all()


@pytest.mark.parametrize("n0,n1,c0,c1", [KS4, NW_A, NW_B], ids=["130x130_B7", "37x70_B2",
                                                                "300x257_B3"])
def test_forward_counts_against_oracle(device, n0, n1, c0, c1):
    smp = samples(n0, n1, c0, c1, seed=300 + n0)
    out = run_counts(device, smp, n0, n1, 20)
    check_against_oracle(out, smp, n0, n1, 20, f"counts {n0}x{n1}")


# ---------------------------------------------------------------- 5. independence
def test_a_sample_does_not_depend_on_its_batch(device):
    n0, n1 = 70, 65
    abc = samples(n0, n1, (50, 70, 33), (65, 40, 64), seed=40)
    axy = [abc[0]] + samples(n0, n1, (70, 1), (2, 65), seed=50)
    a = run_counts(device, abc, n0, n1, 20)
    b = run_counts(device, axy, n0, n1, 20)
    for k in a:
        assert np.array_equal(a[k][0], b[k][0], equal_nan=True), k
    assert not np.array_equal(a["matches0"][1], b["matches0"][1])


def test_padding_and_workspace_contents_do_not_matter(device):
    n0, n1 = 70, 65
    smp = samples(n0, n1, (50, 70, 33), (65, 40, 64), seed=40)
    clean = run_counts(device, smp, n0, n1, 20, fill=0.0, ws_fill=0)
    dirty = run_counts(device, smp, n0, n1, 20, fill=float("nan"), ws_fill=0xFF)
    same(clean, dirty, "NaN padding / 0xFF workspace")


# ---------------------------------------------------------------- 6. empty samples
def test_empty_samples_give_no_match_and_disturb_nothing(device):
    n0, n1 = 40, 33
    smp = samples(n0, n1, (40, 0, 5, 0), (33, 5, 0, 0), seed=60)
    out = run_counts(device, smp, n0, n1, 20, fill=float("nan"), ws_fill=0xFF)
    for b in (1, 2, 3):
        assert np.all(out["matches0"][b] == -1) and np.all(out["matches1"][b] == -1)
        assert np.all(out["matching_scores0"][b] == 0) and np.all(out["matching_scores1"][b] == 0)
        assert np.isnan(out["log_assignment"][b]).all()      # left as the caller gave it
    alone = run_counts(device, smp[:1], n0, n1, 20)
    for k in out:
        assert np.array_equal(out[k][0], alone[k][0], equal_nan=True), k
    assert (out["matches0"][0] > -1).any()
    check_against_oracle({k: v[:1] for k, v in out.items()}, smp[:1], n0, n1, 20, "beside empties")


# ---------------------------------------------------------------- 7. clamping
def test_counts_are_clamped_on_the_device(device):
    n0, n1 = 40, 33
    smp = samples(n0, n1, (40, 40, 20), (33, 33, 33), seed=70)
    arrs = padded(smp, n0, n1)
    hw0, hw1 = [s["hw0"] for s in smp], [s["hw1"] for s in smp]
    got = entry(device, arrs, n0, n1, 20, counts0=[10 ** 6, -3, 20], counts1=[33, 33, 10 ** 6],
                hw0=hw0, hw1=hw1)
    want = entry(device, arrs, n0, n1, 20, counts0=[n0, 0, 20], counts1=[33, 33, n1], hw0=hw0,
                 hw1=hw1)
    same(want, got, "clamped counts")
    assert np.all(got["matches0"][1] == -1) and (got["matches0"][0] > -1).any()
    # an h or w below 1 is read as 1
    a = entry(device, arrs, n0, n1, 20, hw0=[(0, -7)] * 3, hw1=hw1)
    b = entry(device, arrs, n0, n1, 20, hw0=[(1, 1)] * 3, hw1=hw1)
    same(a, b, "clamped sizes")


# ---------------------------------------------------------------- 8. repeats and graphs, 9. module
def module_data(device, smp, n0, n1):
    d = {k: torch.as_tensor(v).to(device) for k, v in padded(smp, n0, n1).items()}
    d["counts0"] = i32(device, [s["scores0"].shape[0] for s in smp])
    d["counts1"] = i32(device, [s["scores1"].shape[0] for s in smp])
    d["image_hw0"] = i32(device, [s["hw0"] for s in smp])
    d["image_hw1"] = i32(device, [s["hw1"] for s in smp])
    return d


def test_module_forward_with_counts_equals_the_entry(device):
    n0, n1 = 70, 65
    smp = samples(n0, n1, (50, 70, 33), (65, 40, 64), seed=40)
    model = model_for(device, 20)
    out = model(module_data(device, smp, n0, n1), return_log_assignment=True)
    torch.cuda.synchronize()
    want = run_counts(device, smp, n0, n1, 20, la_fill=0.0)
    for k in want:
        assert np.array_equal(out[k].cpu().numpy(), want[k]), k
    assert out["matches0"].dtype == torch.int64 and tuple(out["matches0"].shape) == (3, n0)
    # without the new keys: today's call
    d = synthetic.make_superglue_inputs(n0, n1, seed=21, batch=2)
    plain = model({k: torch.as_tensor(v).to(device) for k, v in d.items()},
                  return_log_assignment=True)
    torch.cuda.synchronize()
    ref = entry(device, {k: v for k, v in d.items() if not k.startswith("image")}, n0, n1, 20,
                scalar_hw=((512, 512), (512, 512)), counts_entry=False)
    for k in ref:
        assert np.array_equal(plain[k].cpu().numpy(), ref[k]), k


def test_same_call_twice_and_graph_replay_with_counts_changed_in_place(device):
    n0, n1 = 70, 65
    smp = samples(n0, n1, (50, 70, 33), (65, 40, 64), seed=40)
    model = model_for(device, 20)
    d = module_data(device, smp, n0, n1)
    run = lambda: {k: v.cpu().numpy() for k, v in   # noqa: E731
                   model(d, return_log_assignment=True).items()}
    eager, again = run(), run()
    same(eager, again, "same call twice")
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # warm up on the capture stream
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
    same(eager, {k: v.cpu().numpy() for k, v in out.items()}, "graph replay")
    # other counts, same maxima, changed in place: the replay follows them
    d["counts0"].copy_(i32(device, [70, 20, 33]))
    d["counts1"].copy_(i32(device, [30, 65, 1]))
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: v.cpu().numpy() for k, v in out.items()}
    fresh = run()
    same(fresh, replayed, "graph replay after the counts changed")
    assert not np.array_equal(fresh["matches0"], eager["matches0"])

"""onepose_detect_stage on the GPU: against the numpy oracle (tests/detector_oracle.py), and
against its own parts -- selection on the host, onepose_affine_partial_ransac, the box
arithmetic on the host.

Boxes are integers and must equal the oracle's exactly, every view included.  That is a fair
demand only where no corner lies at an integer before truncation: the refined affine differs
from the oracle's by the summation order (1e-9 / 1e-6 px, tests/test_affine_partial_gpu.py), so
every fixture is checked here, on the CPU, to keep each corner coordinate 1e-4 away from an
integer."""
import numpy as np
import pytest
import torch

import detector_oracle as D
from detector_cases import stage_case
from onepose_amd import detector

pytestmark = pytest.mark.gpu

CASES = {
    # the hand-built case of the host test: the two ranking modes differ, one view below 6
    "small": dict(),
    # selection over more than one 256-thread pass, views of 0, 5 and 6 matches, views 1 and 6
    # tied at the top in matches (mode 0) and in inliers (mode 1)
    "ragged": dict(spec=((300, 180), (513, 400), (0, 0), (5, 5), (6, 6), (300, 120), (513, 400)),
                   n0=700, n1=600, pad=7, seed=11),
    "per_view": dict(spec=((40, 30), (64, 20), (33, 33)), n0=70, n1=90, pad=1, seed=12,
                     per_view=True),
    # the in-kernel scan over two 256-thread trips: every view has an estimate, and the valid
    # matches of views 0 and 1 cross the wave boundaries and the trip boundary
    "two_trips": dict(spec=((280, 200), (257, 180), (64, 40)), n0=300, n1=320),
}


def fair(ref):
    pre = np.concatenate([p.reshape(-1) for p in ref["pre"] if p is not None])
    return np.abs(pre - np.rint(pre)).min() > 1e-4


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, kw in CASES.items():
        args = stage_case(**kw)
        refs = [D.detect_stage(*args, rank_mode=m) for m in (0, 1)]
        assert fair(refs[0]), name
        out[name] = (args, refs)
    return out


def run(args, device, rank_mode=0, counts0=True):
    m, c0, k0, k1, hw, qhw = args
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    out = detector.detect_stage(t(m), t(c0) if counts0 else None, t(k0), t(k1), t(hw), qhw,
                                rank_mode=rank_mode)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_stage_equals_the_oracle(cases, device, name):
    args, refs = cases[name]
    for mode in (0, 1):
        ref, got = refs[mode], run(args, device, mode)
        for k in ("counts", "status", "n_inliers", "iters", "bbox", "inlier_mask"):
            assert np.array_equal(got[k], ref[k]), (name, mode, k, got[k], ref[k])
        assert int(got["best_view"][0]) == ref["best_view"], (name, mode)
        assert np.array_equal(got["best_bbox"], ref["best_bbox"])
        A = got["affine"].reshape(-1, 2, 3) - ref["affine"].reshape(-1, 2, 3)
        assert np.abs(A[:, :, :2]).max() <= 1e-9 and np.abs(A[:, :, 2]).max() <= 1e-6
        for b, mp in enumerate(ref["mpts"]):
            assert np.array_equal(got["mpts"][b, :len(mp)], mp)
    if name == "small":
        assert refs[0]["best_view"] != refs[1]["best_view"]
    if name == "ragged":   # ties go to the first view; views without an estimate rank 0
        assert list(refs[0]["counts"]) == [300, 513, 0, 5, 6, 300, 513]
        assert list(refs[0]["status"]) == [0, 0, 1, 1, 0, 0, 0]
        r0, r1 = refs[0]["rank"], refs[1]["rank"]
        assert r0[1] == r0[6] == r0.max() and r1[1] == r1[6] == r1.max()
        assert refs[0]["best_view"] == refs[1]["best_view"] == 1
        assert list(refs[0]["bbox"][2]) == [0, 0, 480, 640]   # x1 is the query's height
    if name == "two_trips":
        assert list(refs[0]["counts"]) == [280, 257, 64] and not refs[0]["status"].any()


def test_stage_equals_its_parts(cases, device):
    """Selection on the host, then onepose_affine_partial_ransac (the same kernel: the same
    bits), then the box arithmetic on the host."""
    args, _ = cases["ragged"]
    m, c0, k0, k1, hw, qhw = args
    got = run(args, device)
    B, n0 = m.shape
    frm, to = np.zeros((B, n0, 2), np.float32), np.zeros((B, n0, 2), np.float32)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        valid = m[b, :c0[b]] > -1
        cnt[b] = valid.sum()
        frm[b, :cnt[b]] = k0[b, :c0[b]][valid]
        to[b, :cnt[b]] = k1[m[b, :c0[b]][valid]]
    assert np.array_equal(cnt, got["counts"])
    part = detector.affine_partial_ransac(*(torch.from_numpy(a).to(device) for a in (frm, to, cnt)))
    part = {k: v.cpu().numpy() for k, v in part.items()}
    for b in range(B):
        if cnt[b] < D.MIN_MATCHES:     # the stage asks for 6 matches, the estimator for 2
            assert got["status"][b] == 1 and not got["affine"][b].any()
            assert list(got["bbox"][b]) == [0, 0, qhw[0], qhw[1]] and got["n_inliers"][b] == 0
            continue
        assert got["status"][b] == part["status"][b] == 0
        assert np.array_equal(got["affine"][b], part["affine"][b])
        assert np.array_equal(got["inlier_mask"][b], part["inlier_mask"][b])
        assert got["n_inliers"][b] == part["n_inliers"][b] and got["iters"][b] == part["iters"][b]
        box, pre = D.view_bbox(got["affine"][b], hw[b, 0], hw[b, 1])
        assert np.abs(pre - np.rint(pre)).min() > 1e-4 and np.array_equal(got["bbox"][b], box)


def test_shared_and_per_view_query_strides(cases, device):
    """One shared query (stride 0) equals the same query repeated per view; without counts0
    every one of the n0 keypoints is read."""
    args, _ = cases["small"]
    m, c0, k0, k1, hw, qhw = args
    shared = run(args, device)
    rep = run((m, c0, k0, np.repeat(k1[None], len(m), 0), hw, qhw), device)
    for k in shared:
        assert np.array_equal(shared[k], rep[k], equal_nan=True), k
    # the poison past counts0 cut away: all n0' keypoints are the view's own
    n = int(c0[0])
    cut = run((m[:, :n], None, k0[:, :n], k1, hw, qhw), device, counts0=False)
    for k in ("counts", "status", "n_inliers", "bbox", "best_view", "best_bbox", "affine"):
        assert np.array_equal(cut[k], shared[k]), k

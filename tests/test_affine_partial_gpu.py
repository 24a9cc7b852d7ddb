"""onepose_affine_partial_ransac on the GPU against the numpy oracle
(tests/detector_oracle.py): one batch whose views cover every count at which the kernel takes
another path -- none, one, exactly two (no RANSAC), three, below and at the stage's six, one
wave more or less (63 / 64 / 65), more than one workgroup pass (257), 1000 -- with no, 30 % and
70 % outliers, a view of unrelated points and one whose points all appear twice (subsets of two
coincident points give a non-finite model).

Masks, inlier counts, status and the iteration at which RANSAC stops must equal the oracle's
exactly: both sides run the same float64 minimal model and float32 errors in the same order.
The refined coefficients are the same float64 operations summed in another order (wave
reductions here, numpy there): 1e-9 in the 2x2 part, 1e-6 px in the translation, the bound
ransac_PnP's poses are held to."""
import numpy as np
import pytest
import torch

import detector_oracle as D
from detector_cases import scene
from onepose_amd import detector

pytestmark = pytest.mark.gpu

VIEWS = [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (5, 0.3), (6, 0.0), (63, 0.3), (64, 0.7),
         (65, 0.3), (257, 0.7), (1000, 0.3), (1000, 0.7), (257, 0.0)]
MAXP = 1000


@pytest.fixture(scope="module")
def batch():
    """(from [B, P, 2], to, counts, oracle results); the padding past a view's count is NaN."""
    pts = [scene(n, share, seed=100 + i)[:2] for i, (n, share) in enumerate(VIEWS)]
    rs = np.random.RandomState(77)
    pts.append((rs.uniform(0, 300, (200, 2)).astype(np.float32),       # unrelated points
                rs.uniform(0, 300, (200, 2)).astype(np.float32)))
    f, t, *_ = scene(60, 0.3, seed=200)                                # every point twice
    order = rs.permutation(120)
    pts.append((np.concatenate([f, f])[order], np.concatenate([t, t])[order]))
    B = len(pts)
    frm = np.full((B, MAXP, 2), np.nan, np.float32)
    to = np.full((B, MAXP, 2), np.nan, np.float32)
    for b, (f, t) in enumerate(pts):
        frm[b, :len(f)], to[b, :len(f)] = f, t
    counts = np.array([len(f) for f, _ in pts], np.int32)
    ref = [D.estimate_affine_partial_2d(f, t) for f, t in pts]
    return frm, to, counts, ref


def test_batch_equals_the_oracle(batch, device):
    frm, to, counts, ref = batch
    out = detector.affine_partial_ransac(torch.from_numpy(frm).to(device),
                                         torch.from_numpy(to).to(device),
                                         torch.from_numpy(counts).to(device))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, (st, M, mask, nin, iters) in enumerate(ref):
        n = counts[b]
        what = f"view {b} ({n} points)"
        assert got["status"][b] == st, what
        assert got["n_inliers"][b] == nin, what
        assert got["iters"][b] == iters, what
        assert np.array_equal(got["inlier_mask"][b, :n].astype(bool), mask), what
        assert not got["inlier_mask"][b, n:].any(), what
        A = got["affine"][b]
        print(what, "status", st, "inliers", nin, "iters", iters, "max |dA|",
              np.abs(A - M).max())
        assert np.abs(A[:, :2] - M[:, :2]).max() <= 1e-9, what
        assert np.abs(A[:, 2] - M[:, 2]).max() <= 1e-6, what
    assert [r[0] for r in ref[:4]] == [1, 1, 0, 0]     # the fixture covers the small counts
    assert all(r[0] == 0 and 2 <= r[3] for r in ref[4:])


def test_counts_are_clamped_to_max_points(batch, device):
    """A count above max_points (or below 0) cannot be refused on the host -- counts live on the
    device -- so the kernel clamps it: 300 of view 10's points with a count of 1000 solve as
    300 points, a negative count as none."""
    frm, to, counts, _ = batch
    f, t = frm[10, :300], to[10, :300]
    out = detector.affine_partial_ransac(torch.from_numpy(np.stack([f, f])).to(device),
                                         torch.from_numpy(np.stack([t, t])).to(device),
                                         torch.tensor([1000, -3], dtype=torch.int32, device=device))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    st, M, mask, nin, iters = D.estimate_affine_partial_2d(f, t)
    assert (got["status"][0], got["n_inliers"][0], got["iters"][0]) == (st, nin, iters)
    assert np.array_equal(got["inlier_mask"][0].astype(bool), mask)
    assert np.abs(got["affine"][0, :, :2] - M[:, :2]).max() <= 1e-9
    assert np.abs(got["affine"][0, :, 2] - M[:, 2]).max() <= 1e-6
    assert got["status"][1] == 1 and got["n_inliers"][1] == 0 and not got["inlier_mask"][1].any()


def test_parameters_reach_the_kernel(batch, device):
    """A tighter threshold, fewer iterations and no refinement: still the oracle's result."""
    frm, to, counts, _ = batch
    rows = [7, 10]                                     # 64 points / 70 %, 1000 points / 30 %
    kw = dict(threshold=1.5, max_iters=40, confidence=0.999, refine_iters=0)
    out = detector.affine_partial_ransac(torch.from_numpy(frm[rows]).to(device),
                                         torch.from_numpy(to[rows]).to(device),
                                         torch.from_numpy(counts[rows]).to(device), **kw)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for i, b in enumerate(rows):
        n = counts[b]
        st, M, mask, nin, iters = D.estimate_affine_partial_2d(frm[b, :n], to[b, :n], **kw)
        assert (got["status"][i], got["n_inliers"][i], got["iters"][i]) == (st, nin, iters)
        assert np.array_equal(got["inlier_mask"][i, :n].astype(bool), mask)
        # no refinement: the winning pair's minimal model, the same float64 operations
        assert np.abs(got["affine"][i] - M).max() <= 1e-12 * max(1.0, np.abs(M).max())

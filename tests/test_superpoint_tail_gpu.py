"""The detector tail (onepose_superpoint_detect: simple_nms, threshold, borders, top-k) off the
32x32 NMS tile grid and at the selection kernels' limits, bit-exact against the numpy oracle.

Score maps here are quantised (multiples of 1/8), so plateaus of equal scores cross tile edges
everywhere -- what the == comparisons of simple_nms are sensitive to -- and top-k cuts through
large groups of ties.  Frames are no multiple of the NMS tile; batches mix samples that take
different selection modes (raster output, rank-in-bin, LDS sort); the LDS sort runs at its
capacity; the chunk scan runs with more than one chunk per thread."""
import numpy as np
import pytest
import torch

from onepose_amd import _lib
from onepose_amd.superpoint import detect_from_maps
from oracle import superpoint_np as O

pytestmark = pytest.mark.gpu
THR = 0.005


def unit_dense(b, h, w, seed):
    d = np.random.RandomState(seed).standard_normal((b, h // 8, w // 8, 256)).astype(np.float32)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def run_tail(device, s, dense, **kw):
    """detect_from_maps on a batch [B,H,W]; per sample (keypoints, scores, descriptors, count),
    after checking that the capacity past each count is zero-filled."""
    raw = detect_from_maps(torch.from_numpy(s).to(device), torch.from_numpy(dense).to(device),
                           align_corners=False, **kw)
    out = []
    for i, n in enumerate(raw["counts"].cpu().tolist()):
        assert 0 <= n <= raw["keypoints"].shape[1]
        assert not raw["keypoints"][i, n:].any() and not raw["scores"][i, n:].any()
        assert not raw["descriptors"][i, :, n:].any()
        out.append((raw["keypoints"][i, :n].cpu().numpy(), raw["scores"][i, :n].cpu().numpy(),
                    raw["descriptors"][i, :, :n].cpu().numpy(), n))
    return out


def assert_same(got, kp_o, sc_o, dense=None):
    kp, sc, desc, n = got
    assert n == len(kp_o)
    np.testing.assert_array_equal(kp, kp_o)
    np.testing.assert_array_equal(sc, sc_o)
    if dense is not None and n:
        d_o = O.sample_descriptors(kp_o[None], dense[None].transpose(0, 3, 1, 2), 8, False)[0]
        np.testing.assert_allclose(desc, d_o, atol=1e-6)


def quantised(h, w, seed):
    return (np.random.RandomState(seed).randint(0, 6, (h, w)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("radius", range(9))
@pytest.mark.parametrize("size", [(16, 16), (40, 56), (72, 104)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quantised_maps_match_oracle(size, radius, device):
    """Plateaus and ties everywhere, frames of 0.5 .. 3.25 NMS tiles: the fused NMS (radius
    <= 4) and the five-launch one (5 .. 8) on clipped tiles, then raster output and top-k."""
    h, w = size
    s = quantised(h, w, 100 * h + radius)
    dense = unit_dense(1, h, w, radius)
    nms = O.simple_nms(s, radius)
    for border in (0, 4, h // 2):
        kp_all, sc_all = O.select_keypoints(nms, THR, border, -1)
        total = len(kp_all)
        assert (total == 0) == (border == h // 2)     # h/2: nothing survives
        got = run_tail(device, s[None], dense, nms_radius=radius, keypoint_threshold=THR,
                       remove_borders=border, max_keypoints=-1)[0]
        assert_same(got, kp_all, sc_all)              # raster order, every survivor
        k = max(1, total // 3)
        kp_o, sc_o = O.select_keypoints(nms, THR, border, k)
        got = run_tail(device, s[None], dense, nms_radius=radius, keypoint_threshold=THR,
                       remove_borders=border, max_keypoints=k)[0]
        if total:
            assert total > k == len(kp_o) and np.all(sc_o[:-1] >= sc_o[1:])   # the top-k branch
            assert (sc_all == sc_o[-1]).sum() > 1     # ... cutting through a group of ties
        assert_same(got, kp_o, sc_o, dense[0])


def mixed_samples(h, w):
    rs = np.random.RandomState(42)
    sparse = np.zeros(h * w, np.float32)                 # 40 candidates < k: raster, zero tail
    sparse[rs.choice(h * w, 40, replace=False)] = rs.uniform(0.1, 1.0, 40).astype(np.float32)
    distinct = (0.05 + 0.9 * rs.permutation(h * w) / (h * w)).astype(np.float32)   # rank-in-bin
    assert len(np.unique(distinct)) == h * w
    tied = np.full(h * w, 0.5, np.float32)               # one bin of 4928 > 2048: the LDS sort
    return np.stack([sparse, distinct, tied]).reshape(3, h, w)


@pytest.mark.parametrize("order", [(0, 1, 2), (1, 2, 0), (2, 0, 1)], ids=lambda o: "".join(map(str, o)))
def test_batch_with_mixed_selection_modes(order, device):
    """One batch whose samples end in three different selection modes (chosen per sample on the
    device, read by the later kernels): each equals its single-image run and the oracle."""
    h, w, k = 64, 96, 100
    s = mixed_samples(h, w)[list(order)]
    dense = unit_dense(3, h, w, 3)[list(order)]
    kw = dict(nms_radius=0, keypoint_threshold=THR, remove_borders=4, max_keypoints=k)
    batch = run_tail(device, s, dense, **kw)
    counts = []
    for i in range(3):
        kp_o, sc_o = O.select_keypoints(O.simple_nms(s[i], 0), THR, 4, k)
        assert_same(batch[i], kp_o, sc_o, dense[i])
        one = run_tail(device, s[i:i + 1], dense[i:i + 1], **kw)[0]
        for a, b in zip(batch[i], one):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        counts.append(batch[i][3])
    assert sorted(counts)[0] < k and sorted(counts)[1:] == [k, k]
    tied = batch[order.index(2)]
    np.testing.assert_array_equal(tied[0][:3], [[4, 4], [5, 4], [6, 4]])   # ties: raster order


@pytest.mark.parametrize("k", [16384, 5000, 1])
def test_sort_path_at_its_limits(k, device):
    """25600 equal scores, radius 0: the LDS sort at its capacity (16384 keys), at a k that is
    no power of two, and at 1.  The winners are the first k pixels in raster order."""
    h = w = 160
    s = np.full((1, h, w), 0.5, np.float32)
    dense = unit_dense(1, h, w, k)
    got = run_tail(device, s, dense, nms_radius=0, keypoint_threshold=THR, remove_borders=0,
                   max_keypoints=k)[0]
    kp_o, sc_o = O.select_keypoints(O.simple_nms(s[0], 0), THR, 0, k)
    np.testing.assert_array_equal(kp_o[:, 1] * w + kp_o[:, 0], np.arange(k))
    assert_same(got, kp_o, sc_o, dense[0])


def test_k_at_the_survivor_count(device):
    """max_keypoints == survivors keeps raster order (total <= k); one less sorts."""
    h, w = 40, 56
    s = quantised(h, w, 7)
    dense = unit_dense(1, h, w, 7)
    nms = O.simple_nms(s, 2)
    total = len(O.select_keypoints(nms, THR, 4, -1)[0])
    assert total > 8
    for k in (total + 1, total, total - 1):
        kp_o, sc_o = O.select_keypoints(nms, THR, 4, k)
        raster = bool(np.all(np.diff(kp_o[:, 1] * w + kp_o[:, 0]) > 0))
        assert raster == (k >= total) and len(kp_o) == min(k, total)
        got = run_tail(device, s[None], dense, nms_radius=2, keypoint_threshold=THR,
                       remove_borders=4, max_keypoints=k)[0]
        assert_same(got, kp_o, sc_o, dense[0])


@pytest.mark.parametrize("k", [-1, 1400])
def test_negative_threshold_keeps_suppressed_zeros(k, device):
    """keypoint_threshold < 0: the zeros that NMS wrote over suppressed pixels are candidates
    (k = 1400 of the 1536 inner pixels cuts through that group of equal zeros)."""
    h, w = 40, 56
    s = quantised(h, w, 9) + np.float32(0.125)
    dense = unit_dense(1, h, w, 9)
    nms = O.simple_nms(s, 3)
    kp_o, sc_o = O.select_keypoints(nms, -1.0, 4, k)
    inside = (h - 8) * (w - 8)
    assert (sc_o == 0).any() and len(kp_o) == (inside if k < 0 else k)
    got = run_tail(device, s[None], dense, nms_radius=3, keypoint_threshold=-1.0,
                   remove_borders=4, max_keypoints=k)[0]
    assert_same(got, kp_o, sc_o, dense[0])


@pytest.mark.parametrize("peaks", [3000, 30000])
def test_scan_beyond_256_chunks(peaks, device):
    """1024x1032 = 258 chunks of 4096 pixels: the chunk scan's threads own two chunks each.
    3000 peaks stay below k (raster output straight from the scan's offsets); 30000 go
    through top-k.  Peaks in the last two chunks must come out (no border removed:
    the last chunk is the frame's last four rows)."""
    h, w, k = 1024, 1032, 4096
    rs = np.random.RandomState(peaks)
    s = np.zeros(h * w, np.float32)
    s[rs.choice(h * w, peaks, replace=False)] = rs.uniform(0.01, 0.9, peaks).astype(np.float32)
    s[256 * 4096 + 5::1500] = 1.0                       # chunks 256 and 257, top scores
    s = s.reshape(1, h, w)
    dense = unit_dense(1, h, w, 1)
    kp_o, sc_o = O.select_keypoints(O.simple_nms(s[0], 3), THR, 0, k)
    assert (len(kp_o) < k) == (peaks == 3000)
    idx = kp_o[:, 1] * w + kp_o[:, 0]
    assert (idx >= 257 * 4096).any() and ((idx >= 256 * 4096) & (idx < 257 * 4096)).any()
    got = run_tail(device, s, dense, nms_radius=3, keypoint_threshold=THR, remove_borders=0,
                   max_keypoints=k)[0]
    assert_same(got, kp_o, sc_o, dense[0])


def test_frames_below_16_are_refused(device):
    for h, w in ((8, 8), (8, 64)):
        with pytest.raises(_lib.OnePoseError, match=">= 16"):
            detect_from_maps(torch.zeros(1, h, w, device=device),
                             torch.zeros(1, h // 8, w // 8, 256, device=device))

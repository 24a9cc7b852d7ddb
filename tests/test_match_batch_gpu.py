"""The callers of the variable-count SuperGlue entry on the GPU: sfm.match_pairs(batch_size=4)
against the per-pair loop, and LocalFeatureObjectDetector(batch_views="all") against "equal".

Both comparisons are between two launch shapes of the same fp32 arithmetic (other tile and
workgroup shapes, so other summation orders), hence equal indices only away from the threshold:
each test first asserts, with the float64 oracle on the CPU, that no matching score of its case
lies within 1e-4 of the threshold (above two paths' ATOL = 2e-5)."""
import numpy as np
import pytest
import torch

import detector_cases as C
import superglue_oracle as oracle
from onepose_amd import detector, sfm, superglue, synthetic

pytestmark = pytest.mark.gpu
THR, MARGIN = 0.2, 1e-4
_cache = {}


def weights():
    if "sd" not in _cache:
        _cache["sd"] = synthetic.superglue_state_dict(11, affine_bn=True, bin_score=2.3457)
    return _cache["sd"]


def matcher(device):
    if "sg" not in _cache:
        _cache["sg"] = superglue.from_state_dict(
            weights(), {"sinkhorn_iterations": 20, "match_threshold": THR}).to(device)
    return _cache["sg"]


def views_of_one_image(counts, sizes, seed):
    """len(counts) - 1 views of one base image plus the base itself (last), trimmed to `counts`
    keypoints and scaled to `sizes` (h, w): [(keypoints [n, 2], scores [n], descriptors [256, n],
    (h, w))]."""
    B, n = len(counts) - 1, max(counts)
    d = synthetic.make_superglue_inputs(n, n, seed=seed, batch=B, shared1=True)
    raw = [(d["keypoints0"][b], d["scores0"][b], d["descriptors0"][b]) for b in range(B)]
    raw.append((d["keypoints1"][0], d["scores1"][0], d["descriptors1"][0]))
    out = []
    for (kp, sc, de), c, (h, w) in zip(raw, counts, sizes):
        scale = np.float32([w / synthetic.SUPERGLUE_IMAGE, h / synthetic.SUPERGLUE_IMAGE])
        out.append((np.ascontiguousarray(kp[:c] * scale), sc[:c].copy(),
                    np.ascontiguousarray(de[:, :c]), (h, w)))
    return out


def assert_margin(a, b, hw_a, hw_b, what):
    want = oracle.forward_one(weights(), a[2], a[0], a[1], b[2], b[0], b[1], hw_a, hw_b, 20, THR)
    for k in ("matching_scores0", "matching_scores1"):
        gap = np.abs(want[k] - THR).min()
        assert gap > MARGIN, f"{what}: an oracle {k} lies {gap:.3g} from the threshold; pick a seed"
    return want


class Counting:
    """A matcher wrapped to count its calls."""

    def __init__(self, inner):
        self.inner, self.calls, self.batches = inner, 0, []
        self.supports_counts = getattr(inner, "supports_counts", False)

    def cuda(self):
        return self

    def __call__(self, data):
        self.calls += 1
        self.batches.append(int(data["keypoints0"].shape[0]))
        return self.inner(data)


# ---------------------------------------------------------------- match_pairs
def test_match_pairs_batched_on_the_gpu(device):
    counts = (40, 70, 55, 63, 48, 66)
    sizes = ((480, 640), (384, 512)) * 3
    imgs = views_of_one_image(counts, sizes, seed=81)
    names = [f"obj/color/{i}.png" for i in range(6)]
    feats = {n: {"keypoints": kp, "scores": sc, "descriptors": de,
                 "image_size": np.array([hw[1], hw[0]])}
             for n, (kp, sc, de, hw) in zip(names, imgs)}
    idx = [(0, 5), (1, 5), (2, 5), (3, 4), (0, 1), (2, 3), (4, 5), (1, 3)]
    pairs = [(names[i], names[j]) for i, j in idx]
    n_matched = 0
    for i, j in idx:
        want = assert_margin(imgs[i], imgs[j], sizes[i], sizes[j], f"pair {i}-{j}")
        n_matched += int((want["matches0"] > -1).sum())
    assert n_matched > 50
    loop, batched = Counting(matcher(device)), Counting(matcher(device))
    a = sfm.match_pairs(feats, pairs, loop, device=device)
    b = sfm.match_pairs(feats, pairs, batched, device=device, batch_size=4)
    assert loop.calls == 8 and batched.calls < 8 and max(batched.batches) <= 4
    assert max(batched.batches) > 1
    assert list(a) == list(b)
    for (i, j), pair in zip(idx, a):
        assert list(a[pair]) == list(b[pair]) == ["matches0", "matches1", "matching_scores0",
                                                  "matching_scores1"]
        for k in a[pair]:
            assert a[pair][k].dtype == b[pair][k].dtype and a[pair][k].shape == b[pair][k].shape
        assert len(b[pair]["matches0"]) == counts[i] and len(b[pair]["matches1"]) == counts[j]
        assert np.array_equal(a[pair]["matches0"], b[pair]["matches0"]), pair
        assert np.array_equal(a[pair]["matches1"], b[pair]["matches1"]), pair
        for k in ("matching_scores0", "matching_scores1"):
            # float16: one step below 1 (the fp32 values may differ by 2 ATOL and round apart)
            diff = np.abs(a[pair][k].astype(np.float32) - b[pair][k].astype(np.float32)).max()
            assert diff <= 2.0 ** -11, (pair, k, diff)


# ---------------------------------------------------------------- the detector
def test_detector_with_all_views_in_one_call(device):
    counts = (48, 64, 57, 64, 40, 60)                       # five views, then the query
    sizes = ((240, 320), (240, 320), (250, 300), (240, 320), (250, 300), (480, 640))
    imgs = views_of_one_image(counts, sizes, seed=91)
    db = {}
    for i in range(5):
        kp, sc, de, hw = imgs[i]
        A = C.similarity(0.9 + 0.05 * i, 5.0 * i, 3.0 * i, 2.0)     # every view its own pose
        db[10 + i] = {"keypoints": (kp @ A[:, :2].T + A[:, 2]).astype(np.float32), "scores": sc,
                      "descriptors": de, "size": np.array(hw)}
    qk, qs, qd, qhw = imgs[5]
    for i in range(5):
        v = db[10 + i]
        # (the class hands the matcher (h, w) = the sizes reversed: a quirk it keeps)
        assert_margin((v["keypoints"], v["scores"], v["descriptors"]), (qk, qs, qd),
                      tuple(v["size"])[::-1], qhw[::-1], f"view {i}")
    dets = {}
    for mode in ("equal", "all"):
        sg = Counting(matcher(device))
        det = detector.LocalFeatureObjectDetector(None, sg, db_dict=db, batch_views=mode)
        raw = det.detect_raw(qk, qs, qd, qhw)
        torch.cuda.synchronize()
        dets[mode] = (sg, {k: raw[k].cpu().numpy() for k in ("matches0", "best_view", "best_bbox",
                                                             "bbox", "n_inliers", "status")})
    assert dets["equal"][0].calls == 4                      # (64, 240, 320) twice: one group
    assert dets["all"][0].calls == 1 and dets["all"][0].batches == [5]
    a, b = dets["equal"][1], dets["all"][1]
    assert (a["matches0"] > -1).sum() > 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        detector.LocalFeatureObjectDetector(None, matcher(device), db_dict=db, batch_views="some")

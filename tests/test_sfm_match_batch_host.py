"""Batched pair matching, host side (no GPU): plan_match_batches' three guarantees, and
match_pairs(batch_size=k) / reconstruct(match_batch=k) against the per-pair loop with a stub
matcher -- numpy mutual nearest neighbour that honours counts and per-sample image sizes."""
import numpy as np
import pytest
import torch

import sfm_cases
from onepose_amd import nn_matcher, sfm


# ---------------------------------------------------------------- plan_match_batches
def check_plan(counts, batch_size, ratio):
    groups = sfm.plan_match_batches(counts, batch_size, ratio)
    assert sorted(i for g in groups for i in g) == list(range(len(counts)))   # each pair once
    for g in groups:
        assert 1 <= len(g) <= batch_size
        real = sum(counts[i][0] + counts[i][1] for i in g)
        pad = len(g) * (max(counts[i][0] for i in g) + max(counts[i][1] for i in g))
        assert pad <= (1 + ratio) * real, (g, pad, real)
    assert groups == sfm.plan_match_batches(list(counts), batch_size, ratio)   # deterministic
    return groups


def test_plan_covers_every_pair_once_within_both_caps():
    rs = np.random.RandomState(3)
    counts = [(int(a), int(b)) for a, b in rs.randint(300, 2049, size=(200, 2))]
    for bs in (1, 4, 8, 16):
        for ratio in (0.0, 0.1, 0.25, 1.0):
            groups = check_plan(counts, bs, ratio)
            if bs == 1:
                assert len(groups) == 200
    # the caps bind: a looser ratio never needs more groups here, and batches do form
    assert len(check_plan(counts, 16, 0.25)) < 100
    assert len(check_plan(counts, 16, 1.0)) <= len(check_plan(counts, 16, 0.25))


def test_plan_edge_cases():
    assert sfm.plan_match_batches([], 8) == []
    assert sfm.plan_match_batches([(40, 50)], 8) == [[0]]
    # all equal: full batches in index order (the sort is stable)
    assert check_plan([(64, 64)] * 10, 4, 0.25) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    # one huge pair among small ones stays alone
    counts = [(50, 50)] * 5 + [(2000, 2000)] + [(52, 49)] * 3
    groups = check_plan(counts, 16, 0.25)
    assert [5] in groups and len(groups) == 2
    # zero padding allowed: only identical shapes share a group
    groups = check_plan([(5, 5), (5, 6), (5, 5), (6, 5)], 8, 0.0)
    assert sorted(map(sorted, groups)) == [[0, 2], [1], [3]]
    with pytest.raises(ValueError):
        sfm.plan_match_batches([(1, 1)], 0)
    with pytest.raises(ValueError):
        sfm.plan_match_batches([(1, 1)], 4, -0.5)


# ---------------------------------------------------------------- the stub matcher
class StubMatcher:
    """Mutual nearest neighbour on d0 . d1 - |k0 / s0 - k1 / s1| (s = the longer image side), in
    numpy.  Reads counts0/1 and image_hw0/1 when given (a padded batch), the image tensors'
    shapes otherwise; padded slots are never read and come back as -1 / 0."""
    supports_counts = True

    def __init__(self):
        self.calls, self.batches = 0, []

    def __call__(self, data):
        self.calls += 1
        d0, d1 = data["descriptors0"].numpy(), data["descriptors1"].numpy()
        k0, k1 = data["keypoints0"].numpy(), data["keypoints1"].numpy()
        B, n0, n1 = d0.shape[0], d0.shape[2], d1.shape[2]
        self.batches.append(B)
        counted = "counts0" in data
        assert counted == ("image_hw0" in data) == ("counts1" in data) == ("image_hw1" in data)
        out = {"matches0": np.full((B, n0), -1, np.int64), "matches1": np.full((B, n1), -1, np.int64),
               "matching_scores0": np.zeros((B, n0), np.float32),
               "matching_scores1": np.zeros((B, n1), np.float32)}
        for b in range(B):
            if counted:
                c0, c1 = int(data["counts0"][b]), int(data["counts1"][b])
                hw0, hw1 = data["image_hw0"][b].tolist(), data["image_hw1"][b].tolist()
            else:
                c0, c1 = n0, n1
                hw0, hw1 = data["image0"].shape[-2:], data["image1"].shape[-2:]
            if c0 == 0 or c1 == 0:
                continue
            a0 = k0[b, :c0] / np.float32(max(hw0))
            a1 = k1[b, :c1] / np.float32(max(hw1))
            S = d0[b, :, :c0].T @ d1[b, :, :c1] - np.abs(a0[:, None] - a1[None]).sum(-1)
            i0, i1 = S.argmax(1), S.argmax(0)
            mutual0 = i1[i0] == np.arange(c0)
            mutual1 = i0[i1] == np.arange(c1)
            out["matches0"][b, :c0] = np.where(mutual0, i0, -1)
            out["matches1"][b, :c1] = np.where(mutual1, i1, -1)
            out["matching_scores0"][b, :c0] = np.where(mutual0, S.max(1), 0)
            out["matching_scores1"][b, :c1] = np.where(mutual1, S.max(0), 0)
        return {k: torch.from_numpy(v) for k, v in out.items()}


def ragged_features(n_images=7, seed=5):
    """Images with 40..70 keypoints (one with none), two image sizes."""
    rs = np.random.RandomState(seed)
    base = rs.standard_normal((80, 256)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    feats = {}
    for i in range(n_images):
        n = 0 if i == 3 else int(rs.randint(40, 71))
        w, h = ((640, 480), (512, 384))[i % 2]
        pick = rs.permutation(80)[:n]
        d = base[pick] + 0.05 * rs.standard_normal((n, 256)).astype(np.float32)
        feats[f"seq/color/{i}.png"] = {
            "keypoints": (rs.uniform(0, 1, (n, 2)) * [w, h]).astype(np.float32),
            "descriptors": np.ascontiguousarray(d.T.astype(np.float32)).reshape(256, n),
            "scores": rs.uniform(0.1, 1, n).astype(np.float32),
            "image_size": np.array([w, h])}
    return feats


def assert_same_matches(a, b):
    assert list(a) == list(b)                              # keys, in order
    for pair in a:
        assert list(a[pair]) == list(b[pair]), pair
        for k in a[pair]:
            assert a[pair][k].dtype == b[pair][k].dtype and a[pair][k].shape == b[pair][k].shape
            assert np.array_equal(a[pair][k], b[pair][k]), (pair, k)


def test_match_pairs_batched_equals_the_per_pair_loop():
    feats = ragged_features()
    names = list(feats)
    pairs = [(names[i], names[j]) for i in range(7) for j in range(7) if i != j and (i + j) % 3]
    pairs.insert(4, pairs[0])                              # a repeat and reverses: the skip rule
    loop_stub, stub = StubMatcher(), StubMatcher()
    want = sfm.match_pairs(feats, pairs, loop_stub)
    assert set(loop_stub.batches) == {1} and len(want) == loop_stub.calls
    assert len(want) < len(pairs)                          # reverses were skipped
    for bs in (1, 3, 8):
        stub = StubMatcher()
        got = sfm.match_pairs(feats, pairs, stub, batch_size=bs, max_pad_ratio=0.5)
        assert_same_matches(want, got)
        assert max(stub.batches) <= bs
        if bs > 1:
            assert stub.calls < loop_stub.calls and max(stub.batches) > 1
    # every stored array has its pair's own length and the per-pair dtypes
    for (n0, n1) in [p for p in pairs]:
        grp = got[sfm.names_to_pair(n0, n1)] if sfm.names_to_pair(n0, n1) in got else None
        if grp is not None:
            assert grp["matches0"].dtype == np.int16 and grp["matching_scores0"].dtype == np.float16
            assert len(grp["matches0"]) == len(feats[n0]["scores"])
            assert len(grp["matches1"]) == len(feats[n1]["scores"])
    assert any((g["matches0"] > -1).any() for g in got.values())


def test_pairs_with_an_empty_side_take_the_old_path():
    feats = ragged_features()
    names = list(feats)
    pairs = [(names[0], names[3]), (names[3], names[1]), (names[0], names[1]), (names[2], names[4])]
    stub = StubMatcher()
    got = sfm.match_pairs(feats, pairs, stub, batch_size=8, max_pad_ratio=10.0)
    assert_same_matches(sfm.match_pairs(feats, pairs, StubMatcher()), got)
    assert sorted(stub.batches) == [1, 1, 2]               # one batch of two, the empties alone
    assert len(got[sfm.names_to_pair(names[0], names[3])]["matches1"]) == 0


def test_a_matcher_without_counts_is_refused():
    feats = ragged_features()
    names = list(feats)
    with pytest.raises(ValueError, match="supports_counts"):
        sfm.match_pairs(feats, [(names[0], names[1])], nn_matcher.NearestNeighbour(), batch_size=4)
    from onepose_amd import superglue
    assert superglue.SuperGlue.supports_counts is True
    assert not getattr(nn_matcher.NearestNeighbour, "supports_counts", False)


def test_reconstruct_with_match_batch_equals_without():
    feats, names, poses, Ks, pts, owner = sfm_cases.scene()
    feats = {n: dict(f) for n, f in feats.items()}
    for i, n in enumerate(names):                          # unequal counts: drop trailing features
        keep = len(feats[n]["scores"]) - 9 * (i % 4)
        feats[n]["keypoints"] = feats[n]["keypoints"][:keep]
        feats[n]["scores"] = feats[n]["scores"][:keep]
        feats[n]["descriptors"] = np.ascontiguousarray(feats[n]["descriptors"][:, :keep])
    a = sfm.reconstruct(feats, names, poses, Ks, StubMatcher(), covis_num=10, device=None)
    stub = StubMatcher()
    b = sfm.reconstruct(feats, names, poses, Ks, stub, covis_num=10, device=None, match_batch=6)
    assert max(stub.batches) > 1
    assert len(a["ids"]) > 100
    for k in ("ids", "xyz", "error", "track_len"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("point3D_ids", "track_image_ids", "track_point2D_idxs"):
        assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k

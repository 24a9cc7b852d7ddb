"""Shared by tests/test_match_counts_host.py and tests/test_match_counts_gpu.py: the batches of
unequal keypoint counts the 2D-3D counts matcher (include/onepose_match_counts.h) is held to, their
inputs, and the numpy oracle run per sample on that sample's first c keypoints.

Every case is one object (n3 = 200 points, 8 leaves, synthetic seed below) and B frames of it
padded to n1 keypoints; sample b's count is counts[b].  The oracle results are computed once per
process and shared by every test that needs them (they are never modified).

Which kernel path each case holds (matcher.hip: qkv_tile_for, kFusedFoldMaxBatch; gemm.hip).  MLP
conv 1 is always 64x64 and the score GEMM 128x64W8; the QKV tile is that of the 2D side.

  edges     B = 6, n1 = 160, 32x128 QKV, kv_reduce + m_fold (B = 6 is past kFusedFoldMaxBatch = 4).
            Counts 160 (full), 129, 128, 97, 33: the row edges at 32 (QKV), 64 (MLP conv 1
            statistics) and 128 (score); 1: a single token.
  fused     B = 4, n1 = 160: the same edges on the fused kv_fold256.
  empty     B = 3, n1 = 160, kv_fold256: a count of 0 between two full samples.
  groups_a  B = 2, n1 = 600, kv_fold256: 600 rows = 10 statistic tiles = two first-level
  groups_b  InstanceNorm groups (8 + 2 tiles); counts 600 / 513 and 512 / 511 leave the second
            group whole, with one row, empty, and the first group one row short.
  fold5     B = 5, n1 = 160: the smallest batch on kv_reduce + m_fold.
  wide_w8   B = 8, n1 = 384: 6 x 6 x 8 = 288 >= 256 64-row tiles -> TILE_128x128W8 in layers 1-2
            (32x128 later: n3 gives 4 x 6 x 8 = 192), kv_reduce + m_fold.  Counts 321, 320, 257
            split a 128-row tile's 64-row sub-tiles.
  wide_128  B = 32, n1 = 1408: 22 x 6 x 32 = 4224 >= 4096 -> TILE_128x128 in layers 1-2 and
            TILE_128x128W8 on both sides later (n3: 4 x 6 x 32 = 768).  Count 1281 leaves the last
            128-row KV chunk one row; 385; and 30 small counts with whole tiles past them.  (Its 32
            samples exist to reach the tile; the first ten are held against the oracle.)
"""
import functools

import numpy as np

from onepose_amd import synthetic

N3, L = 200, 8
THR = 0.2
MARGIN = 1e-4      # no oracle score of any case lies this close to the threshold

_SMALL = (1, 17, 33, 64, 65, 100, 128, 129, 160, 31, 96, 0, 2, 63, 97, 150)
CASES = {
    "edges": dict(B=6, n1=160, seed=3, counts=(160, 129, 128, 97, 33, 1)),
    "fused": dict(B=4, n1=160, seed=3, counts=(129, 128, 33, 97)),
    "empty": dict(B=3, n1=160, seed=3, counts=(160, 0, 160)),
    "groups_a": dict(B=2, n1=600, seed=4, counts=(600, 513)),
    "groups_b": dict(B=2, n1=600, seed=4, counts=(512, 511)),
    "fold5": dict(B=5, n1=160, seed=3, counts=(160, 130, 64, 31, 2)),
    "wide_w8": dict(B=8, n1=384, seed=5, counts=(384, 321, 320, 257, 129, 64, 33, 1)),
    "wide_128": dict(B=32, n1=1408, seed=6,
                     counts=(1281, 385) + tuple(_SMALL[i % 16] for i in range(30)),
                     check=range(10)),
}


def checked(name):
    """The samples of the case that are held against the oracle: all, but for wide_128, whose 32
    samples exist to reach the tile (its first 10 are compared: both large counts and 8 small)."""
    c = CASES[name]
    return list(c.get("check", range(c["B"])))


@functools.lru_cache(maxsize=None)
def state_dict(seed=0):
    return synthetic.make_state_dict(seed)     # the well-conditioned synthetic weights


@functools.lru_cache(maxsize=None)
def _inputs(n1, seed, B):
    data, _, _ = synthetic.make_matcher_inputs(n1, N3, L, seed=seed, batch=B)
    return data


def inputs(name):
    """The case's padded inputs (reference layout, numpy; do not modify) and its counts."""
    c = CASES[name]
    return _inputs(c["n1"], c["seed"], c["B"]), np.asarray(c["counts"], np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(n1, seed, B, b, cnt):
    from oracle import matcher_np as M
    data = _inputs(n1, seed, B)
    one = {k: v[b:b + 1] for k, v in data.items()}
    one["keypoints2d"] = one["keypoints2d"][:, :cnt]
    one["descriptors2d_query"] = one["descriptors2d_query"][:, :, :cnt]
    out = M.forward(state_dict(), one)
    if isinstance(out, dict):          # the reference's empty-input result
        return out, np.zeros((0, N3), np.float32)
    return out[0], out[1][0]


def oracle(name, b):
    """(pred, conf [c, n3]) of sample b of the case run alone on its first c keypoints."""
    c = CASES[name]
    return _oracle(c["n1"], c["seed"], c["B"], b, int(c["counts"][b]))


def padded_reference(name, b):
    """The oracle's result of sample b in the padded shapes the counts entries return: past the
    count matches0 = -1, scores 0 and zero conf rows."""
    c = CASES[name]
    n1, cnt = c["n1"], int(c["counts"][b])
    pred, conf = oracle(name, b)
    m0 = np.full(n1, -1, np.int64)
    s0 = np.zeros(n1, np.float32)
    cf = np.zeros((n1, N3), np.float32)
    m0[:cnt] = pred["matches0"]
    s0[:cnt] = pred["matching_scores0"]
    cf[:cnt] = conf
    return {"matches0": m0, "matches1": np.asarray(pred["matches1"], np.int64),
            "matching_scores0": s0,
            "matching_scores1": np.asarray(pred["matching_scores1"], np.float32)}, cf


def threshold_margin(name):
    """min |score - 0.2| over every oracle score of the case, and its matched-row count."""
    c = CASES[name]
    margin, matched = np.inf, 0
    for b in checked(name):
        pred, _ = oracle(name, b)
        for k in ("matching_scores0", "matching_scores1"):
            s = np.asarray(pred[k], np.float64)
            if s.size:
                margin = min(margin, float(np.abs(s - THR).min()))
        matched += int((np.asarray(pred["matches0"]) > -1).sum())
    return margin, matched

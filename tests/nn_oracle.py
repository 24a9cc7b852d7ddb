"""numpy restatement of the NearestNeighbour matcher (nearest_neighbour.py:5-63), test oracle.

Similarities are summed in float64 and rounded once to float32; everything after that is the
reference's float32 arithmetic, operation by operation: ``dist = 2 * (1 - sim)``, the ratio test
``dist_best <= float32(ratio ** 2) * dist_second``, the distance test ``dist_best <=
float32(distance ** 2)``, ``score = (sim_best + 1) / 2``.  ``if ratio:`` / ``if distance:`` are
truthiness tests (None and 0 disable), only matches0 gets the mutual check and scores0 keeps its
value where the check clears a match.

Where torch.topk promises no order this build's rule applies: the best is the lowest index among
equal similarities, and the second value is the second element of the multiset (a duplicated best
value is its own runner-up).

``forward`` also returns, in float64, what the tests select inputs by: each row's and column's
best-minus-second gap (inf with one candidate) and the distance of every enabled decision from
its boundary, ``|lhs - rhs|``.
"""
import numpy as np

F32 = np.float32


def similarities(desc0, desc1):
    """float64 sim [B, n0, n1]; a side with batch dimension 1 is shared."""
    a = np.asarray(desc0, dtype=np.float64)
    b = np.asarray(desc1, dtype=np.float64)
    B = max(a.shape[0], b.shape[0])
    a = np.broadcast_to(a, (B,) + a.shape[1:])
    b = np.broadcast_to(b, (B,) + b.shape[1:])
    return np.einsum("bdn,bdm->bnm", a, b)


def _top2(s):
    """best value, lowest index of it, second element of the multiset (-inf if alone)."""
    ind = np.argmax(s, axis=-1)                       # the first maximum: the lowest index
    best = np.take_along_axis(s, ind[..., None], -1)[..., 0]
    if s.shape[-1] == 1:
        return best, ind, np.full_like(best, -np.inf)
    rest = s.copy()
    np.put_along_axis(rest, ind[..., None], -np.inf, -1)
    return best, ind, rest.max(axis=-1)


def find_nn(sim64, ratio, distance):
    s32 = sim64.astype(F32)
    best, ind, second = _top2(s32)
    if ratio and s32.shape[-1] < 2:
        raise RuntimeError("the ratio test needs 2 candidates (topk(2) raises in the reference)")
    d0 = F32(2) * (F32(1) - best)
    d1 = F32(2) * (F32(1) - second)
    mask = np.ones(best.shape, bool)
    b64, _, s64 = _top2(sim64)
    gap = b64 - s64
    slack = np.full(best.shape, np.inf)
    e0, e1 = 2.0 * (1.0 - b64), 2.0 * (1.0 - s64)
    if ratio:
        mask &= d0 <= F32(ratio ** 2) * d1
        slack = np.minimum(slack, np.abs(e0 - ratio ** 2 * e1))
    if distance:
        mask &= d0 <= F32(distance ** 2)
        slack = np.minimum(slack, np.abs(e0 - distance ** 2))
    matches = np.where(mask, ind, -1).astype(np.int64)
    scores = np.where(mask, (best + F32(1)) / F32(2), F32(0)).astype(F32)
    return matches, scores, gap, slack


def forward(desc0, desc1, ratio=None, distance=None, mutual=True):
    sim = similarities(desc0, desc1)
    m0, s0, gap0, slack0 = find_nn(sim, ratio, distance)
    m1, s1, gap1, slack1 = find_nn(np.ascontiguousarray(sim.transpose(0, 2, 1)), ratio, distance)
    if mutual:
        loop = np.take_along_axis(m1, np.where(m0 > -1, m0, 0), -1)
        ok = (m0 > -1) & (loop == np.arange(m0.shape[-1])[None])
        m0 = np.where(ok, m0, -1)
    return {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1,
            "gap0": gap0, "gap1": gap1, "slack0": slack0, "slack1": slack1,
            "scale": max(1.0, float(np.abs(sim).max()))}


def from_conf(desc0, desc1, conf):
    """forward with the reference's conf dict (missing keys: its defaults)."""
    return forward(desc0, desc1, conf.get("ratio_threshold"), conf.get("distance_threshold"),
                   conf.get("do_mutual_check", True))


def well_separated(out):
    """The input-selection bounds: every gap >= 2e-5 x scale, every decision >= 1e-3 x scale
    from its boundary (scale = max(1, largest |sim|))."""
    s = out["scale"]
    return (min(out["gap0"].min(), out["gap1"].min()) >= 2e-5 * s
            and min(out["slack0"].min(), out["slack1"].min()) >= 1e-3 * s)

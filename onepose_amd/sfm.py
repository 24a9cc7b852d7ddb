"""Sparse reconstruction: from posed images and their features to an SfM model.

The reference's ``sfm_core`` (``run.py:140-193``) after feature extraction, stage by stage:

* ``get_pairwise_distances`` / ``covis_from_pose`` / ``write_pairs``
                              -- ``src/sfm/pairs_from_poses.py:7-70``, quirks included
* ``names_to_pair`` / ``match_pairs``
                              -- ``src/sfm/match_features.py:20-84`` (the pair loop, its skip rule
                                 and output dtypes; the matcher is any module of this package)
* ``import_matches``          -- ``src/sfm/triangulation.py:83-116``, into graph edges instead of
                                 a sqlite database
* ``rotmat2qvec`` / ``empty_model`` / ``write_model_binary``
                              -- ``src/sfm/generate_empty.py:31-90`` and COLMAP's binary model
                                 format, byte for byte what the reference's ``write_model`` writes
* ``fundamental_from_poses`` / ``verify_matches``
                              -- the step the reference leaves to COLMAP's ``matches_importer``
                                 (``triangulation.py:18-35``), between ``import_matches`` and the
                                 triangulator.  **This project's own**: per pair a fundamental
                                 matrix by RANSAC over the normalised 8-point algorithm (or the F of
                                 the given poses), squared Sampson error, as stated in
                                 ``include/onepose_two_view.h``.  Parity with COLMAP is not verified.
* ``build_tracks`` / ``triangulate_tracks``
                              -- what the reference leaves to a COLMAP binary
                                 (``triangulation.py:122-148``).  **This project's own**: tracks
                                 are the connected components of the match graph, and the
                                 triangulator is the one stated in ``include/onepose_hip.h``
                                 ("Sparse reconstruction").  Parity with COLMAP is not verified.
* ``global_bundle_adjust``    -- the step the reference leaves to COLMAP's ``bundle_adjuster``
                                 (``src/sfm/global_ba.py``: extrinsics refined, intrinsics
                                 fixed).  **This project's own**: Levenberg-Marquardt with
                                 preconditioned CG on the implicit Schur complement, as stated in
                                 ``include/onepose_global_ba.h`` (``onepose_amd/global_ba.py``).
                                 Parity with COLMAP or Ceres is not claimed.
* ``reconstruct``             -- the chain; its result feeds ``object_builder.build_object``.

The host stages are numpy only.  ``verify_matches``, ``build_tracks`` and ``triangulate_tracks``
take ``device=``: with a GPU device the HIP kernels of ``csrc/two_view.hip`` and ``csrc/sfm.hip``
run; with ``device=None`` the same contract runs on the host.

Out of scope: COLMAP's own verifier (E and H models, LO-RANSAC, cheirality tests, two-view
geometries written to a database), its RANSAC triangulation, its bundle adjuster's
parametrisation, robust losses and refinement of intrinsics, filtering or re-triangulating
points after the adjustment, point colours, the sqlite database, ``model_analyzer`` statistics,
PLY export, batching pairs into one matcher call.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib
from .global_ba import global_bundle_adjust  # noqa: F401  (a stage of this module's chain)
from .object_builder import _gpu

MIN_ROTATION = 10   # degrees, pairs_from_poses.py:45
MAX_REPROJ, MIN_ANGLE_DEG = 4.0, 1.5
REASONS = {0: "kept", 1: "fewer than 2 inliers", 2: "triangulation angle too small",
           3: "track length outside 2..256", 4: "non-finite"}
TRI_STATUS = {1: "track_start is not a monotone CSR over the observations",
              2: "an image id outside the cameras"}
CC_ROUNDS, CC_MAX_CALLS = 16, 8


# ------------------------------------------------------------------ pairs from poses
def _load_poses(poses):
    if isinstance(poses, np.ndarray):
        return np.asarray(poses, dtype=np.float64)
    return np.stack([np.loadtxt(p) if isinstance(p, (str, os.PathLike)) else np.asarray(p, float)
                     for p in poses], axis=0)


def get_pairwise_distances(poses):
    """``poses``: ``[n, 4, 4]`` world-to-camera matrices or a list of pose files.  Returns
    ``(dist, dR)``: the distances between the camera centres ``-R^T t`` and the rotation angles
    between the views in degrees."""
    P = _load_poses(poses)
    Rs = P[:, :3, :3].transpose(0, 2, 1)
    ts = -(Rs @ P[:, :3, 3:])[:, :, 0]
    d = ts[:, None, :] - ts[None, :, :]
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    trace = np.einsum('nji,mji->mn', Rs, Rs, optimize=True)
    dR = np.clip((trace - 1) / 2, -1., 1.)
    dR = np.rad2deg(np.abs(np.arccos(dR)))
    return dist, dR


def _sequences(n, poses, seq_ids):
    if seq_ids is None:
        if isinstance(poses, np.ndarray) or not all(isinstance(p, (str, os.PathLike)) for p in poses):
            seq_ids = [""] * n
        else:
            seq_ids = [os.path.basename(os.path.dirname(os.path.dirname(os.fspath(p)))) for p in poses]
    seqs = {}
    for i, s in enumerate(seq_ids):
        seqs.setdefault(s, []).append(i)
    return seqs


def covis_from_pose(img_lists, poses, num_matched, max_rotation=None, seq_ids=None):
    """The reference's covisible pairs as a list of ``(name0, name1)``.  As there: a pair needs
    more than 10 degrees between its views; ``max_rotation`` is never read; every sequence
    contributes ``num_matched // n_seqs`` candidates per image, every second one of numpy's
    ``argpartition`` order; when twice that count is out of range the whole sequence is taken
    (and that fallback itself raises unless the sequence is all the images).  Sequence names are
    ``basename(dirname(dirname(pose_file)))`` unless ``seq_ids`` gives one per image."""
    dist, dR = get_pairwise_distances(poses)
    seqs = _sequences(len(img_lists), poses, seq_ids)
    valid = dR > MIN_ROTATION
    np.fill_diagonal(valid, False)
    dist = np.where(valid, dist, np.inf)
    pairs = []
    per_seq = num_matched // len(seqs)
    for i in range(len(img_lists)):
        dist_i = dist[i]
        for ids in seqs.values():
            ids = np.array(ids)
            try:
                idx = np.argpartition(dist_i[ids], per_seq * 2)[:per_seq:2]
            except Exception:
                idx = np.argpartition(dist_i[ids], dist_i.shape[0] - 1)
            idx = ids[idx]
            idx = idx[np.argsort(dist_i[idx])]
            idx = idx[valid[i][idx]]
            pairs.extend((img_lists[i], img_lists[j]) for j in idx)
    return pairs


def write_pairs(path, pairs):
    with open(path, "w") as f:
        f.write("\n".join(" ".join([i, j]) for i, j in pairs))


# ------------------------------------------------------------------ match export / import
def names_to_pair(name0, name1):
    return "_".join((name0.replace("/", "-"), name1.replace("/", "-")))


def plan_match_batches(counts, batch_size, max_pad_ratio=0.25):
    """Groups of pair indices for padded matcher calls.  ``counts``: the list of ``(n0, n1)`` of
    the pairs to match (after the skip rule).  Every pair appears in exactly one group; no group
    has more than ``batch_size`` pairs; and in every group the padded token count
    ``B * (max n0 + max n1)`` is at most ``(1 + max_pad_ratio)`` times the group's real token
    count ``sum(n0 + n1)`` (a pair alone always satisfies this).  Pure Python and deterministic:
    a stable sort by ``(n0, n1)`` and a greedy walk that closes a group when the next pair would
    break a cap.  The default of 0.25 is a first guess, not a tuned value."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}: at least 1")
    if not max_pad_ratio >= 0:
        raise ValueError(f"max_pad_ratio {max_pad_ratio}: a number >= 0")
    counts = [(int(a), int(b)) for a, b in counts]
    order = sorted(range(len(counts)), key=lambda i: counts[i])
    groups, cur, m0, m1, real = [], [], 0, 0, 0
    for i in order:
        n0, n1 = counts[i]
        if cur:
            g0, g1, r = max(m0, n0), max(m1, n1), real + n0 + n1
            if len(cur) < batch_size and (len(cur) + 1) * (g0 + g1) <= (1 + max_pad_ratio) * r:
                cur.append(i)
                m0, m1, real = g0, g1, r
                continue
            groups.append(cur)
        cur, m0, m1, real = [i], n0, n1, n0 + n1
    if cur:
        groups.append(cur)
    return groups


def _pair_outputs(pred, b, n0, n1):
    """Sample ``b`` of a matcher's prediction as ``match_pairs`` stores it: trimmed to the pair's
    own counts, int16 matches and float16 scores."""
    grp = {"matches0": pred["matches0"][b, :n0].cpu().short().numpy(),
           "matches1": pred["matches1"][b, :n1].cpu().short().numpy()}
    for k, n in (("matching_scores0", n0), ("matching_scores1", n1)):
        if k in pred:
            grp[k] = pred[k][b, :n].cpu().half().numpy()
    return grp


def _match_group(features, todo, matcher, device):
    """One padded matcher call over the pairs ``todo`` (``(name0, name1)``, both sides non-empty):
    every per-keypoint key padded with zeros to the group's maxima, ``counts0/1`` and
    ``image_hw0/1`` saying where each sample ends and how large its image is."""
    sides = [[features[p[s]] for p in todo] for s in (0, 1)]
    data = {}
    for s, feats in enumerate(sides):
        ns = [int(np.asarray(f["keypoints"]).reshape(-1, 2).shape[0]) for f in feats]
        nmax = max(ns)
        for k in feats[0].keys():
            if k == "image_size":
                continue
            arrs = [np.asarray(f[k], dtype=np.float32) for f in feats]
            # the keypoint axis: the first for keypoints [n, 2] and scores [n], the last for
            # descriptors [256, n]
            axis = arrs[0].ndim - 1 if k == "descriptors" else 0
            if any(a.ndim == 0 or a.shape[axis] != n for a, n in zip(arrs, ns)):
                raise ValueError(f"match_pairs: feature key {k!r} has no keypoint axis; batched "
                                 "matching pads keypoints, scores and descriptors only")
            shape = list(arrs[0].shape)
            shape[axis] = nmax
            buf = np.zeros([len(feats)] + shape, np.float32)
            for b, (a, n) in enumerate(zip(arrs, ns)):
                idx = [b] + [slice(None)] * a.ndim
                idx[1 + axis] = slice(0, n)
                buf[tuple(idx)] = a
            data[f"{k}{s}"] = torch.from_numpy(buf).to(device or "cpu")
        data[f"counts{s}"] = torch.tensor(ns, dtype=torch.int32, device=device or "cpu")
        # image_size is (w, h)
        data[f"image_hw{s}"] = torch.tensor(
            [[int(v) for v in np.asarray(f["image_size"]).reshape(2)[::-1]] for f in feats],
            dtype=torch.int32, device=device or "cpu")
        data[f"image_size{s}"] = torch.tensor(
            np.stack([np.asarray(f["image_size"], np.float32).reshape(-1) for f in feats])
        ).to(device or "cpu")
    return matcher(data), data["counts0"].tolist(), data["counts1"].tolist()


@torch.no_grad()
def match_pairs(features, pairs, matcher, device=None, batch_size=None, max_pad_ratio=0.25):
    """One matcher call per pair -> ``{pair name: {'matches0' int16, 'matches1' int16,
    'matching_scores0' float16, 'matching_scores1' float16}}``.  A pair is skipped when it or its
    reverse was matched before.  ``features``: ``name -> {key: array}`` with ``image_size`` (w, h)
    among the keys; every key reaches the matcher with the side's suffix, as a float tensor with
    a batch axis on ``device``.

    ``batch_size``: None is the loop above.  A number batches the pairs: ``plan_match_batches``
    groups them (at most ``batch_size`` pairs and ``max_pad_ratio`` of padding per group), each
    group is one padded matcher call with ``counts0/1`` and ``image_hw0/1``, and every pair's
    outputs are trimmed to its own counts; the mapping has the same keys in the same order.  The
    matcher must declare ``supports_counts = True`` (``SuperGlue`` does).  A pair with an empty
    side never enters a batch and takes the per-pair path."""
    if batch_size is not None and not getattr(matcher, "supports_counts", False):
        raise ValueError(f"match_pairs(batch_size={batch_size}): {type(matcher).__name__} does not "
                         "declare supports_counts (padded batches with per-sample counts)")
    out, matched, todo = {}, set(), []
    for name0, name1 in pairs:
        pair = names_to_pair(name0, name1)
        if len({(name0, name1), (name1, name0)} & matched) or pair in out:
            continue
        out[pair] = None   # (keeps the mapping in pair order)
        todo.append((name0, name1))
        matched |= {(name0, name1), (name1, name0)}
    count = lambda name: int(np.asarray(features[name]["keypoints"]).reshape(-1, 2).shape[0])  # noqa: E731
    batched = ([p for p in todo if count(p[0]) > 0 and count(p[1]) > 0]
               if batch_size is not None else [])
    for group in plan_match_batches([(count(a), count(b)) for a, b in batched], batch_size or 1,
                                    max_pad_ratio):
        names = [batched[i] for i in group]
        pred, ns0, ns1 = _match_group(features, names, matcher, device)
        for b, (name0, name1) in enumerate(names):
            out[names_to_pair(name0, name1)] = _pair_outputs(pred, b, ns0[b], ns1[b])
    for name0, name1 in todo:
        pair = names_to_pair(name0, name1)
        if out[pair] is not None:
            continue
        feats0, feats1 = features[name0], features[name1]
        data = {}
        for k in feats0.keys():
            data[k + "0"] = np.asarray(feats0[k])
        for k in feats1.keys():
            data[k + "1"] = np.asarray(feats1[k])
        data = {k: torch.from_numpy(np.ascontiguousarray(v))[None].float().to(device or "cpu")
                for k, v in data.items()}
        data["image0"] = torch.empty((1, 1) + tuple(int(v) for v in feats0["image_size"])[::-1])
        data["image1"] = torch.empty((1, 1) + tuple(int(v) for v in feats1["image_size"])[::-1])
        pred = matcher(data)
        grp = {"matches0": pred["matches0"][0].cpu().short().numpy(),
               "matches1": pred["matches1"][0].cpu().short().numpy()}
        for k in ("matching_scores0", "matching_scores1"):
            if k in pred:
                grp[k] = pred[k][0].cpu().half().numpy()
        out[pair] = grp
    return out


def import_matches(pairs, matches, image_ids, min_match_score=None, *, offsets):
    """The matches the reference imports into COLMAP's database, as the edges ``[E, 2]`` int32
    of the feature graph: a feature's node is ``offsets[name]`` + its keypoint index.  Pairs are
    deduplicated by their image-id set; ``matches0 > -1``, and ``scores > min_match_score`` when
    that is given (and not zero, as in the reference), select the matches."""
    matched, edges = set(), []
    for name0, name1 in pairs:
        id0, id1 = image_ids[name0], image_ids[name1]
        if len({(id0, id1), (id1, id0)} & matched) > 0:
            continue
        pair = names_to_pair(name0, name1)
        if pair not in matches:
            raise ValueError(
                f'Could not find pair {(name0, name1)}... '
                'Maybe you matched with a different list of pairs? '
                f'Reverse in file: {names_to_pair(name0, name1) in matches}.')
        m = np.asarray(matches[pair]["matches0"])
        valid = m > -1
        if min_match_score:
            valid = valid & (np.asarray(matches[pair]["matching_scores0"]) > min_match_score)
        edges.append(np.stack([np.where(valid)[0] + offsets[name0],
                               m[valid].astype(np.int64) + offsets[name1]], -1))
        matched |= {(id0, id1), (id1, id0)}
    if not edges:
        return np.zeros((0, 2), dtype=np.int32)
    return np.concatenate(edges).astype(np.int32)


# ------------------------------------------------------------------ two-view verification
TWO_VIEW_STATUS = {0: "verified", 1: "fewer matches than min_num_inliers", 2: "no model",
                   3: "too few inliers"}
_SQRT2 = 1.4142135623730951


def fundamental_from_poses(T0, K0, T1, K1):
    """``F = K1^-T [t]x R K0^-1`` with ``x1^T F x0 = 0`` for world-to-camera ``T0``, ``T1``
    (``[4, 4]`` or ``[3, 4]``) and intrinsics ``K0``, ``K1``; host, float64, ``[3, 3]``."""
    T0, T1 = np.asarray(T0, np.float64), np.asarray(T1, np.float64)
    R = T1[:3, :3] @ T0[:3, :3].T
    t = T1[:3, 3] - R @ T0[:3, 3]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    return (np.linalg.inv(np.asarray(K1, np.float64)).T @ tx @ R
            @ np.linalg.inv(np.asarray(K0, np.float64)))


def two_view_verify_device(pts0, pts1, counts, F_in=None, max_error=4.0, confidence=0.999,
                           max_trials=10000, min_num_inliers=15, min_inlier_ratio=0.25,
                           refine_iters=2):
    """onepose_two_view_verify on device tensors (``pts0``, ``pts1`` float32 ``[B, P, 2]``,
    ``counts`` int32 ``[B]``, ``F_in`` float64 ``[B, 9]`` or None) -> ``(F [B, 9], inlier_mask
    uint8 [B, P], n_inliers, iters, status)`` tensors; nothing is synchronised."""
    dev = pts0.device
    B, P = pts0.shape[0], pts0.shape[1]
    F = torch.empty(B, 9, dtype=torch.float64, device=dev)
    mask = torch.empty(B, P, dtype=torch.uint8, device=dev)
    n_inliers, iters, status = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    nbytes = _lib.call("onepose_two_view_workspace_bytes", batch=B, max_points=P)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.run("onepose_two_view_verify", pts0=pts0, pts1=pts1, counts=counts, max_points=P, batch=B,
             F_in=F_in, max_error=float(max_error), confidence=float(confidence),
             max_trials=int(max_trials), min_num_inliers=int(min_num_inliers),
             min_inlier_ratio=float(min_inlier_ratio), refine_iters=int(refine_iters), F=F,
             inlier_mask=mask, n_inliers=n_inliers, iters=iters, status=status, workspace=ws,
             workspace_bytes=nbytes, stream=_lib.stream_ptr(dev))
    return F, mask, n_inliers, iters, status


def _tv_jacobi(A):
    """The header's J(k) on a batch [g, k, k] of symmetric matrices; every matrix takes its own
    branches.  -> the eigenvector of the smallest eigenvalue, [g, k]."""
    A = A.copy()
    g, k = A.shape[0], A.shape[1]
    V = np.tile(np.eye(k), (g, 1, 1))
    running = np.ones(g, dtype=bool)
    for _ in range(24):
        rotated = np.zeros(g, dtype=bool)
        for p in range(k - 1):
            for q in range(p + 1, k):
                apq, app, aqq = A[:, p, q].copy(), A[:, p, p].copy(), A[:, q, q].copy()
                skip = (np.abs(apq) <= 1e-20 * np.sqrt(np.abs(app * aqq))) | (apq == 0.0)
                rot = running & ~skip
                rotated |= rot
                theta = (aqq - app) / (2.0 * apq)
                tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(tt * tt + 1.0)
                sn = tt * cs
                for r in range(k):
                    if r == p or r == q:
                        continue
                    arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                    A[:, r, p] = A[:, p, r] = np.where(rot, cs * arp - sn * arq, arp)
                    A[:, r, q] = A[:, q, r] = np.where(rot, sn * arp + cs * arq, arq)
                bpp, bpq = cs * app - sn * apq, sn * app + cs * apq
                bqp, bqq = cs * apq - sn * aqq, sn * apq + cs * aqq
                A[:, p, p] = np.where(rot, cs * bpp - sn * bqp, app)
                A[:, q, q] = np.where(rot, sn * bpq + cs * bqq, aqq)
                A[:, p, q] = A[:, q, p] = np.where(running, 0.0, apq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                r2 = rot[:, None]
                V[:, :, p] = np.where(r2, cs[:, None] * vp - sn[:, None] * vq, vp)
                V[:, :, q] = np.where(r2, sn[:, None] * vp + cs[:, None] * vq, vq)
        running &= rotated
        if not running.any():
            break
    best = np.zeros(g, dtype=np.int64)
    rows = np.arange(g)
    for j in range(1, k):
        best = np.where(A[rows, j, j] < A[rows, best, best], j, best)
    return V[rows, :, best]


def _tv_solve(X, S):
    """The header's solver S(list) on a batch: X [g, L, 4] = (x0, y0, x1, y1) float64, S [g, L]
    which positions belong to the list (in ascending position) -> F [g, 9]."""
    g, L = S.shape
    m = S.sum(1).astype(np.float64)
    c = np.zeros((g, 4))
    for p in range(L):
        c = np.where(S[:, p, None], c + X[:, p], c)
    c = c / m[:, None]
    d = np.zeros((g, 2))
    for p in range(L):
        dx = X[:, p] - c
        r = np.sqrt(np.stack([dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1],
                              dx[:, 2] * dx[:, 2] + dx[:, 3] * dx[:, 3]], 1))
        d = np.where(S[:, p, None], d + r, d)
    s = _SQRT2 / (d / m[:, None])
    iu, ju = np.triu_indices(9)
    M = np.zeros((g, 45))
    one = np.ones(g)
    for p in range(L):
        u0, v0 = (X[:, p, 0] - c[:, 0]) * s[:, 0], (X[:, p, 1] - c[:, 1]) * s[:, 0]
        u1, v1 = (X[:, p, 2] - c[:, 2]) * s[:, 1], (X[:, p, 3] - c[:, 3]) * s[:, 1]
        a = np.stack([u1 * u0, u1 * v0, u1, v1 * u0, v1 * v0, v1, u0, v0, one], 1)
        M = np.where(S[:, p, None], M + a[:, iu] * a[:, ju], M)
    A = np.zeros((g, 9, 9))
    A[:, iu, ju] = M
    A[:, ju, iu] = M
    N = _tv_jacobi(A).reshape(g, 3, 3)
    G = np.empty((g, 3, 3))
    for i in range(3):
        for j in range(3):
            G[:, i, j] = (N[:, 0, i] * N[:, 0, j] + N[:, 1, i] * N[:, 1, j]) + N[:, 2, i] * N[:, 2, j]
    v = _tv_jacobi(G)
    w = (N[:, :, 0] * v[:, None, 0] + N[:, :, 1] * v[:, None, 1]) + N[:, :, 2] * v[:, None, 2]
    N = N - w[:, :, None] * v[:, None, :]
    a0, a1 = N[:, :, 0] * s[:, None, 0], N[:, :, 1] * s[:, None, 0]
    a2 = (N[:, :, 2] - a0 * c[:, None, 0]) - a1 * c[:, None, 1]
    Am = np.stack([a0, a1, a2], 2)   # [g, i, j]
    f0, f1 = s[:, None, 1] * Am[:, 0, :], s[:, None, 1] * Am[:, 1, :]
    f2 = (Am[:, 2, :] - c[:, None, 2] * f0) - c[:, None, 3] * f1
    return np.concatenate([f0, f1, f2], 1)


def _tv_inliers(F, X, n, thr2):
    """[.., 9] models against X [L, 4] (the first n positions count) -> bool [.., L]."""
    F = F[..., None, :]
    x0, y0, x1, y1 = X[:, 0], X[:, 1], X[:, 2], X[:, 3]
    a0 = (F[..., 0] * x0 + F[..., 1] * y0) + F[..., 2]
    a1 = (F[..., 3] * x0 + F[..., 4] * y0) + F[..., 5]
    a2 = (F[..., 6] * x0 + F[..., 7] * y0) + F[..., 8]
    b0 = (F[..., 0] * x1 + F[..., 3] * y1) + F[..., 6]
    b1 = (F[..., 1] * x1 + F[..., 4] * y1) + F[..., 7]
    e = (x1 * a0 + y1 * a1) + a2
    err = (e * e) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)
    ok = np.isfinite(F).all(-1)
    return (err <= thr2) & ok & (np.arange(len(X)) < n)


def _tv_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters with 8 model points."""
    tiny = 2.2250738585072014e-308
    num = max(1.0 - min(max(p, 0.0), 1.0), tiny)
    denom = 1.0 - (1.0 - min(max(ep, 0.0), 1.0)) ** 8
    if denom < tiny:
        return 0
    num, denom = np.log(num), np.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


def _host_two_view(pts0, pts1, counts, F_in, max_error, confidence, max_trials, min_num_inliers,
                   min_inlier_ratio, refine_iters, chunk=64):
    """onepose_two_view_verify's contract on the host: the hypotheses of a round of 64 iterations
    of up to `chunk` pairs are solved in one batch, every step in the header's order, and each
    pair replays the acceptance rule in iteration order."""
    B, P = pts0.shape[0], pts0.shape[1]
    X = np.concatenate([pts0, pts1], 2).astype(np.float64)   # [B, P, 4]
    n = np.clip(np.asarray(counts, np.int64), 0, P)
    thr2 = float(max_error) * float(max_error)
    F = np.zeros((B, 9)) if F_in is None else np.array(F_in, np.float64).reshape(B, 9)
    mask = np.zeros((B, P), bool)
    iters = np.zeros(B, np.int32)
    status = np.where(n < min_num_inliers, 1, 0).astype(np.int32)
    run = np.nonzero(status == 0)[0]
    with np.errstate(all="ignore"):
        if F_in is not None:
            for b in run:
                mask[b] = _tv_inliers(F[b], X[b], n[b], thr2)
        else:
            state = {b: [0xFFFFFFFFFFFFFFFF, 0, max(int(max_trials), 1), 0] for b in run}
            active = list(run)
            while active:
                for c0 in range(0, len(active), chunk):
                    part = active[c0:c0 + chunk]
                    sub = np.empty((len(part), 64, 8), np.int64)
                    for a, b in enumerate(part):   # 64 subsets of 8 distinct indices per pair
                        z, nb = state[b][0], int(n[b])
                        for h in range(64):
                            got = []
                            while len(got) < 8:
                                z = ((z & 0xFFFFFFFF) * 4164903690 + (z >> 32)) & 0xFFFFFFFFFFFFFFFF
                                v = (z & 0xFFFFFFFF) % nb
                                if v not in got:
                                    got.append(v)
                            sub[a, h] = got
                        state[b][0] = z
                    pb = np.asarray(part)[:, None, None]
                    hyp = _tv_solve(X[pb, sub].reshape(-1, 8, 4),
                                    np.ones((len(part) * 64, 8), bool)).reshape(len(part), 64, 9)
                    for a, b in enumerate(part):
                        good = _tv_inliers(hyp[a], X[b], n[b], thr2).sum(1)
                        _, it, niters, best = state[b]
                        for h in range(64):
                            if it >= niters:
                                break
                            if good[h] > max(best, 7):
                                best = int(good[h])
                                F[b] = hyp[a, h]
                                niters = _tv_num_iters(confidence, (int(n[b]) - best) / int(n[b]),
                                                       niters)
                            it += 1
                        state[b][1:] = [it, niters, best]
                active = [b for b in active if state[b][1] < state[b][2]]
            for b in run:
                iters[b] = state[b][1]
                if state[b][3] <= 0:
                    status[b] = 2
                    F[b] = 0.0
            run = np.nonzero(status == 0)[0]
            for b in run:
                mask[b] = _tv_inliers(F[b], X[b], n[b], thr2)
            going = list(run)
            for _ in range(int(refine_iters)):
                if not going:
                    break
                L = int(n[going].max())
                cand = _tv_solve(X[going][:, :L], mask[going][:, :L])
                kept = []
                for a, b in enumerate(going):
                    cm = _tv_inliers(cand[a], X[b], n[b], thr2)
                    if np.isfinite(cand[a]).all() and cm.sum() >= mask[b].sum():
                        F[b], mask[b] = cand[a], cm
                        kept.append(b)
                going = kept
    nin = mask.sum(1).astype(np.int32)
    weak = (nin < min_num_inliers) | (nin.astype(np.float64) < min_inlier_ratio * n.astype(np.float64))
    status[(status == 0) & weak] = 3
    return F, mask.astype(np.uint8), nin, iters, status


def verify_matches(pairs, matches, features, geometry="estimate", poses=None, Ks=None,
                   img_lists=None, max_error=4.0, confidence=0.999, max_trials=10000,
                   min_num_inliers=15, min_inlier_ratio=0.25, refine_iters=2, device=None):
    """Two-view geometric verification of ``match_pairs``' output, every pair in one padded call.
    ``geometry="estimate"``: a fundamental matrix per pair by RANSAC; ``"poses"``: the F of the
    given world-to-camera ``poses [m, 4, 4]`` and ``Ks [m, 3, 3]`` (in the order of
    ``img_lists``).  Matches are scored at keypoint + 0.5 in float32.

    Returns ``(verified, report)``.  ``verified`` is a new mapping like ``matches``: a rejected
    match has ``matches0[i] = -1``, every match of a pair whose status is not 0 has, and
    ``matches1[j] = -1`` where ``j``'s partner was rejected; scores are copied unchanged.
    ``report[pair]`` holds ``status`` (``TWO_VIEW_STATUS``), ``n_matches``, ``n_inliers``,
    ``iters`` and ``F [3, 3]``.  The library's contract is in ``include/onepose_two_view.h``; with
    ``device=None`` the same contract runs on the host."""
    if geometry not in ("estimate", "poses"):
        raise ValueError(f"verify_matches: geometry {geometry!r} is not 'estimate' or 'poses'")
    if geometry == "poses":
        if poses is None or Ks is None or img_lists is None:
            raise ValueError("verify_matches: geometry='poses' needs poses, Ks and img_lists")
        index = {name: k for k, name in enumerate(img_lists)}
        T, Kall = _load_poses(poses), np.asarray(Ks, np.float64)
    todo, seen = [], set()
    for name0, name1 in pairs:
        pair = names_to_pair(name0, name1)
        if pair in matches and pair not in seen:
            seen.add(pair)
            todo.append((pair, name0, name1))
    verified = {pair: {k: np.array(v) for k, v in grp.items()} for pair, grp in matches.items()}
    report = {}
    if not todo:
        return verified, report
    sel = []
    for pair, name0, name1 in todo:
        m0 = np.asarray(matches[pair]["matches0"]).astype(np.int64)
        i0 = np.nonzero(m0 > -1)[0]
        sel.append((i0, m0[i0]))
    P = max(1, max(len(i0) for i0, _ in sel))
    B = len(todo)
    pts0, pts1 = np.zeros((B, P, 2), np.float32), np.zeros((B, P, 2), np.float32)
    counts = np.asarray([len(i0) for i0, _ in sel], np.int32)
    F_in = np.zeros((B, 9)) if geometry == "poses" else None
    for b, ((pair, name0, name1), (i0, i1)) in enumerate(zip(todo, sel)):
        k0 = np.asarray(features[name0]["keypoints"], np.float32).reshape(-1, 2)
        k1 = np.asarray(features[name1]["keypoints"], np.float32).reshape(-1, 2)
        pts0[b, :len(i0)] = k0[i0] + np.float32(0.5)
        pts1[b, :len(i1)] = k1[i1] + np.float32(0.5)
        if F_in is not None:
            a, c = index[name0], index[name1]
            F_in[b] = fundamental_from_poses(T[a], Kall[a], T[c], Kall[c]).reshape(9)
    opts = dict(max_error=max_error, confidence=confidence, max_trials=max_trials,
                min_num_inliers=min_num_inliers, min_inlier_ratio=min_inlier_ratio,
                refine_iters=refine_iters)
    dev = _gpu(device)
    if dev is None:
        if min_num_inliers < 8 or max_trials < 1 or refine_iters < 0:
            raise _lib.OnePoseError("two_view: min_num_inliers below 8, max_trials below 1 or "
                                    "refine_iters negative")
        F, mask, nin, iters, status = _host_two_view(pts0, pts1, counts, F_in, **opts)
    else:
        out = two_view_verify_device(
            torch.from_numpy(pts0).to(dev), torch.from_numpy(pts1).to(dev),
            torch.from_numpy(counts).to(dev),
            None if F_in is None else torch.from_numpy(F_in).to(dev), **opts)
        F, mask, nin, iters, status = (t.cpu().numpy() for t in out)
    for b, ((pair, _, _), (i0, i1)) in enumerate(zip(todo, sel)):
        keep = mask[b, :len(i0)].astype(bool) & (status[b] == 0)
        grp = verified[pair]
        rejected = np.zeros(len(grp["matches0"]), bool)
        rejected[i0[~keep]] = True
        grp["matches0"][rejected] = -1
        if "matches1" in grp:
            m1 = grp["matches1"].astype(np.int64)
            back = (m1 > -1) & (m1 < len(rejected))
            back[back] = rejected[m1[back]]
            grp["matches1"][back] = -1
        report[pair] = {"status": int(status[b]), "n_matches": int(counts[b]),
                        "n_inliers": int(nin[b]), "iters": int(iters[b]),
                        "F": np.array(F[b], np.float64).reshape(3, 3)}
    return verified, report


# ------------------------------------------------------------------ the model and its files
def rotmat2qvec(R):
    """The unit quaternion (w, x, y, z) of a rotation matrix, w >= 0: the eigenvector of the
    largest eigenvalue of the symmetric 4 x 4 matrix built from R (COLMAP's convention)."""
    R = np.asarray(R, dtype=np.float64)
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = R
    K = np.array([[xx - yy - zz, 0, 0, 0],
                  [yx + xy, yy - xx - zz, 0, 0],
                  [zx + xz, zy + yz, zz - xx - yy, 0],
                  [zy - yz, xz - zx, yx - xy, xx + yy + zz]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[[3, 0, 1, 2], np.argmax(w)]
    return -q if q[0] < 0 else q


def _stem_order(img_lists):
    return sorted(range(len(img_lists)),
                  key=lambda i: int(os.path.splitext(os.path.basename(img_lists[i]))[0]))


def empty_model(img_lists, poses, Ks, sizes):
    """``generate_empty.import_data`` without the file reads: images sorted by their integer
    stem, image and camera ids 1, 2, ..., one PINHOLE camera ``[fx, fy, cx, cy]`` per image, no
    points.  ``poses [m, 4, 4]``, ``Ks [m, 3, 3]``, ``sizes [m, 2]`` as (width, height), all in the
    order of ``img_lists``."""
    P, Ks, sizes = _load_poses(poses), np.asarray(Ks, dtype=np.float64), np.asarray(sizes)
    order = _stem_order(img_lists)
    m = len(order)
    ids = np.arange(1, m + 1, dtype=np.int32)
    return {
        "camera_ids": ids.copy(), "camera_sizes": sizes[order].astype(np.int64).reshape(m, 2),
        "camera_params": np.stack([Ks[order, 0, 0], Ks[order, 1, 1], Ks[order, 0, 2],
                                   Ks[order, 1, 2]], axis=1).reshape(m, 4),
        "image_ids": ids, "image_camera_ids": ids.copy(), "names": [img_lists[i] for i in order],
        "qvec": np.stack([rotmat2qvec(P[i, :3, :3]) for i in order]).reshape(m, 4),
        "tvec": P[order, :3, 3].reshape(m, 3),
        "xys": [np.zeros((0, 2)) for _ in order],
        "point3D_ids": [np.full(0, -1, dtype=np.int64) for _ in order],
        "ids": np.zeros(0, np.int64), "xyz": np.zeros((0, 3)), "rgb": np.zeros((0, 3), np.uint8),
        "error": np.zeros(0), "track_len": np.zeros(0, np.int64), "file_order": np.zeros(0, np.int64),
        "track_image_ids": [], "track_point2D_idxs": [],
    }


def write_model_binary(model, path):
    """``cameras.bin``, ``images.bin`` and ``points3D.bin`` of COLMAP's binary format into the
    directory ``path`` (little-endian, PINHOLE cameras, points in the model's order)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(model["camera_ids"])))
        for cid, (w, h), params in zip(model["camera_ids"], model["camera_sizes"],
                                       model["camera_params"]):
            f.write(struct.pack("<iiQQ", int(cid), 1, int(w), int(h)))
            f.write(struct.pack("<4d", *(float(p) for p in params)))
    with open(os.path.join(path, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(model["image_ids"])))
        for k, iid in enumerate(model["image_ids"]):
            f.write(struct.pack("<i4d3di", int(iid), *model["qvec"][k].tolist(),
                                *model["tvec"][k].tolist(), int(model["image_camera_ids"][k])))
            f.write(model["names"][k].encode("utf-8") + b"\x00")
            p3d = np.asarray(model["point3D_ids"][k], dtype=np.int64)
            rec = np.empty(len(p3d), dtype=[("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            xys = np.asarray(model["xys"][k], dtype=np.float64).reshape(-1, 2)
            rec["x"], rec["y"], rec["id"] = xys[:, 0], xys[:, 1], p3d
            f.write(struct.pack("<Q", len(p3d)))
            f.write(rec.tobytes())
    with open(os.path.join(path, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(model["ids"])))
        for k, pid in enumerate(model["ids"]):
            f.write(struct.pack("<Q3d3BdQ", int(pid), *model["xyz"][k].tolist(),
                                *(int(c) for c in model["rgb"][k]), float(model["error"][k]),
                                len(model["track_image_ids"][k])))
            tr = np.stack([model["track_image_ids"][k], model["track_point2D_idxs"][k]], axis=-1)
            f.write(tr.astype("<i4").tobytes())


# ------------------------------------------------------------------ tracks
def track_components_device(edges, n_nodes, rounds=CC_ROUNDS, max_calls=CC_MAX_CALLS):
    """onepose_track_components until it reports convergence -> ``(labels int32 [n_nodes],
    status rows)``.  ``edges``: int32 ``[E, 2]`` on the device."""
    dev = edges.device
    edges = edges.contiguous()
    parent = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    rows = []
    for call in range(max_calls):
        _lib.run("onepose_track_components", edges=edges if edges.shape[0] else None,
                 n_edges=edges.shape[0], n_nodes=n_nodes, rounds=rounds,
                 init=1 if call == 0 else 0, parent=parent, status=status,
                 stream=_lib.stream_ptr(dev))
        rows.append(status.tolist())
        if rows[-1][0] == 0:
            return parent, rows
    raise _lib.OnePoseError(f"track_components: {rows[-1][0]} edges still open after "
                            f"{max_calls} calls of {rounds} rounds")


def _host_components(edges, n_nodes):
    parent = np.arange(n_nodes, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for u, v in np.asarray(edges).reshape(-1, 2).tolist():
        if not (0 <= u < n_nodes and 0 <= v < n_nodes):
            continue
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.asarray([find(x) for x in range(n_nodes)], dtype=np.int32)


def build_tracks(n_feats_per_image, edges, device=None):
    """Tracks = the components of the feature graph with at least 2 features, ordered by their
    smallest feature id, observations by (image, feature).  Returns ``{'track_start' int32
    [T + 1], 'obs_image' int32 [n_obs], 'obs_feat' int32 [n_obs]}`` (numpy).  A component longer
    than ``onepose_sfm_max_track()`` stays a track; the triangulation gives it reason 3."""
    counts = np.asarray(n_feats_per_image, dtype=np.int64).reshape(-1)
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    n_nodes = int(offsets[-1])
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    empty = {"track_start": np.zeros(1, np.int32), "obs_image": np.zeros(0, np.int32),
             "obs_feat": np.zeros(0, np.int32)}
    if n_nodes == 0:
        return empty
    dev = _gpu(device)
    if dev is None:
        labels = torch.from_numpy(_host_components(edges, n_nodes))
    else:
        labels, _ = track_components_device(torch.from_numpy(edges).to(dev), n_nodes)
    # feature ids ascend already, so a stable sort by label orders by (label, feature id)
    _, order = torch.sort(labels, stable=True)
    _, sizes = torch.unique_consecutive(labels[order], return_counts=True)
    keep = torch.repeat_interleave(sizes >= 2, sizes)
    ids = order[keep].cpu().numpy()
    lens = sizes[sizes >= 2].cpu().numpy()
    if len(lens) == 0:
        return empty
    start = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=start[1:])
    img = np.searchsorted(offsets, ids, side="right") - 1
    return {"track_start": start, "obs_image": img.astype(np.int32),
            "obs_feat": (ids - offsets[img]).astype(np.int32)}


# ------------------------------------------------------------------ triangulation
def tracks_triangulate_device(Rt, K4, track_start, obs_image, obs_xy, max_reproj, min_angle_deg):
    """onepose_tracks_triangulate on device tensors -> ``(xyz, err, reason, n_kept, obs_keep,
    status)`` tensors; nothing is synchronised."""
    dev = Rt.device
    n_tracks, n_obs = track_start.shape[0] - 1, obs_image.shape[0]
    xyz = torch.empty(n_tracks, 3, dtype=torch.float64, device=dev)
    err = torch.empty(n_tracks, dtype=torch.float64, device=dev)
    reason = torch.empty(n_tracks, dtype=torch.int32, device=dev)
    n_kept = torch.empty(n_tracks, dtype=torch.int32, device=dev)
    obs_keep = torch.empty(n_obs, dtype=torch.uint8, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.run("onepose_tracks_triangulate", Rt=Rt, K4=K4, n_images=Rt.shape[0],
             track_start=track_start, obs_image=obs_image, obs_xy=obs_xy, n_tracks=n_tracks,
             n_obs=n_obs, max_reproj=float(max_reproj), min_angle_deg=float(min_angle_deg), xyz=xyz,
             err=err, reason=reason, n_kept=n_kept, obs_keep=obs_keep, status=status,
             stream=_lib.stream_ptr(dev))
    return xyz, err, reason, n_kept, obs_keep, status


def _residuals(R, K, X, uv):
    """[g, L] camera coordinates and pixel residuals at X [g, 3], in the header's order."""
    x = X[:, None, :]
    pc = [((R[:, :, r, 0] * x[..., 0] + R[:, :, r, 1] * x[..., 1]) + R[:, :, r, 2] * x[..., 2])
          + R[:, :, r, 3] for r in range(3)]
    ru = (K[..., 0] * (pc[0] / pc[2]) + K[..., 2]) - uv[..., 0]
    rv = (K[..., 1] * (pc[1] / pc[2]) + K[..., 3]) - uv[..., 1]
    return pc, ru, rv


def _errors(R, K, X, uv):
    pc, ru, rv = _residuals(R, K, X, uv)
    e = np.sqrt(ru * ru + rv * rv)
    return np.where(np.isnan(e) | np.isnan(pc[2]), np.nan, np.where(pc[2] > 0.0, e, np.inf))


def _serial_sum(terms, S):
    """sum over ascending position of terms [g, L] where S, as m = m + term."""
    m = np.zeros(terms.shape[0])
    for p in range(terms.shape[1]):
        m = np.where(S[:, p], m + terms[:, p], m)
    return m


def _jacobi_smallest(M):
    """The cyclic Jacobi of the header on a batch [g, 4, 4]; every matrix takes its own branches."""
    M = M.copy()
    g = M.shape[0]
    V = np.tile(np.eye(4), (g, 1, 1))
    running = np.ones(g, dtype=bool)
    for _ in range(24):
        rotated = np.zeros(g, dtype=bool)
        for p in range(3):
            for q in range(p + 1, 4):
                apq = M[:, p, q].copy()
                skip = (np.abs(apq) <= 1e-20 * np.sqrt(np.abs(M[:, p, p] * M[:, q, q]))) | (apq == 0.0)
                rot = running & ~skip
                rotated |= rot
                theta = (M[:, q, q] - M[:, p, p]) / (2.0 * apq)
                tt = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(tt * tt + 1.0)
                sn = tt * cs
                for k in range(4):
                    mkp, mkq = M[:, k, p].copy(), M[:, k, q].copy()
                    M[:, k, p] = np.where(rot, cs * mkp - sn * mkq, mkp)
                    M[:, k, q] = np.where(rot, sn * mkp + cs * mkq, mkq)
                for k in range(4):
                    mpk, mqk = M[:, p, k].copy(), M[:, q, k].copy()
                    M[:, p, k] = np.where(rot, cs * mpk - sn * mqk, mpk)
                    M[:, q, k] = np.where(rot, sn * mpk + cs * mqk, mqk)
                zero = running
                M[:, p, q] = np.where(zero, 0.0, M[:, p, q])
                M[:, q, p] = np.where(zero, 0.0, M[:, q, p])
                for k in range(4):
                    vkp, vkq = V[:, k, p].copy(), V[:, k, q].copy()
                    V[:, k, p] = np.where(rot, cs * vkp - sn * vkq, vkp)
                    V[:, k, q] = np.where(rot, sn * vkp + cs * vkq, vkq)
        running &= rotated
        if not running.any():
            break
    best = np.zeros(g, dtype=np.int64)
    rows = np.arange(g)
    for j in range(1, 4):
        best = np.where(M[:, j, j] < M[rows, best, best], j, best)
    return V[rows, :, best]


def _host_group(R, K, img, uv, max_reproj, min_angle_deg):
    """All tracks of one length L >= 2 at once: R [G, L, 3, 4], K [G, L, 4], img [G, L], uv
    [G, L, 2] -> (reason [G], X [G, 3], err [G], S [G, L]).  Every step is the header's, in its
    order, so the numbers are the kernel's."""
    G, L = img.shape
    xn = (uv[..., 0] - K[..., 2]) / K[..., 0]
    yn = (uv[..., 1] - K[..., 3]) / K[..., 1]
    ra = xn[..., None] * R[:, :, 2, :] - R[:, :, 0, :]
    rb = yn[..., None] * R[:, :, 2, :] - R[:, :, 1, :]
    S = np.ones((G, L), dtype=bool)
    reason = np.zeros(G, dtype=np.int32)
    X = np.full((G, 3), np.nan)
    e = np.full((G, L), np.nan)
    todo = np.arange(G)
    while len(todo):   # 1, 2 on the tracks that still have a failing observation
        M = np.zeros((len(todo), 4, 4))
        for i in range(4):
            for j in range(i, 4):
                M[:, i, j] = M[:, j, i] = _serial_sum(
                    ra[todo, :, i] * ra[todo, :, j] + rb[todo, :, i] * rb[todo, :, j], S[todo])
        h = _jacobi_smallest(M)
        x = h[:, :3] / h[:, 3:]
        ee = _errors(R[todo], K[todo], x, uv[todo])
        bad = ~np.isfinite(x).all(1) | (np.isnan(ee) & S[todo]).any(1)
        reason[todo[bad]] = 4
        X[todo], e[todo] = x, ee
        es = np.where(S[todo], ee, -1.0)
        worst = np.argmax(np.where(np.isnan(es), -1.0, es), axis=1)   # the first of the largest
        fail = ~bad & (es[np.arange(len(todo)), worst] > max_reproj)
        S[todo[fail], worst[fail]] = False
        few = fail & (S[todo].sum(1) < 2)
        reason[todo[few]] = 1
        todo = todo[fail & ~few]
    ok = reason == 0
    # 3
    same = (img[:, :, None] == img[:, None, :]) & S[:, :, None] & S[:, None, :]
    pos = np.arange(L)
    better = (e[:, None, :] < e[:, :, None]) | ((e[:, None, :] == e[:, :, None])
                                                & (pos[None, None, :] < pos[None, :, None]))
    S &= ~(same & better).any(2)
    reason[ok & (S.sum(1) < 2)] = 1
    # 4
    going = reason == 0
    for _ in range(5):
        if not going.any():
            break
        t = np.nonzero(going)[0]
        Rg, Kg, Sg = R[t], K[t], S[t]
        pc, ru, rv = _residuals(Rg, Kg, X[t], uv[t])
        iz = 1.0 / pc[2]
        xz, yz, fu, fv = pc[0] * iz, pc[1] * iz, Kg[..., 0] * iz, Kg[..., 1] * iz
        Ju = [fu * (Rg[:, :, 0, k] - xz * Rg[:, :, 2, k]) for k in range(3)]
        Jv = [fv * (Rg[:, :, 1, k] - yz * Rg[:, :, 2, k]) for k in range(3)]
        H = {(i, j): _serial_sum(Ju[i] * Ju[j] + Jv[i] * Jv[j], Sg) for i in range(3)
             for j in range(i, 3)}
        g = [_serial_sum(Ju[i] * ru + Jv[i] * rv, Sg) for i in range(3)]
        cost = _serial_sum(ru * ru + rv * rv, Sg)
        l00 = np.sqrt(H[0, 0])
        l10, l20 = H[0, 1] / l00, H[0, 2] / l00
        d11 = H[1, 1] - l10 * l10
        l11 = np.sqrt(d11)
        l21 = (H[1, 2] - l20 * l10) / l11
        d22 = (H[2, 2] - l20 * l20) - l21 * l21
        l22 = np.sqrt(d22)
        pivots = (H[0, 0] > 0.0) & (d11 > 0.0) & (d22 > 0.0)
        y0 = -g[0] / l00
        y1 = (-g[1] - l10 * y0) / l11
        y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
        d2 = y2 / l22
        d1 = (y1 - l21 * d2) / l11
        d0 = ((y0 - l10 * d1) - l20 * d2) / l00
        Xn = X[t] + np.stack([d0, d1, d2], axis=1)
        _, ru, rv = _residuals(Rg, Kg, Xn, uv[t])
        accept = pivots & (_serial_sum(ru * ru + rv * rv, Sg) < cost)
        X[t[accept]] = Xn[accept]
        going[t[~accept]] = False
    # 5
    e = _errors(R, K, X, uv)
    ok = reason == 0
    reason[ok & (np.isnan(e) & S).any(1)] = 4
    S &= e <= max_reproj
    reason[(reason == 0) & (S.sum(1) < 2)] = 1
    d = [-((R[:, :, 0, k] * R[:, :, 0, 3] + R[:, :, 1, k] * R[:, :, 1, 3])
           + R[:, :, 2, k] * R[:, :, 2, 3]) - X[:, None, k] for k in range(3)]
    nrm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    u = [v / nrm for v in d]
    cos = (u[0][:, :, None] * u[0][:, None, :] + u[1][:, :, None] * u[1][:, None, :]) \
        + u[2][:, :, None] * u[2][:, None, :]
    pair = S[:, :, None] & S[:, None, :] & (pos[None, :, None] < pos[None, None, :])
    reason[(reason == 0) & (np.isnan(cos) & pair).any((1, 2))] = 4
    cmin = np.where(pair, cos, 2.0).min((1, 2))
    angle = np.arccos(np.clip(cmin, -1.0, 1.0)) * (180.0 / np.pi)
    reason[(reason == 0) & (angle < min_angle_deg)] = 2
    err = _serial_sum(e, S) / S.sum(1)
    return reason, X, err, S


def triangulate_tracks(Rt, K4, track_start, obs_image, obs_xy, max_reproj=MAX_REPROJ,
                       min_angle_deg=MIN_ANGLE_DEG, device=None):
    """The project's own multi-view triangulation (contract in the header) of tracks given as a
    CSR over observations: ``Rt [m, 3, 4]``, ``K4 [m, 4]`` = (fx, fy, cx, cy), ``obs_xy`` in
    COLMAP's pixel convention (keypoint + 0.5).  Returns numpy arrays ``{'xyz' [T, 3], 'err' [T],
    'reason' int32 [T], 'n_kept' int32 [T], 'obs_keep' bool [n_obs]}``; a track with
    ``reason != 0`` has NaN, NaN, 0 and no observation kept.  A malformed CSR raises."""
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(-1, 3, 4)
    K4 = np.ascontiguousarray(K4, dtype=np.float64).reshape(-1, 4)
    ts = np.ascontiguousarray(track_start, dtype=np.int32).reshape(-1)
    oi = np.ascontiguousarray(obs_image, dtype=np.int32).reshape(-1)
    xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    T, n_obs = len(ts) - 1, len(oi)
    if len(K4) != len(Rt) or len(xy) != n_obs:
        raise ValueError("triangulate_tracks: array lengths do not agree")
    if T < 1 or n_obs < 1:
        return {"xyz": np.zeros((max(T, 0), 3)), "err": np.zeros(max(T, 0)),
                "reason": np.full(max(T, 0), 3, np.int32), "n_kept": np.zeros(max(T, 0), np.int32),
                "obs_keep": np.zeros(n_obs, bool)}
    dev = _gpu(device)
    if dev is not None:
        xyz, err, reason, n_kept, keep, status = tracks_triangulate_device(
            *(torch.from_numpy(a).to(dev) for a in (Rt, K4, ts, oi, xy)), max_reproj, min_angle_deg)
        st = status.tolist()
        if st[0] != 0:
            raise _lib.OnePoseError(f"tracks_triangulate: {TRI_STATUS.get(st[0], st[0])} "
                                    f"(index {st[1]})")
        return {"xyz": xyz.cpu().numpy(), "err": err.cpu().numpy(), "reason": reason.cpu().numpy(),
                "n_kept": n_kept.cpu().numpy(), "obs_keep": keep.cpu().numpy().astype(bool)}
    if ts[0] != 0 or ts[-1] != n_obs or np.any(np.diff(ts) < 0):
        raise _lib.OnePoseError(f"tracks_triangulate: {TRI_STATUS[1]}")
    if np.any(oi < 0) or np.any(oi >= len(Rt)):
        raise _lib.OnePoseError(f"tracks_triangulate: {TRI_STATUS[2]}")
    out = {"xyz": np.full((T, 3), np.nan), "err": np.full(T, np.nan),
           "reason": np.full(T, 3, np.int32), "n_kept": np.zeros(T, np.int32),
           "obs_keep": np.zeros(n_obs, bool)}
    lens = np.diff(ts)
    with np.errstate(all="ignore"):
        for L in np.unique(lens[(lens >= 2) & (lens <= 256)]):
            t = np.nonzero(lens == L)[0]
            for c in range(0, len(t), 4096):   # bounded scratch
                tc = t[c:c + 4096]
                obs = ts[tc][:, None] + np.arange(L)[None, :]
                img = oi[obs]
                reason, X, err, S = _host_group(Rt[img], K4[img], img, xy[obs], max_reproj,
                                                min_angle_deg)
                out["reason"][tc] = reason
                good = reason == 0
                out["xyz"][tc[good]], out["err"][tc[good]] = X[good], err[good]
                out["n_kept"][tc[good]] = S[good].sum(1)
                out["obs_keep"][obs[good]] = S[good]
    return out


# ------------------------------------------------------------------ the chain
def reconstruct(features, img_lists, poses, Ks, matcher, covis_num=10, min_match_score=None,
                out_dir=None, device=None, seq_ids=None, max_reproj=MAX_REPROJ,
                min_angle_deg=MIN_ANGLE_DEG, match_device=None, verify=None, verify_options=None,
                match_batch=None, refine=None, refine_options=None):
    """Pairs, match export, match import, tracks, triangulation and the compaction of the kept
    tracks.  ``poses``: world-to-camera ``[m, 4, 4]`` (or pose files), ``Ks [m, 3, 3]``, both in
    the order of ``img_lists``; ``features[name]`` holds ``keypoints [n, 2]``, ``image_size``
    (w, h) and whatever the matcher reads.  Point ids are 1, 2, ... in track order.  The matcher
    gets its tensors on ``match_device`` (default: ``device``).  ``verify``: None (no geometric
    verification), ``"estimate"`` or ``"poses"`` -- ``verify_matches`` with that geometry (and
    ``verify_options`` as its keywords) between the match export and the import; its report is
    the model's ``'two_view'``.  ``match_batch``: ``match_pairs``' ``batch_size`` (None: one
    matcher call per pair).  ``refine``: None (the input poses are taken as exact) or
    ``"global_ba"`` -- ``global_bundle_adjust`` on the triangulated model (``refine_options`` as
    its keywords, on ``device``); the refined model is what is returned and written, and its
    ``'global_ba'`` holds the solver's report.

    Returns one mapping with the keys of ``object_builder.read_points3d_binary`` and
    ``read_images_binary`` (and of ``empty_model``), plus ``'pairs'`` and ``'tracks'``; with
    ``out_dir`` the three ``.bin`` files are written there as well."""
    if refine not in (None, "global_ba"):
        raise ValueError(f"reconstruct: refine={refine!r}; expected None or 'global_ba'")
    img_lists = list(img_lists)
    P = _load_poses(poses)
    pairs = covis_from_pose(img_lists, poses, covis_num, seq_ids=seq_ids)
    matches = match_pairs(features, pairs, matcher,
                          device=device if match_device is None else match_device,
                          batch_size=match_batch)
    two_view = None
    if verify is not None:
        matches, two_view = verify_matches(pairs, matches, features, geometry=verify, poses=P,
                                           Ks=Ks, img_lists=img_lists, device=device,
                                           **(verify_options or {}))
    sizes = [np.asarray(features[n]["image_size"]).reshape(2) for n in img_lists]
    model = empty_model(img_lists, P, Ks, sizes)
    names = model["names"]
    kps = [np.asarray(features[n]["keypoints"], dtype=np.float64).reshape(-1, 2) for n in names]
    counts = np.asarray([len(k) for k in kps], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    image_ids = {n: int(i) for n, i in zip(names, model["image_ids"])}
    edges = import_matches(pairs, matches, image_ids, min_match_score,
                           offsets={n: int(o) for n, o in zip(names, offsets)})
    tracks = build_tracks(counts, edges, device=device)
    order = _stem_order(img_lists)
    Rt = P[order][:, :3, :4]
    K4 = model["camera_params"]
    oi, of = tracks["obs_image"], tracks["obs_feat"]
    xy_all = np.concatenate(kps) + 0.5 if len(kps) else np.zeros((0, 2))
    tri = triangulate_tracks(Rt, K4, tracks["track_start"], oi, xy_all[offsets[oi] + of],
                             max_reproj, min_angle_deg, device=device)
    kept = np.nonzero(tri["reason"] == 0)[0]
    keep = tri["obs_keep"]
    track_of_obs = np.repeat(np.arange(len(tri["reason"])), np.diff(tracks["track_start"]))
    point_of_track = np.full(len(tri["reason"]), -1, dtype=np.int64)
    point_of_track[kept] = np.arange(1, len(kept) + 1)
    p3d = [np.full(int(c), -1, dtype=np.int64) for c in counts]
    for k in range(len(names)):
        sel = keep & (oi == k)
        p3d[k][of[sel]] = point_of_track[track_of_obs[sel]]
    ts = tracks["track_start"]
    model.update({
        "xys": [k + 0.5 for k in kps], "point3D_ids": p3d,
        "ids": np.arange(1, len(kept) + 1, dtype=np.int64), "xyz": tri["xyz"][kept].reshape(-1, 3),
        "rgb": np.zeros((len(kept), 3), np.uint8), "error": tri["err"][kept],
        "track_len": tri["n_kept"][kept].astype(np.int64),
        "file_order": np.arange(len(kept), dtype=np.int64),
        "track_image_ids": [oi[ts[t]:ts[t + 1]][keep[ts[t]:ts[t + 1]]] + 1 for t in kept],
        "track_point2D_idxs": [of[ts[t]:ts[t + 1]][keep[ts[t]:ts[t + 1]]] for t in kept],
        "pairs": pairs, "tracks": tracks, "triangulation": tri,
    })
    if two_view is not None:
        model["two_view"] = two_view
    if refine is not None:
        model = global_bundle_adjust(model, device=device, **(refine_options or {}))
    if out_dir is not None:
        write_model_binary(model, out_dir)
    return model

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
* ``build_tracks`` / ``triangulate_tracks``
                              -- what the reference leaves to a COLMAP binary
                                 (``triangulation.py:122-148``).  **This project's own**: tracks
                                 are the connected components of the match graph, and the
                                 triangulator is the one stated in ``include/onepose_hip.h``
                                 ("Sparse reconstruction").  Parity with COLMAP is not verified.
* ``reconstruct``             -- the chain; its result feeds ``object_builder.build_object``.

The host stages are numpy only.  ``build_tracks`` and ``triangulate_tracks`` take ``device=``:
with a GPU device the HIP kernels of ``csrc/sfm.hip`` run; with ``device=None`` the same contract
runs on the host.

Out of scope: COLMAP's geometric verification, its RANSAC triangulation and bundle adjustment,
point colours, the sqlite database, ``model_analyzer`` statistics, PLY export, batching pairs into
one matcher call.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib
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


@torch.no_grad()
def match_pairs(features, pairs, matcher, device=None):
    """One matcher call per pair -> ``{pair name: {'matches0' int16, 'matches1' int16,
    'matching_scores0' float16, 'matching_scores1' float16}}``.  A pair is skipped when it or its
    reverse was matched before.  ``features``: ``name -> {key: array}`` with ``image_size`` (w, h)
    among the keys; every key reaches the matcher with the side's suffix, as a float tensor with
    a batch axis on ``device``."""
    out, matched = {}, set()
    for name0, name1 in pairs:
        pair = names_to_pair(name0, name1)
        if len({(name0, name1), (name1, name0)} & matched) or pair in out:
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
        matched |= {(name0, name1), (name1, name0)}
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
                min_angle_deg=MIN_ANGLE_DEG, match_device=None):
    """Pairs, match export, match import, tracks, triangulation and the compaction of the kept
    tracks.  ``poses``: world-to-camera ``[m, 4, 4]`` (or pose files), ``Ks [m, 3, 3]``, both in
    the order of ``img_lists``; ``features[name]`` holds ``keypoints [n, 2]``, ``image_size``
    (w, h) and whatever the matcher reads.  Point ids are 1, 2, ... in track order.  The matcher
    gets its tensors on ``match_device`` (default: ``device``).

    Returns one mapping with the keys of ``object_builder.read_points3d_binary`` and
    ``read_images_binary`` (and of ``empty_model``), plus ``'pairs'`` and ``'tracks'``; with
    ``out_dir`` the three ``.bin`` files are written there as well."""
    img_lists = list(img_lists)
    P = _load_poses(poses)
    pairs = covis_from_pose(img_lists, poses, covis_num, seq_ids=seq_ids)
    matches = match_pairs(features, pairs, matcher,
                          device=device if match_device is None else match_device)
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
    if out_dir is not None:
        write_model_binary(model, out_dir)
    return model

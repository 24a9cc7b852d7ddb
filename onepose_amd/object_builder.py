"""The object builder: from an SfM model and per-image features to an object's 3D annotations.

The reference's ``postprocess`` stage (``run.py:196-249``), with its names, argument meaning and
return types:

* ``get_tkl``                  -- ``src/sfm/postprocess/filter_tkl.py:36-53``
* ``filter_by_track_length`` / ``filter_by_3d_box`` / ``filter_3d`` / ``merge``
                               -- ``src/sfm/postprocess/filter_points.py:8-117``
* ``collect_observations`` + ``lift_descriptors``
                               -- ``feature_process.py``'s ``count_features`` / ``gather_3d_ann`` /
                                  ``mean_descriptors`` (``:59-188``, ``:297-305``)
* ``build_annotations``        -- ``run.py:220-249`` end to end, writing ``anno_3d_average.npz``,
                                  ``anno_3d_collect.npz`` and ``idxs.npy`` as ``get_kpt_ann`` does
* ``read_points3d_binary`` / ``read_images_binary`` -- COLMAP's binary model, from its public
  format description.

Every function takes ``device=``.  With a GPU device the HIP kernels of
``csrc/object_build.hip`` run (contract in ``include/onepose_hip.h``, "Object builder"); with
``device=None`` the same arithmetic runs in numpy, neighbour lists instead of the reference's
dense n x n matrix.  Both give the reference's bits for merge, lifting and the files; the box
filter's dot product is this project's own order (see the header).  Score means go through
``data_utils.mean_scores`` on the host, and the leaf permutation through
``data_utils.leaf_indices``, so numpy's pairwise sum and RNG consumption stay the reference's.

Features come in as a mapping ``name -> {'keypoints': [n, 2], 'descriptors': [dim, n] float32,
'scores': [n]}``; an open ``h5py.File`` of the reference's feature file satisfies it.

Out of scope: ``anno_2d.json`` / ``get_assign_matrix`` (training data), ``vis_tkl_filtered_pcds``
(calls a COLMAP binary), COLMAP's own triangulation.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib, data_utils

OBJ_F32, OBJ_F64 = 0, 1   # ONEPOSE_OBJ_*
LIFT_STATUS = {1: "a segment of length < 1", 2: "segment lengths do not add up to the observations",
               3: "an image block outside the bank", 4: "an observation outside its image block"}


# ------------------------------------------------------------------ COLMAP binary readers
def read_points3d_binary(path):
    """``points3D.bin`` -> ``{'ids' int64 [n] ascending, 'xyz' float64 [n, 3], 'track_len' int64
    [n], 'file_order' int64 [n]}``; ``file_order[k]`` is the row of the file's k-th point."""
    with open(path, "rb") as f:
        buf = f.read()
    (n,) = struct.unpack_from("<Q", buf, 0)
    off = 8
    ids = np.empty(n, dtype=np.int64)
    xyz = np.empty((n, 3), dtype=np.float64)
    tl = np.empty(n, dtype=np.int64)
    head = struct.Struct("<Q3d3BdQ")   # id, xyz, rgb, error, track length
    for k in range(n):
        if off + head.size > len(buf):
            raise ValueError(f"{path}: truncated at point {k}")
        pid, x, y, z, _, _, _, _, t = head.unpack_from(buf, off)
        ids[k], tl[k] = pid, t
        xyz[k] = (x, y, z)
        off += head.size + 8 * t
    if off != len(buf):
        raise ValueError(f"{path}: {len(buf) - off} bytes beyond the {n} points")
    order = np.argsort(ids, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return {"ids": ids[order], "xyz": xyz[order], "track_len": tl[order], "file_order": rank}


def read_images_binary(path):
    """``images.bin`` -> ``{'image_ids' int32 [m], 'names' [m] str, 'point3D_ids' [m] arrays of
    int64 [n_i]}`` in file order (-1: a feature without a 3D point)."""
    with open(path, "rb") as f:
        buf = f.read()
    (m,) = struct.unpack_from("<Q", buf, 0)
    off = 8
    ids, names, p3d = np.empty(m, dtype=np.int32), [], []
    head = struct.Struct("<i4d3di")   # image id, qvec, tvec, camera id
    rec = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    for k in range(m):
        ids[k] = head.unpack_from(buf, off)[0]
        off += head.size
        end = buf.index(b"\x00", off)
        names.append(buf[off:end].decode("utf-8"))
        off = end + 1
        (n,) = struct.unpack_from("<Q", buf, off)
        off += 8
        if off + n * rec.itemsize > len(buf):
            raise ValueError(f"{path}: truncated at image {k}")
        p3d.append(np.frombuffer(buf, dtype=rec, count=n, offset=off)["id"].astype(np.int64))
        off += n * rec.itemsize
    if off != len(buf):
        raise ValueError(f"{path}: {len(buf) - off} bytes beyond the {m} images")
    return {"image_ids": ids, "names": names, "point3D_ids": p3d}


def _points(points3D):
    if isinstance(points3D, (str, os.PathLike)):
        p = os.fspath(points3D)
        if os.path.isdir(p):
            p = os.path.join(p, "points3D.bin")
        return read_points3d_binary(p)
    return points3D


def _images(images):
    if isinstance(images, (str, os.PathLike)):
        p = os.fspath(images)
        if os.path.isdir(p):
            p = os.path.join(p, "images.bin")
        return read_images_binary(p)
    return images


def _box(box):
    c = np.loadtxt(box) if isinstance(box, (str, os.PathLike)) else np.asarray(box)
    c = np.asarray(c, dtype=np.float64)
    if c.shape != (8, 3):
        raise ValueError(f"the 3D box is 8 corners x 3, got {c.shape}")
    return c


def _gpu(device):
    """The torch device when the kernels are to run, None for the numpy formulation."""
    if device is None:
        return None
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device={device!r}: the kernels need a GPU; pass None for the numpy path")
    return dev


# ------------------------------------------------------------------ the kernels, tensor in / out
def _i32(n, dev):
    return torch.empty(n, dtype=torch.int32, device=dev)


def filter_points_device(xyz, track_len, min_track, corners, dev):
    """onepose_filter_points -> (xyz_out float32 [m, 3], index int32 [m]) on the device."""
    xyz = torch.as_tensor(xyz, dtype=torch.float64).to(dev).contiguous()
    n = xyz.shape[0]
    tl = None
    if track_len is not None:
        tl = torch.as_tensor(np.minimum(np.asarray(track_len), 2**31 - 1).astype(np.int32)).to(dev)
    cn = None if corners is None else torch.as_tensor(corners, dtype=torch.float64).to(dev).contiguous()
    out, idx, cnt = torch.empty(n, 3, dtype=torch.float32, device=dev), _i32(n, dev), _i32(1, dev)
    _lib.run("onepose_filter_points", xyz=xyz, track_len=tl, n=n,
             min_track=int(min(int(min_track), 2**31 - 1)), corners=cn, xyz_out=out,
             index_out=idx, count=cnt, stream=_lib.stream_ptr(dev))
    m = int(cnt.item())
    return out[:m], idx[:m]


def _xyz_dtype(xyz):
    if xyz.dtype == torch.float32:
        return OBJ_F32
    if xyz.dtype == torch.float64:
        return OBJ_F64
    raise TypeError(f"xyz must be float32 or float64, got {xyz.dtype}")


def radius_neighbours_device(xyz, thr, capacity=None):
    """onepose_radius_neighbours -> (row_start int32 [n + 1], cols int32 [total]); the list is
    sized by a second call when the first capacity (2 n + 1024 by default) is too small."""
    dev, n, dt = xyz.device, xyz.shape[0], _xyz_dtype(xyz)
    rs, info = _i32(n + 1, dev), torch.empty(2, dtype=torch.int64, device=dev)
    cap = int(2 * n + 1024 if capacity is None else capacity)
    for _ in range(2):
        cols = _i32(max(cap, 1), dev)
        _lib.run("onepose_radius_neighbours", xyz=xyz, xyz_dtype=dt, n=n, thr=float(thr),
                 row_start=rs, cols=cols, cols_capacity=cap, info=info,
                 stream=_lib.stream_ptr(dev))
        total, status = (int(v) for v in info.tolist())
        if status == 0:
            return rs, cols[:total]
        if status == 2:
            raise _lib.OnePoseError(f"radius_neighbours: {total} pairs exceed 2^31 - 1")
        cap = total
    raise _lib.OnePoseError("radius_neighbours: the pair count changed between two calls")


def merge_greedy_device(xyz, row_start, cols):
    """onepose_merge_greedy -> (cluster_of [n], member_start [m + 1], members, mean float64 [m, 3])."""
    dev, n = xyz.device, xyz.shape[0]
    cof, ms, mem, info = _i32(n, dev), _i32(n + 1, dev), _i32(n, dev), _i32(2, dev)
    mean = torch.empty(n, 3, dtype=torch.float64, device=dev)
    _lib.run("onepose_merge_greedy", xyz=xyz, xyz_dtype=_xyz_dtype(xyz), n=n, row_start=row_start,
             cols=cols, cluster_of=cof, member_start=ms, members=mem, mean=mean, info=info,
             stream=_lib.stream_ptr(dev))
    m, status = info.tolist()
    if status != 0:
        raise _lib.OnePoseError("merge_greedy: row_start / cols is not a CSR over these points")
    ms = ms[:m + 1]
    return cof, ms, mem[:int(ms[-1])], mean[:m]


def lift_descriptors_device(bank, block_offset, block_cols, obs_block, obs_feat, seg_len, dim):
    """onepose_lift_descriptors on device tensors -> (seg_start int32 [n3 + 1], collected float64
    [dim, n_obs], mean64 [dim, n3], mean32 [dim, n3])."""
    dev, n_obs, n3 = bank.device, obs_block.shape[0], seg_len.shape[0]
    ss, info = _i32(n3 + 1, dev), _i32(2, dev)
    collected = torch.empty(dim, n_obs, dtype=torch.float64, device=dev)
    m64 = torch.empty(dim, n3, dtype=torch.float64, device=dev)
    m32 = torch.empty(dim, n3, dtype=torch.float32, device=dev)
    _lib.run("onepose_lift_descriptors", bank=bank, bank_numel=bank.numel(),
             block_offset=block_offset, block_cols=block_cols, n_blocks=block_cols.shape[0],
             obs_block=obs_block, obs_feat=obs_feat, n_obs=n_obs, seg_len=seg_len, n3=n3, dim=dim,
             seg_start=ss, collected=collected, mean64=m64, mean32=m32, info=info,
             stream=_lib.stream_ptr(dev))
    status, where = info.tolist()
    if status != 0:
        raise _lib.OnePoseError(f"lift_descriptors: {LIFT_STATUS.get(status, status)} (index {where})")
    return ss, collected, m64, m32


def gather_leaves_device(collected, cols):
    """onepose_gather_leaves -> float32 [dim, len(cols)]; ``cols`` int64, dustbin = n_obs."""
    dev = collected.device
    dim, n_obs = collected.shape
    cols = torch.as_tensor(cols, dtype=torch.int64).to(dev).contiguous()
    out = torch.empty(dim, cols.shape[0], dtype=torch.float32, device=dev)
    _lib.run("onepose_gather_leaves", collected=collected, n_obs=n_obs, dim=dim, cols=cols,
             n_cols=cols.shape[0], out=out, stream=_lib.stream_ptr(dev))
    return out


# ------------------------------------------------------------------ the same arithmetic in numpy
def _host_box_mask(p32, corners):
    c = corners.astype(np.float32)
    q = p32 - c[4]
    keep = np.ones(p32.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (5, 0, 7):
            v = c[o] - c[4]
            m = (q[:, 0] * v[0] + q[:, 1] * v[1]) + q[:, 2] * v[2]
            vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
            keep &= (0 < m) & (m < vv)
    return keep


def _host_neighbours(x, thr):
    """CSR of {i : i == j or sqrt(((dx dx) + dy dy) + dz dz) < thr}, float64 on the widened
    values, a block of rows at a time."""
    xd = x.astype(np.float64)
    n = xd.shape[0]
    step = max(1, (1 << 21) // max(n, 1))
    counts, cols = np.zeros(n, dtype=np.int64), []
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, n, step):
            blk = xd[j0:j0 + step]
            d = xd[None, :, :] - blk[:, None, :]
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            hit = np.sqrt(s) < thr
            r = np.arange(blk.shape[0])
            hit[r, j0 + r] = True
            jj, ii = np.nonzero(hit)
            counts[j0:j0 + blk.shape[0]] = np.bincount(jj, minlength=blk.shape[0])
            cols.append(ii.astype(np.int32))
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=row_start[1:])
    return row_start, np.concatenate(cols) if cols else np.zeros(0, np.int32)


def _host_greedy(x, row_start, cols):
    n = x.shape[0]
    recorded = np.zeros(n, dtype=bool)
    cluster_of = np.full(n, -1, dtype=np.int32)
    member_start, members, means = [0], [], []
    for j in range(n):
        nb = cols[row_start[j]:row_start[j + 1]]
        if recorded[nb].any():
            continue
        recorded[nb] = True
        cluster_of[nb] = len(means)
        s = x[nb[0]]
        for i in nb[1:]:
            s = s + x[i]
        means.append((s / x.dtype.type(len(nb))).astype(np.float64))
        members.append(nb)
        member_start.append(member_start[-1] + len(nb))
    mem = np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32)
    mean = np.stack(means) if means else np.zeros((0, 3))
    return cluster_of, np.asarray(member_start, dtype=np.int32), mem, mean


# ------------------------------------------------------------------ the reference's functions
def get_tkl(points3D, thres, show=False):
    """The track length that limits the 3D points to ``thres``: the smallest length at which the
    number of points LONGER than it first drops to <= thres.  Points of exactly that length pass
    ``filter_by_track_length`` too, so the filtered count may exceed ``thres``, as in the
    reference.  ``points3D``: a model directory, a ``points3D.bin`` path or
    ``read_points3d_binary``'s result.  Returns ``(track_length, points_count_list)``, the list in
    the file's point order."""
    pts = _points(points3D)
    tl = pts["track_len"]
    keys, counts = np.unique(tl, return_counts=True)
    left = tl.shape[0] - np.cumsum(counts)
    hit = np.nonzero(left <= thres)[0]
    if hit.size == 0:
        raise ValueError(f"get_tkl: no track length limits {tl.shape[0]} points to {thres}")
    return keys[hit[0]], tl[pts["file_order"]].tolist()


def filter_by_track_length(points3D, track_length, device=None):
    """Points with at least ``track_length`` observations, in ascending id order ->
    ``(xyzs float64 [m, 3], points_idxs int64 [m])``."""
    pts = _points(points3D)
    dev = _gpu(device)
    if dev is None or pts["ids"].shape[0] == 0:
        keep = np.nonzero(pts["track_len"] >= track_length)[0]
    else:
        _, idx = filter_points_device(pts["xyz"], pts["track_len"], track_length, None, dev)
        keep = idx.cpu().numpy().astype(np.int64)
    return pts["xyz"][keep].reshape(-1, 3), pts["ids"][keep].astype(np.int64)


def filter_by_3d_box(points, points_idxs, box, device=None):
    """Points strictly inside the box -> ``(float32 tensor [m, 3], points_idxs[passed])``.
    ``box``: the path of ``box3d_corners.txt`` or the 8 x 3 corners."""
    corners = _box(box)
    if not isinstance(points, torch.Tensor):
        points = torch.as_tensor(np.asarray(points), dtype=torch.float32)
    assert points.dim() == 2 and points.shape[1] == 3, "Input pcds must have shape (n, 3)"
    points = points.detach().cpu().to(torch.float32)
    points_idxs = np.asarray(points_idxs)
    dev = _gpu(device)
    if dev is None or points.shape[0] == 0:
        passed = np.nonzero(_host_box_mask(points.numpy(), corners))[0]
    else:
        _, idx = filter_points_device(points.to(torch.float64), None, 0, corners, dev)
        passed = idx.cpu().numpy().astype(np.int64)
    return points[torch.from_numpy(passed)], points_idxs[passed]


def filter_3d(model_path, track_length, box_path, device=None):
    """Track-length and box filter of a model's points (one kernel call on a GPU)."""
    pts = _points(model_path)
    dev = _gpu(device)
    if dev is None or pts["ids"].shape[0] == 0:
        xyzs, idxs = filter_by_track_length(pts, track_length)
        return filter_by_3d_box(xyzs, idxs, box_path)
    out, idx = filter_points_device(pts["xyz"], pts["track_len"], track_length, _box(box_path), dev)
    return out.cpu(), pts["ids"][idx.cpu().numpy().astype(np.int64)].astype(np.int64)


def _merge_arrays(xyzs, dist_threshold, dev):
    """(cluster_of, member_start, members, mean) as numpy arrays."""
    if dev is None:
        rs, cols = _host_neighbours(xyzs, dist_threshold)
        return _host_greedy(xyzs, rs, cols)
    x = torch.from_numpy(np.ascontiguousarray(xyzs)).to(dev)
    rs, cols = radius_neighbours_device(x, dist_threshold)
    return tuple(t.cpu().numpy() for t in merge_greedy_device(x, rs, cols))


def merge(xyzs, points_idxs, dist_threshold=1e-3, device=None):
    """Merge points closer than ``dist_threshold`` -> ``(ret_points float64 [m, 3], {new_idx:
    old ids})``.  The reference's greedy pass, quirk included: a point skipped because a
    neighbour was already merged, and picked up by no later cluster, is dropped.  Distances are
    float64 on the given values; the mean is summed in the dtype of ``xyzs`` (float32 in the real
    flow, where ``filter_by_3d_box`` hands over a float32 tensor)."""
    if isinstance(xyzs, torch.Tensor):
        xyzs = xyzs.detach().cpu().numpy()
    if not isinstance(xyzs, np.ndarray):
        xyzs = np.array(xyzs)
    if xyzs.dtype not in (np.float32, np.float64):
        xyzs = xyzs.astype(np.float64)
    xyzs = np.ascontiguousarray(xyzs).reshape(-1, 3)
    points_idxs = np.asarray(points_idxs)
    if not (dist_threshold > 0 and np.isfinite(dist_threshold)):
        raise ValueError(f"merge: dist_threshold={dist_threshold} is not positive and finite")
    if xyzs.shape[0] != points_idxs.shape[0]:
        raise ValueError(f"merge: {xyzs.shape[0]} points but {points_idxs.shape[0]} ids")
    if xyzs.shape[0] == 0:
        return np.empty((0, 3)), {}
    _, ms, mem, mean = _merge_arrays(xyzs, float(dist_threshold), _gpu(device))
    ret_idxs = {c: points_idxs[mem[ms[c]:ms[c + 1]]] for c in range(len(ms) - 1)}
    return mean.astype(np.float64).reshape(-1, 3), ret_idxs


# ------------------------------------------------------------------ descriptor lifting
def collect_observations(images, img_lists, points_idxs):
    """The observation list in the reference's collect order: per new point in cluster order,
    per old point in the cluster's order, per image in ``img_lists`` order, per feature of that
    image in ascending index order whose ``point3D_ids`` entry is that old id.

    Returns ``(obs_image int32 [S], obs_feat int32 [S], idxs int64 [N3])``: ``obs_image`` indexes
    ``img_lists``, ``idxs[p]`` is the number of observations of new point ``p``.  An old point
    without an observation in ``img_lists``, or an image that the model lacks, raises
    ``KeyError`` as ``gather_3d_ann`` does."""
    images = _images(images)
    name_to_row = {name: k for k, name in enumerate(images["names"])}
    lens = np.asarray([len(v) for v in points_idxs.values()], dtype=np.int64)
    old = (np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in points_idxs.values()])
           if len(lens) else np.zeros(0, np.int64))
    order = np.argsort(old, kind="stable")
    sorted_old = old[order]
    if np.any(sorted_old[1:] == sorted_old[:-1]):
        raise AssertionError("an old point belongs to two new points")   # id_mapping's assert
    pos_l, img_l, feat_l = [], [], []
    for k, name in enumerate(img_lists):
        ids = images["point3D_ids"][name_to_row[name]]   # KeyError: not in the model
        at = np.minimum(np.searchsorted(sorted_old, ids), max(len(sorted_old) - 1, 0))
        feat = np.nonzero((ids != -1) & (sorted_old[at] == ids))[0] if len(sorted_old) else at[:0]
        pos_l.append(order[at[feat]])
        img_l.append(np.full(feat.shape[0], k, dtype=np.int32))
        feat_l.append(feat.astype(np.int32))
    pos = np.concatenate(pos_l) if pos_l else np.zeros(0, np.int64)
    per_old = np.bincount(pos, minlength=old.shape[0])
    if np.any(per_old == 0):
        raise KeyError(int(old[np.nonzero(per_old == 0)[0][0]]))
    by_pos = np.argsort(pos, kind="stable")   # images and features keep their order
    new_of_old = np.repeat(np.arange(len(lens)), lens)
    idxs = np.bincount(new_of_old, weights=per_old, minlength=len(lens)).astype(np.int64)
    return np.concatenate(img_l)[by_pos], np.concatenate(feat_l)[by_pos], idxs


def _feature_arrays(features, img_lists):
    desc, scores = [], []
    for name in img_lists:
        f = features[name]
        d = np.asarray(f["descriptors"])
        if d.dtype != np.float32 or d.ndim != 2:
            raise TypeError(f"{name}: descriptors must be float32 [dim, n], got {d.dtype} {d.shape}")
        if desc and d.shape[0] != desc[0].shape[0]:
            raise ValueError(f"{name}: descriptor dim {d.shape[0]} != {desc[0].shape[0]}")
        desc.append(d)
        scores.append(np.asarray(f["scores"]).reshape(-1))
    return desc, scores


def lift_descriptors(descriptors, obs_image, obs_feat, idxs, device=None):
    """``descriptors``: per image of ``img_lists`` its float32 ``[dim, n_i]`` block.  Returns
    ``(collected float64 [dim, S], mean64 [dim, N3], mean32 float32 [dim, N3])``, numpy arrays on
    the host path and device tensors on a GPU."""
    dim = descriptors[0].shape[0]
    ncols = np.asarray([d.shape[1] for d in descriptors], dtype=np.int64)
    obs_image, obs_feat = np.asarray(obs_image), np.asarray(obs_feat)
    idxs = np.asarray(idxs).reshape(-1)
    if not 1 <= dim <= 1024:
        raise ValueError(f"lift_descriptors: dim={dim} outside 1..1024")
    if idxs.shape[0] == 0 or np.any(idxs < 1):
        raise ValueError("lift_descriptors: a 3D point without observations")
    if int(idxs.sum()) != obs_image.shape[0] or obs_image.shape != obs_feat.shape:
        raise ValueError("lift_descriptors: idxs do not add up to the observations")
    if np.any(obs_image < 0) or np.any(obs_image >= len(descriptors)) or np.any(obs_feat < 0) \
            or np.any(obs_feat >= ncols[obs_image]):
        raise ValueError("lift_descriptors: an observation outside its image's features")
    dev = _gpu(device)
    if dev is None:
        collected = np.empty((dim, obs_image.shape[0]), dtype=np.float64)
        for b in np.unique(obs_image):
            sel = obs_image == b
            collected[:, sel] = descriptors[b][:, obs_feat[sel]]
        mean64 = np.ascontiguousarray(
            data_utils.mean_descriptors(np.ascontiguousarray(collected.T), idxs).T)
        return collected, mean64, mean64.astype(np.float32)
    bank = torch.from_numpy(np.concatenate([np.ascontiguousarray(d).reshape(-1)
                                            for d in descriptors])).to(dev)
    off = np.zeros(len(descriptors), dtype=np.int64)
    np.cumsum(ncols[:-1] * dim, out=off[1:])

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    _, collected, m64, m32 = lift_descriptors_device(
        bank, up(off, np.int64), up(ncols, np.int32), up(obs_image, np.int32),
        up(obs_feat, np.int32), up(idxs, np.int32), dim)
    return collected, m64, m32


def build_object(model_dir, features, img_lists, box, max_num_kp3d=2500, dist_threshold=1e-3,
                 device=None):
    """``run.py:220-249`` up to the arrays: ``{'keypoints3d' float64 [N3, 3], 'idxs' int64 [N3],
    'collected', 'mean64', 'mean32' (as ``lift_descriptors``), 'scores' float64 [S, 1],
    'track_length'}``."""
    pts = _points(model_dir)
    track_length, _ = get_tkl(pts, max_num_kp3d)
    xyzs, points_idxs = filter_3d(pts, track_length, box, device=device)
    merge_xyzs, merge_idxs = merge(xyzs, points_idxs, dist_threshold, device=device)
    if not merge_idxs:
        raise ValueError("build_object: no 3D point is left after the filters")
    obs_image, obs_feat, idxs = collect_observations(_images(model_dir), img_lists, merge_idxs)
    desc, scores = _feature_arrays(features, img_lists)
    collected, mean64, mean32 = lift_descriptors(desc, obs_image, obs_feat, idxs, device=device)
    sc = np.empty((obs_image.shape[0], 1), dtype=np.float64)
    for b in np.unique(obs_image):
        sel = obs_image == b
        sc[sel, 0] = scores[b][obs_feat[sel]]
    return {"keypoints3d": merge_xyzs, "idxs": idxs, "collected": collected, "mean64": mean64,
            "mean32": mean32, "scores": sc, "track_length": track_length}


def build_annotations(model_dir, features, img_lists, box, out_dir, max_num_kp3d=2500,
                      dist_threshold=1e-3, device=None):
    """Write ``anno_3d_average.npz``, ``anno_3d_collect.npz`` and ``idxs.npy`` into ``out_dir``
    with the reference's keys, dtypes and shapes (``feature_process.py:191-194, 357-363``)."""
    o = build_object(model_dir, features, img_lists, box, max_num_kp3d, dist_threshold, device)

    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "anno_3d_average.npz"), keypoints3d=o["keypoints3d"],
             descriptors3d=host(o["mean64"]), scores3d=data_utils.mean_scores(o["scores"], o["idxs"]))
    np.savez(os.path.join(out_dir, "anno_3d_collect.npz"), keypoints3d=o["keypoints3d"],
             descriptors3d=host(o["collected"]), scores3d=o["scores"])
    np.save(os.path.join(out_dir, "idxs.npy"), o["idxs"])
    return o


def object_tensors(model_dir, features, img_lists, box, num_leaf=8, max_num_kp3d=2500,
                   dist_threshold=1e-3, device="cuda"):
    """The matcher's three tensors straight from the model, on the device: ``(keypoints3d
    float32 [N3, 3], descriptors3d float32 [dim, N3], leaves float32 [dim, N3 * num_leaf])``.
    The leaf indices consume the global numpy stream exactly as
    ``data_utils.load_object_annotations`` does on the written files."""
    dev = _gpu(device)
    if dev is None:
        raise ValueError("object_tensors runs on a GPU device")
    o = build_object(model_dir, features, img_lists, box, max_num_kp3d, dist_threshold, dev)
    n_obs = o["collected"].shape[1]
    cols = data_utils.leaf_indices(o["idxs"], num_leaf, n_obs)
    leaves = gather_leaves_device(o["collected"], cols)
    kp3 = torch.from_numpy(o["keypoints3d"].astype(np.float32)).to(dev)
    return kp3, o["mean32"], leaves

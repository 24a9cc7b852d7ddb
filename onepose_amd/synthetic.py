"""Seeded synthetic weights and scenes for the GATsSPG 2D-3D path.

There are no checkpoints or datasets in this environment, so every
test, fixture and benchmark is driven by the generators below.  They only use
``numpy.random.RandomState`` (legacy stream, version-stable) so fixtures made here
regenerate bit-identically on the GPU box.

* ``make_state_dict`` -- a ``GATsSuperGlue`` state dict with the reference's keys and
  shapes (``src/models/GATsSPG_architectures/GATs_SuperGlue.py:162-201``, ``GATs.py:50-53``).
  ``well_conditioned=True`` follows SURVEY.md §8c: ``final_proj`` orthogonal with zero
  bias and every ``mlp[-1].weight`` scaled by ``mlp_scale`` (0.01-0.05) so the GNN keeps
  descriptors close to their inputs and the matcher produces real matches.
* ``make_object`` -- one object's SfM cloud: 3D points, per-point collected 2D
  descriptors + ``idxs`` (the ``anno_3d_collect.npz`` / ``idxs.npy`` format,
  ``src/sfm/postprocess/feature_process.py:191-194,357-363``) and their averages
  (``anno_3d_average.npz``, ``feature_process.py:297-305``).
* ``make_frame`` -- one query frame of that object: GT pose, crop intrinsics, 2D keypoints
  (projected inliers + uniform outliers) and unit 2D descriptors, using the projection
  convention of ``src/utils/vis_utils.py:209-236`` (``K [R|t] X``).
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

DESC_DIM = 256
HEADS = 4
N_LAYERS = 12          # ['GATs', 'self', 'cross'] * 4  (GATs_SuperGlue.py:184)
KENC_LAYERS = (32, 64, 128)

DEFAULT_HPARAMS = {
    # configs/experiment/train_GATsSPG.yaml:44-60
    "descriptor_dim": 256,
    "keypoints_encoder": [32, 64, 128],
    "match_threshold": 0.2,
    "match_type": "softmax",
    "scale_factor": 0.07,
    "include_self": True,
    "with_linear_transform": False,
    "additional": False,
}


def layer_kind(i: int) -> str:
    return ("GATs", "self", "cross")[i % 3]


def _conv_default(rs, out_c, in_c):
    # torch.nn.Conv1d default init: kaiming_uniform(a=sqrt(5)) -> U(-1/sqrt(fan_in), +)
    bound = 1.0 / np.sqrt(in_c)
    w = rs.uniform(-bound, bound, size=(out_c, in_c, 1)).astype(np.float32)
    b = rs.uniform(-bound, bound, size=(out_c,)).astype(np.float32)
    return w, b


def _xavier_normal(rs, shape, gain=1.414):
    # GATs.py:50-53 -- nn.init.xavier_normal_(gain=1.414); fan_in = size(1), fan_out = size(0)
    fan_out, fan_in = shape[0], shape[1]
    std = gain * np.sqrt(2.0 / (fan_in + fan_out))
    return (rs.standard_normal(size=shape) * std).astype(np.float32)


def make_state_dict(seed: int = 0, well_conditioned: bool = True,
                    mlp_scale: float = 0.03) -> dict[str, np.ndarray]:
    """A full ``GATsSuperGlue`` state dict (5,674,401 parameters) as float32 numpy."""
    rs = np.random.RandomState(seed)
    sd: dict[str, np.ndarray] = {}
    sd["bin_score"] = np.array(1.0, dtype=np.float32)
    for name, inp in (("kenc_2d", 3), ("kenc_3d", 4)):
        chans = [inp, *KENC_LAYERS, DESC_DIM]
        for j in range(len(chans) - 1):
            w, b = _conv_default(rs, chans[j + 1], chans[j])
            if j == len(chans) - 2:
                b[:] = 0.0
            sd[f"{name}.encoder.{3 * j}.weight"] = w
            sd[f"{name}.encoder.{3 * j}.bias"] = b
    for i in range(N_LAYERS):
        p = f"gnn.layers.{i}"
        if layer_kind(i) == "GATs":
            sd[f"{p}.W"] = _xavier_normal(rs, (DESC_DIM, DESC_DIM))
            sd[f"{p}.a"] = _xavier_normal(rs, (2 * DESC_DIM, 1))
            continue
        w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
        sd[f"{p}.attn.merge.weight"], sd[f"{p}.attn.merge.bias"] = w, b
        for j in range(3):
            w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
            sd[f"{p}.attn.proj.{j}.weight"], sd[f"{p}.attn.proj.{j}.bias"] = w, b
        w, b = _conv_default(rs, 2 * DESC_DIM, 2 * DESC_DIM)
        sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"] = w, b
        w, b = _conv_default(rs, DESC_DIM, 2 * DESC_DIM)
        b[:] = 0.0                                    # GATs_SuperGlue.py:128
        if well_conditioned:
            w *= np.float32(mlp_scale)
        sd[f"{p}.mlp.3.weight"], sd[f"{p}.mlp.3.bias"] = w, b
    w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
    if well_conditioned:
        q, r = np.linalg.qr(rs.standard_normal((DESC_DIM, DESC_DIM)))
        q = q * np.sign(np.diag(r))[None, :]
        w = q.astype(np.float32)[:, :, None]
        b = np.zeros(DESC_DIM, np.float32)
    sd["final_proj.weight"], sd["final_proj.bias"] = w, b
    return sd


def state_dict_sha(sd: dict[str, np.ndarray]) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k], dtype=np.float32).tobytes())
    return h.hexdigest()


def _unit_rows(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@dataclass
class SynthObject:
    keypoints3d: np.ndarray        # [N3, 3] float32, metres, object frame
    desc3d_true: np.ndarray        # [N3, 256] unit "true" descriptor per 3D point
    clt_descriptors: np.ndarray    # [256, sum(idxs)] collected 2D descriptors (anno_3d_collect)
    clt_scores: np.ndarray         # [sum(idxs), 1]
    idxs: np.ndarray               # [N3] int64, observations per 3D point
    avg_descriptors: np.ndarray    # [256, N3] mean of each point's observations (anno_3d_average)
    avg_scores: np.ndarray         # [N3, 1]


def make_object(n3: int, seed: int = 0, noise: float = 0.3,
                min_obs: int = 2, max_obs: int = 12, box: float = 0.1) -> SynthObject:
    rs = np.random.RandomState(1000 + seed)
    kp3 = rs.uniform(-box, box, size=(n3, 3)).astype(np.float32)
    d3 = _unit_rows(rs.standard_normal((n3, DESC_DIM))).astype(np.float32)
    idxs = rs.randint(min_obs, max_obs + 1, size=n3).astype(np.int64)
    owner = np.repeat(np.arange(n3), idxs)
    u = _unit_rows(rs.standard_normal((owner.shape[0], DESC_DIM)))
    clt = _unit_rows(d3[owner] + noise * u).astype(np.float32)            # [sum, 256]
    clt_scores = rs.uniform(0.05, 1.0, size=(owner.shape[0], 1)).astype(np.float32)
    # mean_descriptors (feature_process.py:297-305): plain mean, NOT renormalised
    starts = np.concatenate([[0], np.cumsum(idxs)[:-1]])
    avg = np.add.reduceat(clt.astype(np.float64), starts, axis=0) / idxs[:, None]
    avg_s = np.add.reduceat(clt_scores.astype(np.float64), starts, axis=0) / idxs[:, None]
    return SynthObject(kp3, d3, np.ascontiguousarray(clt.T), clt_scores, idxs,
                       np.ascontiguousarray(avg.T.astype(np.float32)), avg_s.astype(np.float32))


def random_rotation(rs) -> np.ndarray:
    q = rs.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([
        [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
    ])


def crop_intrinsics(size: int = 512, f: float = 600.0) -> np.ndarray:
    return np.array([[f, 0.0, size / 2.0], [0.0, f, size / 2.0], [0.0, 0.0, 1.0]])


def project(K, pose34, pts):
    """vis_utils.reproj semantics: K [R|t] X, divided by depth."""
    cam = pts @ pose34[:, :3].T + pose34[:, 3]
    uv = cam @ K.T
    return uv[:, :2] / uv[:, 2:3]


@dataclass
class SynthFrame:
    keypoints2d: np.ndarray        # [N1, 2] float32 (x, y) pixels
    descriptors2d: np.ndarray      # [256, N1] float32 unit columns
    K: np.ndarray                  # [3, 3] float64
    pose_gt: np.ndarray            # [3, 4] float64, object -> camera, metres
    true_match: np.ndarray         # [N1] int64: 3D index for inlier rows, -1 for outliers


def make_frame(obj: SynthObject, n1: int, seed: int = 0, inlier_frac: float = 0.6,
               confuser_frac: float = 0.15, noise: float = 0.3, px_noise: float = 0.5,
               size: int = 512) -> SynthFrame:
    """Rows: ``inlier_frac`` projected 3D points (+``px_noise`` px) with noisy descriptors of
    their point; ``confuser_frac`` rows that carry a (different) 3D point's descriptor at a
    random pixel -- they match, but are gross outliers for PnP; the rest random."""
    rs = np.random.RandomState(2000 + seed)
    n3 = obj.keypoints3d.shape[0]
    n_in = min(int(round(inlier_frac * n1)), n3)
    n_cf = min(int(round(confuser_frac * n1)), n3 - n_in)
    n_out = n1 - n_in - n_cf
    R = random_rotation(rs)
    t = np.array([rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), rs.uniform(0.35, 0.55)])
    pose = np.concatenate([R, t[:, None]], axis=1)
    K = crop_intrinsics(size)
    perm = rs.permutation(n3)
    pts, cpts = perm[:n_in], perm[n_in:n_in + n_cf]
    uv_in = project(K, pose, obj.keypoints3d[pts].astype(np.float64))
    uv_in += rs.normal(0.0, px_noise, size=uv_in.shape)
    uv_rest = rs.uniform(0, size, size=(n_cf + n_out, 2))
    d_in = _unit_rows(obj.desc3d_true[pts] + noise * _unit_rows(rs.standard_normal((n_in, DESC_DIM))))
    d_cf = _unit_rows(obj.desc3d_true[cpts] + noise * _unit_rows(rs.standard_normal((n_cf, DESC_DIM))))
    d_out = _unit_rows(rs.standard_normal((n_out, DESC_DIM)))
    kp = np.concatenate([uv_in, uv_rest]).astype(np.float32)
    desc = np.concatenate([d_in, d_cf, d_out]).astype(np.float32)
    truth = np.concatenate([pts, -np.ones(n_cf + n_out, np.int64)])
    order = rs.permutation(n1)
    return SynthFrame(kp[order], np.ascontiguousarray(desc[order].T), K, pose, truth[order])


def make_matcher_inputs(n1: int, n3: int, num_leaf: int = 8, seed: int = 0, batch: int = 1,
                        frame_ids=None):
    """Matcher inputs in the reference layout (GATs_SuperGlue.py:209-217), numpy float32.

    Leaves come from the build's own ``build_features3d_leaves`` restatement with a
    numpy RNG seeded here, as ``inference.py:113-130`` does after ``seed_everything``.
    Frame b of the object is ``make_frame(obj, n1, seed * 131 + b)``; ``frame_ids`` picks
    which frames of that one sequence to return (default ``range(batch)``), so a rank of a
    frame-sharded run builds exactly its slice of one global batch (distributed.frame_shard).
    """
    from .data_utils import build_features3d_leaves, pad_features3d_random
    obj = make_object(n3, seed)
    np.random.seed(12345 + seed)
    avg, _ = pad_features3d_random(obj.avg_descriptors, obj.avg_scores, n3)
    leaves, _ = build_features3d_leaves(obj.clt_descriptors, obj.clt_scores, obj.idxs, n3, num_leaf)
    avg, leaves = avg.numpy(), leaves.numpy()
    ids = list(range(batch)) if frame_ids is None else list(frame_ids)
    batch = len(ids)
    frames = [make_frame(obj, n1, seed * 131 + b) for b in ids]
    return {
        "keypoints2d": np.stack([f.keypoints2d for f in frames]),
        "keypoints3d": np.broadcast_to(obj.keypoints3d[None], (batch, n3, 3)).copy(),
        "descriptors2d_query": np.stack([f.descriptors2d for f in frames]),
        "descriptors3d_db": np.broadcast_to(avg[None], (batch,) + avg.shape).copy(),
        "descriptors2d_db": np.broadcast_to(leaves[None], (batch,) + leaves.shape).copy(),
    }, obj, frames



def make_frame_bank(n1: int, n3: int, steps: int, batch: int = 1, seed: int = 0, world: int = 1,
                    rank: int = 0):
    """Per-step query inputs of one object's sequence, for a bank of ``steps`` steps of
    ``batch`` frames on this rank: arrays [steps, batch, ...] (keypoints2d, descriptors2d_query
    in the reference's [256, n1] layout, K, pose_gt) and the global frame ids [steps, batch].
    Step j of the sequence holds global frames [j * world * batch, (j + 1) * world * batch),
    sharded contiguously over ranks (distributed.frame_shard), so rank r's frame (j, i) is
    global frame (j * world + r) * batch + i -- frame g is ``make_frame(obj, n1, seed * 131 +
    g)``, the same frames make_matcher_inputs(frame_ids=...) builds.  The object itself is not
    copied per frame (make_matcher_inputs broadcasts it over the batch)."""
    obj = make_object(n3, seed)
    gid = np.array([[(j * world + rank) * batch + i for i in range(batch)] for j in range(steps)],
                   np.int64)
    frames = [[make_frame(obj, n1, seed * 131 + int(g)) for g in row] for row in gid]
    return {
        "keypoints2d": np.stack([np.stack([f.keypoints2d for f in r]) for r in frames]),
        "descriptors2d_query": np.stack([np.stack([f.descriptors2d for f in r]) for r in frames]),
        "K": np.stack([np.stack([f.K for f in r]) for r in frames]),
        "pose_gt": np.stack([np.stack([f.pose_gt for f in r]) for r in frames]),
        "frame_id": gid,
    }

# ------------------------------------------------------------------ SuperPoint
SUPERPOINT_LAYERS = [   # (name, c_in, c_out, kernel)  superpoint.py:147-162
    ("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3),
    ("conv3a", 64, 128, 3), ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3),
    ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1),
    ("convDa", 128, 256, 3), ("convDb", 256, 256, 1)]

# the reference extraction config (extract_features.py:19-24); note 'keypoints_threshold'
# is not a key SuperPoint reads, so its default keypoint_threshold 0.005 applies
SUPERPOINT_CONF = {"descriptor_dim": 256, "nms_radius": 3, "max_keypoints": 4096,
                   "keypoints_threshold": 0.6}


def superpoint_state_dict(seed: int = 0) -> dict[str, np.ndarray]:
    """Random SuperPoint weights (numpy RandomState, version-stable): He-uniform convs,
    small biases.  The trained weights (superpoint_v1.pth) are not available offline."""
    rs = np.random.RandomState(9000 + seed)
    sd = {}
    for name, cin, cout, k in SUPERPOINT_LAYERS:
        bound = np.sqrt(6.0 / (cin * k * k))
        sd[f"{name}.weight"] = rs.uniform(-bound, bound, (cout, cin, k, k)).astype(np.float32)
        sd[f"{name}.bias"] = rs.uniform(-0.05, 0.05, cout).astype(np.float32)
    return sd


def superpoint_image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """A grayscale test image in [0, 1] ([h, w] float32): smooth blobs, edges and texture,
    so the detector finds distinct local maxima."""
    rs = np.random.RandomState(7000 + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w))
    for _ in range(24):
        cy, cx = rs.uniform(0, h), rs.uniform(0, w)
        s = rs.uniform(2.0, 9.0)
        img += rs.uniform(-1, 1) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    for _ in range(6):
        a, b, c = rs.uniform(-1, 1, 3)
        img += 0.3 * (a * (yy - h / 2) + b * (xx - w / 2) + c * h > 0)
    img += 0.05 * rs.randn(h, w)
    img = (img - img.min()) / (img.max() - img.min())
    return img.astype(np.float32)


# ---------------------------------------------------------------------------------------
# SuperGlue 2D-2D matcher (src/models/matchers/SuperGlue/superglue.py)
# ---------------------------------------------------------------------------------------
SUPERGLUE_KENC = (32, 64, 128, 256)     # default_config['keypoint_encoder'] (superglue.py:241)
SUPERGLUE_LAYERS = 18                   # ['self', 'cross'] * 9 (:242)
SUPERGLUE_IMAGE = 512                   # make_superglue_inputs' image side


def _bn_stats(rs, sd, prefix, c):
    # eval-mode BatchNorm1d: default affine (1, 0), running statistics randomised so the fold
    # into the preceding convolution is exercised
    sd[f"{prefix}.weight"] = np.ones(c, np.float32)
    sd[f"{prefix}.bias"] = np.zeros(c, np.float32)
    sd[f"{prefix}.running_mean"] = (0.1 * rs.standard_normal(c)).astype(np.float32)
    sd[f"{prefix}.running_var"] = rs.uniform(0.5, 1.5, size=c).astype(np.float32)
    sd[f"{prefix}.num_batches_tracked"] = np.array(0, dtype=np.int64)


def superglue_state_dict(seed: int = 0, well_conditioned: bool = True, affine_bn: bool = False,
                         bin_score: float = 1.0) -> dict[str, np.ndarray]:
    """A full ``SuperGlue`` state dict with the reference's keys and shapes (superglue.py:247-262):
    torch-default conv initialisation, randomised BatchNorm running statistics; with
    ``well_conditioned`` the last conv of every layer's MLP is scaled by 0.3 and ``final_proj``
    is 20 x a random orthogonal matrix with zero bias, so the matcher produces real matches.
    With ``affine_bn`` every BatchNorm gets a trained-like affine part, gamma ~ U(0.5, 1.5) and
    beta ~ 0.1 N(0, 1), drawn from a stream of their own (every other tensor is what it is without
    the flag); ``bin_score`` is the dustbin score (the trained value is about 2.37)."""
    rs = np.random.RandomState(seed)
    sd: dict[str, np.ndarray] = {"bin_score": np.array(bin_score, dtype=np.float32)}
    chans = [3, *SUPERGLUE_KENC, DESC_DIM]
    for j in range(len(chans) - 1):
        w, b = _conv_default(rs, chans[j + 1], chans[j])
        if j == len(chans) - 2:
            b[:] = 0.0                                   # superglue.py:96
        sd[f"kenc.encoder.{3 * j}.weight"], sd[f"kenc.encoder.{3 * j}.bias"] = w, b
        if j < len(chans) - 2:
            _bn_stats(rs, sd, f"kenc.encoder.{3 * j + 1}", chans[j + 1])
    for i in range(SUPERGLUE_LAYERS):
        p = f"gnn.layers.{i}"
        w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
        sd[f"{p}.attn.merge.weight"], sd[f"{p}.attn.merge.bias"] = w, b
        for j in range(3):
            w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
            sd[f"{p}.attn.proj.{j}.weight"], sd[f"{p}.attn.proj.{j}.bias"] = w, b
        w, b = _conv_default(rs, 2 * DESC_DIM, 2 * DESC_DIM)
        sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"] = w, b
        _bn_stats(rs, sd, f"{p}.mlp.1", 2 * DESC_DIM)
        w, b = _conv_default(rs, DESC_DIM, 2 * DESC_DIM)
        b[:] = 0.0                                       # superglue.py:155
        if well_conditioned:
            w *= np.float32(0.3)
        sd[f"{p}.mlp.3.weight"], sd[f"{p}.mlp.3.bias"] = w, b
    w, b = _conv_default(rs, DESC_DIM, DESC_DIM)
    if well_conditioned:
        q, r = np.linalg.qr(rs.standard_normal((DESC_DIM, DESC_DIM)))
        q = q * np.sign(np.diag(r))[None, :]
        w = (20.0 * q).astype(np.float32)[:, :, None]
        b = np.zeros(DESC_DIM, np.float32)
    sd["final_proj.weight"], sd["final_proj.bias"] = w, b
    if affine_bn:
        ra = np.random.RandomState([seed, 0xB17])
        for k in [k for k in sd if k.endswith(".running_mean")]:
            p = k[: -len(".running_mean")]
            c = sd[k].shape[0]
            sd[f"{p}.weight"] = ra.uniform(0.5, 1.5, size=c).astype(np.float32)
            sd[f"{p}.bias"] = (0.1 * ra.standard_normal(c)).astype(np.float32)
    return sd


def _sg_derive(rs, kp, desc, n):
    """n points of another view of (kp [k,2], desc [k,256]): a random subset (n <= k) or a
    resampling, with 2 px keypoint noise and 0.03 descriptor noise; one third replaced by
    random outliers."""
    k = kp.shape[0]
    idx = rs.permutation(k)[:n] if n <= k else rs.randint(0, k, size=n)
    kp1 = kp[idx] + 2.0 * rs.standard_normal((n, 2))
    d1 = _unit_rows(desc[idx] + 0.03 * rs.standard_normal((n, DESC_DIM)))
    out = rs.permutation(n)[: n // 3]
    kp1[out] = rs.uniform(0, SUPERGLUE_IMAGE, size=(len(out), 2))
    d1[out] = _unit_rows(rs.standard_normal((len(out), DESC_DIM)))
    return kp1, d1


def make_superglue_inputs(n0: int, n1: int, seed: int = 0, batch: int = 1,
                          shared1: bool = False, image_hw0=(SUPERGLUE_IMAGE, SUPERGLUE_IMAGE),
                          image_hw1=(SUPERGLUE_IMAGE, SUPERGLUE_IMAGE)) -> dict[str, np.ndarray]:
    """The reference's ``data`` dict for ``SuperGlue.forward`` (superglue.py:264-284) as float32
    numpy: descriptors0/1 [B,256,n], keypoints0/1 [B,n,2], scores0/1 [B,n], image0/1 (only their
    shape is read: ``image_hw0`` / ``image_hw1`` = (h, w), 512 x 512 by default).  Image 1's
    points are another view of image 0's (``_sg_derive``).  The points are drawn in the 512 x 512
    square and then scaled to each image's (h, w).
    With ``shared1`` image 1 is one set for the whole batch (made from sample 0's image 0; the
    other samples' image 0 are views of it) and is returned with batch dimension 1."""
    rs = np.random.RandomState(seed)
    kp0, d0, kp1, d1 = [], [], [], []
    for b in range(batch):
        if shared1 and b > 0:
            k, d = _sg_derive(rs, kp1[0], d1[0], n0)
        else:
            k = rs.uniform(0, SUPERGLUE_IMAGE, size=(n0, 2))
            d = _unit_rows(rs.standard_normal((n0, DESC_DIM)))
        kp0.append(k)
        d0.append(d)
        if not (shared1 and b > 0):
            k1, dd1 = _sg_derive(rs, k, d, n1)
            kp1.append(k1)
            d1.append(dd1)
    b1 = len(kp1)
    f32 = np.float32
    kp0, kp1 = np.stack(kp0), np.stack(kp1)
    (h0, w0), (h1, w1) = image_hw0, image_hw1
    if (h0, w0) != (SUPERGLUE_IMAGE, SUPERGLUE_IMAGE):
        kp0 = kp0 * (np.array([w0, h0], np.float64) / SUPERGLUE_IMAGE)
    if (h1, w1) != (SUPERGLUE_IMAGE, SUPERGLUE_IMAGE):
        kp1 = kp1 * (np.array([w1, h1], np.float64) / SUPERGLUE_IMAGE)
    return {
        "descriptors0": np.ascontiguousarray(np.stack(d0).transpose(0, 2, 1)).astype(f32),
        "descriptors1": np.ascontiguousarray(np.stack(d1).transpose(0, 2, 1)).astype(f32),
        "keypoints0": kp0.astype(f32),
        "keypoints1": kp1.astype(f32),
        "scores0": rs.uniform(0.01, 1.0, size=(batch, n0)).astype(f32),
        "scores1": rs.uniform(0.01, 1.0, size=(b1, n1)).astype(f32),
        "image0": np.zeros((batch, 1, h0, w0), f32),
        "image1": np.zeros((b1, 1, h1, w1), f32),
    }


def make_nn_inputs(n0: int, n1: int, seed: int, batch: int = 1, shared1: bool = False,
                   d: int = DESC_DIM, inlier_frac: float = 0.6,
                   noise: float = 0.3) -> dict[str, np.ndarray]:
    """``descriptors0 [B,d,n0]`` / ``descriptors1 [B or 1,d,n1]`` for ``NearestNeighbour.forward``
    (nearest_neighbour.py:41-42) as unit-norm float32 columns.  ``int(inlier_frac * min(n0, n1))``
    columns of each side, at random positions, are noisy copies of common unit sources (a
    perturbation of norm about ``noise``, then renormalised); the rest are random directions.
    With ``shared1`` side 1 is one set for the whole batch, returned with batch dimension 1."""
    rs = np.random.RandomState(seed)
    n_src = int(inlier_frac * min(n0, n1))

    def side(n, src):
        x = _unit_rows(rs.standard_normal((n, d)))
        pos = rs.permutation(n)[:n_src]
        x[pos] = _unit_rows(src + noise / np.sqrt(d) * rs.standard_normal((n_src, d)))
        return x

    d0, d1 = [], []
    src = None
    for b in range(batch):
        if not (shared1 and b > 0):
            src = _unit_rows(rs.standard_normal((n_src, d)))
            d1.append(side(n1, src))
        d0.append(side(n0, src))
    f32 = np.float32
    return {
        "descriptors0": np.ascontiguousarray(np.stack(d0).transpose(0, 2, 1)).astype(f32),
        "descriptors1": np.ascontiguousarray(np.stack(d1).transpose(0, 2, 1)).astype(f32),
    }


def _rodrigues_np(aa):
    th = np.linalg.norm(aa)
    K = np.array([[0.0, -aa[2], aa[1]], [aa[2], 0.0, -aa[0]], [-aa[1], aa[0], 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def make_ba_problem(seed: int, n_cams: int, n_points: int, n_obs: int, active_cams: int = None,
                    observed_points: int = None, dist=(0.35, 0.5), perturb: float = 1.0,
                    zero_rot_cam: bool = False, once_point: bool = False,
                    duplicate: bool = False, noise_px: float = 0.5) -> dict[str, np.ndarray]:
    """A bundle adjustment problem as ``BATracker.apply_ba`` hands it to ``Solve``
    (ba_tracker.py:358-407): ``points [P,3]``, ``cam_pose [C,6]`` (angle-axis, t), ``features
    [N,5]`` = (u, v, f, cx, cy), ``ptIdx`` / ``camIdx [N]`` int64, all float64 otherwise.

    The object fills +-5 cm; cameras stand ``dist`` metres away with f in 450..650 and look at it
    under random rotations.  ``active_cams`` of the cameras and ``observed_points`` of the points
    (random subsets, default all) carry the ``n_obs`` observations: each of them at least one,
    (camera, point) pairs distinct.  Pixels are the true projections plus ``noise_px`` of normal
    noise; the returned variables are the true ones perturbed by ``perturb`` x (3 mm, 0.01 rad,
    3 mm).  ``zero_rot_cam``: the first active camera has angle-axis exactly 0, before and after
    the perturbation.  ``once_point``: one observed point is seen exactly once.  ``duplicate``:
    the last observation repeats the first one's (camera, point) pair with its own pixel noise."""
    rs = np.random.RandomState(seed)
    C, P, N = n_cams, n_points, n_obs
    A = C if active_cams is None else active_cams
    Q = P if observed_points is None else observed_points
    pts = rs.uniform(-0.05, 0.05, (P, 3))
    axis = rs.standard_normal((C, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    aa = axis * rs.uniform(0.2, 2.5, (C, 1))
    t = np.concatenate([rs.uniform(-0.02, 0.02, (C, 2)), rs.uniform(dist[0], dist[1], (C, 1))], 1)
    intr = np.concatenate([rs.uniform(450.0, 650.0, (C, 1)), rs.uniform(246.0, 266.0, (C, 2))], 1)
    cams_on = np.sort(rs.permutation(C)[:A])
    pts_on = np.sort(rs.permutation(P)[:Q])
    if zero_rot_cam:
        aa[cams_on[0]] = 0.0
    n_free = N - int(duplicate) - int(once_point)
    pool = pts_on[:-1] if once_point else pts_on
    assert n_free >= max(A, len(pool)) and n_free <= A * len(pool), "n_obs does not fit"
    pairs = set()
    order = []
    for k in range(max(A, len(pool))):          # everyone at least once
        pr = (int(cams_on[k % A]), int(pool[k % len(pool)]))
        if pr not in pairs:
            pairs.add(pr)
            order.append(pr)
    while len(order) < n_free:
        pr = (int(cams_on[rs.randint(A)]), int(pool[rs.randint(len(pool))]))
        if pr not in pairs:
            pairs.add(pr)
            order.append(pr)
    order = [order[i] for i in rs.permutation(len(order))]
    if once_point:
        order.insert(len(order) // 2, (int(cams_on[-1]), int(pts_on[-1])))
    if duplicate:
        order.append(order[0])
    cam_idx = np.array([c for c, _ in order], dtype=np.int64)
    pt_idx = np.array([p for _, p in order], dtype=np.int64)
    feats = np.zeros((N, 5))
    for n in range(N):
        c, p = cam_idx[n], pt_idx[n]
        x = _rodrigues_np(aa[c]) @ pts[p] + t[c]
        feats[n, :2] = intr[c, 0] * x[:2] / x[2] + intr[c, 1:] + noise_px * rs.standard_normal(2)
        feats[n, 2:] = intr[c]
    d_aa = perturb * 0.01 * rs.standard_normal((C, 3))
    if zero_rot_cam:
        d_aa[cams_on[0]] = 0.0
    cam_pose = np.concatenate([aa + d_aa, t + perturb * 0.003 * rs.standard_normal((C, 3))], 1)
    return {
        "points": pts + perturb * 0.003 * rs.standard_normal((P, 3)),
        "cam_pose": cam_pose,
        "features": feats,
        "ptIdx": pt_idx,
        "camIdx": cam_idx,
    }


def make_triangulation_inputs(n: int, seed: int) -> dict[str, np.ndarray]:
    """Two views of ``n`` points for ``BATracker.apply_triangulation`` (ba_tracker.py:267-273):
    ``K1, K2 [3,3]``, ``Tcw1, Tcw2 [4,4]`` (the inverses of the object-to-camera poses, as
    track_ba passes them, :549-554), ``kpt2d_1, kpt2d_2 [n,2]``, float64.  The views are 0.4 m
    from a +-5 cm object and at least 5 degrees apart.  About a tenth of the pairs each are
    pushed past one of track_ba's filters (:556-571): a pixel displaced by 40..80 px in view 1,
    one in view 2, and a point with world z in 0.2..0.3; the rest carry 0.5 px of noise."""
    rs = np.random.RandomState(seed)
    Ks, poses = [], []
    axis = rs.standard_normal(3)
    axis /= np.linalg.norm(axis)
    base = rs.uniform(0.3, 1.5)
    for v in range(2):
        ang = base + v * np.deg2rad(rs.uniform(8.0, 25.0))
        T = np.eye(4)
        T[:3, :3] = _rodrigues_np(axis * ang)
        T[:3, 3] = [rs.uniform(-0.02, 0.02), rs.uniform(-0.02, 0.02), rs.uniform(0.38, 0.42)]
        poses.append(T)
        f = rs.uniform(450.0, 650.0)
        Ks.append(np.array([[f, 0.0, rs.uniform(246, 266)], [0.0, f, rs.uniform(246, 266)],
                            [0.0, 0.0, 1.0]]))
    X = rs.uniform(-0.05, 0.05, (n, 3))
    kind = rs.randint(0, 10, n) if n > 1 else np.full(1, 9)
    X[kind == 2, 2] = rs.uniform(0.2, 0.3, int((kind == 2).sum()))
    uv = []
    for v in range(2):
        x = X @ poses[v][:3, :3].T + poses[v][:3, 3]
        p = x @ Ks[v].T
        p = p[:, :2] / p[:, 2:] + 0.5 * rs.standard_normal((n, 2))
        far = kind == v
        ang = rs.uniform(0.0, 2.0 * np.pi, n)
        p[far] += (rs.uniform(40.0, 80.0, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[far]
        uv.append(p)
    return {"K1": Ks[0], "K2": Ks[1], "Tcw1": np.linalg.inv(poses[0]),
            "Tcw2": np.linalg.inv(poses[1]), "kpt2d_1": uv[0], "kpt2d_2": uv[1]}

"""Fixtures of the sparse-reconstruction tests.

    python tests/golden/make_golden_sfm.py /path/to/reference

writes sfm_pairs.npz, sfm_matches.npz, sfm_model.npz, sfm_model/*.bin and sfm_tri.npz next to
this file.  What the reference computes itself is recorded from the reference: its
pairs_from_poses (scipy's pdist, numpy's argpartition), its import_matches arithmetic, its
rotmat2qvec and its write_model / read_model.  The reference's path_utils (Windows separators),
cv2 and h5py are stubbed; its COLMAP database is replaced by a recorder.  The triangulation is
this project's own, so its expectations come from tests/sfm_oracle.py, with scipy's
least_squares as a second opinion that shares no code with the oracle.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sfm_cases as C   # noqa: E402
import sfm_oracle as O   # noqa: E402


def stub_reference(ref):
    sys.path.insert(0, ref)
    pu = types.ModuleType("src.utils.path_utils")
    pu.get_gt_pose_path_by_color = lambda p, det_type="GT_box": p.replace(
        "/color/", "/poses_ba/").replace(".png", ".txt")
    sys.modules["src.utils.path_utils"] = pu
    import src.utils
    src.utils.path_utils = pu
    sys.modules["cv2"] = types.ModuleType("cv2")
    h5 = types.ModuleType("h5py")
    h5.File = lambda path, mode="r": H5_FILES[path]
    sys.modules["h5py"] = h5


H5_FILES = {}


class Group(dict):
    """Enough of an h5py group: datasets answer __array__()."""
    class DS:
        def __init__(self, a):
            self.a = a

        def __array__(self, *args, **kw):
            return self.a

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        return v if isinstance(v, Group) else Group.DS(v)

    def close(self):
        pass


# ---- pairs ------------------------------------------------------------------------------------
def random_rotation(rng, max_deg=180.0):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(0, max_deg))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def pose_set(kind, n, rng):
    poses = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        if kind == "near_identity" and i > 0:   # image 0 is within 10 degrees of every other one
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            a = np.deg2rad(8.0)
            Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            poses[i, :3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
        elif kind != "near_identity":
            poses[i, :3, :3] = random_rotation(rng, 60.0)
        poses[i, :3, 3] = rng.uniform(-0.5, 0.5, 3)
    if kind == "ring":   # equal distances: a regular ring of centres, and two identical poses
        for i in range(n):
            az = 2 * np.pi * i / (n - 1)
            R = random_rotation(rng, 60.0) if i % 2 else np.eye(3)
            poses[i, :3, :3] = R
            poses[i, :3, 3] = -R @ np.array([np.cos(az), np.sin(az), 0.0])
        poses[n - 1] = poses[3]
    return poses


PAIR_CASES = {   # name: (kind, images per sequence, num_matched)
    "one_seq_try": ("random", (24,), 10),
    "one_seq_except": ("random", (24,), 30),
    "three_seqs": ("random", (20, 21, 20), 12),
    "one_seq_61": ("random", (61,), 20),
    "all_fail": ("near_identity", (24,), 10),
    "duplicates": ("ring", (24,), 10),
}


def make_pairs(out):
    from src.sfm import pairs_from_poses as ref
    rec = {"numpy_version": np.__version__, "cases": list(PAIR_CASES)}
    margin = np.inf
    for name, (kind, per_seq, num_matched) in PAIR_CASES.items():
        rng = np.random.default_rng(sum(map(ord, name)))
        n = sum(per_seq)
        poses = pose_set(kind, n, rng)
        seq = np.repeat(np.arange(len(per_seq)), per_seq)
        with tempfile.TemporaryDirectory() as tmp:
            imgs = []
            for i in range(n):
                d = os.path.join(tmp, f"seq{seq[i]}")
                os.makedirs(os.path.join(d, "poses_ba"), exist_ok=True)
                np.savetxt(os.path.join(d, "poses_ba", f"{i}.txt"), poses[i], fmt="%.18e")
                imgs.append(os.path.join(d, "color", f"{i}.png"))
            files = [ref.path_utils.get_gt_pose_path_by_color(p) for p in imgs]
            poses = np.stack([np.loadtxt(f) for f in files])   # what the reference reads back
            dist, dR, seqs = ref.get_pairswise_distances(files)
            assert list(seqs) == [f"seq{k}" for k in range(len(per_seq))]
            pairs_file = os.path.join(tmp, "pairs.txt")
            ref.covis_from_pose(imgs, pairs_file, num_matched, max_rotation=None)
            text = open(pairs_file).read()
            index = {p: i for i, p in enumerate(imgs)}
            pairs = np.array([[index[a], index[b]] for a, b in
                              (line.split(" ") for line in text.split("\n") if line)], np.int32)
        off = ~np.eye(n, dtype=bool)
        margin = min(margin, np.abs(dR[off] - 10).min())
        branch = "except" if (num_matched // len(per_seq)) * 2 >= min(per_seq) else "try"
        rec.update({f"{name}_poses": poses, f"{name}_seq": seq, f"{name}_num_matched": num_matched,
                    f"{name}_dist": dist, f"{name}_dR": dR, f"{name}_pairs": pairs.reshape(-1, 2),
                    f"{name}_branch": branch})
        print(f"pairs {name}: n={n} {branch} branch, {len(pairs)} pairs, images without a valid "
              f"candidate: {int((~((dR > 10) & off).any(1)).sum())}, duplicate distances: "
              f"{int(sum(len(r) - len(np.unique(r)) for r in dist))}")
    assert margin >= 1e-6, margin
    rec["dR_margin"] = margin
    np.savez_compressed(os.path.join(out, "sfm_pairs.npz"), **rec)
    print("smallest |dR - 10|:", margin)


# ---- match import ---------------------------------------------------------------------------
def make_matches(out):
    from src.sfm import triangulation as ref

    class Recorder:
        rows = []

        @staticmethod
        def connect(path):
            return Recorder()

        def add_matches(self, id0, id1, matches):
            Recorder.rows.append((id0, id1, np.asarray(matches)))

        def add_two_view_geometry(self, *a):
            pass

        def commit(self):
            pass

        def close(self):
            pass
    ref.COLMAPDatabase = Recorder
    rng = np.random.default_rng(77)
    names = [f"obj/color/{k}.png" for k in range(5)]
    counts = np.array([30, 41, 17, 64, 25])
    pairs = [(0, 1), (1, 0), (2, 3), (0, 1), (3, 4), (4, 3), (1, 2), (0, 4)]
    stub = {}
    for a, b in pairs:
        key = ref.names_to_pair(names[a], names[b])
        if ref.names_to_pair(names[b], names[a]) in stub or key in stub:
            continue
        m0 = np.where(rng.random(counts[a]) < 0.6, rng.integers(0, counts[b], counts[a]), -1)
        stub[key] = {"matches0": m0.astype(np.int16),
                     "matching_scores0": rng.random(counts[a]).astype(np.float16)}
    rec = {"names": names, "counts": counts, "pairs": np.array(pairs),
           "stub_keys": list(stub)}
    for k, v in stub.items():
        rec[f"m0_{k}"], rec[f"s0_{k}"] = v["matches0"], v["matching_scores0"]
    image_ids = {n: i + 1 for i, n in enumerate(names)}
    offsets = np.concatenate([[0], np.cumsum(counts)])
    with tempfile.TemporaryDirectory() as tmp:
        pf = os.path.join(tmp, "pairs.txt")
        with open(pf, "w") as f:
            f.write("\n".join(f"{names[a]} {names[b]}" for a, b in pairs))
        H5_FILES["matches"] = Group({k: Group(v) for k, v in stub.items()})
        for label, score in (("none", None), ("half", 0.5), ("zero", 0)):
            Recorder.rows = []
            ref.import_matches(image_ids, "db", pf, "matches", "features", score, True)
            edges = np.concatenate([np.stack([m[:, 0] + offsets[i0 - 1], m[:, 1] + offsets[i1 - 1]], 1)
                                    for i0, i1, m in Recorder.rows])
            rec[f"edges_{label}"] = edges.astype(np.int32)
            print(f"matches, min_match_score={score}: {len(Recorder.rows)} pairs, {len(edges)} edges")
    np.savez_compressed(os.path.join(out, "sfm_matches.npz"), **rec)


# ---- the model files ------------------------------------------------------------------------
def make_model(out):
    from src.utils.colmap import read_write_model as rw
    rng = np.random.default_rng(91)
    Rs = np.stack([random_rotation(rng) for _ in range(24)] + [np.eye(3), np.diag([1.0, -1, -1]),
                                                               np.diag([-1.0, 1, -1])])
    q = np.stack([rw.rotmat2qvec(R) for R in Rs])
    m, n_pts = 5, 40
    n_kp = rng.integers(20, 40, m)
    qvec, tvec = q[:m], rng.uniform(-1, 1, (m, 3))
    params = rng.uniform(300, 700, (m, 4))
    sizes = rng.integers(400, 700, (m, 2))
    names = [f"obj/seq/color/{k}.png" for k in range(m)]
    xys = [rng.uniform(0, 500, (k, 2)) for k in n_kp]
    p3d = [np.full(k, -1, np.int64) for k in n_kp]
    xyz, err = rng.uniform(-0.2, 0.2, (n_pts, 3)), rng.uniform(0, 3, n_pts)
    t_img, t_idx = [], []
    for p in range(n_pts):
        views = np.sort(rng.permutation(m)[:rng.integers(2, m + 1)])
        idx = np.array([rng.integers(0, n_kp[v]) for v in views])
        for v, i in zip(views, idx):
            p3d[v][i] = p + 1
        t_img.append(views + 1)
        t_idx.append(idx)
    cams = {k + 1: rw.Camera(id=k + 1, model="PINHOLE", width=int(sizes[k, 0]),
                             height=int(sizes[k, 1]), params=params[k]) for k in range(m)}
    imgs = {k + 1: rw.Image(id=k + 1, qvec=qvec[k], tvec=tvec[k], camera_id=k + 1, name=names[k],
                            xys=xys[k], point3D_ids=p3d[k]) for k in range(m)}
    pts = {p + 1: rw.Point3D(id=p + 1, xyz=xyz[p], rgb=np.zeros(3, np.uint8), error=err[p],
                             image_ids=t_img[p], point2D_idxs=t_idx[p]) for p in range(n_pts)}
    d = os.path.join(out, "sfm_model")
    os.makedirs(d, exist_ok=True)
    rw.write_model(cams, imgs, pts, d, ext=".bin")
    rc, ri, rp = rw.read_model(d, ext=".bin")
    rec = {"rot": Rs, "rot_qvec": q, "qvec": qvec, "tvec": tvec, "params": params, "sizes": sizes,
           "names": names, "n_kp": n_kp, "xys": np.concatenate(xys), "p3d": np.concatenate(p3d),
           "xyz": xyz, "err": err, "t_len": np.array([len(t) for t in t_img]),
           "t_img": np.concatenate(t_img), "t_idx": np.concatenate(t_idx),
           "read_point_ids": np.array(sorted(rp)), "read_xyz": np.stack([rp[k].xyz for k in sorted(rp)]),
           "read_track_len": np.array([len(rp[k].image_ids) for k in sorted(rp)]),
           "read_image_ids": np.array(list(ri)), "read_names": [ri[k].name for k in ri],
           "read_p3d": np.concatenate([ri[k].point3D_ids for k in ri])}
    np.savez_compressed(os.path.join(out, "sfm_model.npz"), **rec)
    print("model:", {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))})


# ---- triangulation ----------------------------------------------------------------------------
def make_tri(out):
    from scipy.optimize import least_squares
    p = C.tri_problem()
    margins = []
    args = (p["Rt"], p["K4"], p["track_start"], p["obs_image"], p["obs_xy"], C.MAX_REPROJ,
            C.MIN_ANGLE)
    a = O.triangulate_all(*args, margins=margins)   # the contract: cyclic Jacobi
    eig = O.triangulate_all(*args, solver="eigh")
    b = O.triangulate_all(*args, solver="svd")
    for other in (eig, b):
        assert np.array_equal(a["reason"], other["reason"])
        assert np.array_equal(a["obs_keep"], other["obs_keep"])
    margin = min(margins)
    assert margin >= 1e-6, margin
    T = len(C.TRI_NAMES)
    with np.errstate(invalid="ignore"):
        dev = np.maximum(np.abs(eig["xyz"] - b["xyz"]).max(1), np.abs(eig["err"] - b["err"]))
    tol = np.where(a["reason"] == 0, np.maximum(16 * dev, 1e-12), np.nan)
    ls_xyz, ls_dist = np.full((T, 3), np.nan), np.full(T, np.nan)
    for t, name in enumerate(C.TRI_NAMES):
        print(f"tri {name}: reason {a['reason'][t]}, kept {a['n_kept'][t]} of "
              f"{p['track_start'][t + 1] - p['track_start'][t]}, err {a['err'][t]:.3f}, "
              f"eigh-svd {dev[t]:.2e}")
        if name not in C.TRI_REFINED:
            continue
        assert a["reason"][t] == 0, name
        s, e = p["track_start"][t], p["track_start"][t + 1]
        sel = np.nonzero(a["obs_keep"][s:e])[0] + s
        img, uv = p["obs_image"][sel], p["obs_xy"][sel]

        def resid(X):
            pc = np.einsum("kij,j->ki", p["Rt"][img, :, :3], X) + p["Rt"][img, :, 3]
            K = p["K4"][img]
            return np.concatenate([K[:, 0] * pc[:, 0] / pc[:, 2] + K[:, 2] - uv[:, 0],
                                   K[:, 1] * pc[:, 1] / pc[:, 2] + K[:, 3] - uv[:, 1]])
        sol = least_squares(resid, a["xyz"][t], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        ls_xyz[t], ls_dist[t] = sol.x, np.abs(sol.x - a["xyz"][t]).max()
        print(f"    least_squares minimum: the oracle is {ls_dist[t]:.2e} away (tol {tol[t]:.1e})")
    want = {"len1": 3, "len257": 3, "nan_pixel": 4, "wrong_match": 1, "angle_below": 2, "angle_rays": 2,
            "angle_above": 0}
    for name, why in want.items():
        assert a["reason"][C.TRI_NAMES.index(name)] == why, (name, a["reason"])
    np.savez_compressed(os.path.join(out, "sfm_tri.npz"), sha=C.tri_sha(p), margin=margin, tol=tol,
                        ls_xyz=ls_xyz, ls_dist=ls_dist, **a)
    print("smallest decision margin:", margin)


if __name__ == "__main__":
    stub_reference(sys.argv[1])
    make_pairs(HERE)
    make_matches(HERE)
    make_model(HERE)
    make_tri(HERE)

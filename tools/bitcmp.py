"""Bit-identity check of two library builds: the same matcher, pose and detector calls through
each, outputs compared bit for bit.  Each build runs in its own process (ONEPOSE_LIB selects the library):
    ONEPOSE_LIB=tools/ab/lib_base.so python tools/bitcmp.py dump /tmp/a.npz
    python tools/bitcmp.py dump /tmp/b.npz
    python tools/bitcmp.py cmp /tmp/a.npz /tmp/b.npz
Cases: the uncached forward (onepose_match_ex, conf) and the cached bench path
(onepose_object_prepare + onepose_match_cached, with and without GAT tables) in fp32, bf16 and
fp32_split, on ragged and batched shapes (one with a batch above the fused KV fold's limit and
n3 % 4 != 0), and a world-size-1 sharded frame (onepose_amd.sharded.ShardedMatcher, fp32 and
fp32_split).  The launch-kind sequence of each case's first uncached, cached and sharded call
(onepose_profile_begin / _end) is dumped too: equal sequences show the launch order did not
move.  BITCMP_BIG=1 adds configs 5 and 3's shapes (2048 x 8192, 1024 x 16384: more than 64 score
tiles per row); their conf matrices are compared by SHA-256 digest.
Pose and detector cases (dump_pose_detector, seeded and small): onepose_select_correspondences
at n1 = 1, 1023, 1025; onepose_pnp_ransac on one batch of 3 to 1100 points with 0-70 % outliers;
onepose_pose_stage at n1 = 1100, n3 = 1500 with per-frame K; onepose_affine_partial_ransac on 0
to 1000 points; onepose_detect_stage at n0 = 300 with 3 views."""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

CASES = [(1024, 4096, 8, 1), (200, 777, 8, 2), (96, 300, 3, 1), (256, 1024, 12, 3),
         (64, 130, 3, 5)]   # (n1, n3, num_leaf, batch)
SHARDED = [(96, 300, 3, 1)]   # world size 1, no process group
PRECS = ["fp32", "bf16", "fp32_split"]
if os.environ.get("BITCMP_BIG") == "1":
    CASES += [(2048, 8192, 8, 1), (1024, 16384, 8, 1)]


def _conf(c):
    x = c.cpu().numpy()
    if x.size > 8 << 20:   # (a digest: the bits, not the values, are compared)
        return np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8).copy()
    return x


def _kinds(lib, call, cap=1024):
    """call()'s result and the kinds of the launches it made, in order."""
    from onepose_amd import _lib
    _lib.check(lib.onepose_profile_begin(2 ** 64 - 1, cap), "profile_begin")
    try:
        res = call()
    finally:
        kinds, n = np.full(cap, -1, np.int32), ctypes.c_int(0)
        rc = lib.onepose_profile_end(kinds.ctypes.data, None, cap, ctypes.byref(n))
    _lib.check(rc, "profile_end")
    assert 0 < n.value <= cap, n.value
    return res, kinds[:n.value].copy()


def _pose_frames(rs, S, counts, n1, n3):
    """len(counts) frames of n1 keypoints with counts[b] matches into a table of n3 points each,
    0-70 % of them wrong, under a pose and K of the frame's own."""
    nb = len(counts)
    kp3 = rs.uniform(-0.1, 0.1, (nb, n3, 3)).astype(np.float32)
    kp2 = rs.uniform(0, 512, (nb, n1, 2)).astype(np.float32)
    m0 = -np.ones((nb, n1), np.int64)
    Ks, gts = np.zeros((nb, 3, 3)), np.zeros((nb, 3, 4))
    for b, c in enumerate(counts):
        rows = np.sort(rs.permutation(n1)[:c])
        m0[b, rows] = rs.randint(0, n3, c)
        Ks[b] = [[500.0 + 20 * b, 0, 250.0 + b], [0, 520.0 - 10 * b, 260.0 - b], [0, 0, 1]]
        t = np.array([rs.uniform(-0.03, 0.03), rs.uniform(-0.03, 0.03), rs.uniform(0.35, 0.55)])
        gts[b] = np.concatenate([S.random_rotation(rs), t[:, None]], 1)
        good = rows[rs.rand(c) >= 0.7 * b / max(nb - 1, 1)]
        uv = S.project(Ks[b], gts[b], kp3[b, m0[b, good]].astype(np.float64))
        kp2[b, good] = (uv + rs.normal(0, 0.5, uv.shape)).astype(np.float32)
    return m0, kp2, kp3, Ks, gts


def dump_pose_detector(out, lib, dev):
    """Every output the pose and detector entry points define.  Point lists are kept up to
    counts and the index workspace up to n_inliers: the rest is never written."""
    from onepose_amd import _lib, detector, pose as P, synthetic as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "tests"))
    from detector_cases import scene, stage_case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
    sp = _lib.stream_ptr(dev)

    def ragged(key, x, counts):
        for b, c in enumerate(counts.tolist()):
            out[f"{key}_{b}"] = x[b, :c].cpu().numpy()

    rs = np.random.RandomState(31)
    for n1 in (1, 1023, 1025):
        m0, kp2, kp3, _, _ = _pose_frames(rs, S, [n1 // 2, n1], n1, 300)
        p2, p3, cnt = P.select_correspondences(t(m0), t(kp2), t(kp3), scale=1000.0)
        out[f"sel_{n1}_counts"] = cnt.cpu().numpy()
        ragged(f"sel_{n1}_p2", p2, cnt)
        ragged(f"sel_{n1}_p3", p3, cnt)

    # onepose_pnp_ransac: one batch, the points selected on the host
    counts = [3, 4, 5, 6, 16, 60, 300, 1100]
    nb, M = len(counts), 1100
    m0, kp2, kp3, Ks, _ = _pose_frames(rs, S, counts, M, 1500)
    p2, p3 = np.zeros((nb, M, 2), np.float32), np.zeros((nb, M, 3), np.float32)
    for b, c in enumerate(counts):
        v = m0[b] > -1
        p2[b, :c] = kp2[b, v]
        p3[b, :c] = (kp3[b, m0[b, v]].astype(np.float64) * 1000.0).astype(np.float32)
    o = dict(pose=z(nb, 3, 4, dt=torch.float64), mask=z(nb, M, dt=torch.uint8),
             nin=z(nb, dt=torch.int32), status=z(nb, dt=torch.int32))
    wsb = lib.onepose_pnp_workspace_bytes(nb, M, 10000)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    ins = [t(p2), t(p3), t(np.array(counts, np.int32)), t(Ks)]
    _lib.check(lib.onepose_pnp_ransac(
        ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), M, ins[3].data_ptr(), 9, nb,
        1000.0, 5.0, 10000, 0.99, o["pose"].data_ptr(), o["mask"].data_ptr(), o["nin"].data_ptr(),
        o["status"].data_ptr(), ws.data_ptr(), wsb, sp), "pnp_ransac")
    torch.cuda.synchronize()
    for k, v in o.items():
        out[f"pnp_{k}"] = v.cpu().numpy()
    ragged("pnp_idx", ws[:4 * nb * M].view(torch.int32).view(nb, M), o["nin"])

    # onepose_pose_stage: the shapes of test_pipeline_gpu.py's per-frame case
    nb, n1, n3 = 4, 1100, 1500
    m0, kp2, kp3, Ks, gts = _pose_frames(rs, S, [560, 540, 3, 550], n1, n3)
    f = dict(pts2d=z(nb, n1, 2), pts3d=z(nb, n1, 3), counts=z(nb, dt=torch.int32),
             pose=z(nb, 3, 4, dt=torch.float64), mask=z(nb, n1, dt=torch.uint8),
             nin=z(nb, dt=torch.int32), status=z(nb, dt=torch.int32),
             R_err=z(nb, dt=torch.float64), t_err=z(nb, dt=torch.float64),
             cmd=z(nb, 3, dt=torch.uint8))
    wsb = lib.onepose_pnp_workspace_bytes(nb, n1, 100)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    ins = [t(m0), t(kp2), t(kp3), t(Ks), t(gts)]
    _lib.check(lib.onepose_pose_stage(
        ins[0].data_ptr(), ins[1].data_ptr(), n1 * 2, ins[2].data_ptr(), n3 * 3, nb, n1, n3, 1000.0,
        ins[3].data_ptr(), 9, 3.0, 100, 0.99, ins[4].data_ptr(), 12, f["pts2d"].data_ptr(),
        f["pts3d"].data_ptr(), f["counts"].data_ptr(), f["pose"].data_ptr(), f["mask"].data_ptr(),
        f["nin"].data_ptr(), f["status"].data_ptr(), f["R_err"].data_ptr(), f["t_err"].data_ptr(),
        f["cmd"].data_ptr(), ws.data_ptr(), wsb, sp), "pose_stage")
    torch.cuda.synchronize()
    for k, v in f.items():
        if k in ("pts2d", "pts3d"):
            ragged(f"stage_{k}", v, f["counts"])
        else:
            out[f"stage_{k}"] = v.cpu().numpy()
    ragged("stage_idx", ws[:4 * nb * n1].view(torch.int32).view(nb, n1), f["nin"])

    # onepose_affine_partial_ransac and onepose_detect_stage (inlier_mask whole, iters included)
    counts = [0, 1, 2, 3, 6, 63, 64, 65, 257, 1000]
    frm, to = np.zeros((len(counts), 1000, 2), np.float32), np.zeros((len(counts), 1000, 2), np.float32)
    for b, c in enumerate(counts):
        if c:
            frm[b, :c], to[b, :c], _, _ = scene(c, 0.07 * b, seed=40 + b)
    for k, v in detector.affine_partial_ransac(t(frm), t(to), t(np.array(counts, np.int32))).items():
        out[f"aff_{k}"] = v.cpu().numpy()
    m, c0, k0, k1, hw, qhw = stage_case(spec=((280, 200), (257, 180), (64, 40)), n0=300, n1=320)
    for mode in (0, 1):
        r = detector.detect_stage(t(m), t(c0), t(k0), t(k1), t(hw), qhw, rank_mode=mode)
        for k, v in r.items():
            if k == "mpts":
                ragged(f"det{mode}_mpts", v, r["counts"])
            else:
                out[f"det{mode}_{k}"] = v.cpu().numpy()


def dump(path):
    from onepose_amd import _lib, matcher, sharded, synthetic as S
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = {}
    dump_pose_detector(out, lib, dev)
    for (n1, n3, L, B) in SHARDED:
        sd = S.make_state_dict(1)
        data, _, _ = S.make_matcher_inputs(n1, n3, L, seed=3, batch=B)
        for prec in ("fp32", "fp32_split"):
            m = matcher.from_state_dict(sd, {**S.DEFAULT_HPARAMS, "attention_precision": prec}).to(dev)
            sm = sharded.ShardedMatcher(m, None, data["descriptors3d_db"][0],
                                        data["descriptors2d_db"][0], n1, dev, batch=B)
            d2 = torch.from_numpy(data["descriptors2d_query"]).to(dev)
            res, kinds = _kinds(lib, lambda: sm.match(d2))
            torch.cuda.synchronize()
            key = f"s_{n1}_{n3}_{L}_{B}_{prec}"
            for nm, x in zip(("m0", "m1", "s0", "s1"), res):
                out[f"{key}_{nm}"] = x.cpu().numpy()
            out[f"{key}_kinds"] = kinds
    for (n1, n3, L, B) in CASES:
        sd = S.make_state_dict(1)
        data, _, _ = S.make_matcher_inputs(n1, n3, L, seed=3, batch=B)
        t = {k: torch.from_numpy(v).to(dev) for k, v in data.items()}
        for pi, prec in enumerate(PRECS):
            m = matcher.from_state_dict(sd, {**S.DEFAULT_HPARAMS, "attention_precision": prec}).to(dev)
            with torch.no_grad():
                (pred, conf), kinds = _kinds(lib, lambda: m(t))
            key = f"u_{n1}_{n3}_{L}_{B}_{prec}"
            out[f"{key}_kinds"] = kinds
            for k, v in pred.items():
                out[f"{key}_{k}"] = v.cpu().numpy()
            out[f"{key}_conf"] = _conf(conf)
            # cached path (object = sample 0's object, all frames of the batch)
            w = m.packed_weights(dev)
            f32 = dict(dtype=torch.float32, device=dev)
            s = _lib.stream_ptr(dev)
            d3 = t["descriptors3d_db"][0].contiguous()
            lv = t["descriptors2d_db"][0].contiguous()
            pmv = torch.empty(lib.onepose_leaves_prepared_bytes(1, n3, L) // 4, **f32)
            _lib.check(lib.onepose_prepare_leaves(lv.data_ptr(), 0, 1, n3, L, pmv.data_ptr(), s), "lv")
            for flags in (0, _lib.OBJ_GAT_TABLES):
                cache = torch.empty(lib.onepose_object_cache_bytes(n3, L, flags) // 4, **f32)
                wsb = lib.onepose_object_prepare_workspace_bytes(n3, L)
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                _lib.check(lib.onepose_object_prepare(w.data_ptr(), d3.data_ptr(), pmv.data_ptr(), n3,
                                                      L, pi, flags, cache.data_ptr(), ws.data_ptr(),
                                                      wsb, s), "prepare")
                d2 = t["descriptors2d_query"].contiguous()
                o = [torch.empty(B, n1, dtype=torch.int64, device=dev),
                     torch.empty(B, n3, dtype=torch.int64, device=dev),
                     torch.empty(B, n1, **f32), torch.empty(B, n3, **f32)]
                cf = torch.empty(B, n1, n3, **f32)
                wmb = lib.onepose_match_workspace_bytes(B, n1, n3, L, 1)
                wm = torch.empty(wmb, dtype=torch.uint8, device=dev)
                rc, kinds = _kinds(lib, lambda: lib.onepose_match_cached(
                    w.data_ptr(), d2.data_ptr(), 256 * n1, cache.data_ptr(), pmv.data_ptr(), 0, B,
                    n1, n3, L, float(m.hparams["scale_factor"]), float(m.hparams["match_threshold"]),
                    pi, flags, *[x.data_ptr() for x in o], cf.data_ptr(), wm.data_ptr(), wmb, s))
                _lib.check(rc, "match_cached")
                torch.cuda.synchronize()
                lib.onepose_object_release(cache.data_ptr())
                ck = f"c{flags}_{n1}_{n3}_{L}_{B}_{prec}"
                out[f"{ck}_kinds"] = kinds
                for nm, x in zip(("m0", "m1", "s0", "s1"), o):
                    out[f"{ck}_{nm}"] = x.cpu().numpy()
                out[f"{ck}_conf"] = _conf(cf)
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def cmp(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = 0
    for k in sorted(A.files):
        x, y = A[k], Bz[k]
        same = x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        if not same:
            bad += 1
            d = np.abs(x.astype(np.float64) - y.astype(np.float64)).max() if x.shape == y.shape else None
            print("DIFF", k, x.shape, y.shape, "max|d|", d)
    print(f"{len(A.files) - bad} of {len(A.files)} arrays bit-identical")
    return bad == 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(0 if cmp(sys.argv[2], sys.argv[3]) else 1)

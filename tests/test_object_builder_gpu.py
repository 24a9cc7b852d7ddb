"""The object builder's kernels (csrc/object_build.hip) on the GPU: every output bit-equal to the
numpy oracle (tests/object_builder_oracle.py) and, at the fixture size, to what the reference
itself produced (tests/golden/object_builder.npz).  Every buffer is followed by guard words that
must survive, and every case runs twice and must give equal bits.  The second half is the
adversarial pass: order-sensitive sums, clusters longer than a wave, every 1024-chunk edge,
hand-built neighbour lists, special values and the size limits (DESIGN.md 8i has the table)."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import object_builder_cases as C
import object_builder_oracle as O
from ba_cases import Guarded
from conftest import golden
from onepose_amd import _lib, data_utils, object_builder as ob
from onepose_amd.inference import OnePoseObject, seed_reference_stream

pytestmark = pytest.mark.gpu

I32, F32, F64, I64 = torch.int32, torch.float32, torch.float64, torch.int64
UNTOUCHED = np.frombuffer(b"\xa5" * 4, dtype=np.int32)[0]
BOX = os.path.join(C.MODEL_DIR, "box3d_corners.txt")
UNIT_BOX = np.array([[0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1],
                     [0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], dtype=np.float64)


def out_buf(dev, n, dtype):
    return Guarded(dev, nbytes=n * torch.empty(0, dtype=dtype).element_size(), dtype=dtype)


def twice(fn):
    """Run a case twice: equal bits, and the first run's result."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "not repeatable"
    return a


def same(a, ref):
    a, ref = np.asarray(a), np.asarray(ref)
    return a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes()


def stream(dev):
    return _lib.stream_ptr(dev)


# ------------------------------------------------------------------ filter
def run_filter(dev, xyz, tl, min_track, corners):
    lib = _lib.load()
    n = len(xyz)
    X = Guarded(dev, data=np.asarray(xyz, dtype=np.float64))
    T = None if tl is None else Guarded(dev, data=np.asarray(tl, dtype=np.int32))
    B = None if corners is None else Guarded(dev, data=np.asarray(corners, dtype=np.float64))
    out, idx, cnt = out_buf(dev, 3 * n, F32), out_buf(dev, n, I32), out_buf(dev, 1, I32)
    _lib.check(lib.onepose_filter_points(X.ptr, T.ptr if T else None, n, min_track,
                                         B.ptr if B else None, out.ptr, idx.ptr, cnt.ptr,
                                         stream(dev)), "filter_points")
    torch.cuda.synchronize()
    assert all(b.intact() for b in (X, T, B, out, idx, cnt) if b is not None)
    m = int(cnt.numpy()[0])
    i = idx.numpy()
    assert (i[m:] == UNTOUCHED).all()        # rows from count on are not written
    assert (out.numpy((n, 3))[m:].view(np.int32) == UNTOUCHED).all()
    return out.numpy((n, 3))[:m].copy(), i[:m].copy()


def filter_inputs(n, seed):
    rs = np.random.RandomState(seed)
    corners = C.box_corners()[0]
    lo, hi = corners.min(0), corners.max(0)
    xyz = rs.uniform(lo - 0.02, hi + 0.02, size=(n, 3))
    return xyz, rs.randint(1, 9, size=n), corners


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2500])
@pytest.mark.parametrize("box", [True, False])
def test_filter(device, n, box):
    xyz, tl, corners = filter_inputs(n, 40 + n)
    corners = corners if box else None
    for min_track in (4, 0, 100):          # some, all by track, none
        got = twice(lambda: run_filter(device, xyz, tl, min_track, corners))
        want = O.filter_points(xyz, tl, min_track, corners)
        assert same(got[0], want[0]) and same(got[1], want[1])
        if min_track == 100:
            assert len(got[1]) == 0
        if min_track == 0 and not box:
            assert np.array_equal(got[1], np.arange(n))
    got = twice(lambda: run_filter(device, xyz, None, 0, corners))   # no track filter at all
    assert same(got[1], O.filter_points(xyz, None, 0, corners)[1])
    if box and n >= 63:
        assert 0 < len(got[1]) < n


def test_filter_faces_nan_and_the_fixture(device):
    p = np.array([[0.5, 0.5, 0.5], [0.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.5, 0.0, 0.5],
                  [0.5, 0.5, 1.0], [np.nan, 0.5, 0.5], [0.25, 0.75, 0.125], [0.5, np.inf, 0.5]])
    x, i = twice(lambda: run_filter(device, p, None, 0, UNIT_BOX))
    assert i.tolist() == [0, 6] and same(x, p[[0, 6]].astype(np.float32))
    _, i = run_filter(device, p, None, 0, None)      # without a box NaN is no reason to drop
    assert i.tolist() == list(range(8))
    g = golden("object_builder")
    pts = ob.read_points3d_binary(os.path.join(C.MODEL_DIR, "points3D.bin"))
    x, i = twice(lambda: run_filter(device, pts["xyz"], pts["track_len"], int(g["tkl"]),
                                    np.loadtxt(BOX)))
    assert same(x, g["box_xyzs"]) and np.array_equal(pts["ids"][i], g["box_idxs"])
    # the reference's functions on the device
    xs, ids = ob.filter_by_track_length(pts, int(g["tkl"]), device=device)
    assert same(xs, g["tl_xyzs"]) and same(ids, g["tl_idxs"])
    xb, ib = ob.filter_by_3d_box(xs, ids, BOX, device=device)
    assert same(xb.numpy(), g["box_xyzs"]) and same(ib, g["box_idxs"])


# ------------------------------------------------------------------ neighbours and merge
def run_neighbours(dev, x, thr, capacity):
    lib = _lib.load()
    n = len(x)
    X = Guarded(dev, data=x)
    rs, cols, info = out_buf(dev, n + 1, I32), out_buf(dev, max(capacity, 1), I32), out_buf(dev, 2, I64)
    _lib.check(lib.onepose_radius_neighbours(X.ptr, 0 if x.dtype == np.float32 else 1, n, thr,
                                             rs.ptr, cols.ptr if capacity else None, capacity,
                                             info.ptr, stream(dev)), "radius_neighbours")
    torch.cuda.synchronize()
    assert X.intact() and rs.intact() and cols.intact() and info.intact()
    return rs.numpy().copy(), cols.numpy().copy(), info.numpy().copy()


def run_merge(dev, x, rs, cols):
    lib = _lib.load()
    n = len(x)
    X, R, Cc = Guarded(dev, data=x), Guarded(dev, data=rs.astype(np.int32)), Guarded(dev, data=cols)
    cof, ms, mem = out_buf(dev, n, I32), out_buf(dev, n + 1, I32), out_buf(dev, n, I32)
    mean, info = out_buf(dev, 3 * n, F64), out_buf(dev, 2, I32)
    _lib.check(lib.onepose_merge_greedy(X.ptr, 0 if x.dtype == np.float32 else 1, n, R.ptr, Cc.ptr,
                                        cof.ptr, ms.ptr, mem.ptr, mean.ptr, info.ptr, stream(dev)),
               "merge_greedy")
    torch.cuda.synchronize()
    assert all(b.intact() for b in (X, R, Cc, cof, ms, mem, mean, info))
    m, status = info.numpy()
    assert status == 0
    ms = ms.numpy()[:m + 1].copy()
    return cof.numpy().copy(), ms, mem.numpy()[:ms[-1]].copy(), mean.numpy((n, 3))[:m].copy()


@functools.lru_cache(maxsize=None)
def cloud(n, dtype):
    """n points with natural near pairs (a dense corner) and, from 64 on, planted duplicates,
    clusters and both chains; with its oracle results."""
    x = C.cloud_points(n, dtype)
    rs_o, cols_o = O.radius_neighbours(x, C.THR)
    return x, rs_o, cols_o, O.merge_greedy(x, rs_o, cols_o)


def check_neighbours_and_merge(dev, x, thr, want_rs, want_cols, want_merge):
    total = int(want_rs[-1])
    rs, cols, info = twice(lambda: run_neighbours(dev, x, thr, total))
    assert info.tolist() == [total, 0]
    assert np.array_equal(rs, want_rs) and same(cols[:total], want_cols)
    got = twice(lambda: run_merge(dev, x, rs, cols[:total]))
    for a, b in zip(got, want_merge):
        assert same(a, b)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 64, 65, 257, 4096])
def test_neighbours_and_merge_against_the_oracle(device, n, dtype):
    x, rs_o, cols_o, merge_o = cloud(n, dtype)
    cof, ms, mem, _ = check_neighbours_and_merge(device, x, C.THR, rs_o, cols_o, merge_o)
    if n >= 64:
        sizes = np.diff(ms)
        assert sizes.max() >= 4 and (cof == -1).sum() >= 1     # the quad; the chain's lost end
    if n >= 257:
        assert rs_o[-1] > n + 20                                # natural pairs, not only planted


@pytest.mark.parametrize("name", list(C.MERGE_CASES))
def test_merge_against_the_reference(device, name):
    """The stand-alone fixtures, threshold-edge pairs included, through the public merge()."""
    g = golden("object_builder")
    xyz, ids, thr, _ = C.merge_case(name)
    assert C.sha(xyz, ids) == str(g[f"merge_{name}_sha"])
    pts, ret = ob.merge(xyz, ids, thr, device=device)
    pts2, ret2 = ob.merge(xyz, ids, thr, device=device)
    lens, flat = C.flatten_clusters(ret)
    assert same(pts, g[f"merge_{name}_points"]) and same(pts, pts2)
    assert same(lens, g[f"merge_{name}_lens"]) and same(flat, g[f"merge_{name}_ids"])
    assert same(C.flatten_clusters(ret2)[1], flat)
    pairs = g[f"merge_{name}_edge_pairs"]
    if len(pairs):      # the raw neighbour lists decide the edge pairs as the reference did
        rs_o, cols_o = O.radius_neighbours(xyz, thr)
        rs, cols, _ = run_neighbours(device, xyz, thr, int(rs_o[-1]))
        assert np.array_equal(rs, rs_o) and same(cols[:rs_o[-1]], cols_o)
        for (p, q), below in zip(pairs, g[f"merge_{name}_edge_below"]):
            assert (q in cols[rs[p]:rs[p + 1]]) == bool(below)


def test_merge_in_the_flow(device):
    g = golden("object_builder")
    pts, ret = ob.merge(torch.from_numpy(g["box_xyzs"]), g["box_idxs"], C.THR, device=device)
    lens, flat = C.flatten_clusters(ret)
    assert same(pts, g["merge_points"]) and same(lens, g["merge_lens"]) and same(flat, g["merge_ids"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_all_points_identical(device, dtype):
    n = 300
    x = np.tile(np.array([[0.1, 0.2, 0.3]], dtype=dtype), (n, 1))
    want_rs = np.arange(n + 1, dtype=np.int64) * n
    want_cols = np.tile(np.arange(n, dtype=np.int32), n)
    merge_o = O.merge_greedy(x, want_rs, want_cols)
    assert len(merge_o[1]) == 2                      # one cluster
    check_neighbours_and_merge(device, x, C.THR, want_rs, want_cols, merge_o)
    # the public function sizes the list itself (its first guess is too small here)
    pts, ret = ob.merge(x, np.arange(n), C.THR, device=device)
    assert same(pts, merge_o[3]) and list(ret) == [0] and np.array_equal(ret[0], np.arange(n))


def test_capacity_too_small_reports_the_total(device):
    x, rs_o, cols_o, _ = cloud(257, np.float64)
    total = int(rs_o[-1])
    for cap in (total - 1, 1, 0):
        rs, cols, info = twice(lambda: run_neighbours(device, x, C.THR, cap))
        assert info.tolist() == [total, 1]
        assert (cols == UNTOUCHED).all()             # no list is written
    _, cols, info = run_neighbours(device, x, C.THR, total + 7)
    assert info.tolist() == [total, 0] and same(cols[:total], cols_o)
    assert (cols[total:] == UNTOUCHED).all()


def test_merge_refuses_a_broken_csr(device):
    lib = _lib.load()
    x = cloud(65, np.float64)[0]
    n = len(x)
    for rs, cols in ((np.arange(n + 1), np.full(n, n)),                # an entry outside [0, n)
                     (np.zeros(n + 1, np.int64), np.zeros(1, np.int32)),   # empty rows
                     (np.arange(n + 1) * 2, np.repeat(np.arange(n), 2))):   # too many members
        X, R = Guarded(device, data=x), Guarded(device, data=rs.astype(np.int32))
        Cc = Guarded(device, data=cols.astype(np.int32))
        cof, ms, mem = out_buf(device, n, I32), out_buf(device, n + 1, I32), out_buf(device, n, I32)
        mean, info = out_buf(device, 3 * n, F64), out_buf(device, 2, I32)
        _lib.check(lib.onepose_merge_greedy(X.ptr, 1, n, R.ptr, Cc.ptr, cof.ptr, ms.ptr, mem.ptr,
                                            mean.ptr, info.ptr, stream(device)), "merge_greedy")
        torch.cuda.synchronize()
        assert info.numpy().tolist() == [0, 1]
        assert all(b.intact() for b in (X, R, Cc, cof, ms, mem, mean, info))


# ------------------------------------------------------------------ lifting
@functools.lru_cache(maxsize=None)
def lift_case(dim):
    bank, off, ncols, blk, feat, seg = C.lift_inputs_old(dim)
    return bank, off, ncols, blk, feat, seg, O.lift(bank, off, ncols, blk, feat, seg, dim)


def run_lift(dev, bank, off, ncols, blk, feat, seg, dim):
    lib = _lib.load()
    S, n3 = len(blk), len(seg)
    ins = [Guarded(dev, data=a) for a in (bank, off, ncols, blk, feat, seg)]
    ss, col = out_buf(dev, n3 + 1, I32), out_buf(dev, dim * S, F64)
    m64, m32, info = out_buf(dev, dim * n3, F64), out_buf(dev, dim * n3, F32), out_buf(dev, 2, I32)
    _lib.check(lib.onepose_lift_descriptors(ins[0].ptr, len(bank), ins[1].ptr, ins[2].ptr, len(ncols),
                                            ins[3].ptr, ins[4].ptr, S, ins[5].ptr, n3, dim, ss.ptr,
                                            col.ptr, m64.ptr, m32.ptr, info.ptr, stream(dev)),
               "lift_descriptors")
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins + [ss, col, m64, m32, info])
    return (info.numpy().copy(), ss.numpy().copy(), col.numpy((dim, S)).copy(),
            m64.numpy((dim, n3)).copy(), m32.numpy((dim, n3)).copy())


@pytest.mark.parametrize("dim", [256, 128, 3])
def test_lifting_against_the_oracle(device, dim):
    bank, off, ncols, blk, feat, seg, want = lift_case(dim)
    assert 2 not in blk
    info, ss, col, m64, m32 = twice(lambda: run_lift(device, bank, off, ncols, blk, feat, seg, dim))
    assert info.tolist() == [0, 0]
    for a, b in zip((ss, col, m64, m32), want):
        assert same(a, b)


def test_lifting_against_the_reference(device):
    g = golden("object_builder")
    feats = C.features(g["feature_counts"].tolist())
    assert C.features_sha(feats) == str(g["features_sha"])
    imgs = ob.read_images_binary(os.path.join(C.MODEL_DIR, "images.bin"))
    cl, pos = {}, 0
    for c, n in enumerate(g["merge_lens"]):
        cl[c] = g["merge_ids"][pos:pos + n]
        pos += n
    oi, of, idxs = ob.collect_observations(imgs, C.IMG_LISTS, cl)
    desc = [feats[n]["descriptors"] for n in C.IMG_LISTS]
    col, m64, m32 = twice(lambda: [t.cpu().numpy() for t in
                                   ob.lift_descriptors(desc, oi, of, idxs, device=device)])
    want = g["anno_3d_collect_descriptors3d_f32"].astype(np.float64)
    assert C.sha(want) == str(g["anno_3d_collect_descriptors3d_sha"])
    assert same(col, want) and same(m64, g["anno_3d_average_descriptors3d"])
    assert same(m32, g["anno_3d_average_descriptors3d"].astype(np.float32))


def test_lifting_refuses_on_the_device(device):
    bank, off, ncols, blk, feat, seg, _ = lift_case(128)
    zero = seg.copy()
    zero[3], zero[4] = 0, seg[3] + seg[4]            # a zero-length segment, same total
    short = seg.copy()
    short[-1] -= 1
    wild = feat.copy()
    wild[77] = ncols[blk[77]]
    outside = off.copy()
    outside[4] += 1
    for args, status, where in (((bank, off, ncols, blk, feat, zero), 1, 3),
                                ((bank, off, ncols, blk, feat, short), 2, len(blk) - 1),
                                ((bank, outside, ncols, blk, feat, seg), 3, 4),
                                ((bank, off, ncols, blk, wild, seg), 4, 77)):
        info, ss, col, m64, m32 = twice(lambda: run_lift(device, *args, 128))
        assert info.tolist() == [status, where]
        for a in (col, m64, m32):                    # nothing is written
            assert (a.view(np.uint8) == 0xA5).all()


# ------------------------------------------------------------------ leaves
def test_leaves_equal_the_host_gather(device):
    g = golden("object_builder")
    col = g["anno_3d_collect_descriptors3d_f32"].astype(np.float64)
    idxs, scores = g["idxs"], g["anno_3d_collect_scores3d"]
    assert idxs.min() < 8 < idxs.max()               # points of fewer and of more than 8 observations
    n3, S = len(idxs), col.shape[1]
    np.random.seed(5)
    want = data_utils.build_features3d_leaves(col, scores, idxs, n3, 8)[0].numpy()
    np.random.seed(5)
    cols = data_utils.leaf_indices(idxs, 8, S)
    lib = _lib.load()

    def run(cols):
        Cd, K = Guarded(device, data=col), Guarded(device, data=cols)
        out = out_buf(device, C.DIM * len(cols), F32)
        _lib.check(lib.onepose_gather_leaves(Cd.ptr, S, C.DIM, K.ptr, len(cols), out.ptr,
                                             stream(device)), "gather_leaves")
        torch.cuda.synchronize()
        assert Cd.intact() and K.intact() and out.intact()
        return (out.numpy((C.DIM, len(cols))).copy(),)
    (got,) = twice(lambda: run(cols))
    assert same(got, want) and same(got, O.gather_leaves(col, cols))
    assert (cols == S).any() and (got[:, cols == S] == 1.0).all()
    (got,) = run(np.array([0, S, S + 1, -1, S - 1], dtype=np.int64))
    assert np.isnan(got[:, 2:4]).all() and (got[:, 1] == 1).all()
    assert same(got[:, [0, 4]], col[:, [0, S - 1]].astype(np.float32))


# ------------------------------------------------------------------ end to end
def test_build_annotations_writes_the_reference_files(device, tmp_path):
    g = golden("object_builder")
    feats = C.features(g["feature_counts"].tolist())
    out = str(tmp_path / "anno")
    ob.build_annotations(C.MODEL_DIR, feats, C.IMG_LISTS, BOX, out, max_num_kp3d=C.MAX_KP3D,
                         dist_threshold=C.THR, device=device)
    for f in ("anno_3d_average", "anno_3d_collect"):
        z = np.load(os.path.join(out, f + ".npz"))
        assert sorted(z.files) == ["descriptors3d", "keypoints3d", "scores3d"]
        for k in z.files:
            want = (g[f"{f}_{k}"] if f"{f}_{k}" in g.files
                    else g[f"{f}_{k}_f32"].astype(str(g[f"{f}_{k}_dtype"])))
            assert same(z[k], want), (f, k)
    assert same(np.load(os.path.join(out, "idxs.npy")), g["idxs"])

    seed_reference_stream()
    a = OnePoseObject.from_anno_dir(out, num_leaf=8, device=device)
    seed_reference_stream()
    b = OnePoseObject.from_sfm_model(C.MODEL_DIR, feats, C.IMG_LISTS, BOX, num_leaf=8,
                                     max_num_kp3d=C.MAX_KP3D, dist_threshold=C.THR, device=device)
    assert b.num_leaf == a.num_leaf == 8
    for name in ("keypoints3d", "descriptors3d", "leaves"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert tb.device.type == "cuda" and same(tb.cpu().numpy(), ta.cpu().numpy()), name


# ================================================================== the second pass
# Inputs from tests/object_builder_cases.py; the reference's bits for them from
# tests/golden/object_builder_edges.npz (make_golden_object_builder_edges.py);
# tests/test_object_builder_model_host.py shows which wrong kernel each input separates.
@functools.lru_cache(maxsize=None)
def wide_lift(n3, dim):
    args = C.lift_inputs(n3, dim)
    return args, O.lift(*args, dim)


@pytest.mark.parametrize("n3,dim", C.LIFT_GPU)
def test_lifting_on_a_wide_bank_past_the_first_chunk(device, n3, dim):
    """Sums whose float64 value depends on their order, segment starts carried over 1024-chunks
    of points, blocks and observations."""
    args, want = wide_lift(n3, dim)
    info, ss, col, m64, m32 = twice(lambda: run_lift(device, *args, dim))
    assert info.tolist() == [0, 0]
    for a, b in zip((ss, col, m64, m32), want):
        assert same(a, b)
    key = f"lift_{n3}_{dim}_ref_sha"
    assert (C.sha(m64) == str(golden("object_builder_edges")[key])) == (dim >= 2)


def test_lifting_refuses_past_the_first_chunk(device):
    dim = 3
    (bank, off, ncols, blk, feat, seg), _ = wide_lift(2500, dim)
    S = len(blk)
    assert S > 16000

    def changed(a, **at):
        a = a.copy()
        for k, v in at.items():
            a[int(k[1:])] = v
        return a
    cases = (
        ((off, blk, feat, changed(seg, _2047=0, _2048=seg[2047] + seg[2048])), [1, 2047]),
        ((off, blk, feat, changed(seg, _1500=0, _40=-3)), [1, 40]),
        ((off, blk, feat, changed(seg, _2499=seg[2499] - 1)), [2, S - 1]),
        ((off, blk, feat, changed(seg, _0=seg[0] + 1)), [2, S + 1]),
        ((changed(off, _1499=off[1499] + 1), blk, feat, seg), [3, 1499]),
        ((off, blk, changed(feat, _16000=ncols[blk[16000]], _1030=ncols[blk[1030]]), seg), [4, 1030]),
    )
    assert cases[0][0][3].sum() == S
    for (o, b, f, s), want in cases:
        info, ss, col, m64, m32 = twice(lambda: run_lift(device, bank, o, ncols, b, f, s, dim))
        assert info.tolist() == want
        for a in (col, m64, m32):                    # nothing is written
            assert (a.view(np.uint8) == 0xA5).all()


def test_lifting_through_the_public_function_at_scale(device):
    (bank, off, ncols, blk, feat, seg), want = wide_lift(2500, 256)
    desc = C.lift_blocks(bank, off, ncols, 256)
    got = twice(lambda: [t.cpu().numpy() for t in ob.lift_descriptors(desc, blk, feat, seg,
                                                                      device=device)])
    host = ob.lift_descriptors(desc, blk, feat, seg, device=None)
    for a, b, c in zip(got, host, want[1:]):
        assert same(a, b) and same(a, c)
    # dim 1: the device is sequential (the oracle); the host path follows the reference's
    # pairwise np.mean and differs on this bank (include/onepose_hip.h)
    (bank, off, ncols, blk, feat, seg), want = wide_lift(1025, 1)
    desc = C.lift_blocks(bank, off, ncols, 1)
    got = twice(lambda: [t.cpu().numpy() for t in ob.lift_descriptors(desc, blk, feat, seg,
                                                                      device=device)])
    for a, c in zip(got, want[1:]):
        assert same(a, c)
    assert not same(ob.lift_descriptors(desc, blk, feat, seg, device=None)[1], got[1])


@pytest.mark.parametrize("n", C.FILTER_N)
@pytest.mark.parametrize("box", [True, False])
def test_filter_at_the_chunk_edges(device, n, box):
    xyz, _, corners = filter_inputs(n, 40 + n)
    corners = corners if box else None
    for pattern in C.FILTER_PATTERNS:
        tl = C.filter_pattern(n, pattern)
        got = twice(lambda: run_filter(device, xyz, tl, 3, corners))
        want = O.filter_points(xyz, tl, 3, corners)
        assert same(got[0], want[0]) and same(got[1], want[1]), pattern
        if not box:
            assert np.array_equal(got[1], np.nonzero(tl >= 3)[0]), pattern
        if pattern == "none":
            assert len(got[1]) == 0
    if box:
        assert 0 < len(O.filter_points(xyz, None, 0, corners)[1]) < n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", C.CSR_CASES)
def test_merge_structure_on_hand_built_lists(device, name, dtype):
    x, rs, cols = C.csr_case(name, dtype)
    want = O.merge_greedy(x, rs, cols)
    got = twice(lambda: run_merge(device, x, rs, cols))     # run_merge: info == [m, 0]
    for a, b in zip(got, want):
        assert same(a, b)
    cof, ms, mem, mean = got
    if name == "all_alone":
        assert np.array_equal(cof, np.arange(C.CSR_N)) and np.array_equal(mem, np.arange(C.CSR_N))
    if name == "group_multi":
        assert len(ms) - 1 == 64 + 32 + 2 and (cof >= 0).all()
    if name == "seen_at_100":
        assert cof[1] == -1 and len(ms) - 1 == C.CSR_N - 1
    if name == "row_order":
        row = cols[:129].tolist()
        assert len(ms) - 1 == 2 and mem[:129].tolist() == row != sorted(row)
        if dtype == np.float32:      # the row's order, not ascending order
            assert not same(mean[0], C.mean_in_order(x, sorted(row)))
    if name == "asym_ab":
        assert cof[40] == cof[20] and len(ms) - 1 == C.CSR_N - 1
    if name == "asym_ba":
        assert cof[40] == -1 and cof[20] == 20
    if name == "not_self":
        assert cof[30] == -1 and cof[31] == 30 and cof[127] == -1


@pytest.mark.parametrize("name", list(C.LONG_MERGE_CASES))
def test_long_clusters_against_the_reference(device, name):
    g = golden("object_builder_edges")
    xyz, ids, thr, groups = C.long_merge_case(name)
    assert C.sha(xyz, ids) == str(g[f"merge_{name}_sha"])
    pts, ret = ob.merge(xyz, ids, thr, device=device)
    pts2, ret2 = ob.merge(xyz, ids, thr, device=device)
    lens, flat = C.flatten_clusters(ret)
    assert same(pts, g[f"merge_{name}_points"]) and same(pts, pts2)
    assert same(lens, g[f"merge_{name}_lens"]) and same(flat, g[f"merge_{name}_ids"])
    assert same(C.flatten_clusters(ret2)[1], flat)
    rs_o, cols_o = O.radius_neighbours(xyz, thr)
    cof, ms, mem, _ = check_neighbours_and_merge(device, xyz, thr, rs_o, cols_o,
                                                 O.merge_greedy(xyz, rs_o, cols_o))
    assert sorted(np.diff(ms))[-7:] == [63, 64, 65, 65, 128, 129, 200]
    assert cof[groups["skip"][0][65]] == -1


@pytest.mark.parametrize("name", list(C.threshold_cases()))
def test_neighbours_across_the_bound_limits(device, name):
    x, thr = C.threshold_cases()[name]
    rs_o, cols_o = O.radius_neighbours(x, thr)
    total = int(rs_o[-1])
    assert total >= len(x) + 30                      # the planted groups survive the scaling
    rs, cols, info = twice(lambda: run_neighbours(device, x, thr, total))
    assert info.tolist() == [total, 0]
    assert np.array_equal(rs, rs_o) and same(cols[:total], cols_o)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_neighbours_of_special_values(device, dtype):
    cases = [C.special_cloud(dtype)]
    if dtype == np.float64:
        cases += [C.underflow_case(), (C.sq_separator(), C.THR32)]
    for x, thr in cases:
        rs_o, cols_o = O.radius_neighbours(x, thr)
        total = int(rs_o[-1])
        rs, cols, info = twice(lambda: run_neighbours(device, x, thr, total))
        assert info.tolist() == [total, 0]
        assert np.array_equal(rs, rs_o) and same(cols[:total], cols_o)


def test_pair_count_refusal(device):
    t0 = time.perf_counter()
    for n, status in ((46340, 1), (46341, 2)):
        x = np.tile(np.array([[0.1, 0.2, 0.3]], dtype=np.float32), (n, 1))
        rs, cols, info = twice(lambda: run_neighbours(device, x, C.THR, 0))
        assert info.tolist() == [n * n, status]
        assert np.array_equal(rs, np.minimum(np.arange(n + 1, dtype=np.int64) * n, 2**31 - 1))
        assert (cols == UNTOUCHED).all()
    assert n * n > 2**31 - 1
    rs, cols, info = twice(lambda: run_neighbours(device, x, C.THR, 1024))
    assert info.tolist() == [n * n, 2]
    assert len(cols) == 1024 and (cols == UNTOUCHED).all()       # nothing is written through the list
    with pytest.raises(_lib.OnePoseError, match=str(n * n)):
        ob.radius_neighbours_device(torch.from_numpy(x).to(device), C.THR)
    print(f"pair-count refusal: {time.perf_counter() - t0:.2f} s")


def test_the_largest_cloud(device):
    """n = 65536: the last word of the recorded bitmap, against a pruned host search that
    tests/test_object_builder_model_host.py holds to the oracle."""
    t0 = time.perf_counter()
    x, pairs, triple = C.big_cloud()
    rs_o, cols_o = C.pruned_neighbours(x, C.THR)
    merge_o = O.merge_greedy(x, rs_o, cols_o)
    t1 = time.perf_counter()
    cof, ms, mem, _ = check_neighbours_and_merge(device, x, C.THR, rs_o, cols_o, merge_o)
    t2 = time.perf_counter()
    c = cof[65535]
    assert c >= 0 and mem[ms[c]:ms[c + 1]].tolist() == list(triple)
    assert cof[0] == cof[40000] == 0
    assert rs_o[-1] >= len(x) + 2 * len(pairs) + 6
    print(f"n = 65536: host {t1 - t0:.2f} s, device calls and comparison {t2 - t1:.2f} s")


def test_chain_at_scale_equals_the_host_path(device):
    pts, imgs, corners, desc = C.chain_model()

    def chain(dev):
        x, ids = ob.filter_3d(pts, C.CHAIN_TKL, corners, device=dev)
        mp, mi = ob.merge(x, ids, C.THR, device=dev)
        oi, of, idxs = ob.collect_observations(imgs, C.CHAIN_IMAGES, mi)
        lifted = ob.lift_descriptors(desc, oi, of, idxs, device=dev)
        lens, flat = C.flatten_clusters(mi)
        return [x.numpy(), ids, mp, lens, flat, oi, of, idxs] + [
            t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in lifted]
    got = twice(lambda: chain(device))
    want = chain(None)
    assert len(got) == len(want) == 11
    for a, b in zip(got, want):
        assert same(a, b)
    n3 = len(got[7])
    assert 1024 < n3 < len(got[1]) < len(pts["ids"]) and got[3].max() >= 2

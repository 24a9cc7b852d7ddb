"""onepose_lk_build_pyramid and onepose_lk_track on the GPU against the numpy oracle
(tests/lk_oracle.py), computed live on the scenes of tests/lk_cases.py: pyramids, derivatives,
next_pts and status must be equal bit for bit (the contract in include/onepose_hip.h is integer
arithmetic plus single fp32 operations, which numpy and the kernel round alike).  Every device
buffer carries guard words."""
import numpy as np
import pytest
import torch

import lk_cases
import lk_oracle
from ba_cases import Guarded
from onepose_amd import _lib, tracker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Pyr:
    """A guarded batch of pyramid blobs built from numpy images [B, h, w]."""

    def __init__(self, lib, device, imgs, win, max_level, with_deriv=True, stream=None):
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        self.B, self.h, self.w = imgs.shape
        self.win, self.max_level = win, max_level
        self.nbytes = lib.onepose_lk_pyramid_bytes(self.h, self.w, win, max_level)
        self.levels = lib.onepose_lk_levels(self.h, self.w, win, max_level)
        assert self.nbytes > 0 and self.levels > 0
        self.src = Guarded(device, data=imgs)
        self.blob = Guarded(device, nbytes=self.B * self.nbytes, dtype=torch.uint8)
        rc = lib.onepose_lk_build_pyramid(self.src.ptr, self.h * self.w, self.B, self.h, self.w,
                                          win, max_level, int(with_deriv), self.blob.ptr,
                                          stream if stream is not None else _lib.stream_ptr(device))
        _lib.check(rc, "onepose_lk_build_pyramid")

    def level(self, b, l):
        """numpy (image, derivative) of level l of item b, cut out with the layout query."""
        lh, lw, io, do = tracker.lk_pyramid_layout(self.h, self.w, self.win, self.max_level, l)
        raw = self.blob.numpy().reshape(self.B, self.nbytes)[b]
        img = raw[io:io + lh * lw].reshape(lh, lw)
        der = raw[do:do + 4 * lh * lw].view(np.int16).reshape(lh, lw, 2)
        return img, der

    def intact(self):
        return self.src.intact() and self.blob.intact()


def run_track(lib, device, prev, nxt, pts, counts, max_points, max_count=10,
              epsilon=lk_cases.EPSILON, min_eig=lk_cases.MIN_EIG, shared=False, stream=None,
              expect=0):
    """pts numpy [max_points, 2] (shared) or [B, max_points, 2] -> (next_pts, status) numpy, the
    outputs pre-filled with 0xA5 bytes so that untouched rows show."""
    B = nxt.B
    gp = Guarded(device, data=np.ascontiguousarray(pts, dtype=np.float32))
    gc = Guarded(device, data=np.asarray(counts, dtype=np.int32))
    out = Guarded(device, nbytes=max(B * max_points * 8, 8), dtype=torch.float32)
    st = Guarded(device, nbytes=max(B * max_points, 1), dtype=torch.uint8)
    out.raw.fill_(0xA5)
    st.raw.fill_(0xA5)
    rc = lib.onepose_lk_track(prev.blob.ptr, 0 if (shared or prev.B == 1) else prev.nbytes,
                              nxt.blob.ptr, gp.ptr, 0 if np.ndim(pts) == 2 else 2 * max_points,
                              gc.ptr, B, max_points, nxt.h, nxt.w, nxt.win, nxt.max_level,
                              max_count, epsilon, min_eig, out.ptr, st.ptr,
                              stream if stream is not None else _lib.stream_ptr(device))
    assert (rc == 0) == (expect == 0), _lib.load().onepose_last_error()
    torch.cuda.synchronize(device)
    for g in (gp, gc, out, st):
        assert g.intact(), "guard words overwritten"
    assert prev.intact() and nxt.intact(), "guard words overwritten"
    return (out.numpy()[:B * max_points * 2].reshape(B, max_points, 2),
            st.numpy()[:B * max_points].reshape(B, max_points))


UNTOUCHED_F = np.frombuffer(b"\xa5" * 4, dtype=np.uint32)[0]


@pytest.mark.parametrize("name", list(lk_cases.CASES)[:6])   # the last two repeat the first's images
def test_pyramids_and_derivatives_equal_the_oracle(name, lib, device):
    s = lk_cases.scene(name)
    _, _, _, p, q = lk_cases.oracle(name)
    third = np.ascontiguousarray(s["prev"][::-1, ::-1])
    r = lk_oracle.build_pyramid(third, s["win"], s["max_level"])
    one = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    three = Pyr(lib, device, np.stack([s["prev"], s["next"], third]), s["win"], s["max_level"])
    bare = Pyr(lib, device, np.stack([s["next"], third]), s["win"], s["max_level"], False)
    torch.cuda.synchronize(device)
    assert one.levels == three.levels == len(p)
    for l in range(len(p)):
        for got, want in ((one.level(0, l), p[l]), (three.level(0, l), p[l]),
                          (three.level(1, l), q[l]), (three.level(2, l), r[l])):
            assert np.array_equal(got[0], want[0]), (name, l, "image")
            assert np.array_equal(got[1], want[1]), (name, l, "derivative")
        for b, want in ((0, q[l]), (1, r[l])):
            img, der = bare.level(b, l)
            assert np.array_equal(img, want[0]), (name, l, "image without derivatives")
            assert (der.view(np.uint8) == 0xA5).all(), "derivative written with with_deriv = 0"
    assert one.intact() and three.intact() and bare.intact()


@pytest.mark.parametrize("name", list(lk_cases.CASES))
def test_track_equals_the_oracle_bit_for_bit(name, lib, device):
    s = lk_cases.scene(name)
    want, wst, why, _, _ = lk_cases.oracle(name)
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    for n in lk_cases.COUNTS:
        out, st = run_track(lib, device, prev, nxt, s["pts"][:max(n, 1)], [n], n,
                            max_count=s["max_count"])
        bad = np.where((bits(out[0]) != bits(want[:n])).any(1) | (st[0] != wst[:n]))[0]
        assert bad.size == 0, (name, n, bad[:5], out[0][bad[:5]], want[bad[:5]], why[bad[:5]])
    # n = 0 through counts with room for points: nothing is written
    out, st = run_track(lib, device, prev, nxt, s["pts"][:8], [0], 8, max_count=s["max_count"])
    assert (out.view(np.uint32) == UNTOUCHED_F).all() and (st == 0xA5).all()


def test_batch_counts_and_shared_keyframe(lib, device):
    s = lk_cases.scene("base")
    want, wst, _, _, _ = lk_cases.oracle("base")
    nexts = np.stack([s["next"], s["prev"], np.roll(s["next"], 1, axis=1)])
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, nexts, s["win"], s["max_level"], False)
    counts = (300, 0, 17)
    out, st = run_track(lib, device, prev, nxt, s["pts"], counts, 300, shared=True)
    assert np.array_equal(bits(out[0]), bits(want)) and np.array_equal(st[0], wst)
    for b, c in enumerate(counts):
        single = Pyr(lib, device, nexts[b][None], s["win"], s["max_level"], False)
        o1, s1 = run_track(lib, device, prev, single, s["pts"], [300], 300)
        assert np.array_equal(bits(out[b, :c]), bits(o1[0, :c])) and np.array_equal(st[b, :c], s1[0, :c])
        assert (out[b, c:].view(np.uint32) == UNTOUCHED_F).all() and (st[b, c:] == 0xA5).all()
    # the same with per-item keyframes and points (non-zero strides): item b tracks its own pair
    prev3 = Pyr(lib, device, np.stack([s["prev"]] * 3), s["win"], s["max_level"])
    pts3 = np.stack([s["pts"], s["pts"][::-1], s["pts"]])
    o3, s3 = run_track(lib, device, prev3, nxt, pts3, (300, 300, 300), 300)
    assert np.array_equal(bits(o3[0]), bits(want)) and np.array_equal(s3[0], wst)
    o1, s1 = run_track(lib, device, prev, Pyr(lib, device, nexts[1][None], s["win"],
                                              s["max_level"], False), s["pts"][::-1], [300], 300)
    assert np.array_equal(bits(o3[1]), bits(o1[0])) and np.array_equal(s3[1], s1[0])
    # an over-long or negative count is clamped on the device
    oc, sc = run_track(lib, device, prev, nxt, s["pts"], (1000, -5, 2 ** 31 - 1), 300, shared=True)
    assert np.array_equal(bits(oc[0]), bits(want)) and (sc[1] == 0xA5).all()
    assert np.array_equal(sc[0], wst) and not (sc[2] == 0xA5).any()


def test_hostile_points_are_refused_before_any_address(lib, device):
    s = lk_cases.scene("base")
    want, wst, _, p, q = lk_cases.oracle("base")
    pts = s["pts"].copy()
    hostile = {5: (np.nan, 10.0), 6: (10.0, np.nan), 64: (np.inf, 3.0), 65: (7.0, -np.inf),
               100: (1e30, 5.0), 101: (5.0, -1e30), 130: (3e9, 3e9), 131: (-3e9, 40.0),
               200: (np.nan, np.inf)}
    for i, v in hostile.items():
        pts[i] = v
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    out, st = run_track(lib, device, prev, nxt, pts, [300], 300)
    o_out, o_st, o_why = lk_oracle.track(p, q, pts, s["win"])
    for i in hostile:
        assert st[0, i] == 0 and np.array_equal(bits(out[0, i]), bits(pts[i])), i
        assert o_why[i] == lk_oracle.R_HOSTILE
    rest = np.setdiff1d(np.arange(300), list(hostile))
    assert np.array_equal(bits(out[0, rest]), bits(want[rest]))
    assert np.array_equal(st[0, rest], wst[rest])
    assert np.array_equal(bits(out[0]), bits(o_out)) and np.array_equal(st[0], o_st)


@pytest.mark.parametrize("name", ["base", "level0"])
def test_points_exactly_at_the_bounds(name, lib, device):
    """floor(p - half) equal to -win - 1, -win, cols - 1 and cols on each axis: the first and the
    last are out before the loop, the two between are inside the rule."""
    s = lk_cases.scene(name)
    _, _, _, p, q = lk_cases.oracle(name)
    win, (h, w) = s["win"], s["prev"].shape
    half = (win - 1) / 2
    pts = []
    for v in (-win - 1, -win, w - 1, w):
        pts += [(v + half + 0.25, 40.0), (v + half, 41.5)]
    for v in (-win - 1, -win, h - 1, h):
        pts += [(50.0, v + half + 0.25), (51.5, v + half)]
    pts = np.array(pts, np.float32)
    o_out, o_st, o_why = lk_oracle.track(p, q, pts, win)
    pre = o_why == lk_oracle.R_OOB_PRE
    assert pre.tolist() == [True, True, False, False, False, False, True, True] * 2
    prev = Pyr(lib, device, s["prev"][None], win, s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], win, s["max_level"], False)
    out, st = run_track(lib, device, prev, nxt, pts, [len(pts)], len(pts))
    assert np.array_equal(bits(out[0]), bits(o_out)) and np.array_equal(st[0], o_st)
    assert not st[0][pre].any()


def test_min_eig_threshold_exactly_at_a_points_eigenvalue(lib, device):
    """min_eig_threshold set to a point's own level-0 minEig (kept: the test is <) and to the next
    float above it (rejected).  A minEig one ulp off the oracle's, from a square root or a
    division that is not correctly rounded, flips one of the two."""
    s = lk_cases.scene("level0")
    _, _, _, p, q = lk_cases.oracle("level0")
    eig = {}
    lk_oracle.track(p, q, s["pts"], s["win"], eig_out=eig)
    chosen = [i for i in sorted(eig) if eig[i] > 0][::3]
    assert len(chosen) >= 90
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    for i in chosen:
        one = s["pts"][i:i + 1]
        at = eig[i]
        above = np.nextafter(at, np.float32(np.inf))
        for thr, rejected in ((at, False), (above, True)):
            want, wst, why = lk_oracle.track(p, q, one, s["win"], min_eig=thr)
            assert (why[0] == lk_oracle.R_EIG) == rejected
            out, st = run_track(lib, device, prev, nxt, one, [1], 1, min_eig=float(thr))
            assert st[0, 0] == wst[0] and np.array_equal(bits(out[0]), bits(want)), (i, thr)


@pytest.mark.parametrize("h,w", [(1024, 1024), (1024, 1025)])
def test_large_image_pyramid_on_both_sides_of_the_per_level_launches(h, w, lib, device):
    """Up to 1024 x 1024 pixels the levels >= 1 come from one workgroup per image, above from one
    grid launch per level: the same pyramid either way, with and without derivatives."""
    f = lk_cases.cosine_field(h, w, 31)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.rint(f(x, y)).astype(np.uint8)
    want = lk_oracle.build_pyramid(img, 15, 3)
    full = Pyr(lib, device, np.stack([img, img[::-1]]), 15, 3)
    bare = Pyr(lib, device, img[None], 15, 3, False)
    torch.cuda.synchronize(device)
    assert full.levels == len(want) == 4
    flipped = lk_oracle.build_pyramid(np.ascontiguousarray(img[::-1]), 15, 3)
    for l in range(4):
        for b, ref in ((0, want), (1, flipped)):
            got = full.level(b, l)
            assert np.array_equal(got[0], ref[l][0]) and np.array_equal(got[1], ref[l][1]), (b, l)
        img_l, der_l = bare.level(0, l)
        assert np.array_equal(img_l, want[l][0]) and (der_l.view(np.uint8) == 0xA5).all(), l
    assert full.intact() and bare.intact()


def test_repeat_stream_and_graph_are_bit_identical(lib, device):
    s = lk_cases.scene("far")
    want, wst, _, _, _ = lk_cases.oracle("far")
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    first = run_track(lib, device, prev, nxt, s["pts"], [300], 300)
    again = run_track(lib, device, prev, nxt, s["pts"], [300], 300)
    assert np.array_equal(bits(first[0][0]), bits(want)) and np.array_equal(first[1][0], wst)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(first[1], again[1])
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        prev_s = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"],
                     stream=side.cuda_stream)
        nxt_s = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False,
                    stream=side.cuda_stream)
        other = run_track(lib, device, prev_s, nxt_s, s["pts"], [300], 300,
                          stream=side.cuda_stream)
    assert np.array_equal(prev_s.blob.numpy(), prev.blob.numpy())
    assert np.array_equal(bits(first[0]), bits(other[0])) and np.array_equal(first[1], other[1])
    # the Python layer, captured: pyramid of the next image and the track call, replayed twice
    img_a = torch.from_numpy(s["prev"]).to(device)
    img_b = torch.from_numpy(s["next"]).to(device)
    pts = torch.from_numpy(s["pts"]).to(device)
    kf = tracker.build_lk_pyramid(img_a, s["win"], s["max_level"])
    counts = torch.full((1,), 300, dtype=torch.int32, device=device)
    eager = tracker.lk_track(kf, tracker.build_lk_pyramid(img_b, s["win"], s["max_level"], False),
                             pts, counts)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = tracker.lk_track(kf, tracker.build_lk_pyramid(img_b, s["win"], s["max_level"],
                                                            False), pts, counts)
    for _ in range(2):
        cap[0].zero_()
        cap[1].fill_(7)
        graph.replay()
        torch.cuda.synchronize(device)
        for got in (eager, cap):
            assert np.array_equal(bits(got[0][0].cpu().numpy()), bits(want))
            assert np.array_equal(got[1][0].cpu().numpy(), wst)


def assert_pyramid_equals(pyr, b, want, what):
    for l, (img, der) in enumerate(want):
        got = pyr.level(b, l)
        assert np.array_equal(got[0], img), (what, l, "image")
        assert np.array_equal(got[1], der), (what, l, "derivative")


@pytest.mark.parametrize("name", list(lk_cases.EDGE_CASES))
def test_edge_scene_equals_the_oracle_bit_for_bit(name, lib, device):
    """tests/lk_cases.py EDGE_CASES: windows 3, 5 (lk_track_kernel<1>), 9 (<4>), 17 (<8>), 23 and
    31 (<16>) on block noise and on the cosine field, 75 x 97 at window 23, window sums beyond
    2^31 (noise_w23, noise_w31, cosine_w23, cosine_w31, stripes_w31, quilt_w15), two warps, the
    tight criteria.  Pyramids and derivatives of both frames, next_pts and status."""
    s = lk_cases.scene(name)
    want, wst, why, p, q = lk_cases.oracle(name)
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"])
    torch.cuda.synchronize(device)
    assert prev.levels == nxt.levels == len(p)
    assert_pyramid_equals(prev, 0, p, name)
    assert_pyramid_equals(nxt, 0, q, name)
    n = len(s["pts"])
    out, st = run_track(lib, device, prev, nxt, s["pts"], [n], n, max_count=s["max_count"],
                        epsilon=s["epsilon"])
    bad = np.where((bits(out[0]) != bits(want)).any(1) | (st[0] != wst))[0]
    assert bad.size == 0, (name, bad[:5], out[0][bad[:5]], want[bad[:5]], why[bad[:5]])


@pytest.mark.parametrize("name", ["noise_w31", "cosine_w3"])
@pytest.mark.parametrize("max_points", [1, 3, 5])
def test_small_buffers_and_clamped_counts(name, max_points, lib, device):
    """Buffers of 1, 3 and 5 points: a grid of one partly filled workgroup (3), one full plus
    one wave (5).  counts equal to max_points, above it, one below it, zero and negative: the
    rows up to the clamped count equal the oracle's, the rows past it keep their 0xA5 bytes."""
    s = lk_cases.scene(name)
    want, wst, _, _, _ = lk_cases.oracle(name)
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    pts = s["pts"][20:20 + max_points]      # past the hand-placed points: most of these track
    for count in (max_points, max_points + 1, 1000, 2 ** 31 - 1, max_points - 1, 0, -1, -2 ** 31):
        out, st = run_track(lib, device, prev, nxt, pts, [count], max_points)
        c = min(max(count, 0), max_points)
        assert np.array_equal(bits(out[0, :c]), bits(want[20:20 + c])), (name, count)
        assert np.array_equal(st[0, :c], wst[20:20 + c]), (name, count)
        assert (out[0, c:].view(np.uint32) == UNTOUCHED_F).all() and (st[0, c:] == 0xA5).all()


def test_batch_of_a_saturated_and_a_smooth_frame_shares_no_state(lib, device):
    """Window 31, one keyframe pyramid (block noise) for two next frames in one call: its own
    rolled copy (window sums up to 4.8e9) and a cosine field.  Each item equals the oracle's
    result for its pair, in either order of the two, and with per-item counts."""
    a, b = lk_cases.scene("noise_w31"), lk_cases.scene("cosine_w31")
    win, ml, pts = a["win"], a["max_level"], a["pts"]
    want_a, st_a, _, p, _ = lk_cases.oracle("noise_w31")
    q = lk_oracle.build_pyramid(b["next"], win, ml, with_deriv=False)
    want_b, st_b, _ = lk_oracle.track(p, q, pts, win)
    assert st_b.any() and not st_b.all()
    prev = Pyr(lib, device, a["prev"][None], win, ml)
    n = len(pts)
    for order in ((0, 1), (1, 0)):
        frames = np.stack([(a["next"], b["next"])[i] for i in order])
        nxt = Pyr(lib, device, frames, win, ml, False)
        for counts in ((n, n), (n, 7), (5, n)):
            out, st = run_track(lib, device, prev, nxt, pts, counts, n, shared=True)
            for item, i in enumerate(order):
                w, ws = ((want_a, st_a), (want_b, st_b))[i]
                c = counts[item]
                assert np.array_equal(bits(out[item, :c]), bits(w[:c])), (order, counts, item)
                assert np.array_equal(st[item, :c], ws[:c]), (order, counts, item)
                assert (out[item, c:].view(np.uint32) == UNTOUCHED_F).all()
                assert (st[item, c:] == 0xA5).all()


@pytest.mark.parametrize("name", lk_cases.WARPS)
def test_warp_scene_is_within_the_model_bar(name, lib, device):
    """The one comparison that does not pass through the oracle: the GPU against the float64
    model (tests/lk_model.py) on the rotated and scaled scenes, on the grid points of the host
    test.  Status equal on every point; where the model ends level 0 by its epsilon rule (all
    154 points on both warps) the positions agree within the host test's bar, 0.03 px, which
    was set from the oracle against the model on the CPU (lk_cases.MODEL_BAR; measured there
    0.0064 and 0.0068 px on these two scenes)."""
    import lk_model
    s = lk_cases.scene(name)
    _, m, pts = lk_cases.model_pair(name)
    pts = pts.copy()      # the shared one is read-only, which torch.from_numpy warns about
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    out, st = run_track(lib, device, prev, nxt, pts, [len(pts)], len(pts))
    by_eps = m[2] == lk_model.EPS
    d = np.abs(out[0].astype(np.float64) - m[0]).max(1)
    print(f"{name}: {int(by_eps.sum())} of {len(pts)} compared, max |GPU - model| "
          f"{d[by_eps].max():.5f} px")
    assert np.array_equal(st[0], m[1])
    assert by_eps.mean() >= lk_cases.COMPARED_SHARE
    assert d[by_eps].max() <= lk_cases.MODEL_BAR


def test_saturated_repeat_stream_and_graph_are_bit_identical(lib, device):
    """test_repeat_stream_and_graph_are_bit_identical on block noise at window 31 (the
    16-pixels-per-lane kernel, window sums beyond 2^31)."""
    s = lk_cases.scene("noise_w31")
    want, wst, _, _, _ = lk_cases.oracle("noise_w31")
    win, ml, n = s["win"], s["max_level"], len(s["pts"])
    prev = Pyr(lib, device, s["prev"][None], win, ml)
    nxt = Pyr(lib, device, s["next"][None], win, ml, False)
    first = run_track(lib, device, prev, nxt, s["pts"], [n], n)
    again = run_track(lib, device, prev, nxt, s["pts"], [n], n)
    assert np.array_equal(bits(first[0][0]), bits(want)) and np.array_equal(first[1][0], wst)
    assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(first[1], again[1])
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        prev_s = Pyr(lib, device, s["prev"][None], win, ml, stream=side.cuda_stream)
        nxt_s = Pyr(lib, device, s["next"][None], win, ml, False, stream=side.cuda_stream)
        other = run_track(lib, device, prev_s, nxt_s, s["pts"], [n], n, stream=side.cuda_stream)
    assert np.array_equal(prev_s.blob.numpy(), prev.blob.numpy())
    assert np.array_equal(bits(first[0]), bits(other[0])) and np.array_equal(first[1], other[1])
    img_a = torch.from_numpy(s["prev"]).to(device)
    img_b = torch.from_numpy(s["next"]).to(device)
    pts = torch.from_numpy(s["pts"]).to(device)
    kf = tracker.build_lk_pyramid(img_a, win, ml)
    counts = torch.full((1,), n, dtype=torch.int32, device=device)
    eager = tracker.lk_track(kf, tracker.build_lk_pyramid(img_b, win, ml, False), pts, counts)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = tracker.lk_track(kf, tracker.build_lk_pyramid(img_b, win, ml, False), pts, counts)
    for _ in range(2):
        cap[0].zero_()
        cap[1].fill_(7)
        graph.replay()
        torch.cuda.synchronize(device)
        for got in (eager, cap):
            assert np.array_equal(bits(got[0][0].cpu().numpy()), bits(want))
            assert np.array_equal(got[1][0].cpu().numpy(), wst)


def test_rejected_arguments_write_nothing(lib, device):
    s = lk_cases.scene("one_level")
    prev = Pyr(lib, device, s["prev"][None], s["win"], s["max_level"])
    nxt = Pyr(lib, device, s["next"][None], s["win"], s["max_level"], False)
    h, w = s["prev"].shape
    for kw in (dict(win=14), dict(win=33), dict(win=1), dict(max_level=6), dict(max_level=-1),
               dict(h=15), dict(w=15), dict(h=8193), dict(batch=0), dict(n=-1),
               dict(eps=float("nan")), dict(eig=float("nan")), dict(pbs=1), dict(ptbs=1),
               dict(counts=None), dict(pts=None)):
        gp = Guarded(device, data=s["pts"])
        gc = Guarded(device, data=np.array([300], np.int32))
        out = Guarded(device, nbytes=300 * 8, dtype=torch.float32)
        st = Guarded(device, nbytes=300, dtype=torch.uint8)
        out.raw.fill_(0xA5)
        st.raw.fill_(0xA5)
        a = dict(prev=prev.blob.ptr, pbs=0, next=nxt.blob.ptr, pts=gp.ptr, ptbs=0, counts=gc.ptr,
                 batch=1, n=300, h=h, w=w, win=s["win"], max_level=s["max_level"], count=10,
                 eps=0.03, eig=1e-4, out=out.ptr, status=st.ptr, stream=_lib.stream_ptr(device))
        a.update(kw)
        assert lib.onepose_lk_track(*a.values()) == 1, kw
        assert lib.onepose_last_error()
        torch.cuda.synchronize(device)
        assert (out.raw == 0xA5).all() and (st.raw == 0xA5).all(), kw
    blob = Guarded(device, nbytes=prev.nbytes, dtype=torch.uint8)
    for kw in (dict(win=14), dict(max_level=6), dict(h=15), dict(batch=0), dict(deriv=3),
               dict(image=None)):
        a = dict(image=prev.src.ptr, bs=h * w, batch=1, h=h, w=w, win=s["win"],
                 max_level=s["max_level"], deriv=1, out=blob.ptr, stream=_lib.stream_ptr(device))
        a.update(kw)
        assert lib.onepose_lk_build_pyramid(*a.values()) == 1, kw
        torch.cuda.synchronize(device)
        assert (blob.raw == 0xA5).all(), kw
    # the clamps are not refusals: max_count 1000 runs as 100, -3 as 0; epsilon 50 as 10
    _, _, _, p, q = lk_cases.oracle("one_level")
    for count, eps in ((1000, 0.0), (-3, 0.03), (10, 50.0), (10, -1.0)):
        o_out, o_st, _ = lk_oracle.track(p, q, s["pts"], s["win"], count, eps)
        out, st = run_track(lib, device, prev, nxt, s["pts"], [300], 300, max_count=count,
                            epsilon=eps)
        assert np.array_equal(bits(out[0]), bits(o_out)) and np.array_equal(st[0], o_st)


def test_python_layer_has_cv2_shapes(device):
    s = lk_cases.scene("base")
    want, wst, _, _, _ = lk_cases.oracle("base")
    nxt, status, err = tracker.calc_optical_flow_pyr_lk(s["prev"], s["next"], s["pts"][:, None, :])
    assert err is None and isinstance(nxt, np.ndarray)
    assert nxt.shape == (300, 1, 2) and nxt.dtype == np.float32
    assert status.shape == (300, 1) and status.dtype == np.uint8
    assert np.array_equal(bits(nxt[:, 0]), bits(want)) and np.array_equal(status[:, 0], wst)
    # GPU tensors in, GPU tensors out
    t = [torch.from_numpy(x).to(device) for x in (s["prev"], s["next"], s["pts"])]
    gn, gs, _ = tracker.calc_optical_flow_pyr_lk(*t)
    assert gn.is_cuda and gn.shape == (300, 1, 2) and gs.shape == (300, 1)
    assert np.array_equal(bits(gn.cpu().numpy()), bits(nxt))
    # criteria bits: without COUNT the count is 30, without EPS the epsilon 0.001
    _, _, _, p, q = lk_cases.oracle("base")
    for crit, (count, eps) in (((2, 4, 0.05), (30, 0.05)), ((1, 4, 0.05), (4, 0.001))):
        o_out, o_st, _ = lk_oracle.track(p, q, s["pts"], 15, count, eps)
        n2, s2, _ = tracker.calc_optical_flow_pyr_lk(s["prev"], s["next"], s["pts"], criteria=crit)
        assert np.array_equal(bits(n2[:, 0]), bits(o_out)) and np.array_equal(s2[:, 0], o_st)
    kpt_new, valid_id = tracker.kpt_flow_track(s["prev"], s["next"], s["pts"])
    assert isinstance(valid_id, tuple) and len(valid_id) == 1
    assert kpt_new.shape == (300, 2) and kpt_new.dtype == np.float32
    assert np.array_equal(valid_id[0], np.where(wst == 1)[0])
    assert np.array_equal(bits(kpt_new), bits(want))
    kf = tracker.build_lk_pyramid(t[0])
    reuse, valid2 = tracker.kpt_flow_track(None, s["next"], s["pts"], kf_pyramid=kf)
    assert np.array_equal(bits(reuse), bits(kpt_new)) and np.array_equal(valid2[0], valid_id[0])
    empty = tracker.calc_optical_flow_pyr_lk(s["prev"], s["next"], np.zeros((0, 1, 2), np.float32))
    assert empty[0].shape == (0, 1, 2) and empty[1].shape == (0, 1)
    lv = kf.level(1)
    assert lv[0].shape == (1, 60, 80) and lv[1].shape == (1, 60, 80, 2)

"""CPU tests of the 2D object detector: the numpy oracle (tests/detector_oracle.py) against
known answers, its cv::RNG against oracle/epnp_ransac.c's, and the host-side argument checks of
the library's detector entry points (nothing here launches a kernel)."""
import numpy as np
import pytest

import detector_oracle as D
from detector_cases import ramp, scene, stage_case, view_size
from oracle import pnp_oracle

INVALID, WORKSPACE = 1, 4


@pytest.fixture(scope="module")
def lib():
    from onepose_amd import _lib
    return _lib.load()


def test_rng_matches_the_c_oracle():
    rng = D.CvRng()
    mine = np.array([rng.next() for _ in range(1000)], np.uint32)
    assert np.array_equal(mine, pnp_oracle.rng_draws(1000))
    assert D.CvRng().uniform(3, 3) == 3


def test_known_answer_scene():
    """600 inliers with sigma = 0.5 px under scale 0.6 / 25 degrees, 40 % gross outliers.  The
    least-squares similarity over N points predicts a position inside the cloud with a standard
    error below 2 sigma sqrt(4 / 2N) = 0.058 px (4 parameters, 2N equations, leverage <= 2 at the
    cloud's corners); 5 standard errors = 0.29 px bound the corners' error, so a view whose
    true corners lie 0.35 px from an integer truncates to the true box."""
    f, t, inl, A = scene(1000, 0.4, seed=1)
    st, M, mask, nin, iters = D.estimate_affine_partial_2d(f, t)
    assert st == 0 and np.array_equal(mask, inl) and nin == inl.sum() == 600
    assert 0 < iters < 2000
    h, w = view_size(A, 0.35)
    _, pre_true = D.view_bbox(A, h, w)
    box, pre = D.view_bbox(M, h, w)
    bound = 5 * 2 * 0.5 * np.sqrt(4 / (2 * 600))
    assert np.abs(pre - pre_true).max() < bound
    tb = pre_true.astype(np.int32)
    assert np.array_equal(box, [tb[:, 0].min(), tb[:, 1].min(), tb[:, 0].max(), tb[:, 1].max()])
    # the refinement is the least-squares similarity over the inliers
    x, y = f[inl].astype(np.float64).T
    J = np.zeros((2 * len(x), 4))
    J[0::2] = np.stack([x, -y, np.ones_like(x), np.zeros_like(x)], 1)
    J[1::2] = np.stack([y, x, np.zeros_like(x), np.ones_like(x)], 1)
    ls = np.linalg.lstsq(J, t[inl].astype(np.float64).reshape(-1), rcond=None)[0]
    np.testing.assert_allclose([M[0, 0], M[1, 0], M[0, 2], M[1, 2]], ls, rtol=0, atol=1e-9)
    assert M[0, 1] == -M[1, 0] and M[1, 1] == M[0, 0]


def test_small_counts_and_degenerate_models():
    f, t, _, A = scene(8, 0.0, seed=2, sigma=0.0)
    assert D.estimate_affine_partial_2d(f[:0], t[:0])[0] == 1
    assert D.estimate_affine_partial_2d(f[:1], t[:1])[0] == 1
    st, M, mask, nin, iters = D.estimate_affine_partial_2d(f[:2], t[:2])
    assert st == 0 and mask.all() and nin == 2 and iters == 0
    np.testing.assert_allclose(M, A, atol=1e-3)
    # coincident source points: a non-finite model without inliers, no model at all
    same = np.repeat(f[:1], 5, 0)
    st, M, mask, nin, _ = D.estimate_affine_partial_2d(same, t[:5], max_iters=50)
    assert st == 2 and nin == 0 and not mask.any() and not M.any()
    # no refinement: the minimal model of the winning pair
    st, M0, *_ = D.estimate_affine_partial_2d(f, t, refine_iters=0)
    assert st == 0
    np.testing.assert_allclose(M0, A, atol=1e-3)


def test_ranking_modes_differ_on_a_hand_built_case():
    m, c0, k0, k1, hw, qhw = stage_case()
    ref = D.detect_stage(m, c0, k0, k1, hw, qhw, rank_mode=0)
    assert list(ref["counts"]) == [30, 20, 5] and list(ref["status"]) == [0, 0, 1]
    assert list(ref["n_inliers"]) == [12, 18, 0]
    assert ref["best_view"] == 0                       # the reference: most matched points
    true = D.detect_stage(m, c0, k0, k1, hw, qhw, rank_mode=1)
    assert true["best_view"] == 1                      # most inliers
    assert np.array_equal(true["best_bbox"], true["bbox"][1])
    # fewer than 6 matches: the reference's fallback box, whose x1 is the query's height
    assert list(ref["bbox"][2]) == [0, 0, 480, 640] and list(ref["rank"]) == [30, 20, 0]
    # ties go to the first view in input order
    tie = D.detect_stage(np.stack([m[1], m[1]]), c0[:2], np.stack([k0[1], k0[1]]), k1, hw[:2], qhw)
    assert tie["best_view"] == 0


def test_crop_at_an_integer_box_is_the_slice():
    img = ramp(40, 56)
    K = np.array([[500.0, 0, 28.5], [0, 510.0, 20.25], [0, 0, 1]])
    crop, K_crop, st = D.crop_resize(img, [8, 4, 24, 20], K, 16)
    assert st == 0 and np.array_equal(crop, img[4:20, 8:24])
    np.testing.assert_allclose(K_crop, [[500, 0, 20.5], [0, 510, 16.25], [0, 0, 1]], rtol=1e-15)
    # overhanging the image: zero outside
    crop, _, _ = D.crop_resize(img, [-4, -2, 12, 14], None, 16)
    assert not crop[:2].any() and not crop[:, :4].any()
    assert np.array_equal(crop[2:, 4:], img[:14, :12])
    # degenerate boxes: the reference would raise
    for box in ([5, 5, 5, 9], [5, 9, 8, 9], [9, 5, 3, 8]):
        crop, K_crop, st = D.crop_resize(img, box, K, 16)
        assert st == 1 and not crop.any() and np.array_equal(K_crop, K)
    # a coordinate outside warpAffine's short maps: refused, not walked out of int range
    crop, K_crop, st = D.crop_resize(img, [-40000, 3, 20, 19], K, 16)
    assert st == 2 and not crop.any() and np.array_equal(K_crop, K)


def test_crop_scales_both_axes_by_the_width():
    """get_affine_transform reads src_w only: an 8 x 16 box cropped to 16 x 16 is scaled by
    16 / 8 = 2 in x AND y (not 1 in y), centred: ty = 8 - 2 * 16 / 2 = -8, so output row y shows
    window row (y + 8) / 2 -- rows 4..11 of the window, the rest is cut off."""
    img = ramp(40, 56)
    x0, y0 = 10, 6
    crop, K_crop, st = D.crop_resize(img, [x0, y0, x0 + 8, y0 + 16], np.eye(3), 16)
    assert st == 0
    win = img[y0:y0 + 16, x0:x0 + 8]
    ys, xs = np.mgrid[0:16:2, 0:16:2]
    assert np.array_equal(crop[0::2, 0::2], win[(ys + 8) // 2, xs // 2])
    assert not np.array_equal(crop[0::2, 0::2], win[ys, xs // 2])   # not the per-axis scale
    np.testing.assert_allclose(K_crop, [[2, 0, -2 * x0], [0, 2, -2 * y0 - 8], [0, 0, 1]])


def test_detector_prototypes(lib):
    from onepose_amd import _lib, detector
    assert lib.onepose_detector_version() == 1 == detector.DETECTOR_VERSION
    assert lib.onepose_abi_version() == 9
    for name in ("onepose_detector_version", "onepose_affine_partial_max_points",
                 "onepose_affine_partial_workspace_bytes", "onepose_affine_partial_ransac",
                 "onepose_detect_stage", "onepose_crop_resize"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    limit = lib.onepose_affine_partial_max_points()
    assert 8192 < limit < 10240   # 160 KB at 16 B per point, less the solver's state
    assert lib.onepose_affine_partial_workspace_bytes(15, 4096) >= 15 * 4
    assert lib.onepose_affine_partial_workspace_bytes(0, 8) == 0
    assert lib.onepose_affine_partial_workspace_bytes(3, 0) == 0


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every refusal happens before a launch: the pointers are dummies, never dereferenced."""
    P = 0x1000
    err = lambda: lib.onepose_last_error().decode()   # noqa: E731
    limit = lib.onepose_affine_partial_max_points()

    def ransac(frm=P, cnt=P, maxp=64, batch=2, thr=6.0, conf=0.99, refine=10, aff=P, mask=P,
               ws=P, wsb=1 << 20):
        return lib.onepose_affine_partial_ransac(frm, P, cnt, maxp, batch, thr, 2000, conf, refine,
                                                 aff, mask, P, P, ws, wsb, None)
    assert ransac(frm=None) == INVALID and "null input" in err()
    assert ransac(cnt=None) == INVALID and "null input" in err()
    assert ransac(aff=None) == INVALID and "null output" in err()
    assert ransac(mask=None) == INVALID and "null output" in err()
    assert ransac(maxp=limit + 1) == INVALID and "onepose_affine_partial_max_points" in err()
    assert ransac(maxp=0) == INVALID and ransac(batch=0) == INVALID
    assert ransac(conf=1.0) == INVALID and "confidence" in err()
    assert ransac(thr=-1.0) == INVALID and ransac(refine=-1) == INVALID
    need = lib.onepose_affine_partial_workspace_bytes(2, 64)
    assert ransac(wsb=need - 1) == WORKSPACE and f"{need - 1} < {need}" in err()
    assert ransac(ws=None) == WORKSPACE
    assert ransac(maxp=limit, ws=None) == WORKSPACE   # the limit itself gets as far as this

    def stage(m0=P, n0=64, n1=50, rank=0, bbox=P, best=P, ws=P, wsb=1 << 20, hw=P):
        return lib.onepose_detect_stage(m0, None, P, P, 0, hw, 3, n0, n1, 480, 640, 6.0, 2000,
                                        0.99, 10, rank, P, None, P, P, P, P, bbox, best, P, ws,
                                        wsb, None)
    assert stage(m0=None) == INVALID and "null input" in err()
    assert stage(hw=None) == INVALID and "null input" in err()
    assert stage(bbox=None) == INVALID and "null output" in err()
    assert stage(best=None) == INVALID and "null output" in err()
    assert stage(n1=0) == INVALID and stage(n0=0) == INVALID
    assert stage(rank=2) == INVALID and "rank_mode" in err()
    assert stage(n0=limit + 1) == INVALID and "onepose_affine_partial_max_points" in err()
    assert stage(wsb=8) == WORKSPACE and stage(ws=None) == WORKSPACE

    def crop(img=P, h=40, w=56, box=P, K=P, size=16, u8=P, Kc=P, st=P):
        return lib.onepose_crop_resize(img, h, w, box, K, size, u8, P, Kc, st, None)
    assert crop(img=None) == INVALID and "null input" in err()
    assert crop(box=None) == INVALID and "null input" in err()
    assert crop(u8=None) == INVALID and crop(st=None) == INVALID and "null output" in err()
    assert crop(K=None) == INVALID and crop(Kc=None) == INVALID and "go together" in err()
    assert crop(h=0) == INVALID and crop(w=-1) == INVALID
    assert crop(size=0) == INVALID and crop(size=8193) == INVALID and "crop_size" in err()


def test_detector_refuses_what_it_cannot_do():
    from onepose_amd import detector
    with pytest.raises(NotImplementedError, match="reference_views"):
        detector.LocalFeatureObjectDetector(None, None, sfm_ws_dir="/nowhere/sfm_ws/model")
    with pytest.raises(ValueError, match="rank_by"):
        detector.LocalFeatureObjectDetector(None, None, db_dict={1: {}}, rank_by="votes")
    with pytest.raises(ValueError, match="sample gap"):
        detector.reference_views([np.zeros((8, 8))] * 3, None, n_ref_view=15)
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    import torch
    back = detector.image_to_u8(torch.from_numpy(u8.astype(np.float32) / 255.0)[None, None])
    assert np.array_equal(back.numpy(), u8)

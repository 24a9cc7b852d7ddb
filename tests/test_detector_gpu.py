"""LocalFeatureObjectDetector on the GPU (onepose_amd/detector.py): the class's logic with a stub
matcher that returns prescribed matches (pinned independently of SuperGlue, against the numpy
oracle), one run with the real SuperGlue against the stage-by-stage composition, a captured
graph of detect_raw, and run_object_detector writing what object_detect_mode="feature_matching"
reads."""
import os

import numpy as np
import pytest
import torch

import detector_oracle as D
from detector_cases import ramp, stage_case
from onepose_amd import detector, inference as I, synthetic as S

pytestmark = pytest.mark.gpu

SPEC = ((30, 12), (20, 18), (5, 5), (25, 20))


def make_db(device, counts=(36, 36, 30, 36)):
    """The hand-built stage case as a db_dict: views 0, 1 and 3 have 36 keypoints (views 0 and 1
    share an image size and so a matcher call, view 3's size differs), view 2 has 30."""
    m, c0, k0, k1, hw, qhw = stage_case(spec=SPEC, pad=4)
    hw = hw.copy()
    hw[1] = hw[0]
    rs = np.random.RandomState(3)
    # unmatched keypoints anywhere (the stub recognises a view by its first keypoint)
    k0 = np.where(m[..., None] > -1, k0, rs.uniform(0, 300, k0.shape).astype(np.float32))
    db, table = {}, {}
    for b, n in enumerate(counts):   # (a count below 36 drops the view's last matches)
        db[10 + 7 * b] = {"keypoints": k0[b, :n], "scores": rs.uniform(0, 1, n).astype(np.float32),
                          "descriptors": rs.standard_normal((256, n)).astype(np.float32),
                          "size": hw[b]}
        table[tuple(k0[b, 0].tolist())] = torch.from_numpy(m[b, :n]).to(device)
    query = {"keypoints": k1, "scores": rs.uniform(0, 1, len(k1)).astype(np.float32),
             "descriptors": rs.standard_normal((256, len(k1))).astype(np.float32),
             "size": np.array(qhw)}
    n0 = max(counts)
    ref_args = (np.stack([np.pad(m[b, :n], (0, n0 - n), constant_values=-1)
                          for b, n in enumerate(counts)]), np.array(counts, np.int32),
                k0[:, :n0], k1, hw, qhw)
    return db, table, query, ref_args


class StubMatcher:
    """SuperGlue's forward contract with prescribed matches: a view is recognised by its first
    keypoint."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def cuda(self):
        return self

    def __call__(self, data):
        k0 = data["keypoints0"]
        self.calls.append((tuple(k0.shape), tuple(data["keypoints1"].shape),
                           tuple(data["image0"].shape[-2:]), tuple(data["image1"].shape[-2:]),
                           data["keypoints1"].stride(0)))
        rows = [self.table[tuple(k0[i, 0].tolist())] for i in range(k0.shape[0])]
        return {"matches0": torch.stack(rows)}


class StubExtractor:
    def __init__(self, query, device):
        self.out = {k: [torch.from_numpy(np.asarray(query[k])).to(device)]
                    for k in ("keypoints", "scores", "descriptors")}

    def cuda(self):
        return self

    def __call__(self, img):
        return self.out


def test_class_with_prescribed_matches(tmp_path, device):
    db, table, query, ref_args = make_db(device)
    stub = StubMatcher(table)
    refs = [D.detect_stage(*ref_args, rank_mode=m) for m in (0, 1)]
    assert refs[0]["best_view"] != refs[1]["best_view"]
    det = detector.LocalFeatureObjectDetector(StubExtractor(query, device), stub, db_dict=db)
    # equal (count, size) share one matcher call with the query at stride 0
    box = det.detect_by_matching(query)
    assert box.dtype == np.int32 and np.array_equal(box, refs[0]["best_bbox"])
    assert sorted(c[0] for c in stub.calls) == [(1, 30, 2), (1, 36, 2), (2, 36, 2)]
    # image0 / image1 carry the sizes reversed, [.., W, H], as the reference's pack_match_data
    # builds them from (H, W) sizes (:26-39): the query is 480 x 640, the views 240 x 320 (two),
    # 200 x 300 and 240 x 290
    assert all(c[1][1:] == (64, 2) and c[3] == (640, 480) for c in stub.calls)
    assert all(c[4] == 0 for c in stub.calls if c[0][0] > 1)
    assert sorted(c[2] for c in stub.calls) == [(290, 240), (300, 200), (320, 240)]
    raw = det.detect_raw(query["keypoints"], query["scores"], query["descriptors"], query["size"])
    for k in ("counts", "status", "n_inliers", "bbox", "inlier_mask"):
        assert np.array_equal(raw[k].cpu().numpy(), refs[0][k]), k
    assert np.array_equal(raw["matches0"].cpu().numpy(), ref_args[0])
    # the ranking the reference evidently meant
    det1 = detector.LocalFeatureObjectDetector(StubExtractor(query, device), stub, db_dict=db,
                                               rank_by="inliers")
    assert np.array_equal(det1.detect_by_matching(query), refs[1]["best_bbox"])

    # detect(): the reference's return values, the crop of the image file at the winning box
    from PIL import Image
    img = ramp(480, 640)
    path = str(tmp_path / "7.png")
    Image.fromarray(img, mode="L").save(path)
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    (tmp_path / "det").mkdir()
    (tmp_path / "Kc").mkdir()
    det = detector.LocalFeatureObjectDetector(
        StubExtractor(query, device), stub, db_dict=db, output_results=True,
        detect_save_dir=str(tmp_path / "det"), K_crop_save_dir=str(tmp_path / "Kc"))
    x = torch.from_numpy(img.astype(np.float32) / 255)[None, None]
    bbox, crop, K_crop = det.detect(x, path, K, crop_size=64)
    ref_u8, ref_K, st = D.crop_resize(img, refs[0]["best_bbox"], K, 64)
    assert st == 0 and np.array_equal(bbox, refs[0]["best_bbox"])
    assert tuple(crop.shape) == (1, 1, 64, 64) and crop.dtype == torch.float32 and crop.is_cuda
    assert np.array_equal(crop[0, 0].cpu().numpy(), ref_u8.astype(np.float32) / 255)
    np.testing.assert_allclose(K_crop, ref_K, rtol=1e-12)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "det" / "7.png")), ref_u8)
    np.testing.assert_allclose(np.loadtxt(tmp_path / "Kc" / "7.txt"), ref_K, rtol=1e-12)
    # the float image alone (no file) gives the same crop; crop_img_by_bbox's return values
    assert np.array_equal(det.detect(x, None, K, crop_size=64)[1].cpu().numpy(),
                          crop.cpu().numpy())
    image_crop, K2 = det.crop_img_by_bbox(path, bbox, K, crop_size=64)
    assert image_crop.dtype == np.uint8 and np.array_equal(image_crop, ref_u8)
    assert np.array_equal(K2, K_crop) and det.crop_img_by_bbox(path, bbox, None, 64)[1] is None

    # previous_pose_detect: the projected 3D box, astype(int32), the same crop entry
    corners = np.array([[x, y, z] for x in (-.1, .1) for y in (-.08, .08) for z in (-.05, .05)])
    pose = np.concatenate([np.eye(3), [[0.02], [-0.01], [0.9]]], 1)
    uv = (np.concatenate([K, np.zeros((3, 1))], 1) @ np.concatenate([pose, [[0, 0, 0, 1]]], 0)
          @ np.concatenate([corners, np.ones((8, 1))], 1).T)          # vis_utils.reproj
    uv = (uv / uv[2:])[:2].T
    want = np.array([*uv.min(0), *uv.max(0)]).astype(np.int32)
    bbox, crop, K_crop = det.previous_pose_detect(path, K, pose, corners, crop_size=64)
    ref_u8, ref_K, _ = D.crop_resize(img, want, K, 64)
    assert np.array_equal(bbox, want) and tuple(crop.shape) == (1, 1, 64, 64)
    assert np.array_equal(crop[0, 0].cpu().numpy(), ref_u8.astype(np.float32) / 255)
    np.testing.assert_allclose(K_crop, ref_K, rtol=1e-12)


class FixedMatcher:
    """Prescribed matches by keypoint count, without touching the host (capturable)."""

    def __init__(self, by_count):
        self.by_count = by_count

    def cuda(self):
        return self

    def __call__(self, data):
        return {"matches0": self.by_count[data["keypoints0"].shape[1]]}


def test_detect_raw_replays_from_a_graph(device):
    db, table, query, ref_args = make_db(device, counts=(36, 34, 30, 32))
    by_count = {n: torch.from_numpy(ref_args[0][b, :n]).to(device)[None]
                for b, n in enumerate((36, 34, 30, 32))}
    det = detector.LocalFeatureObjectDetector(StubExtractor(query, device), FixedMatcher(by_count),
                                              db_dict=db, rank_by="inliers")
    q = [torch.from_numpy(np.asarray(query[k])).to(device)
         for k in ("keypoints", "scores", "descriptors")]
    img = torch.from_numpy(ramp(480, 640)).to(device)
    K = torch.tensor([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]], dtype=torch.float64,
                     device=device)
    keys = ("counts", "status", "n_inliers", "bbox", "inlier_mask", "affine", "best_view",
            "best_bbox", "crop_u8", "crop_f32", "K_crop", "crop_status", "iters")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = det.detect_raw(*q, query["size"], image_u8=img, K=K, crop_size=64)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = {k: eager[k].clone() for k in keys}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = det.detect_raw(*q, query["size"], image_u8=img, K=K, crop_size=64)
    for _ in range(2):
        for k in keys:
            out[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out[k], eager[k]), k
    ref = D.detect_stage(*ref_args, rank_mode=1)
    assert np.array_equal(out["best_bbox"].cpu().numpy(), ref["best_bbox"])


def test_detect_with_superglue_equals_the_composition(device):
    """The real SuperGlue at 128 keypoints and 3 views: detect() equals matcher -> stage ->
    crop called one by one."""
    from onepose_amd import superglue
    data = S.make_superglue_inputs(128, 128, seed=4, batch=3, shared1=True)
    sg = superglue.from_state_dict(S.superglue_state_dict(0)).to(device)
    side = S.SUPERGLUE_IMAGE
    db = {i: {"keypoints": data["keypoints0"][i], "scores": data["scores0"][i],
              "descriptors": data["descriptors0"][i], "size": np.array([side, side])}
          for i in range(3)}
    query = {"keypoints": data["keypoints1"][0], "scores": data["scores1"][0],
             "descriptors": data["descriptors1"][0], "size": np.array([side, side])}
    det = detector.LocalFeatureObjectDetector(StubExtractor(query, device), sg, db_dict=db,
                                              rank_by="inliers")
    img = (S.superpoint_image(side, side, 3) * 255).round().astype(np.uint8)
    K = np.array([[600.0, 0, 256], [0, 600.0, 256], [0, 0, 1]])
    x = torch.from_numpy(img.astype(np.float32) / 255)[None, None]
    bbox, crop, K_crop = det.detect(x, None, K, crop_size=64)

    t = {k: torch.from_numpy(v).to(device) for k, v in data.items()}
    with torch.no_grad():
        pred = sg({**t, "keypoints1": t["keypoints1"].expand(3, -1, -1),
                   "scores1": t["scores1"].expand(3, -1),
                   "descriptors1": t["descriptors1"].expand(3, -1, -1)})
    assert int((pred["matches0"] > -1).sum(1).min()) >= 6      # every view gets an estimate
    hw = torch.full((3, 2), side, dtype=torch.int32, device=device)
    st = detector.detect_stage(pred["matches0"], None, t["keypoints0"], t["keypoints1"][0], hw,
                               (side, side), rank_mode=1)
    cr = detector.crop_resize(torch.from_numpy(img).to(device), st["best_bbox"],
                              torch.from_numpy(K).to(device), 64)
    assert int(st["status"].abs().sum()) == 0
    assert np.array_equal(bbox, st["best_bbox"].cpu().numpy())
    assert torch.equal(crop[0, 0], cr["crop_f32"]) and int(cr["crop_status"]) == 0
    assert np.array_equal(K_crop, cr["K_crop"].cpu().numpy())


class RecordingMatcher:
    """The real SuperGlue, with the image shapes of every call noted."""

    def __init__(self, sg):
        self.sg, self.shapes = sg, []

    def cuda(self):
        return self

    def __call__(self, data):
        self.shapes.append((tuple(data["image0"].shape), tuple(data["image1"].shape)))
        return self.sg(data)


def test_non_square_images_reach_superglue_as_the_reference_passes_them(device):
    """pack_match_data (:26-39) hands SuperGlue torch.empty((1, 1) + tuple(size)[::-1]) with
    size = (H, W), so normalize_keypoints reads height W and width H and centres the keypoints
    on (H/2, W/2).  The class keeps that: on 384 x 512 views and a 400 x 512 query its matches
    are those of SuperGlue called with [.., W, H] shapes, bit for bit, and the order matters --
    the [.., H, W] call gives other scores."""
    from onepose_amd import superglue
    data = S.make_superglue_inputs(128, 128, seed=6, batch=3, shared1=True)
    data["keypoints0"][..., 1] *= 384 / 512        # the points of a 384-row / 400-row image
    data["keypoints1"][..., 1] *= 400 / 512
    sg = RecordingMatcher(superglue.from_state_dict(S.superglue_state_dict(0)).to(device))
    db = {i: {"keypoints": data["keypoints0"][i], "scores": data["scores0"][i],
              "descriptors": data["descriptors0"][i], "size": np.array([384, 512])}
          for i in range(3)}
    det = detector.LocalFeatureObjectDetector(None, sg, db_dict=db)
    raw = det.detect_raw(data["keypoints1"][0], data["scores1"][0], data["descriptors1"][0],
                         (400, 512))
    assert sg.shapes == [((3, 1, 512, 384), (3, 1, 512, 400))]
    t = {k: torch.from_numpy(v).to(device) for k, v in data.items()
         if not k.startswith("image")}
    t.update(keypoints1=t["keypoints1"].expand(3, -1, -1), scores1=t["scores1"].expand(3, -1),
             descriptors1=t["descriptors1"].expand(3, -1, -1))

    def run(shape0, shape1):
        with torch.no_grad():
            return sg.sg({**t, "image0": torch.empty((3, 1) + shape0, device="meta"),
                          "image1": torch.empty((3, 1) + shape1, device="meta")})
    as_reference = run((512, 384), (512, 400))
    as_images = run((384, 512), (400, 512))
    assert torch.equal(raw["matches0"], as_reference["matches0"])
    assert int((raw["matches0"] > -1).sum()) > 0
    assert not torch.equal(as_reference["matching_scores0"], as_images["matching_scores0"])


def test_run_object_detector_feeds_feature_matching_mode(tmp_path, device):
    """Three 64 x 64 frames in color_full/ -> color_det/<name>.png and intrin_det/<name>.txt,
    which default_paths(..., "feature_matching") and the intrinsics path rule then find."""
    from PIL import Image
    from onepose_amd import superglue
    from onepose_amd.superpoint import SuperPoint
    seq = tmp_path / "root" / "seq-1"
    (seq / "color_full").mkdir(parents=True)
    images = [(S.superpoint_image(64, 64, 30 + i) * 255).round().astype(np.uint8) for i in range(3)]
    for i, im in enumerate(images):
        Image.fromarray(im, mode="L").save(seq / "color_full" / f"{i}.png")
    (seq / "intrinsics.txt").write_text("fx: 500.0\nfy: 510.0\ncx: 32.0\ncy: 31.5\n")
    with pytest.raises(FileNotFoundError, match="run_object_detector"):
        I.default_paths(str(seq), str(tmp_path / "sfm"), object_detect_mode="feature_matching")
    sp = SuperPoint({"nms_radius": 3, "max_keypoints": 64}).cuda()
    sp.load_state_dict(S.superpoint_state_dict(0))
    sg = superglue.from_state_dict(S.superglue_state_dict(0)).to(device)
    out = I.run_object_detector(str(seq), sp, sg, ref_images=images, n_ref_view=1, crop_size=32)
    assert [os.path.basename(p) for p, _ in out] == ["0.png", "1.png", "2.png"]
    imgs, _ = I.default_paths(str(seq), str(tmp_path / "sfm"),
                              object_detect_mode="feature_matching")
    assert [os.path.basename(p) for p in imgs] == ["0.png", "1.png", "2.png"]
    K, _ = I.get_K(str(seq / "intrinsics.txt"))
    for (p, bbox), full in zip(out, images):
        crop = np.asarray(Image.open(os.path.join(str(seq), "color_det", os.path.basename(p))))
        Kc = np.loadtxt(I.get_intrin_path_by_color(imgs[0].replace("0.png", os.path.basename(p)),
                                                   "feature_matching"))
        ref_u8, ref_K, _ = D.crop_resize(full, bbox, K, 32)
        assert crop.shape == (32, 32) and np.array_equal(crop, ref_u8)
        np.testing.assert_allclose(Kc, ref_K, rtol=1e-12)
    # a second run empties both directories first, as the reference does
    (seq / "color_det" / "stale.png").write_bytes(b"")
    I.run_object_detector(str(seq), sp, sg, ref_images=images, n_ref_view=1, crop_size=32)
    assert sorted(os.listdir(seq / "color_det")) == ["0.png", "1.png", "2.png"]


def test_inference_runs_in_feature_matching_mode_after_the_detector(tmp_path, device):
    """inference(cfg) with object_detect_mode="feature_matching" reads color_det/ and
    intrin_det/: it raises before run_object_detector wrote them and runs end to end after."""
    from PIL import Image
    from onepose_amd import data_utils as DU, superglue
    from onepose_amd.superpoint import SuperPoint, confs
    obj = S.make_object(300, seed=9)
    frames = [S.make_frame(obj, 100, seed=70 + i) for i in range(3)]
    images = [(S.superpoint_image(128, 128, 50 + i) * 255).round().astype(np.uint8)
              for i in range(3)]
    root, sfm = tmp_path / "root", tmp_path / "sfm" / "obj"
    seq = root / "seq-1"
    for d in ("color_full", "poses_ba"):
        (seq / d).mkdir(parents=True)
    _, paths = I.default_paths(str(seq), str(sfm))
    DU.save_object_annotations(paths["anno_dir"], obj.keypoints3d, obj.clt_descriptors,
                               obj.clt_scores, obj.idxs)
    for i, (f, im) in enumerate(zip(frames, images)):
        Image.fromarray(im, mode="L").save(seq / "color_full" / f"{i}.png")
        np.savetxt(seq / "poses_ba" / f"{i}.txt", np.concatenate([f.pose_gt, [[0, 0, 0, 1]]]))
    (seq / "intrinsics.txt").write_text("fx: 600.0\nfy: 600.0\ncx: 64.0\ncy: 64.0\n")
    from types import SimpleNamespace as N
    ckpt, spp = tmp_path / "GATsSPG.ckpt", tmp_path / "superpoint_v1.pth"
    torch.save({"state_dict": {"matcher." + k: torch.from_numpy(v)
                               for k, v in S.make_state_dict(0).items()},
                "hyper_parameters": dict(S.DEFAULT_HPARAMS)}, ckpt)
    torch.save({k: torch.from_numpy(v) for k, v in S.superpoint_state_dict(0).items()}, spp)
    cfg = N(type="inference", num_leaf=8, object_detect_mode="feature_matching", save_wis3d=False,
            model=N(onepose_model_path=str(ckpt), extractor_model_path=str(spp)),
            network=N(detection="superpoint", matching="superglue"),
            input=N(data_dirs=f"{root} seq-1", sfm_model_dirs=str(sfm)),
            output=N(eval_dir=str(tmp_path / "runs" / "eval" / "GATsSPG")))
    with pytest.raises(FileNotFoundError, match="run_object_detector"):
        I.inference(cfg)
    sp = SuperPoint(confs["superpoint"]["conf"]).cuda()
    sp.load_network(str(spp))
    sg = superglue.from_state_dict(S.superglue_state_dict(0)).to(device)
    I.run_object_detector(str(seq), sp, sg, ref_images=images, n_ref_view=1, crop_size=128)
    res = list(I.inference(cfg).values())[0]
    assert set(res) == {"cmd1", "cmd3", "cmd5"}
    text = (tmp_path / "runs" / "eval" / "GATsSPG" / "objseq-1.txt").read_text()
    assert text == "".join(f"{k}: {res[k]}\n" for k in ("cmd1", "cmd3", "cmd5"))

"""``inference.py``-compatible driver on the HIP engine (reference ``inference.py:17-200``).

The reference's entry chain, with its signatures and ``cfg`` keys (any attribute-style
object: a Hydra ``DictConfig``, ``types.SimpleNamespace``; Hydra itself is out of scope):

* ``inference(cfg)`` (``inference.py:185-198``): ``cfg.input.data_dirs`` /
  ``cfg.input.sfm_model_dirs``, each data dir ``"<data_root> <seq> <seq> ..."``;
* ``inference_core(cfg, data_root, seq_dir, sfm_model_dir)`` (``:97-182``): per frame
  extractor -> ``pack_data`` -> ``pred, _ = matching_model(inp)`` -> valid matches ->
  ``ransac_PnP(K_crop, mkpts2d, mkpts3d, scale=1000)`` -> ``Evaluator``; then
  ``record_eval_result(cfg.output.eval_dir, obj, seq, summary)`` (``eval_utils.py:7-15``);
* ``load_model(cfg)`` (``:49-77``): ``cfg.model.onepose_model_path`` (a ``LitModelGATsSPG``
  checkpoint) and ``cfg.model.extractor_model_path`` (SuperPoint weights),
  ``cfg.network.detection``;
* ``get_default_paths(cfg, data_root, data_dir, sfm_model_dir)`` (``:17-46``),
  ``pack_data(...)`` (``:80-94``), ``cfg.num_leaf``, ``cfg.object_detect_mode``;
* ``run_object_detector(seq_dir, extractor, matcher, ...)``
  (``feature_matching_object_detector.py:117-148``): the 2D object detector over a sequence's
  ``color_full/`` frames, writing the ``color_det/`` and ``intrin_det/`` directories that
  ``object_detect_mode="feature_matching"`` reads.

What changes against the reference loop:

* the matcher is ``onepose_amd.matcher.GATsSuperGlue`` (C-ABI, HIP) inside
  ``onepose_amd.lightning_model.LitModelGATsSPG``, the extractor ``onepose_amd.superpoint.SuperPoint``
  (HIP), the pose solve ``onepose_amd.pose.ransac_PnP`` (HIP RANSAC-EPnP), the evaluator
  ``onepose_amd.pose.Evaluator``;
* the object's descriptors are moved to the GPU once per sequence, before the frame loop;
  ``pack_data``'s ``.cuda()`` is then a no-op instead of a per-frame re-upload
  (``inference.py:89-90``);
* images are read with PIL instead of ``cv2.imread`` (cv2 is absent here; for the 8-bit
  grayscale crops OnePose stores the two give the same array), and listed in sorted order
  (the reference takes ``glob`` order);
* ``cfg.save_wis3d`` visualisation is out of scope and is skipped.

Frames keep their own keypoint count: the detector keeps every keypoint above its threshold,
up to ``max_keypoints`` = 4096. That threshold is SuperPoint's default 0.005:
``extract_features.py:19-24`` spells the key ``keypoints_threshold``, which
``SuperPoint.default_config`` (``keypoint_threshold``) does not read, so its 0.6 never
applies. Each frame runs at its true size: padding would change the matcher's attention and
InstanceNorm results. For fixed-size streams, ``FramePipeline`` is the graph-replayed
throughput path.

The round-1 helpers stay, under their own names: ``default_paths`` (``get_default_paths``
without a cfg), ``inference_core_with_models`` (``inference_core`` over already-built
models), ``run_frames`` and ``match_and_pose``.
"""
from __future__ import annotations

import glob
import os
import re

import numpy as np
import torch

from . import data_utils, pose
from .matcher import GATsSuperGlue, from_state_dict

REFERENCE_SEED = 12345   # inference.py:14  seed_everything(12345)


# ------------------------------------------------------------------ paths (path_utils.py)
def _swap_dir(path: str, old: str, new: str) -> str:
    """Replace the ``old`` directory component (either separator) by ``new``."""
    return re.sub(r"([\\/])" + re.escape(old) + r"([\\/])", lambda m: m.group(1) + new + m.group(2),
                  path, count=1)


def get_gt_pose_path_by_color(color_path: str, det_type: str = "GT_box") -> str:
    """path_utils.py:22-31 (the reference spells the separators as backslashes)."""
    src = {"GT_box": "color", "feature_matching": "color_det"}.get(det_type)
    if src is None:
        raise NotImplementedError(det_type)
    return _swap_dir(color_path, src, "poses_ba").replace(".png", ".txt")


def get_intrin_path_by_color(color_path: str, det_type: str = "GT_box") -> str:
    """path_utils.py:43-52."""
    if det_type == "GT_box":
        return _swap_dir(color_path, "color", "intrin_ba").replace(".png", ".txt")
    if det_type == "feature_matching":
        return _swap_dir(color_path, "color_det", "intrin_det").replace(".png", ".txt")
    raise NotImplementedError(det_type)


def default_paths(data_dir: str, sfm_model_dir: str, detection: str = "superpoint",
                  matching: str = "superglue", object_detect_mode: str = "GT_box"):
    """inference.py:17-47 without the cfg: (image list, paths). Images are sorted (the
    reference takes glob order)."""
    anno_dir = os.path.join(sfm_model_dir, f"outputs_{detection}_{matching}", "anno")
    if object_detect_mode == "GT_box":
        color_dir = os.path.join(data_dir, "color")
    elif object_detect_mode == "feature_matching":
        color_dir = os.path.join(data_dir, "color_det")
        if not os.path.exists(color_dir):
            raise FileNotFoundError("color_det directory not found: run the 2D object detector "
                                    "first (onepose_amd.inference.run_object_detector; "
                                    "reference README)")
    else:
        raise NotImplementedError(object_detect_mode)
    img_lists = sorted(glob.glob(color_dir + "/*.png"))
    paths = {"data_dir": data_dir, "sfm_model_dir": sfm_model_dir, "anno_dir": anno_dir,
             "avg_anno_3d_path": os.path.join(anno_dir, "anno_3d_average.npz"),
             "clt_anno_3d_path": os.path.join(anno_dir, "anno_3d_collect.npz"),
             "idxs_path": os.path.join(anno_dir, "idxs.npy"),
             "intrin_full_path": os.path.join(data_dir, "intrinsics.txt")}
    return img_lists, paths


def get_default_paths(cfg, data_root, data_dir, sfm_model_dir):
    """``inference.py:17-46``: the reference signature; ``cfg.network.detection`` /
    ``.matching`` name the annotation directory, ``cfg.object_detect_mode`` the image one."""
    img_lists, paths = default_paths(data_dir, sfm_model_dir, cfg.network.detection,
                                     cfg.network.matching, cfg.object_detect_mode)
    return img_lists, {"data_root": data_root, **paths}


# ------------------------------------------------------------------ model and object
def load_matcher(model_path: str | None = None, state_dict=None, hparams=None) -> GATsSuperGlue:
    """The matcher of a ``LitModelGATsSPG`` checkpoint (``inference.py:50-59``).

    The checkpoint is read with ``torch.load(weights_only=True)``: only tensors and plain
    containers are accepted, nothing in the file is executed. ``state_dict['matcher.*']``
    holds the weights; ``hyper_parameters`` (flat, ``GATsSPG_lightning_model.py:17-21``)
    the matcher config unless ``hparams`` is given. A checkpoint whose hyper-parameters need
    unpickling of foreign classes is refused by the safe loader; pass ``state_dict`` +
    ``hparams`` explicitly then."""
    from .lightning_model import matcher_hparams, read_checkpoint
    if state_dict is None:
        sd, ckpt_hp = read_checkpoint(model_path)
        if hparams is None:
            hparams = ckpt_hp
    else:
        sd = state_dict
        if any(k.startswith("matcher.") for k in sd):
            sd = {k[len("matcher."):]: v for k, v in sd.items() if k.startswith("matcher.")}
    if hparams is not None:
        hparams = matcher_hparams(hparams)
    return from_state_dict(sd, hparams)


class OnePoseObject:
    """One object's SfM model on the device (``inference.py:108-130``, uploaded once)."""

    def __init__(self, keypoints3d, descriptors3d, leaves, device):
        f32 = dict(dtype=torch.float32, device=device)
        self.keypoints3d = torch.as_tensor(keypoints3d).to(**f32).contiguous()   # [N3, 3]
        self.descriptors3d = torch.as_tensor(descriptors3d).to(**f32).contiguous()  # [256, N3]
        self.leaves = torch.as_tensor(leaves).to(**f32).contiguous()             # [256, N3*L]
        self.num_leaf = self.leaves.shape[1] // self.keypoints3d.shape[0]

    @classmethod
    def from_anno_dir(cls, anno_dir: str, num_leaf: int = 8, device="cuda"):
        """Reads the three annotation files and builds padded / leaf descriptors with the
        global numpy stream, as the reference does after ``seed_everything``."""
        kp3, avg, leaves = data_utils.load_object_annotations(anno_dir, num_leaf)
        return cls(kp3, avg, leaves, device)

    @classmethod
    def from_sfm_model(cls, model_dir: str, features, img_lists, box, num_leaf: int = 8,
                       max_num_kp3d: int = 2500, dist_threshold: float = 1e-3, device="cuda"):
        """Builds the object from its SfM model (``points3D.bin`` / ``images.bin`` in
        ``model_dir``) and the per-image features on the device (``onepose_amd.object_builder``:
        filter, merge, descriptor lifting, leaf gather) without touching the disk.  Seeded like
        ``from_anno_dir`` (``seed_reference_stream``), its tensors equal those read back from the
        files ``object_builder.build_annotations`` writes."""
        from . import object_builder
        kp3, avg, leaves = object_builder.object_tensors(
            model_dir, features, img_lists, box, num_leaf=num_leaf, max_num_kp3d=max_num_kp3d,
            dist_threshold=dist_threshold, device=device)
        return cls(kp3, avg, leaves, device)


# ------------------------------------------------------------------ per frame
def load_image(path: str, grayscale: bool = True):
    """NormalizedDataset.__getitem__ (normalized_dataset.py:22-41): float32 / 255,
    [1,H,W] grayscale or [3,H,W]; returns (image, (H, W))."""
    from PIL import Image
    img = Image.open(path)
    img = np.asarray(img.convert("L" if grayscale else "RGB"), dtype=np.float32)
    img = img[None] if grayscale else img[..., ::-1].transpose(2, 0, 1)   # cv2 reads BGR
    return np.ascontiguousarray(img / 255.0, dtype=np.float32), img.shape[-2:]


def match_and_pose(matcher: GATsSuperGlue, obj: OnePoseObject, keypoints2d, descriptors2d, K,
                   scale: float = 1000.0):
    """One frame of ``inference.py:143-155``: matcher -> valid matches -> RANSAC-EPnP.
    Returns (pose [3,4], pose_homo [4,4], inliers, mkpts2d, mkpts3d, mconf)."""
    dev = obj.keypoints3d.device
    kp2 = torch.as_tensor(np.asarray(keypoints2d, np.float32), device=dev)
    d2 = torch.as_tensor(np.asarray(descriptors2d, np.float32), device=dev)
    inp = {"keypoints2d": kp2[None], "keypoints3d": obj.keypoints3d[None],
           "descriptors2d_query": d2[None], "descriptors3d_db": obj.descriptors3d[None],
           "descriptors2d_db": obj.leaves[None]}
    with torch.no_grad():
        pred, _ = matcher(inp)
    matches = pred["matches0"].cpu().numpy()
    valid = matches > -1
    kpts2d = np.asarray(keypoints2d)
    kpts3d = obj.keypoints3d.cpu().numpy()
    conf = pred["matching_scores0"].cpu().numpy()
    mk2, mk3, mconf = kpts2d[valid], kpts3d[matches[valid]], conf[valid]
    pose_pred, pose_homo, inliers = pose.ransac_PnP(K, mk2, mk3, scale=scale)
    return pose_pred, pose_homo, inliers, mk2, mk3, mconf


def run_frames(matcher: GATsSuperGlue, obj: OnePoseObject, frames, scale: float = 1000.0):
    """The evaluation loop over precomputed detections: each frame a dict with keypoints2d
    [n,2], descriptors2d [256,n], K [3,3], pose_gt [3,4] or [4,4]. Returns (summary,
    per-frame [(pose_pred, n_inliers)])."""
    ev = pose.Evaluator()
    out = []
    for f in frames:
        p, _, inl, *_ = match_and_pose(matcher, obj, f["keypoints2d"], f["descriptors2d"], f["K"],
                                       scale)
        ev.evaluate(p, f["pose_gt"])
        out.append((p, len(inl)))
    return ev.summarize(), out


def inference_core_with_models(matcher: GATsSuperGlue, extractor, seq_dir: str,
                               sfm_model_dir: str, num_leaf: int = 8,
                               object_detect_mode: str = "GT_box", device="cuda",
                               detection: str = "superpoint", matching: str = "superglue"):
    """inference.py:97-177 for one sequence over already-built models (no visualisation, no
    result file): returns the evaluator summary. ``extractor(image [1,1,H,W] on device)``
    returns the reference SuperPoint's output dict (keys 'keypoints' [1][n,2],
    'descriptors' [1][256,n])."""
    img_lists, paths = default_paths(seq_dir, sfm_model_dir, detection, matching,
                                     object_detect_mode)
    obj = OnePoseObject.from_anno_dir(paths["anno_dir"], num_leaf, device)
    ev = pose.Evaluator()
    for img_path in img_lists:
        img, _ = load_image(img_path)
        det = extractor(torch.from_numpy(img)[None].to(device))
        det = {k: (v[0].detach().cpu().numpy() if torch.is_tensor(v[0]) else np.asarray(v[0]))
               for k, v in det.items()}
        K = np.loadtxt(get_intrin_path_by_color(img_path, object_detect_mode))
        p, _, _, *_ = match_and_pose(matcher, obj, det["keypoints"], det["descriptors"], K)
        ev.evaluate(p, np.loadtxt(get_gt_pose_path_by_color(img_path, object_detect_mode)))
    return ev.summarize()


def get_K(intrin_file: str):
    """data_utils.get_K (:282-301): ``intrinsics.txt``'s four ``name: value`` lines (fx, fy, cx,
    cy) -> (K [3,3], K_homo [3,4])."""
    with open(intrin_file) as f:
        fx, fy, cx, cy = (float(line.rstrip("\n").split(":")[1]) for line in f.readlines()[:4])
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    return K, np.concatenate([K, np.zeros((3, 1))], 1)


@torch.no_grad()
def run_object_detector(seq_dir: str, extractor, matcher, db_dict=None, ref_images=None,
                        n_ref_view: int = 15, K=None, crop_size: int = 512,
                        rank_by: str = "reference", device="cuda"):
    """``feature_matching_object_detector.inference_core`` (:117-148) for one sequence over
    already-built models: every ``<seq_dir>/color_full/*.png`` goes through
    ``LocalFeatureObjectDetector.detect``, which writes ``color_det/<name>.png`` (the crop) and
    ``intrin_det/<name>.txt`` (K_crop) -- what ``object_detect_mode="feature_matching"`` reads.
    Both directories are emptied first, as the reference does.  The reference views come from
    ``db_dict`` or from ``ref_images`` (``detector.reference_views``; the reference reads them
    from the object's COLMAP model, which is out of scope).  ``K``: the full image's intrinsics,
    by default ``<seq_dir>/intrinsics.txt``.  Returns ``[(image path, bbox)]``."""
    import shutil
    from .detector import LocalFeatureObjectDetector, reference_views
    color_dir = os.path.join(seq_dir, "color_full")
    if not os.path.exists(color_dir):
        raise FileNotFoundError(f"{color_dir} not found (extracting Frames.m4v is out of scope)")
    img_lists = sorted(glob.glob(color_dir + "/*.png"))
    det_dir, K_dir = os.path.join(seq_dir, "color_det"), os.path.join(seq_dir, "intrin_det")
    for d in (det_dir, K_dir):
        if os.path.exists(d):
            shutil.rmtree(d)
        os.makedirs(d)
    if K is None:
        K, _ = get_K(os.path.join(seq_dir, "intrinsics.txt"))
    if db_dict is None:
        if ref_images is None:
            raise ValueError("run_object_detector needs db_dict or ref_images")
        db_dict = reference_views(ref_images, extractor, n_ref_view)
    detector = LocalFeatureObjectDetector(extractor, matcher, db_dict=db_dict,
                                          n_ref_view=n_ref_view, output_results=True,
                                          detect_save_dir=det_dir, K_crop_save_dir=K_dir,
                                          rank_by=rank_by, device=device)
    out = []
    for img_path in img_lists:
        img, _ = load_image(img_path)
        bbox, _, _ = detector.detect(torch.from_numpy(img)[None], img_path, K, crop_size)
        out.append((img_path, bbox))
    return out


def seed_reference_stream(seed: int = REFERENCE_SEED):
    """The numpy / torch seeding ``inference.py:14`` performs at import."""
    np.random.seed(seed)
    torch.manual_seed(seed)


# ------------------------------------------------------------------ the reference entry chain
def load_matching_model(model_path):
    """``inference.py:51-60``: the checkpoint's ``LitModelGATsSPG``, on the GPU, frozen."""
    from .lightning_model import LitModelGATsSPG
    trained_model = LitModelGATsSPG.load_from_checkpoint(checkpoint_path=model_path)
    trained_model.cuda()
    trained_model.eval()
    trained_model.freeze()
    return trained_model


def load_extractor_model(cfg, model_path):
    """``inference.py:62-73``: SuperPoint with ``confs[cfg.network.detection]['conf']``
    (``extract_features.py:7-26``), weights by ``model_io.load_network`` semantics."""
    from .superpoint import SuperPoint, confs
    extractor_model = SuperPoint(confs[cfg.network.detection]["conf"])
    extractor_model.cuda()
    extractor_model.eval()
    extractor_model.load_network(model_path)
    return extractor_model


def load_model(cfg):
    """``inference.py:49-77``: ``(matching_model, extractor_model)`` from
    ``cfg.model.onepose_model_path`` and ``cfg.model.extractor_model_path``."""
    matching_model = load_matching_model(cfg.model.onepose_model_path)
    extractor_model = load_extractor_model(cfg, cfg.model.extractor_model_path)
    return matching_model, extractor_model


def pack_data(avg_descriptors3d, clt_descriptors, keypoints3d, detection, image_size):
    """``inference.py:80-94``: the matcher's input dict (batch of one). Tensors already on
    the GPU stay where they are (``.cuda()`` is a no-op for them)."""
    keypoints2d = torch.Tensor(detection["keypoints"])
    descriptors2d = torch.Tensor(detection["descriptors"])
    return {
        "keypoints2d": keypoints2d[None].cuda(),                 # [1, n1, 2]
        "keypoints3d": keypoints3d[None].cuda(),                 # [1, n2, 3]
        "descriptors2d_query": descriptors2d[None].cuda(),       # [1, dim, n1]
        "descriptors3d_db": avg_descriptors3d[None].cuda(),      # [1, dim, n2]
        "descriptors2d_db": clt_descriptors[None].cuda(),        # [1, dim, n2*num_leaf]
        "image_size": image_size,
    }


class NormalizedDataset:
    """``src/datasets/normalized_dataset.py:8-45`` (images already cropped): item ``{'path',
    'image' [1,H,W] or [3,H,W] float32 / 255, 'size' [H, W]}``. PIL reads the file."""
    default_conf = {"globs": ["*.jpg", "*.png"], "grayscale": True}

    def __init__(self, img_lists, conf):
        self.img_lists = img_lists
        self.conf = {**self.default_conf, **conf}
        if len(img_lists) == 0:
            raise ValueError("Could not find any image.")

    def __getitem__(self, index):
        img_path = self.img_lists[index]
        image, size = load_image(img_path, self.conf["grayscale"])
        return {"path": str(img_path), "image": image, "size": np.array(size)}

    def __len__(self):
        return len(self.img_lists)

    def batches(self, prefetch: int = 2):
        """What ``DataLoader(dataset, num_workers=1)`` (inference.py:108) yields: each item
        collated into a batch of one (``path`` a list, ``image`` [1,...] and ``size`` [1,2]
        tensors), in order.  As with that loader's one worker (default prefetch_factor 2), the
        items are read ahead by one background worker -- a thread here: the image decode
        releases the GIL -- so reading frame k + 1 overlaps frame k's GPU work.  A worker
        error is raised to the consumer at the item it belongs to."""
        import queue
        import threading
        q = queue.Queue(maxsize=max(1, prefetch))
        done = object()
        stop = threading.Event()

        def put(x):
            while not stop.is_set():
                try:
                    q.put(x, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def work():
            try:
                for i in range(len(self)):
                    d = self[i]
                    item = {"path": [d["path"]], "image": torch.from_numpy(d["image"])[None],
                            "size": torch.from_numpy(d["size"])[None]}
                    if not put(item):
                        return
            except BaseException as e:   # handed to the consumer
                put(e)
                return
            put(done)

        th = threading.Thread(target=work, name="onepose-image-reader", daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is done:
                    break
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()
            th.join()


def load_object(paths, num_leaf):
    """``inference.py:112-130``: keypoints3d, padded average descriptors and leaf descriptors
    from the three annotation files (the leaves consume the global numpy stream)."""
    avg_data = np.load(paths["avg_anno_3d_path"])
    clt_data = np.load(paths["clt_anno_3d_path"])
    idxs = np.load(paths["idxs_path"])
    keypoints3d = torch.Tensor(clt_data["keypoints3d"]).cuda()
    num_3d = keypoints3d.shape[0]
    avg_descriptors3d, _ = data_utils.pad_features3d_random(
        avg_data["descriptors3d"], avg_data["scores3d"], num_3d)
    clt_descriptors, _ = data_utils.build_features3d_leaves(
        clt_data["descriptors3d"], clt_data["scores3d"], idxs, num_3d, num_leaf)
    # The reference keeps the two descriptor tensors on the host and re-uploads them in every
    # frame's pack_data (inference.py:89-90).  Here they move to the GPU once: pack_data's
    # .cuda() is then a no-op, and the matcher sees the same object tensors every frame and keeps
    # the object resident (GATsSuperGlue.resident_object).  Same values, same results.
    return keypoints3d, avg_descriptors3d.cuda(), clt_descriptors.cuda()


def frame_step(matching_model, extractor_model, data, K_crop, keypoints3d, avg_descriptors3d,
               clt_descriptors):
    """One iteration of ``inference.py:133-155`` up to the pose: ``(pose_pred,
    pose_pred_homo, inliers, mkpts2d, mkpts3d, mconf)``."""
    inp = data["image"].cuda()
    pred_detection = extractor_model(inp)
    pred_detection = {k: v[0].cpu().numpy() for k, v in pred_detection.items()}
    inp_data = pack_data(avg_descriptors3d, clt_descriptors, keypoints3d, pred_detection,
                         data["size"])
    pred, _ = matching_model(inp_data)
    matches = pred["matches0"].detach().cpu().numpy()
    valid = matches > -1
    kpts2d = pred_detection["keypoints"]
    kpts3d = inp_data["keypoints3d"][0].detach().cpu().numpy()
    confidence = pred["matching_scores0"].detach().cpu().numpy()
    mkpts2d, mkpts3d, mconf = kpts2d[valid], kpts3d[matches[valid]], confidence[valid]
    pose_pred, pose_pred_homo, inliers = pose.ransac_PnP(K_crop, mkpts2d, mkpts3d, scale=1000)
    return pose_pred, pose_pred_homo, inliers, mkpts2d, mkpts3d, mconf


@torch.no_grad()
def inference_core(cfg, data_root, seq_dir, sfm_model_dir):
    """``inference.py:97-182``: evaluate one sequence and write
    ``<cfg.output.eval_dir>/<obj><seq>.txt``. Returns the evaluator summary (the reference
    returns None; the file is the same)."""
    from .superpoint import confs
    matching_model, extractor_model = load_model(cfg)
    img_lists, paths = get_default_paths(cfg, data_root, seq_dir, sfm_model_dir)
    dataset = NormalizedDataset(img_lists, confs[cfg.network.detection]["preprocessing"])
    evaluator = pose.Evaluator()
    keypoints3d, avg_descriptors3d, clt_descriptors = load_object(paths, cfg.num_leaf)
    # resident for the whole sequence: pack_data's .cuda() is then free per frame
    avg_descriptors3d, clt_descriptors = avg_descriptors3d.cuda(), clt_descriptors.cuda()
    if getattr(cfg, "save_wis3d", False):
        print("onepose_amd: save_wis3d visualisation is out of scope; skipped")
    for data in dataset.batches():
        img_path = data["path"][0]
        K_crop = np.loadtxt(get_intrin_path_by_color(img_path, det_type=cfg.object_detect_mode))
        pose_pred, _, _, *_ = frame_step(matching_model, extractor_model, data, K_crop,
                                         keypoints3d, avg_descriptors3d, clt_descriptors)
        gt_pose_path = get_gt_pose_path_by_color(img_path, det_type=cfg.object_detect_mode)
        evaluator.evaluate(pose_pred, np.loadtxt(gt_pose_path))
    eval_result = evaluator.summarize()
    obj_name = sfm_model_dir.split("/")[-1]
    seq_name = seq_dir.split("/")[-1]
    pose.record_eval_result(cfg.output.eval_dir, obj_name, seq_name, eval_result)
    return eval_result


def inference(cfg, seed: bool = True):
    """``inference.py:185-198``: every ``"<data_root> <seq> ..."`` entry of
    ``cfg.input.data_dirs`` against the matching ``cfg.input.sfm_model_dirs`` entry.

    The reference seeds numpy / torch once, when ``inference.py`` is imported
    (``seed_everything(12345)``, :14), and the 3D padding and leaf sampling of every sequence
    draw from that stream; so this entry seeds the same way before its first sequence (pass
    ``seed=False`` to keep the caller's stream, e.g. to continue one across calls).

    Parity note: the numpy draws (leaf sampling, ``data_utils``) are pinned to the reference's
    fixtures; the torch draws of ``pad_keypoints3d_random`` match the reference's only if model
    construction consumed the torch stream exactly as the reference's does before them -- no
    test covers that, so those padding draws are parity unpinned."""
    if seed:
        seed_reference_stream()
    data_dirs = cfg.input.data_dirs
    sfm_model_dirs = cfg.input.sfm_model_dirs
    if isinstance(data_dirs, str) and isinstance(sfm_model_dirs, str):
        data_dirs = [data_dirs]
        sfm_model_dirs = [sfm_model_dirs]
    results = {}
    for data_dir, sfm_model_dir in zip(data_dirs, sfm_model_dirs):
        splits = data_dir.split(" ")
        data_root = splits[0]
        for seq_name in splits[1:]:
            seq_dir = os.path.join(data_root, seq_name)
            print(f"Eval {seq_dir}")
            results[seq_dir] = inference_core(cfg, data_root, seq_dir, sfm_model_dir)
    return results

"""Drop-in ``LocalFeatureObjectDetector`` on libonepose_hip (MI355X).

The reference class (``src/local_feature_2D_detector/local_feature_2D_detector.py``) matches
one query frame against ``n_ref_view`` reference views with SuperGlue and then, per view, goes
device -> host -> OpenCV: ``cv2.estimateAffinePartial2D``, the box of the warped view corners,
the choice of view and two ``cv2.warpAffine`` crops.  Here everything after the SuperGlue
forwards is three launches (``onepose_detect_stage``: RANSAC + ranking, ``onepose_crop_resize``)
and nothing leaves the device before the result does:

* the reference views are uploaded once, at construction; views with the same keypoint count
  and image size go through one matcher call with the query shared (batch stride 0), the others
  get a call of their own -- no padding, which would change the attention;
  ``batch_views="all"`` instead uploads the non-empty views as one group padded to the largest
  count, with device counts and per-view image sizes, and makes one matcher call per query
  (the matcher's counts entry keeps the padding out of the attention and the transport);
* ``detect`` / ``detect_by_matching`` / ``crop_img_by_bbox`` / ``previous_pose_detect`` /
  ``save_detection`` / ``save_K_crop`` keep the reference's signatures and return values;
  ``detect_raw`` returns the device tensors without a host synchronisation of its own;
* the matcher is handed ``image0`` / ``image1`` of shape [.., W, H], as the reference's
  ``pack_match_data`` builds them from (H, W) sizes (``_shape_only``): a quirk kept, because on
  non-square images it decides the matches;
* ``rank_by="reference"`` ranks the views as the reference does -- by the number of *matched*
  points (``inliers.shape[0]`` of OpenCV's N x 1 mask); ``rank_by="inliers"`` ranks by the
  inlier count, evidently what was meant;
* a view where the reference would crash (``affine is None``) reports status 2 and the fallback
  box; a degenerate box crops to a zero image with ``K_crop = K`` (the reference would raise);
* images are read with PIL (cv2 is absent); reading a COLMAP model is out of scope:
  ``reference_views`` builds ``db_dict`` from a list of images instead.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib

DETECTOR_VERSION = 1
RANK_MODES = {"reference": 0, "inliers": 1}
RANSAC_DEFAULTS = dict(threshold=6.0, max_iters=2000, confidence=0.99, refine_iters=10)


# ---------------------------------------------------------------------------- entry points
def _ransac_workspace(lib, batch, max_points, dev):
    n = lib.onepose_affine_partial_workspace_bytes(batch, max_points)
    return torch.zeros(max(n, 256), dtype=torch.uint8, device=dev)


def affine_partial_ransac(from_pts, to_pts, counts, threshold=6.0, max_iters=2000,
                          confidence=0.99, refine_iters=10):
    """``onepose_affine_partial_ransac``: from_pts, to_pts [B, P, 2] float32 and counts [B] int32
    on the GPU -> dict of device tensors: affine [B, 2, 3] float64, inlier_mask [B, P] uint8,
    n_inliers, status, iters [B] int32.  No host synchronisation."""
    lib = _lib.load()
    dev = from_pts.device
    if dev.type != "cuda":
        raise RuntimeError("onepose_amd.detector runs on a ROCm GPU only")
    f = from_pts.float().contiguous()
    t = to_pts.float().contiguous()
    c = counts.to(torch.int32).contiguous()
    B, P = f.shape[0], f.shape[1]
    out = {"affine": torch.empty(B, 2, 3, dtype=torch.float64, device=dev),
           "inlier_mask": torch.empty(B, P, dtype=torch.uint8, device=dev),
           "n_inliers": torch.empty(B, dtype=torch.int32, device=dev),
           "status": torch.empty(B, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        ws = _ransac_workspace(lib, B, P, dev)
        _lib.run("onepose_affine_partial_ransac", from_=f, to=t, counts=c, max_points=P, batch=B,
                 threshold=float(threshold), max_iters=int(max_iters),
                 confidence=float(confidence), refine_iters=int(refine_iters), **out,
                 workspace=ws, workspace_bytes=ws.numel(), stream=_lib.stream_ptr(dev))
    out["iters"] = ws[:4 * B].view(torch.int32)
    return out


def detect_stage(matches0, counts0, kpts0, kpts1, db_hw, query_hw, threshold=6.0, max_iters=2000,
                 confidence=0.99, refine_iters=10, rank_mode=0):
    """``onepose_detect_stage``: matches0 [B, n0] int64, counts0 [B] int32 or None, kpts0
    [B, n0, 2], kpts1 [n1, 2] (shared) or [B, n1, 2], db_hw [B, 2] int32 on the GPU, query_hw
    (H, W) -> dict of device tensors (counts, mpts, affine, inlier_mask, n_inliers, status, bbox,
    iters, best_view, best_bbox).  No host synchronisation."""
    lib = _lib.load()
    dev = matches0.device
    if dev.type != "cuda":
        raise RuntimeError("onepose_amd.detector runs on a ROCm GPU only")
    m = matches0.to(torch.int64).contiguous()
    B, n0 = m.shape
    k0 = kpts0.float().contiguous()
    k1 = kpts1.float().contiguous()
    if tuple(k0.shape) != (B, n0, 2):
        raise ValueError(f"kpts0 {tuple(k0.shape)}, expected {(B, n0, 2)}")
    shared = k1.dim() == 2
    if not shared and k1.shape[0] != B:
        raise ValueError(f"kpts1 {tuple(k1.shape)}: batch {B} expected")
    n1 = k1.shape[-2]
    c0 = None if counts0 is None else counts0.to(torch.int32).contiguous()
    hw = db_hw.to(torch.int32).contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"counts": torch.empty(B, **i32),
           "mpts": torch.zeros(B, n0, 4, dtype=torch.float32, device=dev),
           "affine": torch.empty(B, 2, 3, dtype=torch.float64, device=dev),
           "inlier_mask": torch.empty(B, n0, dtype=torch.uint8, device=dev),
           "n_inliers": torch.empty(B, **i32), "status": torch.empty(B, **i32),
           "bbox": torch.empty(B, 4, **i32), "best_view": torch.empty(1, **i32),
           "best_bbox": torch.empty(4, **i32)}
    with torch.cuda.device(dev):
        ws = _ransac_workspace(lib, B, n0, dev)
        _lib.run("onepose_detect_stage", matches0=m, counts0=c0, kpts0=k0, kpts1=k1,
                 kpts1_bstride=0 if shared else n1 * 2, db_hw=hw, batch=B, n0=n0, n1=n1,
                 query_h=int(query_hw[0]), query_w=int(query_hw[1]), threshold=float(threshold),
                 max_iters=int(max_iters), confidence=float(confidence),
                 refine_iters=int(refine_iters), rank_mode=int(rank_mode), **out,
                 workspace=ws, workspace_bytes=ws.numel(), stream=_lib.stream_ptr(dev))
    out["iters"] = ws[:4 * B].view(torch.int32)
    return out


def crop_resize(image_u8, bbox, K=None, crop_size=512):
    """``onepose_crop_resize``: image [h, w] uint8 and bbox [4] int32 on the GPU, K [3, 3] float64
    (GPU) or None -> dict of device tensors: crop_u8 [S, S], crop_f32 [S, S] = u8 / 255, K_crop
    [3, 3] float64 (absent without K), crop_status [1] int32.  No host synchronisation."""
    dev = image_u8.device
    if dev.type != "cuda":
        raise RuntimeError("onepose_amd.detector runs on a ROCm GPU only")
    if image_u8.dtype != torch.uint8 or image_u8.dim() != 2:
        raise ValueError("crop_resize takes a [h, w] uint8 image")
    img = image_u8.contiguous()
    box = bbox.to(torch.int32).contiguous()
    S = int(crop_size)
    out = {"crop_u8": torch.empty(S, S, dtype=torch.uint8, device=dev),
           "crop_f32": torch.empty(S, S, dtype=torch.float32, device=dev),
           "crop_status": torch.empty(1, dtype=torch.int32, device=dev)}
    Kd = None
    if K is not None:
        Kd = K.to(torch.float64).contiguous()
        out["K_crop"] = torch.empty(3, 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.run("onepose_crop_resize", image=img, h=img.shape[0], w=img.shape[1], bbox=box, K=Kd,
                 crop_size=S, **{"K_crop": None, **out}, stream=_lib.stream_ptr(dev))
    return out


# ---------------------------------------------------------------------------- images
def read_gray_u8(path):
    """cv2.imread(path, IMREAD_GRAYSCALE) with PIL: [h, w] uint8."""
    from PIL import Image
    return np.array(Image.open(path).convert("L"), dtype=np.uint8)


def image_to_u8(image):
    """The uint8 image behind a float image / 255 (``round(x * 255)`` is exact): [h, w] uint8."""
    x = torch.as_tensor(image)
    x = x.reshape(x.shape[-2], x.shape[-1])
    return torch.round(x.float() * 255.0).clamp_(0, 255).to(torch.uint8)


def reference_views(images, extractor, n_ref_view=15):
    """``extract_ref_view_features`` over a list of images instead of a COLMAP model: the views
    ``range(1, len(images), len(images) // n_ref_view)`` (the reference's sampling), each run
    through the extractor.  ``images``: paths, or [h, w] arrays (uint8, or float in [0, 1]).
    Returns the reference's ``db_dict``: ``{idx: {keypoints, scores, descriptors, size}}``."""
    gap = len(images) // n_ref_view
    if gap < 1:
        raise ValueError(f"{len(images)} images for n_ref_view={n_ref_view}: the reference's "
                         "sample gap len(images) // n_ref_view would be 0")
    dev = getattr(extractor, "device", None)
    if dev is None or torch.device(dev).type != "cuda":
        dev = torch.device("cuda")
    db = {}
    for idx in range(1, len(images), gap):
        im = images[idx]
        if isinstance(im, (str, os.PathLike)):
            im = read_gray_u8(im)
        im = np.asarray(im)
        im = im.astype(np.float32) / 255.0 if im.dtype == np.uint8 else im.astype(np.float32)
        with torch.no_grad():
            det = extractor(torch.from_numpy(im)[None, None].to(dev))
        det = {k: v[0].detach().cpu().numpy() for k, v in det.items()}
        det["size"] = np.array(im.shape[-2:])
        db[idx] = det
    return db


def _shape_only(batch, size_hw):
    """``pack_match_data``'s ``image0`` / ``image1`` (:26-39), of which the matcher reads only the
    shape: ``torch.empty((1, 1) + tuple(size)[::-1])``.  ``size`` is (H, W), so the tensor is
    [.., W, H] and SuperGlue's ``normalize_keypoints``, which reads ``shape[-2:]`` as (height,
    width), centres the keypoints on (H/2, W/2) instead of (W/2, H/2).  A quirk of the
    reference, kept: on a non-square image the other order gives other matches."""
    return torch.empty((batch, 1) + tuple(int(s) for s in size_hw)[::-1], device="meta")


# ---------------------------------------------------------------------------- the class
class LocalFeatureObjectDetector:
    def __init__(self, extractor, matcher, db_dict=None, sfm_ws_dir=None, n_ref_view=15,
                 output_results=False, detect_save_dir=None, K_crop_save_dir=None,
                 rank_by="reference", device=None, batch_views="equal"):
        if rank_by not in RANK_MODES:
            raise ValueError(f"rank_by {rank_by!r}: one of {sorted(RANK_MODES)}")
        if batch_views not in ("equal", "all"):
            raise ValueError(f"batch_views {batch_views!r}: 'equal' or 'all'")
        if batch_views == "all" and not getattr(matcher, "supports_counts", False):
            raise ValueError(f"batch_views='all': {type(matcher).__name__} does not declare "
                             "supports_counts (padded batches with per-sample counts)")
        self.batch_views = batch_views
        if db_dict is None:
            if sfm_ws_dir is not None:
                raise NotImplementedError(
                    "reading a COLMAP model (sfm_ws_dir) is out of scope: build db_dict with "
                    "onepose_amd.detector.reference_views(images, extractor, n_ref_view)")
            raise ValueError("LocalFeatureObjectDetector needs db_dict (see reference_views)")
        if len(db_dict) == 0:
            raise ValueError("db_dict is empty")
        self.device = torch.device("cuda" if device is None else device)
        self.extractor = extractor.cuda() if hasattr(extractor, "cuda") else extractor
        self.matcher = matcher.cuda() if hasattr(matcher, "cuda") else matcher
        self.db_dict = db_dict
        self.n_ref_view = n_ref_view
        self.output_results = output_results
        self.detect_save_dir = detect_save_dir
        self.K_crop_save_dir = K_crop_save_dir
        self.rank_by = rank_by
        self.ransac = dict(RANSAC_DEFAULTS)
        self._upload()

    # the reference views, on the device once: per (count, h, w) group the matcher's stacked
    # inputs, and for the stage one [B, n0max] layout in input order
    def _upload(self):
        dev = self.device
        self.view_ids = list(self.db_dict.keys())
        views = [self.db_dict[i] for i in self.view_ids]
        counts = [int(np.asarray(v["keypoints"]).shape[0]) for v in views]
        B, n0max = len(views), max(1, max(counts))
        kp = np.zeros((B, n0max, 2), np.float32)
        for b, v in enumerate(views):
            kp[b, :counts[b]] = np.asarray(v["keypoints"], np.float32).reshape(-1, 2)
        self.kpts0 = torch.from_numpy(kp).to(dev)
        self.counts0 = torch.tensor(counts, dtype=torch.int32, device=dev)
        self.db_hw = torch.tensor([[int(v["size"][0]), int(v["size"][1])] for v in views],
                                  dtype=torch.int32, device=dev)
        groups = {}
        for b, v in enumerate(views):
            if counts[b] > 0:
                groups.setdefault((counts[b], int(v["size"][0]), int(v["size"][1])), []).append(b)
        self.groups = []
        rows = [b for b in range(B) if counts[b] > 0]
        if self.batch_views == "all" and rows:
            # one padded group: zeros past a view's count, counts and (h, w) on the device
            G, n = len(rows), max(counts[b] for b in rows)
            kp0 = np.zeros((G, n, 2), np.float32)
            sc0 = np.zeros((G, n), np.float32)
            de0 = np.zeros((G, 256, n), np.float32)
            for g, b in enumerate(rows):
                c = counts[b]
                kp0[g, :c] = np.asarray(views[b]["keypoints"], np.float32).reshape(c, 2)
                sc0[g, :c] = np.asarray(views[b]["scores"], np.float32).reshape(c)
                de0[g, :, :c] = np.asarray(views[b]["descriptors"], np.float32).reshape(256, c)
            # (_shape_only's quirk, per view: the matcher reads (h, w) = the size reversed)
            hw = [[int(views[b]["size"][1]), int(views[b]["size"][0])] for b in rows]
            self.groups.append({
                "n": n, "rows": torch.tensor(rows, dtype=torch.int64, device=dev),
                "keypoints0": torch.from_numpy(kp0).to(dev), "scores0": torch.from_numpy(sc0).to(dev),
                "descriptors0": torch.from_numpy(de0).to(dev),
                "counts0": torch.tensor([counts[b] for b in rows], dtype=torch.int32, device=dev),
                "image_hw0": torch.tensor(hw, dtype=torch.int32, device=dev)})
            return
        for (n, h, w), rows in groups.items():
            f32 = lambda key: torch.from_numpy(np.stack(   # noqa: E731
                [np.asarray(views[b][key], np.float32) for b in rows])).to(dev)
            self.groups.append({
                "n": n, "rows": torch.tensor(rows, dtype=torch.int64, device=dev),
                "keypoints0": f32("keypoints").reshape(len(rows), n, 2),
                "scores0": f32("scores").reshape(len(rows), n),
                "descriptors0": f32("descriptors").reshape(len(rows), 256, n),
                "image0": _shape_only(len(rows), (h, w))})

    def extract_ref_view_features(self, sfm_ws_dir, n_ref_views):
        raise NotImplementedError(
            "reading a COLMAP model is out of scope: build db_dict with "
            "onepose_amd.detector.reference_views(images, extractor, n_ref_view)")

    # ------------------------------------------------------------------ device path
    @torch.no_grad()
    def match_raw(self, keypoints, scores, descriptors, query_hw):
        """The SuperGlue forwards of one query (device tensors keypoints [n1, 2], scores [n1],
        descriptors [256, n1]) against every reference view: matches0 [B, n0max] int64, row b
        view b's first counts0[b] entries (-1 elsewhere)."""
        dev = self.device
        B, n0max = self.kpts0.shape[:2]
        m0 = torch.full((B, n0max), -1, dtype=torch.int64, device=dev)
        n1 = keypoints.shape[0]
        if n1 == 0:
            return m0
        H, W = int(query_hw[0]), int(query_hw[1])
        for g in self.groups:
            G = g["rows"].shape[0]
            data = {k: g[k] for k in ("keypoints0", "scores0", "descriptors0", "image0",
                                      "counts0", "image_hw0") if k in g}
            data = {**data,
                    "keypoints1": keypoints[None].expand(G, n1, 2),
                    "scores1": scores[None].expand(G, n1),
                    "descriptors1": descriptors[None].expand(G, 256, n1),
                    "image1": _shape_only(G, (H, W))}
            pred = self.matcher(data)
            m0[:, :g["n"]].index_copy_(0, g["rows"], pred["matches0"].to(torch.int64))
        return m0

    @torch.no_grad()
    def detect_raw(self, keypoints, scores, descriptors, query_hw, image_u8=None, K=None,
                   crop_size=512):
        """One query frame on the device: the matcher forwards, ``onepose_detect_stage`` and, with
        ``image_u8`` ([H, W] uint8 on the GPU), ``onepose_crop_resize`` at the winning box.
        Returns the stage's dict plus matches0 and the crop's tensors; no host synchronisation
        (capturable in a graph when the matcher's forward is)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        kp = torch.as_tensor(keypoints).to(**f32).reshape(-1, 2)
        sc = torch.as_tensor(scores).to(**f32).reshape(-1)
        de = torch.as_tensor(descriptors).to(**f32).reshape(256, -1)
        m0 = self.match_raw(kp, sc, de, query_hw)
        k1 = kp if kp.shape[0] > 0 else torch.zeros(1, 2, **f32)
        out = detect_stage(m0, self.counts0, self.kpts0, k1, self.db_hw, query_hw,
                           rank_mode=RANK_MODES[self.rank_by], **self.ransac)
        out["matches0"] = m0
        if image_u8 is not None:
            Kd = None if K is None else torch.as_tensor(K).to(dtype=torch.float64,
                                                             device=self.device)
            out.update(crop_resize(image_u8.to(self.device), out["best_bbox"], Kd, crop_size))
        return out

    # ------------------------------------------------------------------ the reference's methods
    def _query_tensors(self, query):
        return query["keypoints"], query["scores"], query["descriptors"], query["size"]

    def detect_by_matching(self, query):
        """query: the extractor's output for one image (keypoints [n, 2], scores [n], descriptors
        [256, n]) plus ``size`` (H, W).  Returns bbox [x0, y0, x1, y1] (numpy int32)."""
        out = self.detect_raw(*self._query_tensors(query))
        return out["best_bbox"].cpu().numpy()

    def _image_u8(self, query_img_path, query_img=None):
        if query_img is not None and (query_img_path is None or not os.path.exists(query_img_path)):
            return image_to_u8(query_img).to(self.device)
        return torch.from_numpy(read_gray_u8(query_img_path)).to(self.device)

    def _crop(self, query_img_path, bbox, K, crop_size, query_img):
        """crop_resize of the image at a host box: the dict of device tensors."""
        box = torch.as_tensor(np.asarray(bbox).astype(np.int32)).to(self.device)
        Kd = None if K is None else torch.as_tensor(np.asarray(K, np.float64)[:3, :3].copy()
                                                     ).to(self.device)
        return crop_resize(self._image_u8(query_img_path, query_img), box, Kd, crop_size)

    def crop_img_by_bbox(self, query_img_path, bbox, K=None, crop_size=512, query_img=None):
        """Returns (image_crop [crop_size, crop_size] uint8 numpy, K_crop [3, 3] or None)."""
        out = self._crop(query_img_path, bbox, K, crop_size, query_img)
        return (out["crop_u8"].cpu().numpy(),
                out["K_crop"].cpu().numpy() if K is not None else None)

    def save_detection(self, crop_img, query_img_path):
        if self.output_results and self.detect_save_dir is not None:
            from PIL import Image
            Image.fromarray(np.asarray(crop_img, np.uint8)).save(
                os.path.join(self.detect_save_dir, os.path.basename(query_img_path)))

    def save_K_crop(self, K_crop, query_img_path):
        if self.output_results and self.K_crop_save_dir is not None:
            name = os.path.splitext(os.path.basename(query_img_path))[0] + ".txt"
            np.savetxt(os.path.join(self.K_crop_save_dir, name), K_crop)   # K_crop: 3*3

    @torch.no_grad()
    def detect(self, query_img, query_img_path, K, crop_size=512):
        """Detect the object by local feature matching and crop the image.  query_img
        [1, 1, H, W] (or [1, H, W]) float / 255, K [3, 3] of the original image.  Returns
        (bbox [x0, y0, x1, y1] numpy, image_crop_tensor [1, 1, S, S] float32 / 255 on the GPU,
        K_crop [3, 3] numpy)."""
        query_img = torch.as_tensor(query_img)
        inp = (query_img[None] if query_img.dim() != 4 else query_img).to(self.device)
        det = self.extractor(inp)
        out = self.detect_raw(det["keypoints"][0], det["scores"][0], det["descriptors"][0],
                              tuple(query_img.shape[-2:]),
                              image_u8=self._image_u8(query_img_path, query_img), K=K,
                              crop_size=crop_size)
        bbox = out["best_bbox"].cpu().numpy()
        K_crop = out["K_crop"].cpu().numpy() if K is not None else None
        if self.output_results and query_img_path is not None:
            self.save_detection(out["crop_u8"].cpu().numpy(), query_img_path)
            if K_crop is not None:
                self.save_K_crop(K_crop, query_img_path)
        return bbox, out["crop_f32"][None, None], K_crop

    def previous_pose_detect(self, query_img_path, K, pre_pose, bbox3D_corner, crop_size=512,
                             query_img=None):
        """The box of the 3D bounding box's corners projected with the last frame's pose
        (vis_utils.reproj on the host), cropped by the same entry point."""
        K = np.asarray(K, np.float64)
        pose = np.asarray(pre_pose, np.float64)
        K_homo = np.concatenate([K, np.zeros((3, 1))], 1) if K.shape == (3, 3) else K
        pose_homo = np.concatenate([pose, [[0, 0, 0, 1]]], 0) if pose.shape == (3, 4) else pose
        pts = np.asarray(bbox3D_corner, np.float64).reshape(-1, 3)
        proj = K_homo @ pose_homo @ np.concatenate([pts, np.ones((len(pts), 1))], 1).T
        proj = (proj[:] / proj[2:])[:2].T
        x0, y0 = proj.min(0)
        x1, y1 = proj.max(0)
        bbox = np.array([x0, y0, x1, y1]).astype(np.int32)
        out = self._crop(query_img_path, bbox, K, crop_size, query_img)
        K_crop = out["K_crop"].cpu().numpy()
        self.save_detection(out["crop_u8"].cpu().numpy(), query_img_path)
        self.save_K_crop(K_crop, query_img_path)
        return bbox, out["crop_f32"][None, None], K_crop

"""FramePipeline(variable_counts=True): partly filled frames on the graph-replayed path.

A short bank of four 256 x 256 images, one per (slot, sample): the first is a whole synthetic
image, the others the same image with more and more of its right side blanked, so SuperPoint
returns fewer keypoints on them -- the keypoint threshold is set, from the detector's own scores on
the whole image, just below that image's n1-th score, which keeps it full.  The object is built
from the whole image's detections (its keypoints back-projected under a known pose, its
descriptors as the object's), so the frames match it and have a pose (the synthetic SuperPoint's
descriptor head is whitened first, `whitened_superpoint`: its raw descriptors are too alike to
match anything).

The pipeline, from captured graphs, unstaged and staged, must equal ``inference.run_frames`` on
the same frames -- each frame cut to its own count -- under tests/parity.py (indices exact, scores
within 2e-5), with poses within the project's 1e-6 PnP bar.  With ``variable_counts=False`` on a
fully filled bank the pipeline issues today's calls and gives their bits."""
import numpy as np
import pytest
import torch

from onepose_amd import inference, matcher, synthetic
from onepose_amd.pipeline import FramePipeline
from onepose_amd.superpoint import SuperPoint
from parity import assert_pred_equal

pytestmark = pytest.mark.gpu
N1, HW, L, B, SLOTS = 256, (256, 256), 4, 2, 2
CUTS = (256, 208, 160, 112)        # columns kept of the image, per frame


def whitened_superpoint(img, seed=0):
    """Synthetic SuperPoint weights whose descriptors tell keypoints apart: the random weights'
    descriptor field is smooth and nearly rank one (mean cosine between pixels 0.92), so nothing
    would match; the last 1 x 1 conv (convDb) is recomposed with the whitening transform of its
    own output on `img` (computed with the numpy oracle's convolutions).  The detector head, and
    so the keypoints and counts, are untouched."""
    from oracle import superpoint_np as S
    sd = synthetic.superpoint_state_dict(seed)
    da = S._relu(S.conv2d(S.encoder(sd, img), sd["convDa.weight"], sd["convDa.bias"]))
    f = S.conv2d(da, sd["convDb.weight"], sd["convDb.bias"]).reshape(256, -1).astype(np.float64)
    mu = f.mean(1)
    w, V = np.linalg.eigh((f - mu[:, None]) @ (f - mu[:, None]).T / f.shape[1])
    A = (V / np.sqrt(np.maximum(w, w.max() * 1e-4))) @ V.T
    out = dict(sd)
    out["convDb.weight"] = (A @ sd["convDb.weight"].reshape(256, 256).astype(np.float64)) \
        .reshape(256, 256, 1, 1).astype(np.float32)
    out["convDb.bias"] = (A @ (sd["convDb.bias"].astype(np.float64) - mu)).astype(np.float32)
    return out


def _detector(thr, dev, sd):
    sp = SuperPoint({"nms_radius": 3, "max_keypoints": N1, "keypoint_threshold": float(thr)})
    sp.load_state_dict(sd)
    return sp.to(dev)


@pytest.fixture(scope="module")
def bank():
    dev = torch.device("cuda", 0)
    base = synthetic.superpoint_image(*HW, 10)
    imgs = np.stack([base.copy() for _ in CUTS])
    for i, cut in enumerate(CUTS):
        imgs[i][:, cut:] = float(base.mean())
    spsd = whitened_superpoint(base)
    raw = _detector(0.005, dev, spsd).detect_raw(torch.from_numpy(imgs)[:, None].to(dev))
    assert int(raw["counts"][0]) == N1, "the whole image fills the detector's top-k"
    thr = float(raw["scores"][0].min()) * 0.999          # keeps frame 0 full
    sp = _detector(thr, dev, spsd)
    raw = sp.detect_raw(torch.from_numpy(imgs)[:, None].to(dev))
    counts = raw["counts"].cpu().tolist()
    print("keypoint_threshold", thr, "counts", counts)
    # the bank's premise: one frame full, at least half of them partly filled, all different
    assert counts[0] == N1 and sum(c < N1 for c in counts) >= len(counts) // 2
    assert len(set(counts)) == len(counts) and min(counts) >= 8
    # the object: frame 0's keypoints back-projected under a known pose, its descriptors
    rs = np.random.RandomState(7)
    K = synthetic.crop_intrinsics(HW[0], 300.0)
    R = synthetic.random_rotation(rs)
    t = np.array([0.01, -0.02, 0.45])
    pose = np.concatenate([R, t[:, None]], 1)
    kp = raw["keypoints"][0].cpu().numpy().astype(np.float64)
    depth = rs.uniform(0.35, 0.55, N1)
    cam = (np.linalg.inv(K) @ np.concatenate([kp, np.ones((N1, 1))], 1).T).T * depth[:, None]
    kp3 = ((cam - t) @ R).astype(np.float32)
    d3 = raw["descriptors"][0].cpu().numpy()                               # [256, N1]
    leaves = np.repeat(d3, L, axis=1) + 0.05 * rs.standard_normal((256, N1 * L)).astype(np.float32)
    m = matcher.from_state_dict(synthetic.make_state_dict(0))
    obj = inference.OnePoseObject(kp3, d3, leaves.astype(np.float32), dev)
    frames = [{"keypoints2d": raw["keypoints"][i, :c].cpu().numpy(),
               "descriptors2d": raw["descriptors"][i, :, :c].cpu().numpy(), "K": K,
               "pose_gt": pose} for i, c in enumerate(counts)]
    # the reference path: each frame at its own size, with host round trips
    _, poses = inference.run_frames(m, obj, frames)
    preds = []
    for f in frames:
        with torch.no_grad():
            p, _ = m({"keypoints2d": torch.from_numpy(f["keypoints2d"]).to(dev)[None],
                      "keypoints3d": obj.keypoints3d[None],
                      "descriptors2d_query": torch.from_numpy(f["descriptors2d"]).to(dev)[None],
                      "descriptors3d_db": obj.descriptors3d[None],
                      "descriptors2d_db": obj.leaves[None]})
        preds.append({k: v.cpu().numpy() for k, v in p.items()})
    assert (preds[0]["matches0"] > -1).sum() > 50 and all(n > 20 for _, n in poses)
    return dict(dev=dev, imgs=imgs, sp=sp, spsd=spsd, m=m, obj=obj, counts=counts, K=K, pose=pose,
                poses=poses, preds=preds, kp3=kp3, d3=d3, leaves=leaves)


def _pipeline(bk, variable_counts, sp=None, imgs=None):
    pipe = FramePipeline(bk["m"], bk["kp3"], bk["d3"], bk["leaves"], B, N1, bk["dev"],
                         scale=1000.0, slots=SLOTS, detector=sp or bk["sp"], image_hw=HW,
                         variable_counts=variable_counts)
    imgs = bk["imgs"] if imgs is None else imgs
    for s in range(SLOTS):
        pipe.set_images(imgs[s * B:(s + 1) * B], slot=s)
    pipe.K.copy_(torch.as_tensor(bk["K"]).expand_as(pipe.K))
    pipe.pose_gt.copy_(torch.as_tensor(bk["pose"]).expand_as(pipe.pose_gt))
    return pipe


def _check_against_run_frames(pipe, bk, what):
    for s, o in enumerate(pipe.slots):
        assert o.det_counts.cpu().tolist() == bk["counts"][s * B:(s + 1) * B]
        for i in range(B):
            f, c = s * B + i, bk["counts"][s * B + i]
            ref = bk["preds"][f]
            m0 = np.full(N1, -1, np.int64)
            s0 = np.zeros(N1, np.float32)
            m0[:c], s0[:c] = ref["matches0"], ref["matching_scores0"]
            got = {"matches0": o.matches0[i].cpu().numpy(), "matches1": o.matches1[i].cpu().numpy(),
                   "matching_scores0": o.mscores0[i].cpu().numpy(),
                   "matching_scores1": o.mscores1[i].cpu().numpy()}
            assert_pred_equal(got, {**ref, "matches0": m0, "matching_scores0": s0},
                              f"{what} frame {f} c={c}")
            assert int(o.status[i].cpu()) == 0
            assert int(o.n_inliers[i].cpu()) == bk["poses"][f][1]
            np.testing.assert_allclose(o.pose[i].cpu().numpy(), bk["poses"][f][0], atol=1e-6,
                                       err_msg=f"{what} frame {f} pose")


def _clear(pipe):
    for o in pipe.slots:
        for k in ("pose", "matches0", "matches1", "mscores0", "mscores1", "n_inliers"):
            getattr(o, k).zero_()
        o.status.fill_(-1)


def test_variable_counts_pipeline_equals_run_frames(bank):
    pipe = _pipeline(bank, True)
    for s in range(SLOTS):                       # eager, one step per slot
        pipe.enqueue(s)
    torch.cuda.synchronize()
    _check_against_run_frames(pipe, bank, "eager")
    graphs = pipe.capture_stages()               # unstaged, from captured graphs
    _clear(pipe)
    pipe.run_stream(2 * SLOTS, graphs=graphs)
    torch.cuda.synchronize()
    _check_against_run_frames(pipe, bank, "graphs")
    graphs = pipe.capture_stages(staged=True)    # staged: the input stage behind its detector
    pipe.prime_inputs()
    _clear(pipe)
    pipe.run_stream(2 * SLOTS + 1, graphs=graphs, staged=True)
    torch.cuda.synchronize()
    _check_against_run_frames(pipe, bank, "staged graphs")


def test_a_captured_pipeline_follows_new_images(bank):
    """The counts are read on the device: the same graphs, replayed after the slots' images were
    swapped, match the swapped frames at their own counts."""
    pipe = _pipeline(bank, True)
    graphs = pipe.capture_stages()
    pipe.run_stream(SLOTS, graphs=graphs)
    torch.cuda.synchronize()
    order = [2, 3, 0, 1]
    swapped = {**bank, "counts": [bank["counts"][j] for j in order],
               "preds": [bank["preds"][j] for j in order],
               "poses": [bank["poses"][j] for j in order]}
    for s in range(SLOTS):
        pipe.set_images(bank["imgs"][order[s * B:(s + 1) * B]], slot=s)
    pipe.run_stream(SLOTS, graphs=graphs)
    torch.cuda.synchronize()
    _check_against_run_frames(pipe, swapped, "swapped images")


def test_variable_counts_off_on_a_full_bank_gives_todays_bits(bank):
    """Whole images at the default threshold: every frame fills its top-k; the default pipeline
    (variable_counts=False, the uniform calls) and the counts pipeline give the same bits."""
    dev = bank["dev"]
    sp = _detector(0.005, dev, bank["spsd"])
    imgs = np.stack([synthetic.superpoint_image(*HW, s) for s in (10, 11, 12, 13)])
    outs = []
    for vc in (False, True):
        pipe = _pipeline(bank, vc, sp, imgs)
        assert pipe.variable_counts is vc
        graphs = pipe.capture_stages()
        pipe.run_stream(SLOTS, graphs=graphs)
        torch.cuda.synchronize()
        assert all(o.det_counts.cpu().tolist() == [N1] * B for o in pipe.slots)
        outs.append([{k: getattr(o, k).cpu().numpy().copy()
                      for k in ("matches0", "matches1", "mscores0", "mscores1", "pose",
                                "n_inliers", "status", "R_err", "t_err")} for o in pipe.slots])
    for a, b in zip(*outs):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (outs[0][0]["matches0"][0] > -1).sum() > 50     # (slot 0, sample 0: the object's image)

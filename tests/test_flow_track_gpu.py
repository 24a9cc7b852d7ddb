"""tracker.flow_track (BATracker.flow_track, :295-356) on the synthetic pairs of
tests/flow_cases.py: flow -> ransac_PnP -> reprojection distance -> the acceptance rule.

The scene is chosen so that the numpy oracle's flow fed to the C PnP oracle already passes the
rule; test_oracle_chain_passes_the_rule checks that without a GPU (measured there: 281 inliers of
300, kpt_dist 1.20 px, 0.05 cm, 0.70 deg).  The GPU tests assert no more than the rule itself."""
import numpy as np
import pytest

import flow_cases
import lk_oracle
from onepose_amd import tracker


def oracle_chain(which):
    from oracle import pnp_oracle
    kf, q = flow_cases.pair(which)
    out, st, _ = lk_oracle.calc_optical_flow_pyr_lk(kf["im_path"], q["im_path"], kf["mkpts2d"],
                                                    15, 2)
    valid = np.where(st == 1)
    p2, p3 = out[valid], kf["mkpts3d"][valid]
    status, pose, _, n_in, _ = pnp_oracle.pnp_ransac(p2, p3, q["K_crop"])
    kpt_dist = np.mean(np.linalg.norm(tracker.project(p3, q["K_crop"], pose) - p2, axis=1))
    trans, rot = tracker.cm_degree_5_metric(pose, q["pose_gt"][:3])
    print(f"{which}: {len(valid[0])} tracked, PnP status {status}, {n_in} inliers, kpt_dist "
          f"{kpt_dist:.3f} px, {trans:.3f} cm, {rot:.3f} deg")
    return status, kpt_dist, trans, rot


def test_oracle_chain_passes_the_rule():
    status, kpt_dist, trans, rot = oracle_chain("near")
    assert status == 0 and trans <= 7 and rot <= 7 and kpt_dist < 10
    status, kpt_dist, trans, rot = oracle_chain("far")
    assert not (status == 0 and trans <= 7 and rot <= 7 and kpt_dist < 10)


@pytest.mark.gpu
def test_flow_track_accepts_a_near_pose(device):
    kf, q = flow_cases.pair("near")
    assert "mkpts3d" not in q and "mkpts2d" not in q
    pose, kpt_dist, accepted = tracker.flow_track(q, kf)
    trans, rot = tracker.cm_degree_5_metric(pose[:3], q["pose_gt"][:3])
    print(f"near: kpt_dist {kpt_dist:.3f} px, {trans:.3f} cm, {rot:.3f} deg")
    assert accepted
    assert pose.shape == (4, 4) and trans <= 7 and rot <= 7 and kpt_dist < 10
    n = len(q["mkpts2d"])
    assert n > flow_cases.N_POINTS // 2 and q["mkpts2d"].shape == (n, 2)
    assert q["mkpts3d"].shape == (n, 3)
    # the written points are the tracked subset, in order
    new, valid = tracker.kpt_flow_track(kf["im_path"], q["im_path"], kf["mkpts2d"])
    assert np.array_equal(q["mkpts2d"], new[valid])
    assert np.array_equal(q["mkpts3d"], kf["mkpts3d"][valid])
    # the keyframe's prebuilt pyramid gives the same answer
    import torch
    kf2, q2 = flow_cases.pair("near")
    kf2["lk_pyramid"] = tracker.build_lk_pyramid(torch.from_numpy(kf2["im_path"]).to(device))
    pose2, kpt_dist2, accepted2 = tracker.flow_track(q2, kf2)
    assert accepted2 and np.array_equal(pose2, pose) and kpt_dist2 == kpt_dist


@pytest.mark.gpu
def test_flow_track_rejects_a_far_pose(device):
    kf, q = flow_cases.pair("far")
    pose, kpt_dist, accepted = tracker.flow_track(q, kf)
    assert not accepted
    assert "mkpts3d" not in q and "mkpts2d" not in q
    assert pose.shape == (4, 4)

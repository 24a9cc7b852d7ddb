"""The bundle adjustment and triangulation cases shared by tests/golden/make_golden_ba.py (which
records them) and the tests (which regenerate the inputs from the recorded seed)."""
import hashlib
import os

import numpy as np

from onepose_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (make_ba_problem arguments, initial radius, base seed).  Shapes are (C, P, N).
SOLVE_CASES = {
    "one": (dict(n_cams=1, n_points=1, n_obs=1), 1e4, 100),
    "tiny": (dict(n_cams=3, n_points=7, n_obs=15), 1e4, 200),
    "zero_rot": (dict(n_cams=6, n_points=60, n_obs=250, zero_rot_cam=True), 1e4, 300),
    # 21 of 40 cameras and 280 of 300 points carry the observations
    "window": (dict(n_cams=40, n_points=300, n_obs=4400, active_cams=21, observed_points=280),
               1e4, 400),
    # one below, at and above the 256 observations of one workgroup of the per-observation kernels
    "n255": (dict(n_cams=5, n_points=80, n_obs=255, once_point=True), 1e4, 500),
    "n256": (dict(n_cams=5, n_points=80, n_obs=256), 1e4, 600),
    "n257": (dict(n_cams=5, n_points=80, n_obs=257, duplicate=True), 1e4, 700),
    "limit": (dict(n_cams=24, n_points=50, n_obs=600), 1e4, 800),   # A = the limit
    # close cameras, a large perturbation (36 mm, 0.12 rad) and a wide trust region: the oracle's
    # trajectory has a rejected step (4 of the first 20 seeds qualify; none does at perturb <= 5)
    "reject": (dict(n_cams=6, n_points=60, n_obs=250, dist=(0.11, 0.16), perturb=12.0), 1e6, 900),
}
LIN_CASES = {"lin_zero_rot": (dict(n_cams=6, n_points=60, n_obs=250, zero_rot_cam=True), 300),
             "lin_tiny": (dict(n_cams=3, n_points=7, n_obs=15), 200)}
TRI_SIZES = (1, 63, 64, 65, 1000)
TRI_SEED = 50
MAX_SEEDS = 40
KEYS = ("points", "cam_pose", "features", "ptIdx", "camIdx")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def problem(name, seed):
    kw = (SOLVE_CASES.get(name) or LIN_CASES[name])[0]
    return synthetic.make_ba_problem(seed, **kw)


def problem_sha(prob):
    return sha(*[prob[k] for k in KEYS])


def load_solve(name, g):
    """(problem, radius, expectations) of a recorded solve case; the inputs are regenerated from
    the seed and their digest compared."""
    seed = int(g[f"{name}_seed"])
    prob = problem(name, seed)
    assert problem_sha(prob) == str(g[f"{name}_sha"]), "synthetic inputs changed"
    exp = {k: g[f"{name}_{k}"] for k in ("points", "cam_pose", "info", "tol")}
    return prob, SOLVE_CASES[name][1], exp


def tri_inputs(n):
    d = synthetic.make_triangulation_inputs(n, TRI_SEED + n)
    P1 = d["K1"] @ np.linalg.inv(d["Tcw1"])[:3]
    P2 = d["K2"] @ np.linalg.inv(d["Tcw2"])[:3]
    return d, P1, P2


def parse_index(buf, N, C, P):
    """The arrays of onepose_ba_build_index's output (int32 words: an 8-word header magic, N, C,
    P, A, Pa, 0, 0; act_cams [C]; act_pts [P]; cam_start [C+1]; pt_start [P+1]; cam_order [N];
    pt_order [N]), the lists cut to their active lengths."""
    w = np.frombuffer(np.ascontiguousarray(buf).tobytes(), dtype=np.int32)
    head, off = w[:8], 8
    out = {"head": head}
    A, Pa = int(head[4]), int(head[5])
    for name, n, used in (("act_cams", C, A), ("act_pts", P, Pa), ("cam_start", C + 1, A + 1),
                          ("pt_start", P + 1, Pa + 1), ("cam_order", N, N), ("pt_order", N, N)):
        out[name] = w[off:off + used]
        out[name + "_offset"] = off
        off += n
    return out


GUARD = 256


class Guarded:
    """A device buffer followed by GUARD bytes of 0xA5 that must survive."""

    def __init__(self, dev, nbytes=None, data=None, dtype=None):
        import torch
        dtype = dtype or torch.float64
        if data is not None:
            src = torch.from_numpy(np.ascontiguousarray(data))
            nbytes, dtype = src.numel() * src.element_size(), src.dtype
        self.raw = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.t = self.raw[:nbytes].view(dtype)
        if data is not None:
            self.t.copy_(src.reshape(-1))

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def numpy(self, shape=None):
        a = self.t.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def intact(self):
        return bool((self.raw[self.nbytes:] == 0xA5).all())

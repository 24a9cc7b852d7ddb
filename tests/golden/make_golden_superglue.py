"""Golden fixtures of the SuperGlue matcher, from the reference itself.

Run in the build container, where /root/reference exists (it never exists on the GPU box):

    python tests/golden/make_golden_superglue.py [name ...]

With names, only those fixtures are written (the others are left as they are); without, all.
``--search name ...`` writes nothing: it prints, for each trained-like case, the first input seed
from 0 that meets the three conditions below (how the seeds in TRAINED were chosen).

What is imported from the reference (read-only, nothing copied): the module
src/models/matchers/SuperGlue/superglue.py -- its ``SuperGlue`` class, run in fp32 on the CPU on
onepose_amd.synthetic's seeded weights and inputs.  Its ``log_optimal_transport`` is wrapped to
record the log assignment it returns (the forward does not expose it).

Each fixture holds the four outputs, ``log_assignment``, the config entries used and SHA-256
digests of the inputs and weights (the tests regenerate both from the seeds and compare).
The "trained-like" cases (TRAINED) use BatchNorms with a non-trivial affine part, a bin_score
other than 1 and two non-square images of different sizes; their fixtures also record
``affine_bn``, ``bin_score``, ``image_hw0`` and ``image_hw1``.
Before a fixture is written the generator asserts that at least 25% of image 0's points are
matched, that a float64 run of the reference gives identical indices, and that no reference
score lies within 1e-4 of the threshold: so the exact-index contract of tests/parity.py applies
without its threshold exemption.
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from onepose_amd import synthetic  # noqa: E402

THR = 0.2
WEIGHT_SEED = 11
# name -> (n0, n1, batch, shared1, sinkhorn iterations, input seed)
CASES = {
    "superglue_s": (65, 33, 1, False, 20, 1),
    "superglue_m": (300, 257, 1, False, 100, 2),
    "superglue_b3": (130, 200, 3, True, 50, 3),
}
# trained-like: affine BatchNorm, BIN_SCORE; name -> (..., input seed, image0 (h, w), image1 (h, w))
# Each input seed is the first, counting up from 0, that meets the generator's three conditions
# (--search); seed 0 meets them in all three cases.
# BIN_SCORE: the synthetic weights' scores all lie in 60 .. 120 (final_proj is 20 x orthogonal), so
# a dustbin score near the trained 2.37 is e^-60 below every score and the assignment does not
# depend on it at all; 85.3457 lies between the unmatched and the matched rows' best scores, where
# the dustbin competes as it does in the trained network.
BIN_SCORE = 85.3457
TRAINED = {
    "superglue_t_s": (65, 33, 1, False, 20, 0, (480, 640), (384, 512)),
    "superglue_t_m": (300, 257, 1, False, 100, 0, (480, 640), (640, 360)),
    "superglue_t_b2": (130, 200, 2, True, 50, 0, (384, 512), (480, 640)),
}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load_reference():
    path = os.path.join(REF, "src/models/matchers/SuperGlue/superglue.py")
    spec = importlib.util.spec_from_file_location("ref_superglue", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(mod, sd, data, iters, dtype):
    model = mod.SuperGlue({"sinkhorn_iterations": iters, "match_threshold": THR})
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model = model.eval().to(dtype)
    B = data["descriptors0"].shape[0]
    td = {}
    for k, v in data.items():
        t = torch.as_tensor(v)
        if t.shape[0] != B:                      # the shared side, materialised for the reference
            t = t.expand(B, *t.shape[1:]).contiguous()
        td[k] = t.to(dtype)
    seen = {}
    orig = mod.log_optimal_transport

    def recording(scores, alpha, iters):
        z = orig(scores, alpha, iters)
        seen["z"] = z
        return z

    mod.log_optimal_transport = recording
    try:
        with torch.no_grad():
            out = model(td)
    finally:
        mod.log_optimal_transport = orig
    res = {k: v.numpy() for k, v in out.items()}
    res["log_assignment"] = seen["z"].numpy()
    return res


def case_inputs(name, seed=None):
    """(state dict, inputs, iterations, input seed, fields only a trained-like fixture has)."""
    if name in CASES:
        n0, n1, batch, shared1, iters, s = CASES[name]
        sd = synthetic.superglue_state_dict(WEIGHT_SEED)
        data = synthetic.make_superglue_inputs(n0, n1, seed=s if seed is None else seed,
                                               batch=batch, shared1=shared1)
        return sd, data, iters, s if seed is None else seed, {}
    n0, n1, batch, shared1, iters, s, hw0, hw1 = TRAINED[name]
    s = s if seed is None else seed
    sd = synthetic.superglue_state_dict(WEIGHT_SEED, affine_bn=True, bin_score=BIN_SCORE)
    data = synthetic.make_superglue_inputs(n0, n1, seed=s, batch=batch, shared1=shared1,
                                           image_hw0=hw0, image_hw1=hw1)
    return sd, data, iters, s, dict(affine_bn=1, bin_score=BIN_SCORE, image_hw0=np.array(hw0),
                                    image_hw1=np.array(hw1))


def check_case(mod, name, sd, data, iters):
    """The three conditions; returns (fp32 result, matched fraction, fp32-fp64 score difference)."""
    r32 = run_reference(mod, sd, data, iters, torch.float32)
    r64 = run_reference(mod, sd, data, iters, torch.float64)
    frac = (r32["matches0"] > -1).mean(axis=1)
    assert frac.min() >= 0.25, f"{name}: only {frac} of image 0 matched"
    for k in ("matches0", "matches1"):
        assert np.array_equal(r32[k], r64[k]), f"{name}: fp32 and fp64 {k} differ"
    for k in ("matching_scores0", "matching_scores1"):
        gap = np.abs(r32[k] - THR).min()
        assert gap > 1e-4, f"{name}: a score within {gap} of the threshold"
    dscore = max(np.abs(r32[k] - r64[k]).max() for k in ("matching_scores0", "matching_scores1"))
    return r32, frac, dscore


def search_seed(mod, name):
    for seed in range(64):
        sd, data, iters, _, _ = case_inputs(name, seed)
        try:
            _, frac, dscore = check_case(mod, name, sd, data, iters)
        except AssertionError as e:
            print(f"{name}: seed {seed} rejected: {e}")
            continue
        print(f"{name}: first valid input seed {seed} (matched {frac}, score diff {dscore:.2e})")
        return seed
    raise SystemExit(f"{name}: no valid seed below 64")


def make_case(mod, name):
    sd, data, iters, seed, extra = case_inputs(name)
    n0, n1 = data["keypoints0"].shape[1], data["keypoints1"].shape[1]
    batch = data["keypoints0"].shape[0]
    shared1 = data["keypoints1"].shape[0] != batch
    r32, frac, dscore = check_case(mod, name, sd, data, iters)
    out = {k: r32[k] for k in ("matches0", "matches1", "matching_scores0", "matching_scores1",
                               "log_assignment")}
    out.update(sinkhorn_iterations=iters, match_threshold=THR, weight_seed=WEIGHT_SEED,
               input_seed=seed, shape=np.array([n0, n1, batch, int(shared1)]),
               weights_sha=synthetic.state_dict_sha(
                   {k: v for k, v in sd.items() if v.dtype == np.float32}),
               inputs_sha=sha(*[data[k] for k in sorted(data)]), **extra)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(f"{name}: matched {frac}, fp32 vs fp64 score diff {dscore:.2e}, "
          f"{os.path.getsize(os.path.join(HERE, name + '.npz'))} bytes")


def make_empty(mod, sd):
    data = synthetic.make_superglue_inputs(4, 7, seed=4)
    data = dict(data, descriptors0=data["descriptors0"][:, :, :0],
                keypoints0=data["keypoints0"][:, :0], scores0=data["scores0"][:, :0])
    out = run_reference_empty(mod, sd, data)
    np.savez_compressed(os.path.join(HERE, "superglue_empty.npz"), **out)
    print("superglue_empty:", {k: (v.dtype, v.shape) for k, v in out.items()})


def run_reference_empty(mod, sd, data):
    model = mod.SuperGlue({})
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    with torch.no_grad():
        out = model.eval()({k: torch.as_tensor(v) for k, v in data.items()})
    return {k: v.numpy() for k, v in out.items()}


def main():
    assert os.path.isdir(REF), "the reference is only available in the build container"
    torch.manual_seed(0)
    mod = load_reference()
    args = sys.argv[1:]
    if args and args[0] == "--search":
        for name in args[1:] or TRAINED:
            search_seed(mod, name)
        return
    names = args or [*CASES, *TRAINED, "superglue_empty"]
    for name in names:
        if name == "superglue_empty":
            make_empty(mod, synthetic.superglue_state_dict(WEIGHT_SEED))
        else:
            make_case(mod, name)


if __name__ == "__main__":
    main()

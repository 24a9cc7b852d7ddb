"""Golden fixtures of the NearestNeighbour matcher, from the reference itself.

Run in the build container, where /root/reference exists (it never exists on the GPU box):

    python tests/golden/make_golden_nn.py

What is imported from the reference (read-only, nothing copied): the module
src/models/matchers/nn/nearest_neighbour.py -- its ``NearestNeighbour`` class, run in fp32 on the
CPU on onepose_amd.synthetic.make_nn_inputs.

Each fixture holds, for each of the four configurations, the four outputs of every batch entry
(``c<i>_matches0`` ...), the configurations as JSON, the seed taken, the shape and a SHA-256
digest of the inputs (the tests regenerate them from the seed and compare; the inputs are not
stored).  Before a fixture is written the generator asserts, in float64, that

* every row's and every column's best-minus-second similarity gap is >= 2e-5 (fp32 einsum differs
  from float64 by under 5e-7 at d = 256),
* every ratio or distance decision has |lhs - rhs| >= 1e-3,
* a float64 run of the reference gives identical indices,
* at least 15 % of rows are matched under every configuration,

so the exact-index contract of tests/parity.py applies with no exemption.  Seeds are tried in
order from the case's base, at most 32; the first that meets the asserts is recorded.
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from onepose_amd import synthetic  # noqa: E402

CONFIGS = [
    {},
    {"ratio_threshold": 0.8},
    {"distance_threshold": 0.7},
    {"ratio_threshold": 0.9, "distance_threshold": 0.9, "do_mutual_check": False},
]
# name -> (n0, n1, batch, shared1, d, base seed)
CASES = {
    "nn_s": (65, 33, 1, False, 256, 100),
    "nn_m": (300, 257, 1, False, 256, 200),
    "nn_b3": (130, 200, 3, True, 256, 300),
}
MIN_GAP, MIN_SLACK, MIN_MATCHED, MAX_SEEDS = 2e-5, 1e-3, 0.15, 32
KEYS = ("matches0", "matches1", "matching_scores0", "matching_scores1")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load_reference():
    path = os.path.join(REF, "src/models/matchers/nn/nearest_neighbour.py")
    spec = importlib.util.spec_from_file_location("ref_nearest_neighbour", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tensors(data, dtype):
    B = data["descriptors0"].shape[0]
    out = {}
    for k, v in data.items():
        t = torch.as_tensor(v)
        if t.shape[0] != B:                      # the shared side, materialised for the reference
            t = t.expand(B, *t.shape[1:]).contiguous()
        out[k] = t.to(dtype)
    return out


def run_reference(mod, data, conf, dtype):
    with torch.no_grad():
        out = mod.NearestNeighbour(dict(conf))(tensors(data, dtype))
    return {k: out[k].numpy() for k in KEYS}


def margins(data, conf):
    """(smallest top-2 gap, smallest decision slack) over rows and columns, in float64."""
    td = tensors(data, torch.float64)
    sim = torch.einsum("bdn,bdm->bnm", td["descriptors0"], td["descriptors1"]).numpy()
    gap, slack = np.inf, np.inf
    for s in (sim, sim.transpose(0, 2, 1)):
        top = -np.sort(-s, axis=-1)[..., :2]
        gap = min(gap, (top[..., 0] - top[..., 1]).min())
        d0, d1 = 2 * (1 - top[..., 0]), 2 * (1 - top[..., 1])
        if conf.get("ratio_threshold"):
            slack = min(slack, np.abs(d0 - conf["ratio_threshold"] ** 2 * d1).min())
        if conf.get("distance_threshold"):
            slack = min(slack, np.abs(d0 - conf["distance_threshold"] ** 2).min())
    return gap, slack


def try_seed(mod, name, seed):
    n0, n1, batch, shared1, d, _ = CASES[name]
    data = synthetic.make_nn_inputs(n0, n1, seed, batch=batch, shared1=shared1, d=d)
    out, notes = {}, []
    for i, conf in enumerate(CONFIGS):
        gap, slack = margins(data, conf)
        if gap < MIN_GAP or slack < MIN_SLACK:
            return None, f"seed {seed}: config {i} gap {gap:.2e} slack {slack:.2e}"
        r32 = run_reference(mod, data, conf, torch.float32)
        r64 = run_reference(mod, data, conf, torch.float64)
        for k in ("matches0", "matches1"):
            if not np.array_equal(r32[k], r64[k]):
                return None, f"seed {seed}: config {i} fp32 and fp64 {k} differ"
        frac = (r32["matches0"] > -1).mean(axis=1).min()
        if frac < MIN_MATCHED:
            return None, f"seed {seed}: config {i} only {frac:.2f} of rows matched"
        assert r32["matches0"].dtype == np.int64 and r32["matching_scores0"].dtype == np.float32
        for k in KEYS:
            out[f"c{i}_{k}"] = r32[k]
        notes.append(f"c{i}: gap {gap:.1e} slack {slack:.1e} matched {frac:.2f}")
    out.update(configs=json.dumps(CONFIGS), input_seed=seed,
               shape=np.array([n0, n1, batch, int(shared1), d]),
               inputs_sha=sha(*[data[k] for k in sorted(data)]))
    return out, "; ".join(notes)


def make_case(mod, name):
    base = CASES[name][-1]
    for seed in range(base, base + MAX_SEEDS):
        out, note = try_seed(mod, name, seed)
        if out is None:
            print(f"{name}: rejected {note}")
            continue
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seed {seed}, {note}, {os.path.getsize(path)} bytes")
        return
    raise AssertionError(f"{name}: none of {MAX_SEEDS} seeds from {base} meets the asserts")


def main():
    assert os.path.isdir(REF), "the reference is only available in the build container"
    mod = load_reference()
    for name in CASES:
        make_case(mod, name)


if __name__ == "__main__":
    main()

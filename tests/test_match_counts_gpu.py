"""Per-sample keypoint counts for the 2D-3D matcher on the GPU (include/onepose_match_counts.h).

Every case of tests/match_counts_cases.py (its docstring lists which kernel path each holds: the
32x128, 128x128W8 and 128x128 QKV tiles, both KV fold paths, two first-level InstanceNorm groups,
the row edges at 32 / 64 / 128 and a single token, an empty sample) is held, sample by sample,
against oracle/matcher_np.py run alone on that sample's first c keypoints, under tests/parity.py's
bars: indices exact, scores and conf within ATOL = 2e-5, and the threshold exemption capped at 0
rows (tests/test_match_counts_host.py::test_seed_margins: the smallest |oracle score - 0.2| over
all cases is 3.838e-04).  Then the contract's bit-for-bit clauses: padding is harmless, NULL / full
counts give the uniform entry's bits, stage ranges compose, a captured graph follows counts2d,
runs repeat, refusals write nothing; and the module's ``keypoints2d_counts`` key."""
import numpy as np
import pytest
import torch

import match_counts_cases as C
from onepose_amd import _lib, matcher
from onepose_amd.prepared import PreparedObject
from parity import ATOL, assert_pred_equal, assert_scores_close

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4      # ONEPOSE_ERR_*
OUTS = ("m0", "m1", "s0", "s1", "conf")


class Rig:
    """One case's object prepared once (flags / descriptor dtype as asked), and the two cached
    entry points called on it directly."""

    def __init__(self, name, device, flags=0, f16=False):
        self.name, self.dev, self.flags, self.f16 = name, device, flags, f16
        self.data, self.counts = C.inputs(name)
        c = C.CASES[name]
        self.B, self.n1 = c["B"], c["n1"]
        self.m = matcher.from_state_dict(C.state_dict())
        self.w = self.m.packed_weights(device)
        dt = torch.float16 if f16 else torch.float32
        self.dt = _lib.DT_F16 if f16 else _lib.DT_F32
        d3 = torch.from_numpy(self.data["descriptors3d_db"][0]).to(device, dt).contiguous()
        lv = torch.from_numpy(self.data["descriptors2d_db"][0]).to(device, dt).contiguous()
        self.obj = PreparedObject(self.w, d3, lv, 0, flags)
        self.desc2d = torch.from_numpy(self.data["descriptors2d_query"]).to(device, dt).contiguous()
        torch.cuda.synchronize()

    def ws_bytes(self, with_conf=True):
        return _lib.call("onepose_match_counts_workspace_bytes", batch=self.B, n1=self.n1, n3=C.N3,
                         num_leaf=C.L, with_conf=int(with_conf), precision=0)

    def outputs(self, with_conf=True):
        B, n1, dev = self.B, self.n1, self.dev
        o = dict(m0=torch.full((B, n1), -7, dtype=torch.int64, device=dev),
                 m1=torch.full((B, C.N3), -7, dtype=torch.int64, device=dev),
                 s0=torch.full((B, n1), -7.0, device=dev),
                 s1=torch.full((B, C.N3), -7.0, device=dev))
        o["conf"] = torch.full((B, n1, C.N3), -7.0, device=dev) if with_conf else None
        return o

    def call(self, o, ws, counts="case", entry="counts", desc2d=None, stages=(0, 15),
             precision=0, ws_bytes=None, **over):
        """The status of one call: entry "counts" (counts: "case", None, or a device tensor) or
        "uniform" (onepose_match_cached_stages)."""
        if isinstance(counts, str):
            counts = torch.from_numpy(self.counts).to(self.dev)
        args = dict(packed_weights=self.w, desc2d=self.desc2d if desc2d is None else desc2d,
                    desc_dtype=self.dt, desc2d_bstride=256 * self.n1, object_cache=self.obj.cache,
                    leaves_prepared=self.obj.leaves_pm, prepared_bstride=0, batch=self.B,
                    n1=self.n1, n3=C.N3, num_leaf=C.L, scale_factor=0.07, match_threshold=0.2,
                    precision=precision, object_flags=self.flags, matches0=o["m0"],
                    matches1=o["m1"], mscores0=o["s0"], mscores1=o["s1"], conf=o["conf"],
                    workspace=ws, workspace_bytes=ws.numel() if ws_bytes is None else ws_bytes,
                    first_stage=stages[0], last_stage=stages[1], stream=_lib.stream_ptr(self.dev))
        args.update(over)
        if entry == "uniform":
            return _lib.call("onepose_match_cached_stages", **args)
        self._keep = counts          # (alive until the stream has run the call)
        return _lib.call("onepose_match_cached_counts_stages", counts2d=counts, **args)

    def run(self, with_conf=True, fill=0, **kw):
        """Outputs of one whole call as numpy arrays (workspace pre-filled with byte `fill`)."""
        o = self.outputs(with_conf)
        ws = torch.full((self.ws_bytes(with_conf),), fill, dtype=torch.uint8, device=self.dev)
        rc = self.call(o, ws, **kw)
        assert rc == 0, _lib.load().onepose_last_error().decode()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


_RIGS = {}


def rig(name, device, flags=0, f16=False):
    key = (name, flags, f16)
    if key not in _RIGS:
        _RIGS[key] = Rig(name, device, flags, f16)
    return _RIGS[key]


def same_bits(a, b, what, keys=None):
    for k in keys or a:
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8),
                                      err_msg=f"{what}: {k}")


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_each_sample_equals_the_oracle_at_its_own_count(name, device):
    """Every case and sample: the oracle alone on the first c keypoints, padded (-1 / 0 / zero
    conf rows past c), under parity.py's bars with no threshold exemption.  Reaches: edges / fold5
    kv_reduce + m_fold on 32x128; fused / empty / groups_* kv_fold256; groups_* two first-level
    InstanceNorm groups; wide_w8 TILE_128x128W8 and wide_128 TILE_128x128 on the 2D side's QKV
    of layers 1-2 (wide_128 also TILE_128x128W8 on both sides' QKV of the later layers)."""
    r = rig(name, device)
    got = r.run()
    exempt = 0
    for b, cnt in enumerate(r.counts):
        if b in C.checked(name):
            ref, rconf = C.padded_reference(name, b)
            g = {"matches0": got["m0"][b], "matches1": got["m1"][b],
                 "matching_scores0": got["s0"][b], "matching_scores1": got["s1"][b]}
            exempt += assert_pred_equal(g, ref, f"{name}[{b}] c={cnt}")
            assert_scores_close(got["conf"][b], rconf, f"{name}[{b}] conf", ATOL)
        # past the count, exactly: no match, zero score, zero conf rows; no column names such a row
        assert (got["m0"][b, cnt:] == -1).all() and (got["s0"][b, cnt:] == 0).all()
        assert not got["conf"][b, cnt:].any()
        assert (got["m1"][b] < cnt).all()
        if cnt == 0:
            assert (got["m1"][b] == -1).all() and not got["s1"][b].any()
    assert exempt == 0


def test_an_empty_sample_leaves_its_neighbours_unchanged(device):
    """`empty` = counts (160, 0, 160): the full samples give the uniform entry's bits."""
    r = rig("empty", device)
    got, uni = r.run(), r.run(entry="uniform")
    for b in (0, 2):
        same_bits({k: got[k][b] for k in OUTS}, {k: uni[k][b] for k in OUTS}, f"sample {b}")


# ---------------------------------------------------------------- 2. padding is harmless
@pytest.mark.parametrize("name", ["edges", "fused", "wide_w8"])
def test_padding_content_and_workspace_do_not_reach_the_outputs(name, device):
    r = rig(name, device)
    base = r.run()
    for junk in (float("nan"), 1e30):
        d = r.desc2d.clone()
        for b, cnt in enumerate(r.counts):
            d[b, :, int(cnt):] = junk
        same_bits(base, r.run(desc2d=d), f"{junk} past the counts")
    z = r.desc2d.clone()
    for b, cnt in enumerate(r.counts):
        z[b, :, int(cnt):] = 0
    same_bits(base, r.run(desc2d=z), "zeros past the counts")
    same_bits(base, r.run(fill=0xFF), "workspace of 0xFF bytes")
    same_bits(base, r.run(with_conf=False, fill=0xFF), "no conf, 0xFF", ("m0", "m1", "s0", "s1"))


@pytest.mark.parametrize("name,keep", [("edges", 1), ("fused", 0), ("fold5", 2)])
def test_a_sample_does_not_depend_on_the_others(name, keep, device):
    """Sample `keep` keeps its bits when the other samples' data and counts change (same maxima)."""
    r = rig(name, device)
    base = r.run()
    d = torch.roll(r.desc2d, 1, dims=2).flip(0).contiguous()      # other frames, shifted
    d[keep] = r.desc2d[keep]
    cnt = np.asarray([(int(c) * 7 + 11) % (r.n1 + 1) for c in r.counts], np.int32)
    cnt[keep] = r.counts[keep]
    other = r.run(desc2d=d, counts=torch.from_numpy(cnt).to(device))
    same_bits({k: base[k][keep] for k in OUTS}, {k: other[k][keep] for k in OUTS}, f"sample {keep}")
    assert not np.array_equal(base["conf"][1 - min(keep, 1)], other["conf"][1 - min(keep, 1)])


# ---------------------------------------------------------------- 3. the uniform entry's bits
@pytest.mark.parametrize("name", ["fused", "fold5"])
@pytest.mark.parametrize("flags", [0, _lib.OBJ_GAT_TABLES])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("with_conf", [True, False])
def test_null_and_full_counts_give_the_uniform_bits(name, flags, f16, with_conf, device):
    r = rig(name, device, flags, f16)
    uni = r.run(with_conf, entry="uniform")
    assert (uni["m0"] > -1).sum() > 20
    full = torch.full((r.B,), r.n1, dtype=torch.int32, device=device)
    over = torch.full((r.B,), r.n1 + 1000, dtype=torch.int32, device=device)   # clamped to n1
    same_bits(uni, r.run(with_conf, counts=None), "NULL counts")
    same_bits(uni, r.run(with_conf, counts=full), "all-full counts")
    same_bits(uni, r.run(with_conf, counts=over), "counts past n1")


@pytest.mark.parametrize("name", ["groups_a", "wide_w8"])
def test_full_counts_give_the_uniform_bits_on_the_other_paths(name, device):
    r = rig(name, device)
    full = torch.full((r.B,), r.n1, dtype=torch.int32, device=device)
    same_bits(r.run(entry="uniform"), r.run(counts=full), "all-full counts")


# ---------------------------------------------------------------- 4. stages, graphs, repeats
@pytest.mark.parametrize("name", ["fused", "edges"])
def test_stage_ranges_compose_as_the_pipeline_splits_them(name, device):
    r = rig(name, device)
    whole = r.run(fill=0xFF)
    o = r.outputs()
    ws = torch.full((r.ws_bytes(),), 0xFF, dtype=torch.uint8, device=device)
    for rng in ((_lib.STAGE_INPUTS, _lib.STAGE_INPUTS),
                (_lib.STAGE_LAYER0, _lib.STAGE_FINAL - 1),
                (_lib.STAGE_FINAL, _lib.STAGE_WINNERS)):
        assert r.call(o, ws, stages=rng) == 0
    torch.cuda.synchronize()
    same_bits(whole, {k: v.cpu().numpy() for k, v in o.items()}, "INPUTS | layers | FINAL..WINNERS")


def test_a_captured_graph_follows_counts_changed_in_place(device):
    r = rig("fused", device)
    cnt = torch.full((r.B,), r.n1, dtype=torch.int32, device=device)
    o = r.outputs()
    ws = torch.zeros(r.ws_bytes(), dtype=torch.uint8, device=device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):          # (warm-up outside the capture)
        assert r.call(o, ws, counts=cnt) == 0
    torch.cuda.current_stream(device).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert r.call(o, ws, counts=cnt) == 0
    g.replay()
    torch.cuda.synchronize()
    full = {k: v.cpu().numpy() for k, v in o.items()}
    same_bits(r.run(counts=cnt.clone()), full, "replay with full counts")
    cnt.copy_(torch.from_numpy(r.counts).to(device))
    g.replay()
    torch.cuda.synchronize()
    same_bits(r.run(), {k: v.cpu().numpy() for k, v in o.items()}, "replay after counts changed")
    assert not np.array_equal(full["conf"], o["conf"].cpu().numpy())


@pytest.mark.parametrize("name", ["edges", "groups_a"])
def test_two_runs_give_the_same_bits(name, device):
    r = rig(name, device)
    a = r.run()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        b = r.run(fill=0x5A)
    same_bits(a, b, "second run, another stream")


# ---------------------------------------------------------------- 5. refusals
def test_refusals_return_their_status_and_write_nothing(device):
    r = rig("fused", device)
    o = r.outputs()
    ws = torch.zeros(r.ws_bytes(), dtype=torch.uint8, device=device)
    err = lambda: _lib.load().onepose_last_error().decode()      # noqa: E731
    for prec in (1, 2):
        assert r.call(o, ws, precision=prec) == UNSUPPORTED and "FP32" in err()
    assert r.call(o, ws, packed_weights=None) == INVALID and "null input" in err()
    assert r.call(o, ws, object_cache=None, matches0=None) == INVALID and "null input" in err()
    assert r.call(o, ws, leaves_prepared=None) == INVALID and "null input" in err()
    for k in ("matches0", "matches1", "mscores0", "mscores1"):
        assert r.call(o, ws, **{k: None}) == INVALID and "null output" in err()
    assert r.call(o, ws, workspace=None) == INVALID and "null workspace" in err()
    assert r.call(o, ws, ws_bytes=r.ws_bytes() - 1) == WORKSPACE and "workspace" in err()
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v == -7).all(), k
    assert r.call(o, ws) == 0            # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert (o["m0"] > -1).sum() > 20


# ---------------------------------------------------------------- 6. the module
def _module_inputs(name, device):
    data, counts = C.inputs(name)
    t = {k: torch.from_numpy(v).to(device) for k, v in data.items()}
    for k in ("descriptors3d_db", "descriptors2d_db", "keypoints3d"):   # one object for the batch
        t[k] = t[k][:1].expand_as(t[k])
    return t, counts


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_module_forward_with_counts_equals_the_per_sample_oracle(dtype, device):
    name = "fused"
    m = matcher.from_state_dict(C.state_dict()).to(device)
    t, counts = _module_inputs(name, device)
    t["keypoints2d_counts"] = torch.from_numpy(counts).to(device, dtype)
    with torch.no_grad():
        pred, conf = m(t)
    torch.cuda.synchronize()
    n1 = C.CASES[name]["n1"]
    assert conf.shape == (len(counts), n1, C.N3) and pred["matches0"].shape == (n1,)
    assert pred["matches0"].dtype == torch.int64 and pred["matching_scores0"].dtype == torch.float32
    ref, _ = C.padded_reference(name, 0)
    assert assert_pred_equal({k: v.cpu().numpy() for k, v in pred.items()}, ref, "pred") == 0
    conf = conf.cpu().numpy()
    for b, cnt in enumerate(counts):
        assert_scores_close(conf[b], C.padded_reference(name, b)[1], f"conf[{b}]", ATOL)
        assert not conf[b, cnt:].any()


def test_module_forward_without_the_key_is_unchanged(device):
    """No key: the uniform forward (the oracle on the padded batch); and a key of full counts
    gives that forward's bits."""
    from oracle import matcher_np as M
    m = matcher.from_state_dict(C.state_dict()).to(device)
    t, counts = _module_inputs("fused", device)
    with torch.no_grad():
        pred, conf = m(t)
        t["keypoints2d_counts"] = torch.full((len(counts),), C.CASES["fused"]["n1"], device=device)
        pred_f, conf_f = m(t)
    torch.cuda.synchronize()
    opred, oconf = M.forward(C.state_dict(), C.inputs("fused")[0])
    assert_pred_equal({k: v.cpu().numpy() for k, v in pred.items()}, opred, "no key")
    assert_scores_close(conf.cpu().numpy(), oconf, "no key conf", ATOL)
    assert torch.equal(conf, conf_f)
    for k in pred:
        assert torch.equal(pred[k], pred_f[k]), k

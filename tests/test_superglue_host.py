"""SuperGlue matcher, host side (no GPU): the float64 oracle against the reference-generated
fixtures (the trained-like ones included: affine BatchNorm, bin_score != 1, non-square images),
the module's state dict, the packer's layout and its BatchNorm folds, the empty branch and the
argument checks of the new entry points."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import parity
import superglue_oracle as oracle
from onepose_amd import _lib, superglue, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# trained-like fixtures: BatchNorm gamma ~ U(0.5, 1.5), beta ~ 0.1 N(0, 1), images 480 x 640 /
# 384 x 512 / 640 x 360 (tests/golden/make_golden_superglue.py's TRAINED) and a bin_score that
# competes with the scores: these weights' scores lie in 60 .. 120, where the trained network's
# 2.37 (or the default 1) is e^-60 below every score and changes no output bit; 85.3457 lies
# between the best scores of unmatched and of matched rows
T_CASES = ("superglue_t_s", "superglue_t_m", "superglue_t_b2")
CASES = ("superglue_s", "superglue_m", "superglue_b3") + T_CASES
T_BIN_SCORE = 85.3457


def load_case(name):
    """(fixture, state dict, inputs) regenerated from the fixture's seeds, digests checked."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    n0, n1, batch, shared1 = (int(x) for x in g["shape"])
    if "affine_bn" in g.files:
        sd = synthetic.superglue_state_dict(int(g["weight_seed"]), affine_bn=bool(g["affine_bn"]),
                                            bin_score=float(g["bin_score"]))
        sizes = dict(image_hw0=tuple(int(x) for x in g["image_hw0"]),
                     image_hw1=tuple(int(x) for x in g["image_hw1"]))
    else:
        sd, sizes = synthetic.superglue_state_dict(int(g["weight_seed"])), {}
    data = synthetic.make_superglue_inputs(n0, n1, seed=int(g["input_seed"]), batch=batch,
                                           shared1=bool(shared1), **sizes)
    h = hashlib.sha256()
    for k in sorted(data):
        h.update(np.ascontiguousarray(data[k]).tobytes())
    assert h.hexdigest() == str(g["inputs_sha"]), "synthetic inputs changed"
    fsd = {k: v for k, v in sd.items() if v.dtype == np.float32}
    assert synthetic.state_dict_sha(fsd) == str(g["weights_sha"]), "synthetic weights changed"
    return g, sd, data


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


_oracle_cache = {}


def oracle_of(name):
    """The float64 oracle's forward of a fixture's inputs (computed once per session)."""
    if name not in _oracle_cache:
        g, sd, data = load_case(name)
        _oracle_cache[name] = oracle.forward(sd, data, iters=int(g["sinkhorn_iterations"]),
                                             thr=float(g["match_threshold"]))
    return _oracle_cache[name]


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_fixture(name):
    g, sd, data = load_case(name)
    thr = float(g["match_threshold"])
    out = oracle_of(name)
    for b in range(out["matches0"].shape[0]):
        got = {k: out[k][b] for k in ("matches0", "matches1", "matching_scores0",
                                      "matching_scores1")}
        ref = {k: g[k][b] for k in got}
        assert parity.assert_pred_equal(got, ref, f"{name}[{b}]", thr=thr) == 0
        parity.assert_scores_close(np.exp(out["log_assignment"][b][:-1, :-1]),
                                   np.exp(g["log_assignment"][b][:-1, :-1]),
                                   f"{name}[{b}] exp(log_assignment)")


def test_trained_like_defaults_leave_the_old_streams_alone():
    """affine_bn / bin_score / image sizes change only what they name."""
    a = synthetic.superglue_state_dict(11)
    b = synthetic.superglue_state_dict(11, affine_bn=True, bin_score=T_BIN_SCORE)
    assert list(a) == list(b)
    n_bn = 0
    for k in a:
        p = k.rsplit(".", 1)[0]
        if p + ".running_mean" in a and k.endswith((".weight", ".bias")):
            n_bn += 1
            assert a[k].shape == b[k].shape and b[k].dtype == np.float32
            if k.endswith(".weight"):
                assert np.all(a[k] == 1) and b[k].min() >= 0.5 and b[k].max() <= 1.5
                assert b[k].std() > 0.2
            else:
                assert np.all(a[k] == 0) and 0.05 < b[k].std() < 0.2
        elif k == "bin_score":
            assert a[k] == np.float32(1.0) and b[k] == np.float32(T_BIN_SCORE)
        else:
            assert np.array_equal(a[k], b[k]), k
    assert n_bn == 2 * 22
    d = synthetic.make_superglue_inputs(9, 7, seed=3)
    e = synthetic.make_superglue_inputs(9, 7, seed=3, image_hw0=(480, 640), image_hw1=(640, 360))
    assert e["image0"].shape == (1, 1, 480, 640) and e["image1"].shape == (1, 1, 640, 360)
    for k in ("descriptors0", "descriptors1", "scores0", "scores1"):
        assert np.array_equal(d[k], e[k])
    for k, (h, w) in (("keypoints0", (480, 640)), ("keypoints1", (640, 360))):
        np.testing.assert_allclose(e[k], d[k] * np.float32([w / 512, h / 512]), rtol=3e-7)


# ablations of the trained-like inputs: each must move the assignment far more than the tolerance
# the GPU tests allow, or those tests could not tell a kernel that ignores what was ablated
def _swap_hw(sd, data):
    return sd, dict(data, image0=data["image0"].transpose(0, 1, 3, 2),
                    image1=data["image1"].transpose(0, 1, 3, 2))


def _zero_beta(sd, data):
    return {k: (np.zeros_like(v) if k.endswith(".bias") and k[:-4] + "running_mean" in sd else v)
            for k, v in sd.items()}, data


def _bin_one(sd, data):
    return dict(sd, bin_score=np.array(1.0, np.float32)), data


@pytest.mark.parametrize("ablate", [_swap_hw, _zero_beta, _bin_one])
@pytest.mark.parametrize("name", [n for n in T_CASES if n != "superglue_t_b2"])
def test_trained_like_fixtures_discriminate(name, ablate):
    g, sd, data = load_case(name)
    full = np.exp(oracle_of(name)["log_assignment"][0][:-1, :-1])
    sd2, data2 = ablate(sd, data)
    if ablate is _zero_beta:
        assert sum(np.any(sd[k] != sd2[k]) for k in sd) == 22
    out = oracle.forward(sd2, data2, iters=int(g["sinkhorn_iterations"]),
                         thr=float(g["match_threshold"]))
    moved = np.abs(np.exp(out["log_assignment"][0][:-1, :-1]) - full).max()
    print(f"{name} {ablate.__name__}: exp(log_assignment) moves by {moved:.3g}")
    assert moved >= 100 * parity.ATOL


def test_state_dict_matches_reference_keys():
    sd = synthetic.superglue_state_dict(0)
    m = superglue.SuperGlue({})
    msd = m.state_dict()
    assert set(msd.keys()) == set(sd.keys())
    for k, v in msd.items():
        assert tuple(v.shape) == tuple(np.asarray(sd[k]).shape), k
    n_ref = sum(np.asarray(v).size for k, v in sd.items() if np.asarray(v).dtype == np.float32
                and "running_" not in k)
    assert sum(p.numel() for p in m.parameters()) == n_ref
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)


def test_config_contract():
    m = superglue.SuperGlue({"match_threshold": 0.3})
    assert m.config["match_threshold"] == 0.3 and m.config["sinkhorn_iterations"] == 100
    assert m.config["keypoint_encoder"] == [32, 64, 128, 256]
    assert m.config["GNN_layers"] == ["self", "cross"] * 9 and m.config["weights"] == "indoor"
    with pytest.raises(NotImplementedError):
        superglue.SuperGlue({"GNN_layers": ["self", "cross"] * 3})
    with pytest.raises(NotImplementedError):
        superglue.SuperGlue({"descriptor_dim": 128})


def test_tensor_names_match_state_dict(lib):
    sd = synthetic.superglue_state_dict(0)
    names = [lib.onepose_superglue_tensor_name(i).decode()
             for i in range(lib.onepose_superglue_num_tensors())]
    assert lib.onepose_superglue_tensor_name(len(names)) is None
    want = [k for k in sd if not k.endswith("num_batches_tracked")]
    assert sorted(names) == sorted(want) and len(set(names)) == len(names)
    for i, k in enumerate(names):
        assert lib.onepose_superglue_tensor_numel(i) == np.asarray(sd[k]).size, k


def pack(lib, sd):
    names = [lib.onepose_superglue_tensor_name(i).decode()
             for i in range(lib.onepose_superglue_num_tensors())]
    host = [np.ascontiguousarray(sd[k], dtype=np.float32).reshape(-1) for k in names]
    arr = (ctypes.c_void_p * len(host))(*[h.ctypes.data for h in host])
    buf = np.zeros(lib.onepose_superglue_packed_bytes() // 4, dtype=np.float32)
    _lib.check(lib.onepose_superglue_pack(arr, len(host), buf.ctypes.data), "superglue_pack")
    return buf


def test_pack_layout(lib):
    """Head-major q/k/v rows, layer 7's BatchNorm + merge fold against float64, bin_score."""
    sd = synthetic.superglue_state_dict(3)
    sd["bin_score"] = np.array(2.375, dtype=np.float32)
    buf = pack(lib, sd)
    ke = 96 + 32 + 2048 + 64 + 8192 + 128 + 256 * 128 + 256 + 65536 + 256 + 512 + 512
    ly = 768 * 256 + 768 + 512 * 512 + 512 + 256 * 512 + 256
    assert buf.size == ke + 18 * ly + 65536 + 256 + 64
    assert buf[ke + 18 * ly + 65536 + 256] == np.float32(2.375)          # bin_score
    assert np.all(buf[ke - 1024:ke - 512] == 0) and np.all(buf[ke - 512:ke] == 1)
    L = 7
    base = ke + L * ly
    p = f"gnn.layers.{L}"
    wqkv = buf[base:base + 768 * 256].reshape(768, 256)
    bqkv = buf[base + 768 * 256:base + 768 * 256 + 768]
    for j in range(3):
        w = sd[f"{p}.attn.proj.{j}.weight"][:, :, 0]
        for h, d in ((0, 0), (1, 5), (3, 63), (2, 17)):
            assert np.array_equal(wqkv[j * 256 + h * 64 + d], w[d * 4 + h])
            assert bqkv[j * 256 + h * 64 + d] == sd[f"{p}.attn.proj.{j}.bias"][d * 4 + h]
    o = base + 768 * 256 + 768
    w1f = buf[o:o + 512 * 512].reshape(512, 512)
    b1f = buf[o + 512 * 512:o + 512 * 512 + 512]
    f = lambda k: np.asarray(sd[f"{p}.{k}"], dtype=np.float64)
    W1, Wm = f("mlp.0.weight")[:, :, 0], f("attn.merge.weight")[:, :, 0]
    s = f("mlp.1.weight") / np.sqrt(f("mlp.1.running_var") + 1e-5)
    C = W1[:, 256:] @ Wm                               # columns in the reference's d*4+h order
    perm = np.array([d * 4 + h for h in range(4) for d in range(64)])
    want_w = s[:, None] * np.concatenate([W1[:, :256], C[:, perm]], axis=1)
    want_b = s * (f("mlp.0.bias") + W1[:, 256:] @ f("attn.merge.bias")
                  - f("mlp.1.running_mean")) + f("mlp.1.bias")
    np.testing.assert_allclose(w1f, want_w, rtol=0, atol=2.0 ** -24 * np.abs(want_w).max())
    np.testing.assert_allclose(b1f, want_b, rtol=0, atol=2.0 ** -24 * np.abs(want_b).max())
    # the keypoint encoder's first layer, in-major, BatchNorm folded
    s1 = (np.float64(sd["kenc.encoder.1.weight"]) /
          np.sqrt(np.float64(sd["kenc.encoder.1.running_var"]) + 1e-5))
    want = (s1[:, None] * np.float64(sd["kenc.encoder.0.weight"][:, :, 0])).T
    np.testing.assert_allclose(buf[:96].reshape(3, 32), want, rtol=0, atol=1e-7)


def test_pack_folds_affine_batchnorm(lib):
    """All 22 BatchNorm folds with gamma != 1 and beta != 0: s = gamma / sqrt(var + eps),
    W' = s W, b' = s (b - mean) + beta (for the layers' MLP: W, b with the merge conv folded in) in
    float64 from the state dict, in the pack's operation order (the merge products are summed over
    k in ascending order, one product and one add each); the packed value is that float64 number
    rounded to fp32 once, so the comparison is exact."""
    sd = synthetic.superglue_state_dict(5, affine_bn=True, bin_score=T_BIN_SCORE)
    buf = pack(lib, sd)
    f = lambda k: np.asarray(sd[k], dtype=np.float64)

    def scale(p):
        assert np.any(sd[p + ".weight"] != 1) and np.any(sd[p + ".bias"] != 0)
        return f(p + ".weight") / np.sqrt(f(p + ".running_var") + 1e-5)

    chans = [3, 32, 64, 128, 256, 256]
    off = 0
    for j in range(5):
        ci, co = chans[j], chans[j + 1]
        W, b = f(f"kenc.encoder.{3 * j}.weight")[:, :, 0], f(f"kenc.encoder.{3 * j}.bias")
        if j < 4:
            p = f"kenc.encoder.{3 * j + 1}"
            s = scale(p)
            W, b = s[:, None] * W, s * (b - f(p + ".running_mean")) + f(p + ".bias")
        got_w = buf[off:off + ci * co]
        got_w = got_w.reshape(ci, co).T if j < 3 else got_w.reshape(co, ci)     # in-major below 3
        assert np.array_equal(got_w, np.float32(W)), f"kenc conv {j} weight"
        got_b = buf[off + ci * co:off + ci * co + co]
        assert np.array_equal(got_b, np.float32(b)), f"kenc conv {j} bias"
        off += ci * co + co
    ke = off + 1024
    ly = 768 * 256 + 768 + 512 * 512 + 512 + 256 * 512 + 256
    perm = np.array([d * 4 + h for h in range(4) for d in range(64)])
    for L in range(18):
        p = f"gnn.layers.{L}"
        o = ke + L * ly + 768 * 256 + 768
        w1f = buf[o:o + 512 * 512].reshape(512, 512)
        b1f = buf[o + 512 * 512:o + 512 * 512 + 512]
        W1, Wm = f(p + ".mlp.0.weight")[:, :, 0], f(p + ".attn.merge.weight")[:, :, 0]
        bm = f(p + ".attn.merge.bias")
        C, cb = np.zeros((512, 256)), np.zeros(512)
        for k in range(256):
            C += W1[:, 256 + k, None] * Wm[None, k, :]
            cb += W1[:, 256 + k] * bm[k]
        s = scale(p + ".mlp.1")
        want_w = s[:, None] * np.concatenate([W1[:, :256], C[:, perm]], axis=1)
        want_b = (s * ((f(p + ".mlp.0.bias") + cb) - f(p + ".mlp.1.running_mean"))
                  + f(p + ".mlp.1.bias"))
        assert np.array_equal(w1f, np.float32(want_w)), f"layer {L} conv 1 weight"
        assert np.array_equal(b1f, np.float32(want_b)), f"layer {L} conv 1 bias"
    assert buf[ke + 18 * ly + 65536 + 256] == np.float32(T_BIN_SCORE)


def test_empty_branch_matches_fixture():
    g = np.load(os.path.join(GOLDEN, "superglue_empty.npz"))
    data = synthetic.make_superglue_inputs(4, 7, seed=4)
    data = dict(data, descriptors0=data["descriptors0"][:, :, :0],
                keypoints0=data["keypoints0"][:, :0], scores0=data["scores0"][:, :0])
    m = superglue.SuperGlue({})
    out = m({k: torch.as_tensor(v) for k, v in data.items()})      # CPU tensors: no kernel runs
    assert set(out) == set(g.files)
    for k in g.files:
        assert out[k].numpy().dtype == g[k].dtype and out[k].shape == g[k].shape, k
        assert np.array_equal(out[k].numpy(), g[k]), k


def test_cpu_forward_raises():
    data = synthetic.make_superglue_inputs(8, 9, seed=0)
    m = superglue.from_state_dict(synthetic.superglue_state_dict(0))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m({k: torch.as_tensor(v) for k, v in data.items()})


def test_superglue_version(lib):
    assert lib.onepose_superglue_version() == 1 == superglue.SUPERGLUE_VERSION
    assert lib.onepose_abi_version() == 9


def _match(lib, precision=0, n0=5, n1=6, iters=10, ws=256, ws_bytes=1 << 40, batch=1):
    """onepose_superglue_match with dummy (never dereferenced) pointers: every refusal below
    happens on the host before anything is launched."""
    p = 256
    return lib.onepose_superglue_match(p, p, 0, p, 0, p, 0, p, 0, p, 0, p, 0, batch, n0, n1, 480,
                                       640, 480, 640, iters, 0.2, precision, p, p, p, p, None, ws,
                                       ws_bytes, None)


def test_bad_arguments_are_refused_on_the_host(lib):
    err = lambda: lib.onepose_last_error().decode()
    assert _match(lib, precision=1) == 3 and "FP32" in err()          # ONEPOSE_ERR_UNSUPPORTED
    assert _match(lib, precision=2) == 3
    assert _match(lib, n0=0) == 1 and "at least 1" in err()
    assert _match(lib, n1=0) == 1
    assert _match(lib, ws=None) == 1 and "workspace" in err()
    assert _match(lib, iters=-1) == 1 and "negative" in err()
    assert _match(lib, n0=20000) == 1
    assert _match(lib, ws_bytes=16) == 4 and "needed" in err()        # ONEPOSE_ERR_WORKSPACE
    assert lib.onepose_superglue_workspace_bytes(1, 0, 5) == 0
    assert lib.onepose_superglue_workspace_bytes(1, 300, 257) > 300 * 257 * 4
    # the building blocks
    assert lib.onepose_log_optimal_transport(256, 0, 1, 4, 4, 1.0, -1, 256, 256, 1 << 30, None) == 1
    assert lib.onepose_log_optimal_transport(256, 0, 1, 0, 4, 1.0, 1, 256, 256, 1 << 30, None) == 1
    assert lib.onepose_log_optimal_transport(256, 0, 1, 4, 4, 1.0, 1, 256, None, 1 << 30, None) == 1
    assert lib.onepose_log_optimal_transport(256, 0, 1, 4, 4, 1.0, 1, 256, 256, 8, None) == 4
    assert lib.onepose_mha_softmax(256, 0, 256, 0, 256, 0, 1, 0, 4, 256, 0, None) == 1
    assert lib.onepose_mha_softmax(256, 0, 256, 0, 260, 0, 1, 4, 4, 256, 0, None) == 1   # alignment
    assert lib.onepose_mha_softmax(None, 0, 256, 0, 256, 0, 1, 4, 4, 256, 0, None) == 1


def test_new_profile_kinds_are_appended(lib):
    names = []
    for i in range(64):
        n = lib.onepose_profile_kind_name(i)
        if n:
            names.append(n.decode())
    assert names[22] == "sp_desc"                      # the last kind before this family
    assert names[23:] == ["sg_input", "sg_attention", "sg_sinkhorn", "sg_match"]

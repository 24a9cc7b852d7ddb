"""CPU tests of the C-ABI boundary: the library loads, exports every symbol the header
declares, and its host-side weight packer lays the reference weights out as documented."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


def header_symbols():
    src = open(os.path.join(REPO, "include", "onepose_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(onepose_\w+)\s*\(", src)))


def test_header_declares_the_boundary():
    syms = header_symbols()
    for s in ["onepose_match", "onepose_matcher_pack", "onepose_pnp_ransac",
              "onepose_sample_descriptors", "onepose_select_correspondences",
              "onepose_pose_errors", "onepose_last_error"]:
        assert s in syms


def test_library_exports_every_header_symbol():
    from onepose_amd import _lib
    lib = _lib.load()
    missing = [s for s in header_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    assert set(header_symbols()) == set(_lib.PROTOTYPES), "ctypes prototypes out of sync"
    assert lib.onepose_abi_version() == _lib.ABI_VERSION == 9


def test_object_cache_size_follows_its_flags():
    """The GAT prefix tables are reserved only when asked for and only for num_leaf <= 8,
    2 num_leaf rows of 1 KB per point and GAT layer plus 16 sorted logits (header)."""
    from onepose_amd import _lib
    lib = _lib.load()
    T = _lib.OBJ_GAT_TABLES
    for n3 in (1, 77, 4096):
        base = lib.onepose_object_cache_bytes(n3, 8, 0)
        for L in (1, 3, 8):
            assert lib.onepose_object_cache_bytes(n3, L, 0) == base
            assert lib.onepose_object_cache_bytes(n3, L, T) - base == 3 * n3 * (2 * L * 1024 + 64)
        assert lib.onepose_object_cache_bytes(n3, 12, T) == lib.onepose_object_cache_bytes(n3, 12, 0)
    # (+ 3 bf16 activation planes of the cached phi(q), 1.5 KB per point, in every precision)
    assert lib.onepose_object_cache_bytes(4096, 8, T) < 227.3e6
    assert lib.onepose_object_cache_bytes(4096, 8, 0) < 24.7e6
    assert lib.onepose_object_cache_bytes(0, 8, 0) == 0
    assert lib.onepose_object_cache_bytes(16, 17, 0) == 0
    assert lib.onepose_object_cache_bytes(16, 8, 2) == 0 and lib.onepose_object_cache_bytes(16, 8, -1) == 0


def test_tensor_list_matches_reference_state_dict():
    from onepose_amd import _lib, synthetic
    lib = _lib.load()
    sd = synthetic.make_state_dict(0)
    names = [lib.onepose_matcher_tensor_name(i).decode() for i in range(lib.onepose_matcher_num_tensors())]
    assert len(names) == 106
    for i, n in enumerate(names):
        assert n in sd, n
        assert sd[n].size == lib.onepose_matcher_tensor_numel(i)
    unused = set(sd) - set(names)
    assert all(k.startswith(("kenc_", "bin_score")) for k in unused)
    # the used parameter count quoted in SURVEY.md §8b
    assert sum(sd[n].size for n in names) == 5_587_200


def _pack(sd):
    from onepose_amd import _lib
    lib = _lib.load()
    names = [lib.onepose_matcher_tensor_name(i).decode() for i in range(lib.onepose_matcher_num_tensors())]
    host = [np.ascontiguousarray(sd[n], np.float32) for n in names]
    arr = (ctypes.c_void_p * len(host))(*[h.ctypes.data for h in host])
    buf = np.empty(lib.onepose_matcher_packed_bytes() // 4, np.float32)
    assert lib.onepose_matcher_pack(arr, len(host), buf.ctypes.data) == 0
    return buf


AP_FLOATS = 768 * 256 + 768 + 512 * 256 + 512 * 256 + 512 + 256 * 512 + 256 + 512 * 256


def test_pack_layout():
    """Packed panel of the first attention layer (gnn.layers.1), GAT fold, final proj."""
    from onepose_amd import synthetic
    sd = synthetic.make_state_dict(3)
    buf = _pack(sd)
    p = buf[:AP_FLOATS].astype(np.float64)
    off = 0

    def take(n):
        nonlocal off
        out = p[off:off + n]
        off += n
        return out
    wqkv = take(768 * 256).reshape(768, 256)
    bqkv = take(768)
    w1a = take(512 * 256).reshape(512, 256)
    cw = take(512 * 256).reshape(512, 256)
    b1 = take(512)
    w2 = take(256 * 512).reshape(256, 512)
    take(256)
    ct = take(512 * 256).reshape(256, 512)   # [h*64+q][o]
    q_w = sd["gnn.layers.1.attn.proj.0.weight"][:, :, 0]
    k_w = sd["gnn.layers.1.attn.proj.1.weight"][:, :, 0]
    v_w = sd["gnn.layers.1.attn.proj.2.weight"][:, :, 0]
    for h in range(4):
        for d in (0, 17, 63):
            np.testing.assert_array_equal(wqkv[h * 64 + d], q_w[d * 4 + h])
            np.testing.assert_array_equal(wqkv[256 + 128 * h + d], k_w[d * 4 + h])
            np.testing.assert_array_equal(wqkv[256 + 128 * h + 64 + d], v_w[d * 4 + h])
            assert bqkv[256 + 128 * h + 64 + d] == sd["gnn.layers.1.attn.proj.2.bias"][d * 4 + h]
            assert bqkv[h * 64 + d] == sd["gnn.layers.1.attn.proj.0.bias"][d * 4 + h]
    m0 = sd["gnn.layers.1.mlp.0.weight"][:, :, 0].astype(np.float64)
    merge = sd["gnn.layers.1.attn.merge.weight"][:, :, 0].astype(np.float64)
    np.testing.assert_array_equal(w1a, m0[:, :256])
    fold = m0[:, 256:] @ merge                       # columns in reference order q*4+h
    perm = np.array([(c % 64) * 4 + c // 64 for c in range(256)])
    np.testing.assert_allclose(cw, fold[:, perm], rtol=1e-5, atol=1e-6)
    b1f = sd["gnn.layers.1.mlp.0.bias"] + m0[:, 256:] @ sd["gnn.layers.1.attn.merge.bias"]
    np.testing.assert_allclose(b1, b1f, rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(w2, sd["gnn.layers.1.mlp.3.weight"][:, :, 0])
    np.testing.assert_array_equal(ct, cw.T)
    # bf16 planes of layer 1's Wqkv / W1a / W2 after the fp32 panel: hi = bf16 round-to-nearest-
    # even, hi + mid + lo == the fp32 weight exactly (the split gemm.hip applies to A on the fly)
    n_fp32 = 8 * AP_FLOATS + 4 * 512 + 256 * 256 + 256
    planes = buf[n_fp32:].view(np.uint16)
    assert planes.size == 8 * 3 * (768 * 256 + 512 * 256 + 256 * 512)

    def f32(b):
        return (b.astype(np.uint32) << 16).view(np.float32)
    po = 0
    for mat in (wqkv, w1a, w2):
        n = mat.size
        h, m, l = (planes[po + i * n:po + (i + 1) * n] for i in range(3))
        po += 3 * n
        x = mat.astype(np.float32).reshape(-1)
        u = x.view(np.uint32).astype(np.uint64)
        rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        np.testing.assert_array_equal(h, rne)
        np.testing.assert_array_equal((f32(h) + f32(m)) + f32(l), x)
        assert np.all(np.abs(f32(l)) <= np.abs(x) * 2.0 ** -15 + 1e-38)
    # GAT fold: wa = W @ a (layer 0)
    gat0 = buf[8 * AP_FLOATS:8 * AP_FLOATS + 512]
    W, a = sd["gnn.layers.0.W"].astype(np.float64), sd["gnn.layers.0.a"][:, 0].astype(np.float64)
    np.testing.assert_allclose(gat0[:256], W @ a[:256], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gat0[256:], W @ a[256:], rtol=1e-6, atol=1e-7)
    fin = buf[8 * AP_FLOATS + 4 * 512:]
    np.testing.assert_array_equal(fin[:65536], sd["final_proj.weight"].reshape(-1))


def test_pack_rejects_wrong_count():
    from onepose_amd import _lib
    lib = _lib.load()
    arr = (ctypes.c_void_p * 3)()
    assert lib.onepose_matcher_pack(arr, 3, None) != 0
    assert b"null" in lib.onepose_last_error() or b"expected" in lib.onepose_last_error()


def test_workspace_sizes():
    from onepose_amd import _lib
    lib = _lib.load()
    a = lib.onepose_match_workspace_bytes(1, 1024, 4096, 8, 1)
    b = lib.onepose_match_workspace_bytes(1, 1024, 4096, 8, 0)
    assert a > 0 and b - a >= 1024 * 4096 * 4
    assert lib.onepose_match_workspace_bytes(0, 1, 1, 8, 1) == 0
    # ABI 4: per precision -- fp32 carves no bf16 activation planes (x2 / x3 ping-pong and
    # phi(q), 3 planes of 512 B per token each: 6 KB per 2D + 3D token pair ... per token)
    from onepose_amd.matcher import PRECISIONS
    for B, n1, n3 in ((1, 1024, 4096), (3, 200, 330)):
        full = lib.onepose_match_workspace_bytes(B, n1, n3, 8, 1)
        f32 = lib.onepose_match_workspace_bytes_ex(B, n1, n3, 8, 1, PRECISIONS["fp32"])
        assert lib.onepose_match_workspace_bytes_ex(B, n1, n3, 8, 1, PRECISIONS["bf16"]) == full
        assert lib.onepose_match_workspace_bytes_ex(B, n1, n3, 8, 1, PRECISIONS["fp32_split"]) == full
        planes = 3 * 3 * 256 * 2 * B * (n1 + n3)   # (x ping, x pong, phi(q)) x 3 planes x bf16
        assert 0 <= full - f32 - planes < 3 * 256 * 8
    assert lib.onepose_match_workspace_bytes_ex(1, 8, 8, 8, 1, 7) == 0


def test_object_cache_size_per_precision():
    from onepose_amd import _lib
    from onepose_amd.matcher import PRECISIONS
    lib = _lib.load()
    for flags in (0, _lib.OBJ_GAT_TABLES):
        for n3 in (77, 4096):
            full = lib.onepose_object_cache_bytes(n3, 8, flags)
            assert lib.onepose_object_cache_bytes_ex(n3, 8, flags, PRECISIONS["bf16"]) == full
            assert lib.onepose_object_cache_bytes_ex(n3, 8, flags, PRECISIONS["fp32_split"]) == full
            assert full - lib.onepose_object_cache_bytes_ex(n3, 8, flags, PRECISIONS["fp32"]) == 1536 * n3
    assert lib.onepose_object_cache_bytes_ex(16, 8, 0, 9) == 0
    assert lib.onepose_pnp_workspace_bytes(2, 1024, 10000) >= 2 * 1024 * 4


def test_pnp_max_points_is_checked_on_the_host():
    """onepose_pnp_max_points (ABI 8): the solver keeps its state and 20 B per point in a
    workgroup's 160 KB of LDS, so the limit lies below 8192 (8192 points alone are 160 KB) and
    above config 5's n1 = 2048.  Both entry points refuse one more point with
    ONEPOSE_ERR_INVALID before touching an argument; at the limit they get as far as the
    workspace check (a null workspace: ONEPOSE_ERR_WORKSPACE), still without a launch."""
    from onepose_amd import _lib
    lib = _lib.load()
    limit = lib.onepose_pnp_max_points()
    assert 2048 < limit < 8192
    buf = np.zeros(16)
    p = buf.ctypes.data   # non-null; never dereferenced by a call that is refused

    def ransac(m):
        return lib.onepose_pnp_ransac(p, p, p, m, p, 0, 1, 1000.0, 5.0, 100, 0.99, p, p, p, p,
                                      None, 0, None)

    def stage(n1):
        return lib.onepose_pose_stage(p, p, 0, p, 0, 1, n1, 8, 1000.0, p, 0, 5.0, 100, 0.99,
                                      None, 0, p, p, p, p, p, p, p, None, None, None, None, 0,
                                      None)
    for call in (ransac, stage):
        rc_over = call(limit + 1)
        assert rc_over != 0 and b"onepose_pnp_max_points" in lib.onepose_last_error()
        rc_at = call(limit)
        assert rc_at not in (0, rc_over) and b"workspace" in lib.onepose_last_error()
        assert call(8192) == rc_over and call(0) == rc_over


def test_module_state_dict_keys_match_reference():
    """The drop-in module accepts the reference's full state dict (strict)."""
    from onepose_amd import matcher, synthetic
    sd = synthetic.make_state_dict(0)
    m = matcher.from_state_dict(sd)
    assert set(m.state_dict().keys()) == set(sd.keys())
    assert sum(p.numel() for p in m.parameters()) == 5_674_401


def test_empty_input_path_matches_reference():
    """GATs_SuperGlue.py:223-231 -- a bare dict with int32 indices (golden from the reference)."""
    import torch
    from conftest import golden
    from onepose_amd import matcher, synthetic
    g = golden("matcher_empty")
    m = matcher.from_state_dict(synthetic.make_state_dict(0))
    out = m({"keypoints2d": torch.zeros(1, 0, 2), "keypoints3d": torch.zeros(1, 5, 3),
             "descriptors2d_query": torch.zeros(1, 256, 0), "descriptors3d_db": torch.zeros(1, 256, 5),
             "descriptors2d_db": torch.zeros(1, 256, 40)})
    assert isinstance(out, dict) and out["skip_train"] is True
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        assert out[k].numpy().dtype == g[k].dtype
        np.testing.assert_array_equal(out[k].numpy(), g[k])


def test_cpu_forward_fails_loudly():
    import torch
    from onepose_amd import matcher, synthetic
    m = matcher.from_state_dict(synthetic.make_state_dict(0))
    data, _, _ = synthetic.make_matcher_inputs(16, 8, 2, seed=0)
    with pytest.raises(RuntimeError, match="GPU"):
        m({k: torch.from_numpy(v) for k, v in data.items()})


def test_unsupported_match_type():
    import torch
    from onepose_amd import matcher, synthetic
    hp = dict(synthetic.DEFAULT_HPARAMS, match_type="sinkhorn")
    m = matcher.from_state_dict(synthetic.make_state_dict(0), hp)
    data, _, _ = synthetic.make_matcher_inputs(16, 8, 2, seed=0)
    with pytest.raises(NotImplementedError):
        m({k: torch.from_numpy(v) for k, v in data.items()})


def test_match_cached_stages_rejects_bad_ranges():
    """onepose_match_cached_stages (ABI 6) runs a range of the forward's stages; an empty or
    out-of-order range is refused before any argument is touched (no device needed)."""
    from onepose_amd import _lib
    lib = _lib.load()
    assert (_lib.STAGE_INPUTS, _lib.STAGE_LAYER0, _lib.STAGE_FINAL, _lib.STAGE_SCORE,
            _lib.STAGE_WINNERS) == (0, 1, 13, 14, 15)
    for first, last in ((-1, 15), (0, 16), (5, 4), (15, 14), (16, 16)):
        rc = lib.onepose_match_cached_stages(None, None, 0, 0, None, None, 0, 1, 8, 8, 8, 1.0,
                                             0.2, 0, 0, None, None, None, None, None, None, 0,
                                             first, last, None)
        assert rc != 0
        assert b"stages" in lib.onepose_last_error()


def test_matcher_entry_points_refuse_in_order():
    """Every refusal a matcher entry point makes before it touches the device: its status code, a
    distinguishing part of onepose_last_error(), and which refusal wins when two apply.  The
    pointers are dummies that no refused call dereferences (no device needed).  One refusal is
    out of reach here: onepose_match_cached_stages checks the cache registry before the
    workspace size, and only onepose_object_prepare (a device call) registers a cache."""
    from onepose_amd import _lib
    lib = _lib.load()
    P = 0x1000   # never dereferenced
    INVALID, WORKSPACE = 1, 4
    gather = _lib.ALLGATHER_FN(lambda nbytes, stream, user: 0)
    B, n1, n3, L = 2, 70, 130, 5
    ws = lib.onepose_match_workspace_bytes_ex(B, n1, n3, L, 1, 0)
    ws_split = lib.onepose_match_workspace_bytes_ex(B, n1, n3, L, 0, 2)
    ws_obj = lib.onepose_object_prepare_workspace_bytes(n3, L)
    ws_sh = lib.onepose_match_sharded_workspace_bytes(B, n1, n3, 2, 1, L, 1)
    xb = lib.onepose_match_sharded_xchg_bytes(B, n1, n3, 2)
    assert min(ws, ws_split, ws_obj, ws_sh, xb) > 0

    def run(fn, good, rows):
        names = list(good)
        for change, code, text in rows:
            assert set(change) <= set(names), change
            args = [{**good, **change}[k] for k in names]
            rc = getattr(lib, fn)(*args)
            err = lib.onepose_last_error().decode()
            assert rc == code and text in err, (fn, change, rc, err)

    out = dict(m0=P, m1=P, s0=P, s1=P, conf=P)
    shape = dict(batch=B, n1=n1, n3=n3, L=L, scale=1.0, thr=0.2)
    common = [  # check_match_args, shared by the four match entry points
        (dict(w=None), INVALID, "match: null input"),
        (dict(d2=None), INVALID, "match: null input"),
        (dict(leaves=None), INVALID, "match: null input"),
        (dict(m0=None), INVALID, "match: null output"),
        (dict(s1=None), INVALID, "match: null output"),
        (dict(batch=0), INVALID, "match: batch=0 n1=70"),
        (dict(n1=0), INVALID, "match: batch=2 n1=0"),
        (dict(L=17), INVALID, "match: num_leaf=17 not in [1,16]"),
        (dict(L=0), INVALID, "match: num_leaf=0 not in [1,16]"),
        (dict(scale=0.0), INVALID, "match: scale_factor 0"),
        (dict(ws=None), INVALID, "match: null workspace"),
        (dict(w=None, m0=None), INVALID, "match: null input"),
        (dict(m1=None, batch=0), INVALID, "match: null output"),
        (dict(batch=0, L=17), INVALID, "match: batch=0"),
        (dict(L=17, scale=0.0), INVALID, "match: num_leaf=17"),
        (dict(scale=0.0, ws=None), INVALID, "match: scale_factor 0"),
        (dict(ws=None, wsb=0), INVALID, "match: null workspace"),
    ]

    good = dict(w=P, d2=P, d2bs=256 * n1, d3=P, d3bs=256 * n3, leaves=P, lbs=0, dtype=0, **shape,
                prec=0, **out, ws=P, wsb=ws, stream=None)
    run("onepose_match_dt", good, common + [
        (dict(prec=7), INVALID, "match: precision 7"),
        (dict(prec=-1), INVALID, "match: precision -1"),
        (dict(dtype=5), INVALID, "match: dtype 5"),
        (dict(d3=None), INVALID, "match: null input"),
        (dict(n3=0), INVALID, "match: batch=2 n1=70 n3=0"),
        (dict(wsb=ws - 1), WORKSPACE, f"match: workspace {ws - 1} < {ws} bytes"),
        (dict(wsb=0), WORKSPACE, f"match: workspace 0 < {ws} bytes"),
        (dict(prec=2, conf=None, wsb=ws_split - 1), WORKSPACE,
         f"match: workspace {ws_split - 1} < {ws_split} bytes"),
        (dict(prec=7, dtype=5), INVALID, "match: precision 7"),
        (dict(dtype=5, w=None), INVALID, "match: dtype 5"),
        (dict(prec=3, ws=None), INVALID, "match: precision 3"),
        (dict(batch=0, wsb=0), INVALID, "match: batch=0"),
    ])

    good = dict(w=P, d2=P, d2bs=256 * n1, d3=P, d3bs=256 * n3, leaves=P, lbs=0, **shape, prec=0,
                **out, ws=P, wsb=ws, stream=None)
    run("onepose_match_prepared_ex", good, common + [
        (dict(prec=7), INVALID, "match: precision 7"),
        (dict(d3=None), INVALID, "match: null input"),
        (dict(wsb=ws - 1), WORKSPACE, f"match: workspace {ws - 1} < {ws} bytes"),
        (dict(prec=2, conf=None, wsb=ws_split - 1), WORKSPACE,
         f"match: workspace {ws_split - 1} < {ws_split} bytes"),
        (dict(prec=7, w=None), INVALID, "match: precision 7"),
        (dict(scale=0.0, wsb=0), INVALID, "match: scale_factor 0"),
    ])

    good = dict(w=P, d2=P, dtype=0, d2bs=256 * n1, cache=P, leaves=P, lbs=0, **shape, prec=0,
                flags=0, **out, ws=P, wsb=ws, first=0, last=15, stream=None)
    unregistered = "match_cached: object_cache was not built by onepose_object_prepare"
    run("onepose_match_cached_stages", good, common + [
        (dict(first=5, last=4), INVALID, "match_cached: stages [5, 4]"),
        (dict(dtype=5), INVALID, "match_cached: dtype 5"),
        (dict(prec=7), INVALID, "match_cached: precision 7"),
        (dict(flags=2), INVALID, "match_cached: flags 2"),
        (dict(flags=-1), INVALID, "match_cached: flags -1"),
        (dict(cache=None), INVALID, "match: null input"),
        (dict(), INVALID, unregistered),
        (dict(flags=1), INVALID, unregistered),
        (dict(last=16, dtype=5), INVALID, "match_cached: stages [0, 16]"),
        (dict(dtype=5, prec=7), INVALID, "match_cached: dtype 5"),
        (dict(prec=7, flags=2), INVALID, "match_cached: precision 7"),
        (dict(flags=2, w=None), INVALID, "match_cached: flags 2"),
        (dict(ws=None, cache=0x2000), INVALID, "match: null workspace"),
        (dict(wsb=0), INVALID, unregistered),
    ])

    good = dict(w=P, d2=P, d2bs=256 * n1, d3=P, d3bs=256 * n3, leaves=P, lbs=0, batch=B, n1=n1,
                n3=n3, L=L, world=2, rank=1, scale=1.0, thr=0.2, prec=0, send=P, recv=P, xb=xb,
                fn=gather, user=None, **out, ws=P, wsb=ws_sh, stream=None)
    short_x = f"match_sharded: exchange buffers {xb - 1} < {xb} bytes per rank"
    run("onepose_match_sharded", good, common + [
        (dict(prec=7), INVALID, "match_sharded: precision 7"),
        (dict(rank=2), INVALID, "match_sharded: rank 2 of 2"),
        (dict(world=0, rank=0), INVALID, "match_sharded: rank 0 of 0"),
        (dict(send=None), INVALID, "match_sharded: null exchange buffer/callback"),
        (dict(recv=None), INVALID, "match_sharded: null exchange buffer/callback"),
        (dict(fn=_lib.ALLGATHER_FN()), INVALID, "match_sharded: null exchange buffer/callback"),
        (dict(n3=1, rank=0), INVALID, "match_sharded: empty shard (n3_total 1, world 2)"),
        (dict(d3=None), INVALID, "match: null input"),
        (dict(xb=xb - 1), WORKSPACE, short_x),
        (dict(wsb=ws_sh - 1), WORKSPACE, f"match_sharded: workspace {ws_sh - 1} < {ws_sh} bytes"),
        (dict(prec=7, rank=2), INVALID, "match_sharded: precision 7"),
        (dict(rank=-1, send=None), INVALID, "match_sharded: rank -1 of 2"),
        (dict(send=None, n3=1, rank=0), INVALID, "match_sharded: null exchange"),
        (dict(n3=1, rank=0, w=None), INVALID, "match_sharded: empty shard"),
        (dict(ws=None, xb=0), INVALID, "match: null workspace"),
        (dict(xb=xb - 1, wsb=0), WORKSPACE, short_x),
    ])

    good = dict(w=P, d3=P, dtype=0, leaves=P, n3=n3, L=L, prec=0, flags=0, cache=P, ws=P,
                wsb=ws_obj, stream=None)
    run("onepose_object_prepare_dt", good, [
        (dict(dtype=5), INVALID, "object_prepare: dtype 5"),
        (dict(w=None), INVALID, "object_prepare: null pointer"),
        (dict(d3=None), INVALID, "object_prepare: null pointer"),
        (dict(leaves=None), INVALID, "object_prepare: null pointer"),
        (dict(cache=None), INVALID, "object_prepare: null pointer"),
        (dict(prec=7), INVALID, "object_prepare: precision 7"),
        (dict(n3=0), INVALID, "object_prepare: n3=0 num_leaf=5"),
        (dict(L=17), INVALID, "object_prepare: n3=130 num_leaf=17"),
        (dict(flags=2), INVALID, "object_prepare: flags 2"),
        (dict(ws=None), INVALID, "object_prepare: null workspace"),
        (dict(wsb=ws_obj - 1), WORKSPACE,
         f"object_prepare: workspace {ws_obj - 1} < {ws_obj} bytes"),
        (dict(dtype=5, w=None), INVALID, "object_prepare: dtype 5"),
        (dict(cache=None, prec=7), INVALID, "object_prepare: null pointer"),
        (dict(prec=7, L=17), INVALID, "object_prepare: precision 7"),
        (dict(L=17, flags=2), INVALID, "object_prepare: n3=130 num_leaf=17"),
        (dict(flags=2, ws=None), INVALID, "object_prepare: flags 2"),
        (dict(ws=None, wsb=0), INVALID, "object_prepare: null workspace"),
    ])

    good = dict(leaves=P, dtype=0, lbs=0, batch=B, n3=n3, L=L, out=P, stream=None)
    run("onepose_prepare_leaves_dt", good, [
        (dict(leaves=None), INVALID, "prepare_leaves: null pointer"),
        (dict(out=None), INVALID, "prepare_leaves: null pointer"),
        (dict(dtype=5), INVALID, "prepare_leaves: dtype 5"),
        (dict(batch=0), INVALID, "prepare_leaves: batch=0 n3=130 num_leaf=5"),
        (dict(n3=0), INVALID, "prepare_leaves: batch=2 n3=0"),
        (dict(L=17), INVALID, "prepare_leaves: batch=2 n3=130 num_leaf=17"),
        (dict(L=0), INVALID, "prepare_leaves: batch=2 n3=130 num_leaf=0"),
        (dict(out=None, dtype=5), INVALID, "prepare_leaves: null pointer"),
        (dict(dtype=5, batch=0), INVALID, "prepare_leaves: dtype 5"),
    ])


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("B,n1,n3,L", [(1, 65, 97, 8), (6, 200, 330, 6)])
def test_match_workspace_region(B, n1, n3, L, prec):
    """onepose_match_workspace_region (ABI 7), a host-side query: each side's state alternates
    between two workspace buffers, flipping after every layer that writes it ('self' and 'cross'
    for the 2D side; every layer from 2 on for the 3D side of a cached forward, whose state up to
    layer 1 is the object cache's first n3*256 floats); the final descriptors exist from
    ONEPOSE_STAGE_FINAL on; every region lies inside the workspace and none overlaps another."""
    from onepose_amd import _lib
    lib = _lib.load()
    ws_bytes = _lib.workspace_bytes(lib, B, n1, n3, L, True, prec)

    def q(region, stage):
        return _lib.workspace_region(lib, B, n1, n3, L, True, prec, region, stage)
    buf2, buf3 = q(_lib.REGION_STATE2D, _lib.STAGE_INPUTS), q(_lib.REGION_STATE3D, _lib.STAGE_LAYER0 + 2)
    assert buf2 == (_lib.WHERE_WORKSPACE, 0, B * n1 * 1024)
    seen2, seen3 = [buf2], [buf3]
    flips2 = flips3 = 0
    for i in range(12):
        stage = _lib.STAGE_LAYER0 + i
        r2, r3 = q(_lib.REGION_STATE2D, stage), q(_lib.REGION_STATE3D, stage)
        flips2 += i % 3 != 0
        assert r2[0] == _lib.WHERE_WORKSPACE and r2[2] == B * n1 * 1024
        if r2 not in seen2:
            seen2.append(r2)
        assert r2 == seen2[flips2 % 2], (i, r2)
        if i < 2:
            assert r3 == (_lib.WHERE_OBJECT_CACHE, 0, n3 * 1024)
            continue
        flips3 += i > 2
        assert r3[0] == _lib.WHERE_WORKSPACE and r3[2] == B * n3 * 1024
        if r3 not in seen3:
            seen3.append(r3)
        assert r3 == seen3[flips3 % 2], (i, r3)
    assert len(seen2) == 2 and len(seen3) == 2
    last = [q(_lib.REGION_STATE2D, _lib.STAGE_WINNERS), q(_lib.REGION_STATE3D, _lib.STAGE_WINNERS)]
    assert last == [seen2[0], seen3[1]]   # 8 attention layers; 10 layers from the first 3D buffer
    descs = [q(_lib.REGION_DESC2D, _lib.STAGE_FINAL), q(_lib.REGION_DESC3D, _lib.STAGE_SCORE)]
    spans = sorted((off, off + nb) for _, off, nb in seen2 + seen3 + descs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= ws_bytes
    with pytest.raises(_lib.OnePoseError, match="ONEPOSE_STAGE_FINAL"):
        q(_lib.REGION_DESC3D, _lib.STAGE_LAYER0 + 11)
    for bad in ((4, 0), (-1, 0), (0, 16), (0, -1)):
        with pytest.raises(_lib.OnePoseError):
            q(*bad)

"""PreparedObject and _lib.run by parameter name against the same calls made raw, by position:
the object prepared once, a cached forward over B = 1 and B = 2 frames, in fp32 and bf16
arithmetic, on fp32 and fp16 descriptors -- at n1 = 33, n3 = 70 (no multiple of a 64-row tile,
two tiles) and 3 leaves.  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

from onepose_amd import _lib, matcher, synthetic
from onepose_amd.prepared import PreparedObject

pytestmark = pytest.mark.gpu

N1, N3, L = 33, 70, 3
SCALE, THRESHOLD = 0.07, 0.2
OUTPUTS = ("matches0", "matches1", "mscores0", "mscores1", "conf")
_scenes = {}


def raw_prepare(lib, w, d3, lv, dt, prec, fill, dev):
    """The prepare sequence by position, as the other tests make it, into a cache and with a
    workspace whose bytes were `fill` before -> (leaves_pm, cache)."""
    s = _lib.stream_ptr(dev)
    pm = torch.empty(lib.onepose_leaves_prepared_bytes(1, N3, L) // 4, dtype=torch.float32,
                     device=dev)
    _lib.check(lib.onepose_prepare_leaves_dt(lv.data_ptr(), dt, 0, 1, N3, L, pm.data_ptr(), s),
               "leaves")
    nbytes = _lib.object_cache_bytes(lib, N3, L, 0, prec)
    cache = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev).view(torch.float32)
    wsb = lib.onepose_object_prepare_workspace_bytes(N3, L)
    ws = torch.full((wsb,), fill, dtype=torch.uint8, device=dev)
    _lib.check(lib.onepose_object_prepare_dt(w.data_ptr(), d3.data_ptr(), dt, pm.data_ptr(), N3, L,
                                             prec, 0, cache.data_ptr(), ws.data_ptr(), wsb, s),
               "prepare")
    torch.cuda.synchronize()
    return pm, cache


def scene(dev, prec, half):
    """One object per (precision, descriptor type), prepared once through PreparedObject and
    twice by position (over 0x00 and 0xFF bytes: where the two agree, the prepare wrote what
    its inputs alone decide)."""
    if (prec, half) not in _scenes:
        lib = _lib.load()
        w = matcher.from_state_dict(synthetic.make_state_dict(3)).packed_weights(dev)
        data, _, _ = synthetic.make_matcher_inputs(N1, N3, L, seed=5, batch=2)
        dtype = torch.float16 if half else torch.float32
        d2, d3, lv = (torch.from_numpy(data[k]).to(dev, dtype).contiguous()
                      for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))
        d3, lv = d3[0].contiguous(), lv[0].contiguous()
        dt = _lib.DT_F16 if half else _lib.DT_F32
        obj = PreparedObject(w, d3, lv, prec)
        pm, cache = raw_prepare(lib, w, d3, lv, dt, prec, 0x00, dev)
        _, cache_ff = raw_prepare(lib, w, d3, lv, dt, prec, 0xFF, dev)
        lib.onepose_object_release(cache_ff.data_ptr())
        written = (cache.view(torch.uint8) == cache_ff.view(torch.uint8)).cpu().numpy()
        _scenes[prec, half] = dict(w=w, d2=d2, d3=d3, lv=lv, dt=dt, obj=obj, pm=pm, cache=cache,
                                   written=written)
    return _scenes[prec, half]


def outputs(B, dev):
    f32 = dict(dtype=torch.float32, device=dev)
    return dict(matches0=torch.empty(B, N1, dtype=torch.int64, device=dev),
                matches1=torch.empty(B, N3, dtype=torch.int64, device=dev),
                mscores0=torch.empty(B, N1, **f32), mscores1=torch.empty(B, N3, **f32),
                conf=torch.empty(B, N1, N3, **f32))


def forward_by_name(sc, obj, B, prec, dev):
    lib = _lib.load()
    out = outputs(B, dev)
    wsb = _lib.workspace_bytes(lib, B, N1, N3, L, True, prec)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    obj.use_on(torch.cuda.current_stream(dev))
    _lib.run("onepose_match_cached_dt", packed_weights=sc["w"], desc2d=sc["d2"][:B],
             desc_dtype=obj.desc_dt, desc2d_bstride=256 * N1, object_cache=obj.cache,
             leaves_prepared=obj.leaves_pm, prepared_bstride=0, batch=B, n1=N1, n3=obj.n3,
             num_leaf=obj.num_leaf, scale_factor=SCALE, match_threshold=THRESHOLD,
             precision=obj.precision, object_flags=obj.flags, **out, workspace=ws,
             workspace_bytes=wsb, stream=_lib.stream_ptr(dev))
    return out


def forward_by_position(sc, B, prec, dev):
    lib = _lib.load()
    o = outputs(B, dev)
    wsb = _lib.workspace_bytes(lib, B, N1, N3, L, True, prec)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(lib.onepose_match_cached_dt(
        sc["w"].data_ptr(), sc["d2"][:B].data_ptr(), sc["dt"], 256 * N1, sc["cache"].data_ptr(),
        sc["pm"].data_ptr(), 0, B, N1, N3, L, SCALE, THRESHOLD, prec, 0,
        o["matches0"].data_ptr(), o["matches1"].data_ptr(), o["mscores0"].data_ptr(),
        o["mscores1"].data_ptr(), o["conf"].data_ptr(), ws.data_ptr(), wsb,
        _lib.stream_ptr(dev)), "match_cached")
    return o


def assert_same_bits(got, want, tag):
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (tag, k)


@pytest.mark.parametrize("half", [False, True], ids=["desc_fp32", "desc_fp16"])
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
def test_prepared_object_and_named_forward_equal_the_raw_calls(device, B, prec, half):
    """The cache is compared wherever the prepare writes it (padding rows and leaf slots past
    num_leaf keep what the allocator left there) -- its trailing 64-byte header by its fields:
    the generation and the checksum over it are each prepare's own."""
    sc = scene(device, prec, half)
    obj = sc["obj"]
    assert (obj.n3, obj.num_leaf, obj.precision, obj.flags, obj.desc_dt) == (N3, L, prec, 0,
                                                                             sc["dt"])
    assert obj.cache.numel() * 4 == _lib.object_cache_bytes(_lib.load(), N3, L, 0, prec)
    torch.cuda.synchronize()
    assert obj.leaves_pm.cpu().numpy().tobytes() == sc["pm"].cpu().numpy().tobytes()
    mine = obj.cache.view(torch.uint8).cpu().numpy()
    raw = sc["cache"].view(torch.uint8).cpu().numpy()
    body = sc["written"].copy()
    body[-64:] = False
    assert body.sum() >= N3 * 256 * 4 * 2   # (at least the 3D state and phi(q))
    assert np.array_equal(mine[body], raw[body])
    hdr_mine, hdr_raw = mine[-64:].view(np.uint32), raw[-64:].view(np.uint32)
    assert hdr_mine[:5].tolist() == hdr_raw[:5].tolist()
    assert hdr_raw[1:5].tolist() == [N3, L, prec, 0]
    want = forward_by_position(sc, B, prec, device)
    assert_same_bits(forward_by_name(sc, obj, B, prec, device), want, "by name")
    assert int((want["matches0"] > -1).sum()) > 0


def test_use_on_another_stream_and_release(device):
    prec, B = 0, 2
    sc = scene(device, prec, False)
    want = forward_by_position(sc, B, prec, device)
    torch.cuda.synchronize()
    build, side = torch.cuda.Stream(device), torch.cuda.Stream(device)
    with torch.cuda.stream(build):
        obj = PreparedObject(sc["w"], sc["d3"], sc["lv"], prec)
    assert obj.stream == build
    with torch.cuda.stream(side):   # use_on: behind the prepare, without a host synchronisation
        got = forward_by_name(sc, obj, B, prec, device)
    assert_same_bits(got, want, "side stream")
    # released: the host registry refuses the forward before anything is launched
    obj.release()
    with pytest.raises(_lib.OnePoseError, match=r"was not built by onepose_object_prepare "
                                                r"\(or was released\)"):
        forward_by_name(sc, obj, B, prec, device)
    obj.release()   # a second release is a no-op
    other = PreparedObject(sc["w"], sc["d3"], sc["lv"], prec, cache=False)
    assert other.cache is None and other.leaves_pm.cpu().numpy().tobytes() == \
        sc["pm"].cpu().numpy().tobytes()
    other.release()
    assert_same_bits(forward_by_name(sc, sc["obj"], B, prec, device), want, "first object")

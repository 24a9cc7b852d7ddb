"""The Python binding (onepose_amd/_lib.py) against the header it is derived from: signatures,
the parser's strictness, the mirrored constants, and calls by parameter name.  No device."""
import ctypes
import json
import os

import pytest

from conftest import GOLDEN, REPO
from onepose_amd import _lib

HEADER = open(os.path.join(REPO, "include", "onepose_hip.h")).read()


def type_name(t):
    """A ctypes type as the fixture writes it; every pointer compares as "pointer"."""
    if t is None:
        return "void"
    if t is _lib.ALLGATHER_FN:
        return "ALLGATHER_FN"
    return pointer_name(t.__name__)


def pointer_name(name):
    return "pointer" if name == "c_void_p" or name.startswith("LP_") else name


def test_signatures_equal_the_hand_written_table():
    """abi9_prototypes.json is the hand-written PROTOTYPES table as it stood at ABI 9, before
    the table was derived from the header: all 99 functions, return and argument types."""
    with open(os.path.join(GOLDEN, "abi9_prototypes.json")) as f:
        want = json.load(f)
    assert len(want) == 99 and _lib.ABI_VERSION == 9
    assert set(_lib.SIGNATURES) == set(want)
    for name, (res, args) in want.items():
        got_res, got_args = _lib.PROTOTYPES[name]
        assert type_name(got_res) == pointer_name(res), name
        assert [type_name(t) for t in got_args] == [pointer_name(a) for a in args], name
        assert [t for _, t in _lib.SIGNATURES[name][1]] == got_args, name
    assert _lib.PROTOTYPES["onepose_last_error"] == (ctypes.c_char_p, [])
    assert _lib.PROTOTYPES["onepose_profile_begin"][1][0] is ctypes.c_uint64
    assert _lib.load().onepose_abi_version() == 9


def test_parser_is_strict():
    sigs, enums = _lib.parse_header(HEADER)
    assert sigs == _lib.SIGNATURES and enums == _lib.ENUMS
    names = [n for n, _ in sigs["onepose_match_cached_stages"][1]]
    assert len(names) == 25 and names[:3] == ["packed_weights", "desc2d", "desc_dtype"]
    assert names[-3:] == ["first_stage", "last_stage", "stream"]
    # a type the binding does not know: refused, and the declaration is named
    decl = "int onepose_pose_errors(const double* pose_pred,"
    assert HEADER.count(decl) == 1
    with pytest.raises(_lib.OnePoseError, match="onepose_pose_errors.*'wchar_t'"):
        _lib.parse_header(HEADER.replace(decl, "int onepose_pose_errors(wchar_t pose_pred,"))
    with pytest.raises(_lib.OnePoseError, match="onepose_abi_version.*'long'"):
        _lib.parse_header(HEADER.replace("int onepose_abi_version(void);",
                                         "long onepose_abi_version(void);"))
    # anything that is not a declaration is refused too, not skipped
    with pytest.raises(_lib.OnePoseError, match="not a declaration.*struct onepose_plan"):
        _lib.parse_header(HEADER.replace(decl, "struct onepose_plan { int n; };\n" + decl))
    with pytest.raises(_lib.OnePoseError, match="onepose_nn_version.*has no name"):
        _lib.parse_header(HEADER.replace("int onepose_nn_version(void);",
                                         "int onepose_nn_version(int);"))
    # one declaration less: the name set differs by exactly that one
    gone = "int onepose_nn_version(void);"
    assert HEADER.count(gone) == 1
    less, _ = _lib.parse_header(HEADER.replace(gone, ""))
    assert set(sigs) - set(less) == {"onepose_nn_version"} and not set(less) - set(sigs)


def test_constants_mirror_the_header_enums():
    e = _lib.ENUMS
    for prefix in ("STAGE_", "REGION_", "WHERE_", "DT_", "OBJ_", "DEVERR_"):
        in_header = {k[len("ONEPOSE_"):]: v for k, v in e.items()
                     if k.startswith("ONEPOSE_" + prefix)}
        mirrored = {k: v for k, v in vars(_lib).items() if k.startswith(prefix)}
        assert mirrored == in_header and mirrored, prefix
    from onepose_amd.matcher import PRECISIONS
    assert PRECISIONS == {"fp32": e["ONEPOSE_PREC_FP32"], "bf16": e["ONEPOSE_PREC_BF16_ATTN"],
                          "fp32_split": e["ONEPOSE_PREC_FP32_SPLIT"]}


def test_missing_header_is_an_onepose_error(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "onepose_hip.h"))
    with pytest.raises(_lib.OnePoseError, match="onepose_hip.h is missing"):
        _lib._read_header()


B, N1, N3, L = 2, 70, 130, 5
P = 0x1000   # never dereferenced: every call below is refused on the host


def stages_args(ptr):
    """onepose_match_cached_stages's arguments in the header's order, every pointer `ptr`."""
    lib = _lib.load()
    return dict(packed_weights=ptr, desc2d=ptr, desc_dtype=0, desc2d_bstride=256 * N1,
                object_cache=ptr, leaves_prepared=ptr, prepared_bstride=0, batch=B, n1=N1, n3=N3,
                num_leaf=L, scale_factor=1.0, match_threshold=0.2, precision=0, object_flags=0,
                matches0=ptr, matches1=ptr, mscores0=ptr, mscores1=ptr, conf=ptr, workspace=ptr,
                workspace_bytes=lib.onepose_match_workspace_bytes_ex(B, N1, N3, L, 1, 0),
                first_stage=0, last_stage=15, stream=None)


class Entered(Exception):
    pass


@pytest.fixture
def no_entry(monkeypatch):
    """The library's onepose_match_cached_stages replaced by a function that must not run."""
    def entered(*a):
        raise Entered
    monkeypatch.setattr(_lib.load(), "onepose_match_cached_stages", entered)


def test_call_refuses_a_missing_or_unknown_keyword(no_entry):
    args = stages_args(P)
    with pytest.raises(Entered):   # (the stand-in is what a complete call reaches)
        _lib.call("onepose_match_cached_stages", **args)
    for name in args:
        with pytest.raises(TypeError, match=f"onepose_match_cached_stages.*missing.*'{name}'"):
            _lib.call("onepose_match_cached_stages", **{k: v for k, v in args.items() if k != name})
    with pytest.raises(TypeError, match="onepose_match_cached_stages.*unknown.*'num_leaves'"):
        _lib.call("onepose_match_cached_stages", **args, num_leaves=L)
    with pytest.raises(TypeError, match="onepose_match_cached_stages.*'last_stage'"):
        _lib.run("onepose_match_cached_stages", num_leaves=L,
                 **{k: v for k, v in args.items() if k != "last_stage"})
    with pytest.raises(TypeError, match="onepose_match_cashed"):
        _lib.call("onepose_match_cashed", **args)


@pytest.mark.parametrize("ptr,text", [
    (None, "match: null input"),
    (P, "match_cached: object_cache was not built by onepose_object_prepare (or was released)")])
def test_call_by_name_is_the_positional_call(ptr, text):
    """The refusals of test_matcher_entry_points_refuse_in_order, made both ways: the same
    status and the same onepose_last_error; keyword order does not matter."""
    lib = _lib.load()
    args = stages_args(ptr)
    assert list(args) == [n for n, _ in _lib.SIGNATURES["onepose_match_cached_stages"][1]]
    rc_pos = lib.onepose_match_cached_stages(*args.values())
    err_pos = lib.onepose_last_error().decode()
    assert rc_pos == 1 and text in err_pos
    lib.onepose_abi_version()
    rc_name = _lib.call("onepose_match_cached_stages", **dict(reversed(list(args.items()))))
    assert (rc_name, lib.onepose_last_error().decode()) == (rc_pos, err_pos)
    with pytest.raises(_lib.OnePoseError) as e:
        _lib.run("onepose_match_cached_stages", **args)
    assert str(e.value) == f"onepose_match_cached_stages failed (status 1): {err_pos}"


class FakeTensor:
    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def test_call_takes_tensors_and_none_in_pointer_slots():
    """A tensor goes as its data_ptr() (anything with data_ptr(): no device here), None as a
    null pointer -- seen through which refusal answers."""
    lib = _lib.load()
    args = stages_args(FakeTensor(P))
    assert _lib.call("onepose_match_cached_stages", **args) == 1
    assert b"was not built by onepose_object_prepare" in lib.onepose_last_error()
    args["matches1"] = FakeTensor(0)
    assert _lib.call("onepose_match_cached_stages", **args) == 1
    assert b"match: null output" in lib.onepose_last_error()
    with pytest.raises(ctypes.ArgumentError):   # a tensor is not an int
        _lib.call("onepose_match_cached_stages", **{**args, "n1": FakeTensor(N1)})


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("B,n1,n3,L", [(1, 65, 97, 8), (6, 200, 330, 6)])
def test_workspace_region_by_name_is_the_positional_call(B, n1, n3, L, prec):
    """test_match_workspace_region's cases, every region after every stage."""
    lib = _lib.load()
    for region in range(4):
        for stage in range(16):
            where, off, nb = ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
            rc = lib.onepose_match_workspace_region(B, n1, n3, L, 1, prec, region, stage,
                                                    ctypes.byref(where), ctypes.byref(off),
                                                    ctypes.byref(nb))
            if rc != 0:   # the descriptors before ONEPOSE_STAGE_FINAL
                assert region >= _lib.REGION_DESC2D and stage < _lib.STAGE_FINAL
                with pytest.raises(_lib.OnePoseError):
                    _lib.workspace_region(lib, B, n1, n3, L, True, prec, region, stage)
                continue
            w2, o2, n2 = ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
            assert _lib.call("onepose_match_workspace_region", bytes=ctypes.pointer(n2),
                             offset=ctypes.byref(o2), where=ctypes.byref(w2), after_stage=stage,
                             region=region, precision=prec, with_conf=1, num_leaf=L, n3=n3, n1=n1,
                             batch=B) == 0
            triple = (where.value, off.value, nb.value)
            assert (w2.value, o2.value, n2.value) == triple and nb.value > 0
            assert _lib.workspace_region(lib, B, n1, n3, L, True, prec, region, stage) == triple

"""Variable-count SuperGlue batches, host side (no GPU): the binding's table for the new header,
and every host refusal of the three entries, in order, with dummy pointers that are never
dereferenced (a refusal happens before anything is launched)."""
import os
import re

import pytest

from onepose_amd import _lib

HEADER = "onepose_superglue_counts.h"
NEW = ("onepose_superglue_counts_version", "onepose_superglue_match_counts",
       "onepose_log_optimal_transport_counts", "onepose_mha_softmax_counts")
INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4      # ONEPOSE_ERR_*


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------- 1. binding
def test_the_binding_reads_the_counts_header():
    sig = _lib.FAMILIES[HEADER]
    assert set(sig) == set(NEW)
    assert not set(sig) & (set(_lib.SIGNATURES) | set(_lib.FAMILY_SIGNATURES))
    text = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW:       # the parameter names are the header's, in its order
        params = re.search(name + r"\s*\((.*?)\)\s*;", text, re.S).group(1)
        want = [] if params.strip() == "void" else [re.search(r"(\w+)\s*$", p).group(1)
                                                    for p in params.split(",")]
        assert [n for n, _ in sig[name][1]] == want, name
    # each entry is its sibling's parameters plus the arrays
    for name, extra in (("onepose_superglue_match_counts", ["counts0", "counts1", "hw0", "hw1"]),
                        ("onepose_log_optimal_transport_counts", ["counts_m", "counts_n"]),
                        ("onepose_mha_softmax_counts", ["counts_q", "counts_k"])):
        sib = [n for n, _ in _lib.SIGNATURES[name[:-len("_counts")]][1]]
        got = [n for n, _ in sig[name][1]]
        assert [n for n in got if n not in extra] == sib and set(extra) <= set(got), name
        assert all(t is _lib.c_void_p for n, t in sig[name][1] if n in extra)


def test_versions_and_the_pinned_tables(lib):
    assert _lib.call("onepose_superglue_counts_version") == 1
    assert lib.onepose_superglue_version() == 1 and lib.onepose_abi_version() == 9
    assert len(_lib.SIGNATURES) == 99 and not any(n in _lib.SIGNATURES for n in NEW)
    assert set(_lib.FAMILY_SIGNATURES) == {"onepose_twoview_version", "onepose_two_view_max_points",
                                          "onepose_two_view_workspace_bytes",
                                          "onepose_two_view_verify"}
    assert _lib.FAMILY_HEADERS == ("onepose_two_view.h",)
    # onepose_hip.h names the new functions in comments only (tests/test_abi.py scans its text)
    hip = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert not any(n in hip for n in NEW) and f'#include "{HEADER}"' in hip


def test_run_and_call_take_the_new_names_by_parameter_name():
    with pytest.raises(TypeError, match="missing argument 'counts_k'"):
        _lib.call("onepose_mha_softmax_counts", q=256, q_bstride=0, k=256, k_bstride=0, v=256,
                  v_bstride=0, batch=1, n=4, m=4, counts_q=None, out=256, out_bstride=0,
                  stream=None)
    with pytest.raises(_lib.OnePoseError, match="at least 1"):
        _lib.run("onepose_mha_softmax_counts", q=256, q_bstride=0, k=256, k_bstride=0, v=256,
                 v_bstride=0, batch=1, n=0, m=4, counts_q=None, counts_k=None, out=256,
                 out_bstride=0, stream=None)


# ---------------------------------------------------------------- 2. refusals
def _match(precision=0, n0=5, n1=6, iters=10, ws=256, ws_bytes=1 << 40, batch=1, h0=480,
           inp=256, outp=256, stride=30, stride1=None, counts0=None, counts1=None, weights=256):
    p = 256
    s1 = stride if stride1 is None else stride1
    return _lib.call("onepose_superglue_match_counts", packed_weights=weights, desc0=inp,
                     desc0_bstride=stride, kpts0=p, kpts0_bstride=stride, scores0=p,
                     scores0_bstride=stride, desc1=p, desc1_bstride=s1, kpts1=p,
                     kpts1_bstride=s1, scores1=p, scores1_bstride=s1, batch=batch, n0=n0, n1=n1,
                     h0=h0, w0=640, h1=480, w1=640, counts0=counts0, counts1=counts1, hw0=None,
                     hw1=None, sinkhorn_iters=iters, match_threshold=0.2, precision=precision,
                     matches0=outp, matches1=p, mscores0=p, mscores1=p, log_assignment=None,
                     workspace=ws, workspace_bytes=ws_bytes, stream=None)


def test_superglue_match_counts_refusals_in_order(lib):
    err = lambda: lib.onepose_last_error().decode()      # noqa: E731
    # each call below is wrong in the point named and in every later one: the earlier wins
    bad_later = dict(ws=None, counts0=256, stride=0)
    assert _match(precision=1, n0=0, **bad_later) == UNSUPPORTED and "FP32" in err()
    assert _match(n0=0, iters=-1, **bad_later) == INVALID and "at least 1" in err()
    assert _match(n1=0, **bad_later) == INVALID and "at least 1" in err()
    assert _match(n0=20000, **bad_later) == INVALID and "16384" in err()
    assert _match(batch=0, **bad_later) == INVALID and "batch" in err()
    assert _match(iters=-1, h0=0, **bad_later) == INVALID and "negative" in err()
    assert _match(h0=0, inp=None, **bad_later) == INVALID and "image sizes" in err()
    assert _match(inp=None, outp=None, **bad_later) == INVALID and "null input" in err()
    assert _match(weights=None, **bad_later) == INVALID and "null input" in err()
    assert _match(outp=None, **bad_later) == INVALID and "null output" in err()
    assert _match(ws=None, counts0=256, stride=-1) == INVALID and "negative batch stride" in err()
    # the added rule: a shared side (batch stride 0) with counts for that side
    assert _match(**bad_later) == INVALID and "counts0" in err() and "stride 0" in err()
    assert _match(ws=None, counts1=256, stride1=0) == INVALID and "counts1" in err()
    assert _match(ws=None, counts0=256, stride1=0) == INVALID and "null workspace" in err()
    assert _match(ws=None, counts1=256, stride=0, stride1=30) == INVALID and "null workspace" in err()
    assert _match(ws=None, stride=0) == INVALID and "null workspace" in err()   # no counts: allowed
    assert _match(ws=264, ws_bytes=16) == INVALID and "aligned" in err()
    assert _match(weights=260, ws_bytes=16) == INVALID and "aligned" in err()
    assert _match(ws_bytes=16, counts0=256, counts1=256) == WORKSPACE and "needed" in err()


def _lot(m=4, n=4, iters=1, scores=256, out=256, stride=0, ws=256, ws_bytes=1 << 30, batch=1):
    return _lib.call("onepose_log_optimal_transport_counts", scores=scores, scores_bstride=stride,
                     batch=batch, m=m, n=n, counts_m=256, counts_n=None, alpha=1.0, iters=iters,
                     out=out, workspace=ws, workspace_bytes=ws_bytes, stream=None)


def test_log_optimal_transport_counts_refusals_in_order(lib):
    err = lambda: lib.onepose_last_error().decode()      # noqa: E731
    assert _lot(m=0, scores=None, iters=-1, ws=None) == INVALID and "at least 1" in err()
    assert _lot(n=20000, scores=None) == INVALID and "16384" in err()
    assert _lot(batch=70000, scores=None) == INVALID and "batch" in err()
    assert _lot(scores=None, iters=-1, ws=None) == INVALID and "null scores" in err()
    assert _lot(out=None, iters=-1) == INVALID and "null scores" in err()
    assert _lot(iters=-1, stride=-4, ws=None) == INVALID and "iters" in err()
    assert _lot(stride=-4, ws=None) == INVALID and "negative batch stride" in err()
    assert _lot(ws=None, ws_bytes=8) == INVALID and "null workspace" in err()
    assert _lot(ws_bytes=8) == WORKSPACE and "needed" in err()


def _mha(n=4, m=4, q=256, v=256, out=256, stride=0, out_stride=0, batch=1):
    return _lib.call("onepose_mha_softmax_counts", q=q, q_bstride=stride, k=256, k_bstride=0, v=v,
                     v_bstride=0, batch=batch, n=n, m=m, counts_q=256, counts_k=None, out=out,
                     out_bstride=out_stride, stream=None)


def test_mha_softmax_counts_refusals_in_order(lib):
    err = lambda: lib.onepose_last_error().decode()      # noqa: E731
    assert _mha(n=0, q=None, stride=2, v=260) == INVALID and "at least 1" in err()
    assert _mha(m=0, q=None) == INVALID and "at least 1" in err()
    assert _mha(q=None, stride=2, v=260) == INVALID and "null argument" in err()
    assert _mha(out=None, stride=2) == INVALID and "null argument" in err()
    assert _mha(stride=2, v=260) == INVALID and "multiples of 4" in err()
    assert _mha(stride=-4, v=260) == INVALID and "multiples of 4" in err()
    assert _mha(v=260, batch=2) == INVALID and "16-byte aligned" in err()
    assert _mha(batch=2, n=4, out_stride=512) == INVALID and "overlap" in err()

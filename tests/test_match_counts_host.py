"""Per-sample keypoint counts for the 2D-3D matcher, host side (no GPU): the binding's table for
the new header, the Python-side refusals of ``keypoints2d_counts``, the host refusals of the
entries that happen before a pointer is dereferenced, and the seeds of the GPU cases
(tests/match_counts_cases.py): the oracle runs alone at every count used there, and no oracle score
lies within 1e-4 of the match threshold, so the GPU tests' threshold exemption is capped at 0 rows.

Smallest |score - 0.2| per case as computed by the oracle (test_seed_margins prints them):
edges 1.494e-02, fused 2.749e-03, empty 3.838e-04 (the smallest), groups_a 1.341e-03,
groups_b 1.309e-02, fold5 1.494e-02, wide_w8 4.708e-03, wide_128 1.644e-03 (its ten
compared samples)."""
import os
import re

import numpy as np
import pytest
import torch

import match_counts_cases as C
from onepose_amd import _lib, matcher, synthetic

HEADER = "onepose_match_counts.h"
NEW = ("onepose_match_counts_version", "onepose_match_counts_workspace_bytes",
       "onepose_match_cached_counts_stages", "onepose_match_cached_counts")
INVALID, UNSUPPORTED, WORKSPACE = 1, 3, 4      # ONEPOSE_ERR_*


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------- 1. binding
def test_the_binding_reads_the_family_header():
    assert HEADER in _lib.LATER_HEADERS
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


def test_names_and_order_of_the_new_parameters():
    sig = _lib.FAMILIES[HEADER]
    sib = [n for n, _ in _lib.SIGNATURES["onepose_match_cached_stages"][1]]
    got = [n for n, _ in sig["onepose_match_cached_counts_stages"][1]]
    # the sibling's parameters, same names and order, plus counts2d ahead of the outputs
    assert [n for n in got if n != "counts2d"] == sib
    assert got.index("counts2d") == got.index("object_flags") + 1 == got.index("matches0") - 1
    assert dict(sig["onepose_match_cached_counts_stages"][1])["counts2d"] is _lib.c_void_p
    whole = [n for n, _ in sig["onepose_match_cached_counts"][1]]
    assert whole == [n for n in got if n not in ("first_stage", "last_stage")]
    assert [n for n, _ in sig["onepose_match_counts_workspace_bytes"][1]] == \
        [n for n, _ in _lib.SIGNATURES["onepose_match_workspace_bytes_ex"][1]] == \
        ["batch", "n1", "n3", "num_leaf", "with_conf", "precision"]
    assert sig["onepose_match_counts_workspace_bytes"][0] is _lib.c_size_t


def test_versions_and_the_pinned_tables(lib):
    assert _lib.call("onepose_match_counts_version") == 1
    assert lib.onepose_abi_version() == 9 and _lib.ABI_VERSION == 9
    assert len(_lib.SIGNATURES) == 99 and not any(n in _lib.SIGNATURES for n in NEW)
    assert _lib.FAMILY_HEADERS == ("onepose_two_view.h",)
    hip = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert not any(n in hip for n in NEW)
    assert hip.rstrip().splitlines()[-3].strip().startswith(f'#include "{HEADER}"')   # at its end


def test_workspace_query_is_at_least_the_uniform_one(lib):
    for B, n1, n3, L, wc in ((1, 1024, 4096, 8, 0), (6, 160, 200, 8, 1), (32, 1408, 200, 8, 1)):
        for prec in (0, 1, 2):
            a = _lib.call("onepose_match_counts_workspace_bytes", batch=B, n1=n1, n3=n3,
                          num_leaf=L, with_conf=wc, precision=prec)
            b = _lib.call("onepose_match_workspace_bytes_ex", batch=B, n1=n1, n3=n3, num_leaf=L,
                          with_conf=wc, precision=prec)
            assert a >= b > 0
    assert _lib.call("onepose_match_counts_workspace_bytes", batch=0, n1=4, n3=4, num_leaf=1,
                     with_conf=0, precision=0) == 0


# ---------------------------------------------------------------- 2. host refusals
def _stages(precision=0, first=0, last=15, dtype=0, flags=0, weights=256, outp=256, ws=256,
            ws_bytes=1 << 40, counts=256, n1=8):
    p = 256    # dummy non-null pointers: every refusal below comes before any is dereferenced
    return _lib.call("onepose_match_cached_counts_stages", packed_weights=weights, desc2d=p,
                     desc_dtype=dtype, desc2d_bstride=256 * n1, object_cache=p,
                     leaves_prepared=p, prepared_bstride=0, batch=2, n1=n1, n3=16, num_leaf=4,
                     scale_factor=0.07, match_threshold=0.2, precision=precision,
                     object_flags=flags, counts2d=counts, matches0=outp, matches1=p, mscores0=p,
                     mscores1=p, conf=None, workspace=ws, workspace_bytes=ws_bytes,
                     first_stage=first, last_stage=last, stream=None)


def test_counts_entry_refusals_in_order(lib):
    err = lambda: lib.onepose_last_error().decode()      # noqa: E731
    # each call is wrong in the point named and in later ones: the earlier refusal wins
    assert _stages(first=3, last=2, precision=1) == INVALID and "stages" in err()
    assert _stages(dtype=7, precision=1) == INVALID and "dtype" in err()
    assert _stages(precision=9, flags=8) == INVALID and "precision" in err()
    for prec in (1, 2):     # the other two precisions: unsupported, before flags / pointers
        assert _stages(precision=prec, flags=8, weights=None) == UNSUPPORTED and "FP32" in err()
    assert _stages(flags=8, weights=None) == INVALID and "flags" in err()
    assert _stages(weights=None, outp=None) == INVALID and "null input" in err()
    assert _stages(outp=None, n1=0) == INVALID and "null output" in err()
    assert _stages(n1=0, ws=None) == INVALID and "n1=0" in err()
    assert _stages(ws=None) == INVALID and "null workspace" in err()
    # (a cache the library did not prepare: refused by the registry, with or without counts)
    assert _stages() == INVALID and "onepose_object_prepare" in err()
    assert _stages(counts=None) == INVALID and "onepose_object_prepare" in err()


# ---------------------------------------------------------------- 3. the module's key
def _module_data(B=2, n1=8, n3=16, nleaf=2):
    z = torch.zeros
    return {"keypoints2d": z(B, n1, 2), "keypoints3d": z(B, n3, 3),
            "descriptors2d_query": z(B, 256, n1),
            "descriptors3d_db": z(1, 256, n3).expand(B, 256, n3),
            "descriptors2d_db": z(1, 256, n3 * nleaf).expand(B, 256, n3 * nleaf)}


def test_keypoints2d_counts_refusals():
    m = matcher.from_state_dict(C.state_dict())
    d = _module_data()
    with pytest.raises(TypeError, match="int32 or int64"):
        m({**d, "keypoints2d_counts": torch.tensor([3.0, 4.0])})
    with pytest.raises(TypeError, match="int32 or int64"):
        m({**d, "keypoints2d_counts": [3, 4]})
    with pytest.raises(TypeError, match="int32 or int64"):
        m({**d, "keypoints2d_counts": torch.tensor([3, 4], dtype=torch.int16)})
    for bad in (torch.tensor([3, 4, 5]), torch.tensor([[3, 4]]), torch.tensor(3)):
        with pytest.raises(ValueError, match="one count per sample"):
            m({**d, "keypoints2d_counts": bad})
    # a batch of different objects has no shared cache to start from
    dense = {**d, "descriptors3d_db": d["descriptors3d_db"].contiguous()}
    with pytest.raises(ValueError, match="one object for the batch"):
        m({**dense, "keypoints2d_counts": torch.tensor([3, 4])})
    m2 = matcher.from_state_dict(C.state_dict(), {**synthetic.DEFAULT_HPARAMS,
                                                  "attention_precision": "bf16"})
    with pytest.raises(ValueError, match="fp32"):
        m2({**d, "keypoints2d_counts": torch.tensor([3, 4])})
    # a well-formed key gets as far as the device check, like a call without it
    for extra in ({}, {"keypoints2d_counts": torch.tensor([3, 4], dtype=torch.int32)},
                  {"keypoints2d_counts": torch.tensor([3, 4])}):
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            m({**d, **extra})


def test_pipeline_variable_counts_is_off_by_default():
    import inspect
    from onepose_amd.pipeline import FramePipeline
    assert inspect.signature(FramePipeline.__init__).parameters["variable_counts"].default is False


# ---------------------------------------------------------------- 4. the GPU cases' seeds
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_seed_margins(name):
    """The oracle alone on every sample of the case at its count: it runs (a count of 0 gives the
    reference's empty result), matches exist, and no score is within MARGIN of the threshold."""
    c = C.CASES[name]
    assert len(c["counts"]) == c["B"] and max(c["counts"]) <= c["n1"]
    margin, matched = C.threshold_margin(name)
    print(f"{name}: smallest |score - {C.THR}| = {margin:.3e}, {matched} matched rows")
    assert margin >= C.MARGIN
    assert matched >= 10
    for b in C.checked(name):
        cnt = c["counts"][b]
        pred, conf = C.oracle(name, b)
        assert conf.shape == (cnt, C.N3) and len(pred["matches0"]) == cnt
        if cnt == 0:
            assert pred["skip_train"] and (np.asarray(pred["matches1"]) == -1).all()

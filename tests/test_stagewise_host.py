"""CPU proof that the stage-by-stage comparison (tests/stagewise.py) can fail: the comparison is
fed numpy oracle runs in place of the kernels' stages.  The clean float32 oracle is accepted; the
float32 oracle with one deliberate bug of the kind a rewritten kernel could have is rejected, at
the margin K and still at 2K.  And, for the record of why the per-stage tests exist: with the
well-conditioned weights every other test uses, the first of those bugs (the last 4 source tokens
missing from the KV fold) passes the whole end-to-end contract of tests/parity.py."""
import contextlib

import numpy as np
import pytest

import stagewise as SW
from oracle import matcher_np as M
from parity import ATOL, assert_pred_equal

F32 = np.float32


def _linear_attention_dropping(drop_kv, drop_ksum):
    """M.linear_attention with the last 4 source tokens left out of KV and / or sum phi(k) (a
    chunk sum that misses its partial last chunk); v keeps its 1 / v_length."""
    def f(q, k, v, dtype=F32):
        eps = M._const(1e-6, dtype)
        q = M._elu(q, dtype) + dtype(1)
        k = M._elu(k, dtype) + dtype(1)
        n = v.shape[3]
        v = v / dtype(n)
        kk = k[..., :n - 4] if drop_kv else k
        kv = np.einsum("bdhm,bqhm->bqdh", kk, v[..., :kk.shape[3]], optimize=True)
        ks = (k[..., :n - 4] if drop_ksum else k).sum(3)
        z = dtype(1) / (np.einsum("bdhm,bdh->bhm", q, ks, optimize=True) + eps)
        out = np.einsum("bdhm,bqdh->bqhm", q, kv, optimize=True) * z[:, None] * dtype(n)
        return out.astype(dtype)
    return f


def _instance_norm_missing_row(x, eps=1e-5, dtype=F32):
    x64 = x.astype(np.float64)
    part = x64[:, :, :-1] if x.shape[2] > 1 else x64     # statistics without the last token
    mean = part.mean(axis=2, keepdims=True)
    var = ((part - mean) ** 2).mean(axis=2, keepdims=True)
    return ((x64 - mean) / np.sqrt(var + eps)).astype(dtype)


def _instance_norm_eps(x, eps=1e-5, dtype=F32):
    return _ORIG["instance_norm"](x, 1e-4, dtype)


def _attention_without_message(p, x, source, dtype=F32):
    q = dict(p)
    q["attn.merge.weight"] = np.zeros_like(p["attn.merge.weight"])
    q["attn.merge.bias"] = np.zeros_like(p["attn.merge.bias"])
    return _ORIG["attention_propagation"](q, x, source, dtype)


def _softmax_missing_column(x, axis, dtype=F32):
    if axis != 2:
        return _ORIG["_softmax"](x, axis, dtype)
    m = x.max(axis=axis, keepdims=True)
    e = np.exp(x - m)
    return (e * (dtype(1) / e[..., :-1].sum(axis=axis, keepdims=True))).astype(dtype)


_ORIG = {k: getattr(M, k) for k in ("linear_attention", "instance_norm", "attention_propagation",
                                     "_softmax")}
# name -> (the oracle function it replaces, the wrong version, the comparison rows it must trip)
MUTATIONS = {
    "kv-and-ksum-drop-last-4": ("linear_attention", _linear_attention_dropping(True, True), "x"),
    "ksum-drops-last-4": ("linear_attention", _linear_attention_dropping(False, True), "x"),
    "instance-norm-misses-last-row": ("instance_norm", _instance_norm_missing_row, "x"),
    "instance-norm-eps-1e-4": ("instance_norm", _instance_norm_eps, "x"),
    "message-zeroed": ("attention_propagation", _attention_without_message, "x"),
    "softmax-misses-last-column": ("_softmax", _softmax_missing_column, "conf"),
}


@contextlib.contextmanager
def mutated(name):
    attr, fn, _ = MUTATIONS[name]
    setattr(M, attr, fn)
    try:
        yield
    finally:
        setattr(M, attr, _ORIG[attr])


def mutated_float32_oracle(case, mutation):
    sd, data = SW.case_inputs(case)
    with mutated(mutation):
        return SW.oracle_stages(sd, data)


HOST_CASES = ["65x97-raw", "300x1000-raw"]


@pytest.mark.parametrize("case", HOST_CASES + ["65x97-wc", "300x1000-wc"])
def test_clean_float32_oracle_is_accepted(case):
    ref64, ref32 = SW.reference(case)
    sd, data = SW.case_inputs(case)
    rows = SW.assert_stages(f"clean float32 oracle, {case}", SW.oracle_stages(sd, data), ref64,
                            ref32)
    # every layer and side, the descriptors with their norms, S and both conf checks
    assert [r.what for r in rows] == (
        ["x2 L0"] + [f"x{s} L{i}" for i in range(1, 12) for s in (2, 3)] +
        ["desc2d", "desc2d-norm", "desc3d", "desc3d-norm", "S", "conf-rel", "conf-softmax"])


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("case", HOST_CASES)
def test_mutated_float32_oracle_is_rejected(case, mutation):
    ref64, ref32 = SW.reference(case)
    got = mutated_float32_oracle(case, mutation)
    rows, hard = SW.compare(got, ref64, ref32)
    print(SW.table(f"{mutation}, {case}", rows))
    kind = MUTATIONS[mutation][2]
    for k in (SW.K_MARGIN, 2 * SW.K_MARGIN):
        bad = [r.what for r in rows if not r.ok(k)]
        assert bad, f"{mutation} passes every stage check at K = {k}"
        if kind == "x":   # seen in the layer states themselves, not only downstream
            assert any(w.startswith("x") for w in bad), (k, bad)
        else:             # the dual softmax alone: both conf checks, and nothing before them
            assert bad == ["conf-rel", "conf-softmax"], (k, bad)


@pytest.mark.parametrize("case", ["65x97-wc", "300x1000-wc"])
def test_end_to_end_contract_accepts_the_kv_mutation(case):
    """Why the stage checks exist: under the well-conditioned weights, the float32 oracle whose KV
    fold and sum phi(k) miss the last 4 source tokens of every attention layer satisfies the
    whole end-to-end contract against the clean float32 oracle (indices equal, scores and
    conf_matrix within ATOL)."""
    ref64, ref32 = SW.reference(case)
    got = mutated_float32_oracle(case, "kv-and-ksum-drop-last-4")
    assert_pred_equal(got["pred"][0], ref32["pred"][0], f"mutated vs clean, {case}")
    err = float(np.abs(got["conf"] - ref32["conf"]).max())
    print(f"{case}: max |conf(mutated) - conf(clean)| = {err:.3e} (ATOL {ATOL})")
    assert err <= ATOL
    assert (ref32["pred"][0]["matches0"] > -1).sum() >= 20    # the index check is not vacuous
    rows, hard = SW.compare(got, ref64, ref32)
    # (the damped weights hide it from the stage comparison too at the larger shape, which is
    # why the GPU stage tests run raw weights: printed, not asserted)
    print(SW.table(f"kv-and-ksum-drop-last-4, {case}", rows))

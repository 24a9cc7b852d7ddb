"""Float64 numpy restatement of the SuperGlue forward (superglue.py:50-327), written from its
formulas: the yardstick of the SuperGlue tests.  Everything is evaluated in the reference's
channel-major layout ([C, N] per sample) from a reference-format state dict.

    forward(sd, data, iters, thr)   -> matches0/1, matching_scores0/1, log_assignment, and with
                                       keep_states the descriptor states after the encoder and
                                       after every layer, and the score matrix
    mha_softmax(q, k, v)            -> softmax(q k^T / 8) v per head, token-major head-major
                                       [n, 256] operands (the layout of onepose_mha_softmax)
    log_optimal_transport(S, a, it) -> Z + u + v - norm of the (m+1) x (n+1) couplings
"""
import contextlib

import numpy as np

BN_EPS = 1e-5
HEADS, HEAD_DIM = 4, 64
_DT = np.float64    # working precision; float32 inside `precision(np.float32)` (an fp32 evaluation
                    # of the same formulas: the measure of what fp32 rounding alone costs)


@contextlib.contextmanager
def precision(dtype):
    global _DT
    old, _DT = _DT, dtype
    try:
        yield
    finally:
        _DT = old


def _f64(x):
    return np.asarray(x, dtype=_DT)


def _lse(x, axis):
    mx = x.max(axis=axis, keepdims=True)
    return np.squeeze(mx, axis) + np.log(np.exp(x - mx).sum(axis=axis))


def _conv(sd, name, x):
    w = _f64(sd[name + ".weight"])
    w = w.reshape(w.shape[0], w.shape[1])
    return w @ x + _f64(sd[name + ".bias"])[:, None]


def _bn(sd, name, x):
    g, b = _f64(sd[name + ".weight"]), _f64(sd[name + ".bias"])
    mu, var = _f64(sd[name + ".running_mean"]), _f64(sd[name + ".running_var"])
    return (x - mu[:, None]) / np.sqrt(var[:, None] + _DT(BN_EPS)) * g[:, None] + b[:, None]


def _mlp(sd, prefix, x, n_convs):
    """Conv1d(k=1) [BatchNorm ReLU] ... Conv1d: modules 3j (conv), 3j+1 (BN) of the Sequential."""
    for j in range(n_convs):
        x = _conv(sd, f"{prefix}.{3 * j}", x)
        if j < n_convs - 1:
            x = np.maximum(_bn(sd, f"{prefix}.{3 * j + 1}", x), _DT(0))
    return x


def normalize_keypoints(kpts, h, w):
    size = np.array([w, h], dtype=_DT)
    return (_f64(kpts) - size / 2) / (size.max() * _DT(0.7))


def mha_softmax(q, k, v):
    """q [n, 256], k, v [m, 256], channels head-major (h*64 + d)."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    out = np.empty_like(q)
    for h in range(HEADS):
        c = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
        s = q[:, c] @ k[:, c].T / _DT(8.0)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, c] = (p / p.sum(axis=1, keepdims=True)) @ v[:, c]
    return out


def _attention_ref_layout(q, k, v):
    """q [256, n], k, v [256, m] with the reference's channel c = d*4 + h (.view(64, 4, N))."""
    n, m = q.shape[1], k.shape[1]
    q4, k4, v4 = q.reshape(64, 4, n), k.reshape(64, 4, m), v.reshape(64, 4, m)
    s = np.matmul(q4.transpose(1, 2, 0), k4.transpose(1, 0, 2)) / _DT(8.0)      # [h, n, m]
    p = np.exp(s - s.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    o = np.matmul(p, v4.transpose(1, 2, 0))                                    # [h, n, d]
    return np.ascontiguousarray(o.transpose(2, 0, 1)).reshape(256, n)


def _propagate(sd, p, x, src):
    q = _conv(sd, f"{p}.attn.proj.0", x)
    k = _conv(sd, f"{p}.attn.proj.1", src)
    v = _conv(sd, f"{p}.attn.proj.2", src)
    msg = _conv(sd, f"{p}.attn.merge", _attention_ref_layout(q, k, v))
    return _mlp(sd, f"{p}.mlp", np.concatenate([x, msg], axis=0), 2)


def log_optimal_transport(scores, alpha, iters):
    """scores [m, n] -> [m+1, n+1] (superglue.py:181-210)."""
    S = _f64(scores)
    m, n = S.shape
    Z = np.full((m + 1, n + 1), alpha, dtype=_DT)
    Z[:m, :n] = S
    norm = -np.log(_DT(m + n))
    log_mu = np.concatenate([np.full(m, norm), [np.log(_DT(n)) + norm]]).astype(_DT)
    log_nu = np.concatenate([np.full(n, norm), [np.log(_DT(m)) + norm]]).astype(_DT)
    u, v = np.zeros(m + 1, _DT), np.zeros(n + 1, _DT)
    for _ in range(iters):
        u = log_mu - _lse(Z + v[None, :], 1)
        v = log_nu - _lse(Z + u[:, None], 0)
    return Z + u[:, None] + v[None, :] - norm


def matches_from(Z, thr):
    """The mutual check and threshold of superglue.py:310-320 on one sample's log assignment."""
    inner = Z[:-1, :-1]
    i0, i1 = inner.argmax(axis=1), inner.argmax(axis=0)     # first maximum, as torch.max on CPU
    mutual0 = np.arange(inner.shape[0]) == i1[i0]
    mutual1 = np.arange(inner.shape[1]) == i0[i1]
    ms0 = np.where(mutual0, np.exp(inner.max(axis=1)), _DT(0))
    ms1 = np.where(mutual1, ms0[i1], _DT(0))
    valid0 = mutual0 & (ms0 > thr)
    valid1 = mutual1 & valid0[i1]
    return {"matches0": np.where(valid0, i0, -1).astype(np.int64),
            "matches1": np.where(valid1, i1, -1).astype(np.int64),
            "matching_scores0": ms0, "matching_scores1": ms1}


def forward_one(sd, desc0, kpts0, sc0, desc1, kpts1, sc1, hw0, hw1, iters, thr, n_layers=18,
                keep_states=False):
    def encode(desc, kpts, sc, hw):
        kn = normalize_keypoints(kpts, *hw)
        x = np.concatenate([kn.T, _f64(sc)[None, :]], axis=0)
        return _f64(desc) + _mlp(sd, "kenc.encoder", x, 5)

    d0, d1 = encode(desc0, kpts0, sc0, hw0), encode(desc1, kpts1, sc1, hw1)
    states = [(d0, d1)]
    for i in range(n_layers):
        p = f"gnn.layers.{i}"
        s0, s1 = (d1, d0) if i % 2 else (d0, d1)
        d0, d1 = d0 + _propagate(sd, p, d0, s0), d1 + _propagate(sd, p, d1, s1)
        if keep_states:
            states.append((d0, d1))
    m0, m1 = _conv(sd, "final_proj", d0), _conv(sd, "final_proj", d1)
    S = m0.T @ m1 / _DT(16.0)
    Z = log_optimal_transport(S, float(np.asarray(sd["bin_score"])), iters)
    out = matches_from(Z, thr)
    out["log_assignment"] = Z
    if keep_states:
        out["states"] = states          # [layer] (desc0 [256, n0], desc1 [256, n1])
        out["scores"] = S
    return out


def forward(sd, data, iters=100, thr=0.2, keep_states=False):
    """Batched: every output stacked over the batch; a side with batch dimension 1 is shared."""
    B = max(data["descriptors0"].shape[0], data["descriptors1"].shape[0])
    hw0, hw1 = data["image0"].shape[-2:], data["image1"].shape[-2:]
    outs = []
    for b in range(B):
        pick = lambda k: data[k][b if data[k].shape[0] > 1 else 0]
        outs.append(forward_one(sd, pick("descriptors0"), pick("keypoints0"), pick("scores0"),
                                pick("descriptors1"), pick("keypoints1"), pick("scores1"),
                                hw0, hw1, iters, thr, keep_states=keep_states))
    res = {k: np.stack([o[k] for o in outs]) for k in
           ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment")}
    if keep_states:
        res["states"] = [o["states"] for o in outs]
        res["scores"] = np.stack([o["scores"] for o in outs])
    return res

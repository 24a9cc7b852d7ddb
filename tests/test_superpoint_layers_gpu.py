"""SuperPoint's twelve convolution layers one by one (onepose_superpoint_layer, which launches
each layer exactly as the forward does) against a float64 oracle, at map sizes that leave
every tile type partial: a tile larger than the whole map (2x2), last tiles with 4, 9, 13
and 15 of 16 pooled rows valid, and maps narrower than a tile row (2x18, 18x2).

The bound is derived, not fitted.  A layer accumulates K = k*k*cin products (exact, or rounded
once) in fp32 in some order, merges its K-groups and adds the bias: at most K + 3 roundings
stand between any term and the result, so elementwise

    |y_gpu - y64| <= (K + 3) * 2^-24 * abssum,      abssum = |w| @ |cols| + |b|

ReLU and the 2x2 max are 1-Lipschitz, so the bound carries through them (a pooled output takes
the largest bound of its window).  The score head propagates the logit bound d through the
softmax: relative error <= 2 * max_cell(d) + 2^-16, the last term covering the 65-term fp32 sum,
two expf, the subtraction and the divide.

Every comparison also runs against deliberately wrong oracles (3x3 taps transposed, bias
zeroed, score map not pixel-shuffled), which must miss the bound by 100x: the inputs can tell
a wrong kernel from a right one.  A 1x1 layer has no taps to transpose, so that control covers
the ten 3x3 layers.  Measured err / bound maxima: docs/EXPERIMENTS.md."""
import functools

import numpy as np
import pytest
import torch

from onepose_amd import synthetic
from onepose_amd.superpoint import LAYERS, POOLED_LAYERS, SHAPES, pack_state_dict, run_layer
from oracle import superpoint_np as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SOFTMAX_SLACK = 2.0 ** -16
SIZES = [(2, 2), (3, 5), (6, 10), (10, 10), (2, 18), (18, 2), (14, 22)]
CONTROL_FACTOR = 100.0


@functools.lru_cache(maxsize=None)
def state_dict():
    """Seeded weights with the biases scaled x10 (+-0.5), so that a dropped or misindexed bias
    stands far outside the bound."""
    sd = synthetic.superpoint_state_dict(5)
    return {k: (v * np.float32(10) if k.endswith(".bias") else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def packed(device):
    return pack_state_dict(state_dict(), device)


def layer_size(layer, size):
    """3x5 stands for 'odd sides'; the pooled layers need even ones and take 4x6."""
    return (4, 6) if layer in POOLED_LAYERS and size == (3, 5) else size


def make_input(layer, h, w, batch):
    cin = SHAPES[LAYERS[layer]][1]
    rs = np.random.RandomState(1000 * layer + 10 * h + w)
    shape = (batch, h, w) if layer == 0 else (batch, h, w, cin)
    return rs.standard_normal(shape).astype(np.float32)


def chw(x, layer):
    """One sample of the layer's NHWC input as the oracle's [C,H,W]."""
    return x[None] if layer == 0 else x.transpose(2, 0, 1)


def pool_windows(a):
    """[C,H,W] -> [C,H/2,W/2,4]: the four inputs of every 2x2 window."""
    c, h, w = a.shape
    return a.reshape(c, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(c, h // 2, w // 2, 4)


def oracle_layer(layer, x, w, b):
    """(y64, bound) of a non-head layer on one sample, both in the GPU's NHWC output layout."""
    cout, cin, k = SHAPES[LAYERS[layer]]
    y, abssum = O.conv2d_f64(chw(x, layer), w, b)
    bound = (k * k * cin + 3) * U * abssum
    if layer in POOLED_LAYERS:
        y, bound = pool_windows(y).max(axis=-1), pool_windows(bound).max(axis=-1)
    if layer != 11:   # convDb: bias only
        y = np.maximum(y, 0.0)
    return y.transpose(1, 2, 0), bound.transpose(1, 2, 0)


def shuffle(p):
    """[64,h,w] -> [8h,8w] (superpoint.py:181-183)."""
    _, h, w = p.shape
    return p.reshape(8, 8, h, w).transpose(2, 0, 3, 1).reshape(8 * h, 8 * w)


def oracle_head(x, w, b, shuffled=True):
    """(p64, relative bound) of convPb + softmax + pixel shuffle on one sample: [8h,8w] each."""
    logits, abssum = O.conv2d_f64(x.transpose(2, 0, 1), w, b)
    delta = (w.shape[1] + 3) * U * abssum
    e = np.exp(logits - logits.max(axis=0, keepdims=True))
    p = (e / e.sum(axis=0, keepdims=True))[:-1]
    rel = np.broadcast_to(2 * delta.max(axis=0, keepdims=True) + SOFTMAX_SLACK, p.shape)
    if shuffled:
        return shuffle(p), shuffle(rel)
    h, wd = p.shape[1:]
    return p.transpose(1, 2, 0).reshape(8 * h, 8 * wd), shuffle(rel)


def run(device, layer, x, pk=None):
    y = run_layer(packed(device) if pk is None else pk, layer, torch.from_numpy(x).to(device))
    return y.cpu().numpy()


def batch_runs(device, layer, x):
    """The batch-of-2 output, after checking it against the two single runs bit for bit."""
    y = run(device, layer, x)
    for i in range(x.shape[0]):
        np.testing.assert_array_equal(y[i], run(device, layer, x[i:i + 1])[0],
                                      err_msg=f"sample {i} of the batch differs from its own run")
    return y


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layer", [l for l in range(12) if l != 9], ids=lambda l: LAYERS[l])
def test_layer_matches_float64_oracle(layer, size, device):
    h, w = layer_size(layer, size)
    sd = state_dict()
    wt, bias = sd[f"{LAYERS[layer]}.weight"], sd[f"{LAYERS[layer]}.bias"]
    x = make_input(layer, h, w, 2)
    y = batch_runs(device, layer, x)
    worst, ctl_taps, ctl_bias, wins = 0.0, 0.0, 0.0, np.zeros(4)
    for i in range(2):
        ref, bound = oracle_layer(layer, x[i], wt, bias)
        assert y[i].shape == ref.shape
        ratio = np.abs(y[i] - ref) / bound
        worst = max(worst, float(ratio.max()))
        # controls: the same comparison must reject a wrong kernel
        ref_b, _ = oracle_layer(layer, x[i], wt, np.zeros_like(bias))
        ctl_bias = max(ctl_bias, float((np.abs(y[i] - ref_b) / bound).max()))
        if wt.shape[2] == 3:
            ref_t, _ = oracle_layer(layer, x[i], np.ascontiguousarray(wt.transpose(0, 1, 3, 2)), bias)
            ctl_taps = max(ctl_taps, float((np.abs(y[i] - ref_t) / bound).max()))
        if layer in POOLED_LAYERS:
            y64, _ = O.conv2d_f64(chw(x[i], layer), wt, bias)
            wins += np.bincount(pool_windows(y64).argmax(axis=-1).ravel(), minlength=4)
    print(f"{LAYERS[layer]} {h}x{w}: err/bound {worst:.4f}, controls taps {ctl_taps:.3g} "
          f"bias {ctl_bias:.3g}")
    assert worst <= 1.0, f"{LAYERS[layer]} {h}x{w}: error {worst:.3f} x the fp32 bound"
    assert ctl_bias >= CONTROL_FACTOR
    if wt.shape[2] == 3:
        assert ctl_taps >= CONTROL_FACTOR
    if layer in POOLED_LAYERS:   # every window position is the max often enough to be seen
        assert wins.min() >= 0.10 * wins.sum(), wins


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_score_head_matches_float64_softmax(size, device):
    h, w = size
    sd = state_dict()
    wt, bias = sd["convPb.weight"], sd["convPb.bias"]
    x = make_input(9, h, w, 2)
    y = batch_runs(device, 9, x)
    assert y.shape == (2, 8 * h, 8 * w) and np.isfinite(y).all()
    worst, ctl_shuffle, ctl_bias = 0.0, 0.0, 0.0
    for i in range(2):
        p, rel = oracle_head(x[i], wt, bias)
        worst = max(worst, float((np.abs(y[i] - p) / (rel * p)).max()))
        p_b, _ = oracle_head(x[i], wt, np.zeros_like(bias))
        ctl_bias = max(ctl_bias, float((np.abs(y[i] - p_b) / (rel * p)).max()))
        p_n, _ = oracle_head(x[i], wt, bias, shuffled=False)
        ctl_shuffle = max(ctl_shuffle, float((np.abs(y[i] - p_n) / (rel * p)).max()))
    print(f"convPb {h}x{w}: err/bound {worst:.4f}, controls shuffle {ctl_shuffle:.3g} "
          f"bias {ctl_bias:.3g}")
    assert worst <= 1.0, f"convPb {h}x{w}: error {worst:.3f} x the propagated bound"
    assert ctl_shuffle >= CONTROL_FACTOR and ctl_bias >= CONTROL_FACTOR


def exact_head():
    """convPb weights and biases that are multiples of 1/8 in [-60, 60]: with a one-hot input
    every logit is w[c, hot] + b[c], exact in fp32.  The dustbin (channel 64) is far above every
    other logit for hot channels 0..63 and far below for 64..127."""
    rs = np.random.RandomState(77)
    wt = (rs.randint(-480, 481, (65, 256, 1, 1)) / 8.0).astype(np.float32)
    bias = (rs.randint(-480, 481, 65) / 8.0).astype(np.float32)
    bias[64] = 0.0
    wt[64, :64] = 60.0
    wt[:64, :64] = (rs.randint(-480, -239, (64, 64, 1, 1)) / 8.0).astype(np.float32)
    wt[64, 64:128] = -60.0
    wt[:64, 64:128] = (rs.randint(240, 481, (64, 64, 1, 1)) / 8.0).astype(np.float32)
    return wt, bias


@pytest.mark.parametrize("size", [(3, 5), (14, 22)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_score_head_exact_logits(size, device):
    """Logits exact in fp32 (no conv error to hide behind), spanning [-120, 120]: results
    finite and within 2^-16 relative of the float64 softmax; outputs below 1e-30 (where fp32's
    exp underflows) to 1e-30 absolute."""
    h, w = size
    wt, bias = exact_head()
    sd = dict(state_dict())
    sd["convPb.weight"], sd["convPb.bias"] = wt, bias
    pk = pack_state_dict(sd, device)
    hot = np.random.RandomState(h * w).randint(0, 256, (2, h, w))
    hot[:, 0, 0], hot[:, -1, -1] = 3, 100         # both regimes at the corners, whatever the draw
    x = np.zeros((2, h, w, 256), np.float32)
    np.put_along_axis(x, hot[..., None], 1.0, axis=-1)
    y = run(device, 9, x, pk)
    np.testing.assert_array_equal(y[1], run(device, 9, x[1:], pk)[0])
    assert np.isfinite(y).all()
    for i in range(2):
        logits = (wt[:, hot[i], 0, 0] + bias[:, None, None]).astype(np.float64)   # [65,h,w]
        got = O.conv2d_f64(x[i].transpose(2, 0, 1), wt, bias)[0]
        np.testing.assert_array_equal(got, logits)
        assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits)
        e = np.exp(logits - logits.max(axis=0, keepdims=True))
        p_all = e / e.sum(axis=0, keepdims=True)
        assert (p_all[64] > 0.99).any() and (p_all[64] < 1e-30).any()   # dustbin on both sides
        p = shuffle(p_all[:-1])
        big = p >= 1e-30
        assert big.any() and (~big).any()
        rel = np.abs(y[i] - p)[big] / p[big]
        print(f"exact logits {h}x{w} sample {i}: rel err {rel.max() / SOFTMAX_SLACK:.4f} x 2^-16")
        assert rel.max() <= SOFTMAX_SLACK
        assert np.abs(y[i] - p)[~big].max() <= 1e-30


def test_layer_entry_refuses_bad_arguments(device):
    from onepose_amd import _lib
    pk = packed(device)
    with pytest.raises(_lib.OnePoseError, match="even"):
        run_layer(pk, 3, torch.zeros(1, 3, 4, 64, device=device))
    with pytest.raises(ValueError):
        run_layer(pk, 12, torch.zeros(1, 2, 2, 64, device=device))
    with pytest.raises(ValueError):
        run_layer(pk, 4, torch.zeros(1, 2, 2, 128, device=device))
    lib = _lib.load()
    x = torch.zeros(1, 2, 2, 64, device=device)
    assert lib.onepose_superpoint_layer(pk.data_ptr(), 12, x.data_ptr(), 1, 2, 2, x.data_ptr(),
                                        0) != 0
    assert "layer" in lib.onepose_last_error().decode()

"""Drop-in ``NearestNeighbour`` whose forward runs on libonepose_hip (MI355X).

Same constructor (``conf`` dict merged over ``default_conf``) and the same
``forward(data) -> dict`` contract as ``src/models/matchers/nn/nearest_neighbour.py:26-63``:

* inputs ``descriptors0 [B,d,n0]`` and ``descriptors1 [B,d,n1]`` (other keys are ignored), fp32
  or fp16 (fp16 is converted as the kernel loads it); a side with batch dimension 1 or expanded
  over the batch (stride 0) is passed to the library as shared, not copied;
* outputs ``matches0/1`` int64 (-1 = unmatched) and ``matching_scores0/1`` float32, on the
  inputs' device;
* ``ratio_threshold`` / ``distance_threshold`` are truthiness tests as in the reference (None
  and 0 disable); only ``matches0`` gets the mutual check, ``matching_scores0`` keeps its value
  where the check clears a match; ``match_threshold`` is accepted and never read;
* a ratio test with a single keypoint on either side raises ``RuntimeError`` (``topk(2)`` does
  in the reference) before anything is launched.

On equal similarities (``torch.topk`` promises no order) the lowest index wins and a duplicated
best value is its own runner-up (include/onepose_hip.h).  NaN thresholds are refused.

The module has no CPU path: tensors must live on a ROCm device and ``libonepose_hip.so`` must be
built, otherwise forward raises.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib

NN_VERSION = 1
_WS = {}   # (device, stream, B, n0, n1) -> workspace; calls on different streams never share


def _workspace(dev, B, n0, n1):
    lib = _lib.load()
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, B, n0, n1)
    ws = _WS.get(key)
    if ws is None:
        nbytes = lib.onepose_nn_match_workspace_bytes(B, n0, n1)
        if nbytes == 0:
            raise ValueError(f"NearestNeighbour: unsupported shape B={B}, n0={n0}, n1={n1}")
        if len(_WS) >= 8:
            _WS.clear()
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def _operand(x, B, d, dtype):
    """[B or 1, d, n] tensor of `dtype`, samples contiguous; returns (tensor, batch stride in
    elements, 0 when the side is shared by the batch)."""
    if x.dim() != 3 or x.shape[0] not in (1, B) or x.shape[1] != d:
        raise ValueError(f"bad NearestNeighbour descriptor shape {tuple(x.shape)}, expected "
                         f"[{B}, {d}, n]")
    x = x.to(dtype)
    shared = x.shape[0] == 1 or x.stride(0) == 0
    if shared:
        x = x[:1]
    if not x[0].is_contiguous() or (not shared and x.stride(0) != x[0].numel()):
        x = x.contiguous()
    return x, (0 if shared and B > 1 else x[0].numel())


def _threshold(v, name):
    """The reference's ``if v:`` then ``v ** 2``: falsy -> 0.0 (off), else |v|."""
    if not v:
        return 0.0
    v = float(v)
    if math.isnan(v):
        raise ValueError(f"NearestNeighbour: {name} is NaN")
    return abs(v)


def nearest_neighbour_match(desc0, desc1, ratio=None, distance=None, mutual=True, workspace=None):
    """The matcher as a function: (matches0, matches1, matching_scores0, matching_scores1).
    `workspace`: a uint8 tensor of at least onepose_nn_match_workspace_bytes (default: one cached
    per device, stream and shape)."""
    if desc0.device.type != "cuda" or desc1.device.type != "cuda":
        raise RuntimeError("onepose_amd.NearestNeighbour runs on a ROCm GPU only; move the inputs "
                           "with .cuda()")
    ratio, distance = _threshold(ratio, "ratio_threshold"), _threshold(distance,
                                                                       "distance_threshold")
    dev = desc0.device
    B = max(desc0.shape[0], desc1.shape[0])
    d, n0, n1 = desc0.shape[1], desc0.shape[2], desc1.shape[2]
    if ratio and (n0 < 2 or n1 < 2):
        raise RuntimeError("NearestNeighbour: the ratio test needs at least 2 keypoints on both "
                           f"sides (n0 = {n0}, n1 = {n1})")
    half = desc0.dtype == torch.float16 and desc1.dtype == torch.float16
    dtype = torch.float16 if half else torch.float32
    d0, d0s = _operand(desc0, B, d, dtype)
    d1, d1s = _operand(desc1, B, d, dtype)
    with torch.cuda.device(dev):
        ws = _workspace(dev, B, n0, n1) if workspace is None else workspace
        m0 = torch.empty(B, n0, dtype=torch.int64, device=dev)
        m1 = torch.empty(B, n1, dtype=torch.int64, device=dev)
        s0 = torch.empty(B, n0, dtype=torch.float32, device=dev)
        s1 = torch.empty(B, n1, dtype=torch.float32, device=dev)
        _lib.run("onepose_nn_match", desc0=d0, desc0_bstride=d0s, desc1=d1, desc1_bstride=d1s,
                 desc_dtype=_lib.DT_F16 if half else _lib.DT_F32, batch=B, d=d, n0=n0, n1=n1,
                 ratio_threshold=ratio, distance_threshold=distance,
                 do_mutual_check=int(bool(mutual)), matches0=m0, matches1=m1, mscores0=s0,
                 mscores1=s1, workspace=ws, workspace_bytes=ws.numel(),
                 stream=_lib.stream_ptr(dev))
    return m0, m1, s0, s1


class NearestNeighbour(nn.Module):
    default_conf = {
        "match_threshold": None,
        "ratio_threshold": None,
        "distance_threshold": None,
        "do_mutual_check": True,
    }

    def __init__(self, conf=None):
        super().__init__()
        self.conf = {**self.default_conf, **conf} if conf else self.default_conf

    def forward(self, data):
        m0, m1, s0, s1 = nearest_neighbour_match(
            data["descriptors0"], data["descriptors1"], self.conf["ratio_threshold"],
            self.conf["distance_threshold"], self.conf["do_mutual_check"])
        return {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1}

"""Drop-in ``SuperGlue`` whose forward runs on libonepose_hip (MI355X).

Same constructor (``config`` dict over ``default_config``), the same parameter and buffer names
and shapes (a reference state dict loads with ``strict=True``) and the same
``forward(data) -> dict`` contract as ``src/models/matchers/SuperGlue/superglue.py:217-327``:

* inputs ``descriptors0/1 [B,256,n]``, ``keypoints0/1 [B,n,2]``, ``scores0/1 [B,n]`` and
  ``image0/1`` (only ``.shape`` is read); a side expanded over the batch (stride 0) is passed
  to the library as shared, not copied;
* outputs ``matches0/1`` int64 (-1 = unmatched) and ``matching_scores0/1`` float32, whole batch;
* no keypoints on either side returns the reference's dict with int32 indices (:269-276);
* optional ``counts0/1 [B]`` (integers: how many leading keypoints of each sample are real) and
  ``image_hw0/1 [B, 2]`` (per-sample (h, w)): pairs of unequal counts and image sizes in one
  call, padded to the batch maxima.  The four outputs come back padded: -1 and 0 past a
  sample's count, and everywhere for a sample with an empty side.  Without these keys the call
  is what it was;
* ``GNN_layers`` other than ``['self', 'cross'] * 9`` and a ``descriptor_dim`` other than 256
  raise ``NotImplementedError`` (the kernels are built for that network).

The module has no CPU path: tensors must live on a ROCm device and ``libonepose_hip.so`` must be
built, otherwise forward raises.  fp32 only, eval mode (BatchNorm uses its running statistics).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib

PREC_FP32 = 0   # ONEPOSE_PREC_FP32
SUPERGLUE_VERSION = 1


def _version(t):
    return None if torch.is_inference(t) else t._version


def MLP(channels, do_bn=True):
    """Conv1d / BatchNorm1d / ReLU stack with the reference's module indices (:50-64)."""
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            if do_bn:
                layers.append(nn.BatchNorm1d(channels[i]))
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class KeypointEncoder(nn.Module):
    def __init__(self, feature_dim, layers):
        super().__init__()
        self.encoder = MLP([3] + list(layers) + [feature_dim])
        nn.init.constant_(self.encoder[-1].bias, 0.0)


class MultiHeadedAttention(nn.Module):
    def __init__(self, num_heads: int, d_model: int):
        super().__init__()
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])


class AttentionalPropagation(nn.Module):
    def __init__(self, feature_dim: int, num_heads: int):
        super().__init__()
        self.attn = MultiHeadedAttention(num_heads, feature_dim)
        self.mlp = MLP([feature_dim * 2, feature_dim * 2, feature_dim])
        nn.init.constant_(self.mlp[-1].bias, 0.0)


class AttentionalGNN(nn.Module):
    def __init__(self, feature_dim: int, layer_names):
        super().__init__()
        self.layers = nn.ModuleList([AttentionalPropagation(feature_dim, 4)
                                     for _ in range(len(layer_names))])
        self.names = list(layer_names)


class SuperGlue(nn.Module):
    default_config = {
        "descriptor_dim": 256,
        "weights": "indoor",
        "keypoint_encoder": [32, 64, 128, 256],
        "GNN_layers": ["self", "cross"] * 9,
        "sinkhorn_iterations": 100,
        "match_threshold": 0.2,
    }
    # forward takes counts0/1 and image_hw0/1 (sfm.match_pairs(batch_size=...) asks for this)
    supports_counts = True

    def __init__(self, config=None):
        super().__init__()
        self.config = {**self.default_config, **(config or {})}
        if self.config["descriptor_dim"] != 256:
            raise NotImplementedError("onepose_amd kernels are built for descriptor_dim=256")
        if list(self.config["GNN_layers"]) != ["self", "cross"] * 9:
            raise NotImplementedError("onepose_amd's SuperGlue runs GNN_layers = "
                                      "['self', 'cross'] * 9 only")
        if list(self.config["keypoint_encoder"]) != [32, 64, 128, 256]:
            raise NotImplementedError("onepose_amd's SuperGlue runs keypoint_encoder = "
                                      "[32, 64, 128, 256] only")
        self.kenc = KeypointEncoder(256, self.config["keypoint_encoder"])
        self.gnn = AttentionalGNN(256, self.config["GNN_layers"])
        self.final_proj = nn.Conv1d(256, 256, kernel_size=1, bias=True)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self._packed = None
        self._packed_key = None
        self._ws = {}

    # ---------------------------------------------------------------- weight packing
    def _weight_tensors(self):
        lib = _lib.load()
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        out = []
        for i in range(lib.onepose_superglue_num_tensors()):
            name = lib.onepose_superglue_tensor_name(i).decode()
            t = sd[name]
            if t.numel() != lib.onepose_superglue_tensor_numel(i):
                raise ValueError(f"{name}: {t.numel()} elements, expected "
                                 f"{lib.onepose_superglue_tensor_numel(i)}")
            out.append(t)
        return out

    def packed_weights(self, device):
        """The device-resident weight panel (packed again when a parameter or buffer changed)."""
        tensors = self._weight_tensors()
        key = (str(device),) + tuple((t.data_ptr(), _version(t)) for t in tensors)
        if (self._packed is not None and self._packed_key == key
                and all(k[1] is not None for k in key[1:])):
            return self._packed
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in tensors]
        arr = (_lib.c_void_p * len(host))(*[h.data_ptr() for h in host])
        buf = np.empty(lib.onepose_superglue_packed_bytes() // 4, dtype=np.float32)
        _lib.check(lib.onepose_superglue_pack(arr, len(host), buf.ctypes.data), "superglue_pack")
        self._packed = torch.from_numpy(buf).to(device)
        self._packed_key = key
        return self._packed

    def _workspace(self, device, B, n0, n1):
        """One workspace per (device, stream, shape): forwards on different streams never share."""
        lib = _lib.load()
        key = (str(device), torch.cuda.current_stream(device).cuda_stream, B, n0, n1)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = lib.onepose_superglue_workspace_bytes(B, n0, n1)
            if nbytes == 0:
                raise ValueError(f"SuperGlue: unsupported shape B={B}, n0={n0}, n1={n1}")
            if len(self._ws) >= 8:
                self._ws.clear()
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    # ---------------------------------------------------------------- forward
    @staticmethod
    def _operand(x, B, inner):
        """float32 tensor of shape [B or 1, *inner], samples contiguous; returns (tensor, batch
        stride in elements, 0 when the batch dimension is expanded)."""
        x = x.float()
        if x.shape[0] not in (1, B) or tuple(x.shape[1:]) != tuple(inner):
            raise ValueError(f"bad SuperGlue input shape {tuple(x.shape)}, expected "
                             f"[{B}, {', '.join(map(str, inner))}]")
        shared = x.shape[0] == 1 or x.stride(0) == 0
        if shared:
            x = x[:1]
        if not x[0].is_contiguous() or (not shared and x.stride(0) != x[0].numel()):
            x = x.contiguous()
        return x, (0 if shared and B > 1 else x[0].numel())

    @staticmethod
    def _image_hw(data, side):
        """The scalar (h, w) of a side: ``image{side}``'s shape; with ``image_hw{side}`` given the
        image may be left out (the scalars are then not read)."""
        if f"image{side}" in data or f"image_hw{side}" not in data:
            return data[f"image{side}"].shape[-2:]
        return 1, 1

    @staticmethod
    def _int_operand(x, shape, dev, what):
        """None, or the contiguous int32 device tensor of that shape."""
        if x is None:
            return None
        x = torch.as_tensor(x)
        if tuple(x.shape) != tuple(shape) or x.is_floating_point():
            raise ValueError(f"SuperGlue: {what} must be an integer tensor of shape {list(shape)}, "
                             f"got {x.dtype} {list(x.shape)}")
        return x.to(device=dev, dtype=torch.int32).contiguous()

    def forward(self, data, return_log_assignment=False):
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        if kpts0.shape[1] == 0 or kpts1.shape[1] == 0:   # no keypoints
            shape0, shape1 = kpts0.shape[:-1], kpts1.shape[:-1]
            return {
                "matches0": kpts0.new_full(shape0, -1, dtype=torch.int),
                "matches1": kpts1.new_full(shape1, -1, dtype=torch.int),
                "matching_scores0": kpts0.new_zeros(shape0),
                "matching_scores1": kpts1.new_zeros(shape1),
            }
        if kpts0.device.type != "cuda":
            raise RuntimeError("onepose_amd.SuperGlue runs on a ROCm GPU only; move the inputs "
                               "with .cuda()")
        if self.training:
            raise NotImplementedError("onepose_amd.SuperGlue is inference only: call .eval()")
        dev = kpts0.device
        B = max(kpts0.shape[0], kpts1.shape[0])
        n0, n1 = kpts0.shape[1], kpts1.shape[1]
        d0, d0s = self._operand(data["descriptors0"], B, (256, n0))
        k0, k0s = self._operand(kpts0, B, (n0, 2))
        s0, s0s = self._operand(data["scores0"], B, (n0,))
        d1, d1s = self._operand(data["descriptors1"], B, (256, n1))
        k1, k1s = self._operand(kpts1, B, (n1, 2))
        s1, s1s = self._operand(data["scores1"], B, (n1,))
        h0, w0 = self._image_hw(data, 0)
        h1, w1 = self._image_hw(data, 1)
        counted = any(k in data for k in ("counts0", "counts1", "image_hw0", "image_hw1"))
        if counted:
            i32 = lambda k, shape: self._int_operand(data.get(k), shape, dev, k)   # noqa: E731
            extra = dict(counts0=i32("counts0", (B,)), counts1=i32("counts1", (B,)),
                         hw0=i32("image_hw0", (B, 2)), hw1=i32("image_hw1", (B, 2)))
        with torch.cuda.device(dev):
            w = self.packed_weights(dev)
            ws = self._workspace(dev, B, n0, n1)
            m0 = torch.empty(B, n0, dtype=torch.int64, device=dev)
            m1 = torch.empty(B, n1, dtype=torch.int64, device=dev)
            ms0 = torch.empty(B, n0, dtype=torch.float32, device=dev)
            ms1 = torch.empty(B, n1, dtype=torch.float32, device=dev)
            # (with counts only each sample's top-left block is written: zeros elsewhere)
            la = ((torch.zeros if counted else torch.empty)(
                B, n0 + 1, n1 + 1, dtype=torch.float32, device=dev)
                  if return_log_assignment else None)
            _lib.run("onepose_superglue_match_counts" if counted else "onepose_superglue_match",
                     **(extra if counted else {}), packed_weights=w, desc0=d0, desc0_bstride=d0s,
                     kpts0=k0, kpts0_bstride=k0s, scores0=s0, scores0_bstride=s0s, desc1=d1,
                     desc1_bstride=d1s, kpts1=k1, kpts1_bstride=k1s, scores1=s1,
                     scores1_bstride=s1s, batch=B, n0=n0, n1=n1, h0=int(h0), w0=int(w0),
                     h1=int(h1), w1=int(w1),
                     sinkhorn_iters=int(self.config["sinkhorn_iterations"]),
                     match_threshold=float(self.config["match_threshold"]), precision=PREC_FP32,
                     matches0=m0, matches1=m1, mscores0=ms0, mscores1=ms1, log_assignment=la,
                     workspace=ws, workspace_bytes=ws.numel(), stream=_lib.stream_ptr(dev))
        out = {"matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1}
        if return_log_assignment:
            out["log_assignment"] = la
        return out


def from_state_dict(state_dict, config=None) -> SuperGlue:
    """Build the matcher from a reference-format state dict (numpy arrays or tensors)."""
    m = SuperGlue(dict(config or {}))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()},
                      strict=True)
    return m.eval()

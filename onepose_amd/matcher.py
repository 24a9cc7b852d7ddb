"""Drop-in ``GATsSuperGlue`` whose forward runs on libonepose_hip (MI355X).

Same constructor (``hparams`` dict / AttributeDict), same parameter names and shapes (so a
reference state dict or a Lightning checkpoint's ``matcher.*`` entries load unchanged) and
the same ``forward(data) -> (pred, conf_matrix)`` contract as
``src/models/GATsSPG_architectures/GATs_SuperGlue.py:162-278``:

* inputs ``keypoints2d [B,N1,2]``, ``keypoints3d [B,N3,3]``, ``descriptors2d_query
  [B,256,N1]``, ``descriptors3d_db [B,256,N3]``, ``descriptors2d_db [B,256,N3*L]``
  (extra keys ignored; everything upcast to float32 as :219-221 does);
* ``pred`` holds batch element 0 only: ``matches0/1`` int64 (-1 = unmatched),
  ``matching_scores0/1`` float32; ``conf_matrix`` keeps the whole batch (:269-278);
* no keypoints on either side returns the reference's bare dict with int32 indices and
  ``skip_train`` (:223-231);
* a ``match_type`` other than ``'softmax'`` raises ``NotImplementedError`` (:275-276).

onepose_amd extension: the optional key ``keypoints2d_counts`` ([B] int32 / int64 on the inputs'
device) gives each sample's number of real 2D keypoints in a batch padded to N1
(``onepose_match_cached_counts``, include/onepose_match_counts.h; fp32 attention, one object for
the whole batch: 3D tensors of batch 1 or expanded).  Sample b is matched as if it had that many
keypoints; ``pred`` stays batch element 0 at the padded length (-1 / 0 past its count) and
``conf_matrix`` [B, N1, N3] has zero rows past each count.  Without the key nothing changes.

The parameters are ordinary ``nn.Parameter``s (PyTorch is the weight store); the first
forward after they change packs them (head-major q/k/v, folded GAT vectors) into one
device-resident panel.  The module has no CPU path: tensors must live on a ROCm device
and ``libonepose_hip.so`` must be built, otherwise forward raises.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .prepared import PreparedObject

SUPPORTED = {"include_self": True, "additional": False, "with_linear_transform": False}


def _version(t):
    """The tensor's version counter, or None for an inference tensor (torch.inference_mode),
    which has none -- so an in-place write to it cannot be detected."""
    return None if torch.is_inference(t) else t._version


def _hp(hparams, key, default=None):
    if isinstance(hparams, dict):
        return hparams.get(key, default)
    return getattr(hparams, key, default)


def _mlp(channels):
    """Conv1d / InstanceNorm1d / ReLU stack with the reference's module indices (:135-147)."""
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            layers.append(nn.InstanceNorm1d(channels[i]))
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


class KeypointEncoder(nn.Module):
    """Parameter holder for ``kenc_2d`` / ``kenc_3d`` (present in checkpoints, never used by
    the reference forward, :172-182)."""

    def __init__(self, inp_dim, feature_dim, layers):
        super().__init__()
        self.encoder = _mlp([inp_dim, *layers, feature_dim])
        nn.init.constant_(self.encoder[-1].bias, 0.0)


class GraphAttentionLayer(nn.Module):
    """Parameters of ``GATs.py:9-57`` (W [in,out], a [2*out,1])."""

    def __init__(self, in_features=256, out_features=256, dropout=0.6, alpha=0.2, concat=True,
                 include_self=True, additional=False, with_linear_transform=False):
        super().__init__()
        self.dropout, self.alpha, self.concat = dropout, alpha, concat
        self.include_self, self.additional = include_self, additional
        self.with_linear_transform = with_linear_transform
        self.W = nn.Parameter(torch.empty(in_features, out_features))
        nn.init.xavier_normal_(self.W.data, gain=1.414)
        self.a = nn.Parameter(torch.empty(2 * out_features, 1))
        nn.init.xavier_normal_(self.a.data, gain=1.414)


class MultiHeadedAttention(nn.Module):
    def __init__(self, num_heads: int, d_model: int):
        super().__init__()
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])


class AttentionPropagation(nn.Module):
    def __init__(self, feature_dim: int, num_heads: int):
        super().__init__()
        self.attn = MultiHeadedAttention(num_heads, feature_dim)
        self.mlp = _mlp([feature_dim * 2, feature_dim * 2, feature_dim])
        nn.init.constant_(self.mlp[-1].bias, 0.0)


class AttentionalGNN(nn.Module):
    """['GATs', 'self', 'cross'] * 4 (:52-65)."""

    def __init__(self, feature_dim, layer_names, include_self, additional, with_linear_transform):
        super().__init__()
        self.layers = nn.ModuleList([
            GraphAttentionLayer(256, 256, 0.6, 0.2, True, include_self, additional,
                                with_linear_transform)
            if i % 3 == 0 else AttentionPropagation(feature_dim, 4)
            for i in range(len(layer_names))])
        self.names = list(layer_names)


# ONEPOSE_PREC_FP32 / ONEPOSE_PREC_BF16_ATTN / ONEPOSE_PREC_FP32_SPLIT (include/onepose_hip.h)
PRECISIONS = {"fp32": 0, "bf16": 1, "fp32_split": 2}


class GATsSuperGlue(nn.Module):
    def __init__(self, hparams):
        super().__init__()
        self.hparams = hparams
        self.match_type = _hp(hparams, "match_type")
        dim = _hp(hparams, "descriptor_dim", 256)
        if dim != 256:
            raise NotImplementedError("onepose_amd kernels are built for descriptor_dim=256")
        for k, v in SUPPORTED.items():
            if bool(_hp(hparams, k, v)) != v:
                raise NotImplementedError(f"onepose_amd supports {k}={v} only (GATsSPG config)")
        enc = list(_hp(hparams, "keypoints_encoder", [32, 64, 128]))
        self.kenc_2d = KeypointEncoder(3, dim, enc)
        self.kenc_3d = KeypointEncoder(4, dim, enc)
        self.gnn = AttentionalGNN(dim, ["GATs", "self", "cross"] * 4, True, False, False)
        self.final_proj = nn.Conv1d(dim, dim, kernel_size=1, bias=True)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self._packed = None
        self._packed_key = None
        # onepose_amd extension (not a reference hparam): "fp32" (default, the reference's
        # numerics) or "bf16" (attention-layer GEMMs on bf16 MFMA, BASELINE config 5)
        prec = _hp(hparams, "attention_precision", "fp32")
        if prec not in PRECISIONS:
            raise ValueError(f"attention_precision {prec!r} not in {sorted(PRECISIONS)}")
        self.precision = PRECISIONS[prec]

    # ---------------------------------------------------------------- weight packing
    def _weight_tensors(self):
        lib = _lib.load()
        sd = dict(self.named_parameters())
        out = []
        for i in range(lib.onepose_matcher_num_tensors()):
            name = lib.onepose_matcher_tensor_name(i).decode()
            t = sd[name]
            if t.numel() != lib.onepose_matcher_tensor_numel(i):
                raise ValueError(f"{name}: {t.numel()} elements, expected "
                                 f"{lib.onepose_matcher_tensor_numel(i)}")
            out.append(t)
        return out

    def packed_weights(self, device):
        tensors = self._weight_tensors()
        # (a parameter without a version counter -- created under inference_mode -- is packed
        # again on every call: an in-place update of it would otherwise go unseen)
        key = (str(device),) + tuple((t.data_ptr(), _version(t)) for t in tensors)
        if (self._packed is not None and self._packed_key == key
                and all(k[1] is not None for k in key[1:])):
            return self._packed
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in tensors]
        arr = (_lib.c_void_p * len(host))(*[h.data_ptr() for h in host])
        buf = np.empty(lib.onepose_matcher_packed_bytes() // 4, dtype=np.float32)
        _lib.check(lib.onepose_matcher_pack(arr, len(host), buf.ctypes.data), "matcher_pack")
        self._packed = torch.from_numpy(buf).to(device)
        self._packed_key = key
        return self._packed

    # ---------------------------------------------------------------- forward
    @staticmethod
    def _operand(x, keep_half=False):
        """[B, C, N] float32 (or float16 with keep_half) with contiguous (C, N); batch stride may
        be 0 (expanded)."""
        x = x if (keep_half and x.dtype == torch.float16) else x.float()
        if x.stride(2) != 1 or x.stride(1) != x.shape[2]:
            x = x.contiguous()
        bstride = x.stride(0) if x.shape[0] > 1 else x.shape[1] * x.shape[2]
        return x, bstride

    def forward(self, data):
        kpts2d, kpts3d = data["keypoints2d"].float(), data["keypoints3d"].float()
        if kpts2d.shape[1] == 0 or kpts3d.shape[1] == 0:
            shape0, shape1 = kpts2d.shape[:-1], kpts3d.shape[:-1]
            return {
                "matches0": kpts2d.new_full(shape0, -1, dtype=torch.int)[0],
                "matches1": kpts3d.new_full(shape1, -1, dtype=torch.int)[0],
                "matching_scores0": kpts2d.new_zeros(shape0)[0],
                "matching_scores1": kpts3d.new_zeros(shape1)[0],
                "skip_train": True,
            }
        if self.match_type != "softmax":
            raise NotImplementedError
        # GATs_SuperGlue.py:219-221 upcasts every descriptor with .float(); fp16 descriptors
        # (all three) go to the library as they are and are converted as its kernels load
        # them (onepose_match_dt): the same bits as upcasting first, half the input bytes
        half = all(data[k].dtype == torch.float16
                   for k in ("descriptors2d_query", "descriptors3d_db", "descriptors2d_db"))
        d2, s2 = self._operand(data["descriptors2d_query"], half)
        d3, s3 = self._operand(data["descriptors3d_db"], half)
        db, sl = self._operand(data["descriptors2d_db"], half)
        cnt = self._counts_arg(data.get("keypoints2d_counts"), d2, data)
        if d2.device.type != "cuda":
            raise RuntimeError("onepose_amd.GATsSuperGlue runs on a ROCm GPU only; "
                               "move the inputs with .cuda()")
        B, C, n1 = d2.shape
        n3 = d3.shape[2]
        nleaf = int(db.shape[2] / n3)
        if nleaf * n3 != db.shape[2] or C != 256 or d3.shape[0] != B or db.shape[0] != B:
            raise ValueError(f"bad matcher input shapes {tuple(d2.shape)} {tuple(d3.shape)} "
                             f"{tuple(db.shape)}")
        dev = d2.device
        if cnt is not None:
            return self._forward_counts(data, cnt, d2, s2, d3, db, B, n1, n3, nleaf, half, dev)
        obj = None
        # (inference tensors carry no version counter, so an in-place write to the object could
        # not be detected: they take the uncached forward, the same bits)
        tracked = not (torch.is_inference(data["descriptors3d_db"]) or
                       torch.is_inference(data["descriptors2d_db"]))
        if (self.resident_object and tracked and B == 1
                and hasattr(_lib.load(), "onepose_match_cached_dt")):
            obj = self._resident(data["descriptors3d_db"], data["descriptors2d_db"], d3, db, n3,
                                 nleaf, half, dev)
        return self._run(d2, s2, d3, s3, db, sl, B, n1, n3, nleaf, dev, obj)

    def _counts_arg(self, cnt, d2, data):
        """``keypoints2d_counts`` checked (before anything touches the device): None, or a [B]
        int32 / int64 tensor on the descriptors' device, for fp32 attention and one object."""
        if cnt is None:
            return None
        if not torch.is_tensor(cnt) or cnt.dtype not in (torch.int32, torch.int64):
            raise TypeError("keypoints2d_counts must be an int32 or int64 tensor, not "
                            f"{cnt.dtype if torch.is_tensor(cnt) else type(cnt).__name__}")
        if tuple(cnt.shape) != (d2.shape[0],):
            raise ValueError(f"keypoints2d_counts of shape {tuple(cnt.shape)}: expected "
                             f"({d2.shape[0]},), one count per sample")
        if cnt.device != d2.device:
            raise ValueError(f"keypoints2d_counts on {cnt.device}, descriptors on {d2.device}")
        if self.precision != PRECISIONS["fp32"]:
            raise ValueError("keypoints2d_counts: attention_precision 'fp32' only")
        for k in ("descriptors3d_db", "descriptors2d_db"):
            if data[k].shape[0] != 1 and data[k].stride(0) != 0:
                raise ValueError(f"keypoints2d_counts: {k} must be one object for the batch "
                                 "(batch 1, or expanded along the batch)")
        return cnt.to(torch.int32).contiguous()

    def _forward_counts(self, data, cnt, d2, s2, d3, db, B, n1, n3, nleaf, half, dev):
        t3, tl = data["descriptors3d_db"], data["descriptors2d_db"]
        if torch.is_inference(t3) or torch.is_inference(tl):   # untracked: prepared per call
            with torch.cuda.device(dev):
                obj = PreparedObject(self.packed_weights(dev), d3[:1], db[:1], self.precision)
            try:
                return self._run(d2, s2, None, 0, None, 0, B, n1, n3, nleaf, dev, obj, cnt)
            finally:
                obj.release()
        obj = self._resident(t3, tl, d3[:1], db[:1], n3, nleaf, half, dev)
        return self._run(d2, s2, None, 0, None, 0, B, n1, n3, nleaf, dev, obj, cnt)

    # The reference's driver calls forward() once per frame with the same object tensors
    # (inference.py:98-182: load_object once, pack_data per frame).  With resident_object, the
    # object-only prefix of the forward (GAT layer 0, the 3D half of self-attention 1) and the
    # leaves' point-major copy are computed once per object (onepose_object_prepare, flags 0)
    # and every later frame starts from them (onepose_match_cached): the same bits as the
    # uncached forward (tests/test_matcher_gpu.py::test_object_cache_is_bit_identical).  The
    # object is recognised by its two descriptor tensors' storage, layout and version counters
    # (an in-place write bumps the version) and the packed weights; the module holds references
    # to them, so their memory cannot be handed to other tensors while cached.
    resident_object = True

    def _resident(self, t3, tl, d3, db, n3, nleaf, half, dev):
        w = self.packed_weights(dev)
        def ident(t):
            return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape),
                    tuple(t.stride()), t.dtype, t._version)
        key = (str(dev), self.precision, half, n3, nleaf, ident(t3), ident(tl), w.data_ptr(),
               self._packed_key)
        cur = self.__dict__.get("_obj")
        if cur is None or cur["key"] != key:
            self._release_resident()
            cur = self._obj = {"key": key, "refs": (t3, tl, d3, db),
                               "prepared": PreparedObject(w, d3, db, self.precision)}
        return cur["prepared"]

    def _release_resident(self):
        cur = self.__dict__.pop("_obj", None)
        if cur is not None:
            cur["prepared"].release()

    def _run(self, d2, s2, d3, s3, db, sl, B, n1, n3, nleaf, dev, obj=None, counts=None):
        lib = _lib.load()
        with torch.cuda.device(dev):
            w = self.packed_weights(dev)
            m0 = torch.empty(B, n1, dtype=torch.int64, device=dev)
            m1 = torch.empty(B, n3, dtype=torch.int64, device=dev)
            ms0 = torch.empty(B, n1, dtype=torch.float32, device=dev)
            ms1 = torch.empty(B, n3, dtype=torch.float32, device=dev)
            conf = torch.empty(B, n1, n3, dtype=torch.float32, device=dev)
            ws_bytes = _lib.workspace_bytes(lib, B, n1, n3, nleaf, True, self.precision)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            dt = _lib.DT_F16 if d2.dtype == torch.float16 else _lib.DT_F32
            args = dict(packed_weights=w, desc2d=d2, desc2d_bstride=s2, batch=B, n1=n1, n3=n3,
                        num_leaf=nleaf, scale_factor=float(_hp(self.hparams, "scale_factor")),
                        match_threshold=float(_hp(self.hparams, "match_threshold")),
                        precision=self.precision, matches0=m0, matches1=m1, mscores0=ms0,
                        mscores1=ms1, conf=conf, workspace=ws, workspace_bytes=ws_bytes,
                        stream=_lib.stream_ptr(dev))
            if obj is not None:
                # built on another stream: this forward runs behind the prepare
                obj.use_on(torch.cuda.current_stream(dev))
            if counts is not None:
                _lib.run("onepose_match_cached_counts", desc_dtype=dt, object_cache=obj.cache,
                         leaves_prepared=obj.leaves_pm, prepared_bstride=0, object_flags=0,
                         counts2d=counts, **args)
            elif obj is not None:
                _lib.run("onepose_match_cached_dt", desc_dtype=dt, object_cache=obj.cache,
                         leaves_prepared=obj.leaves_pm, prepared_bstride=0, object_flags=0, **args)
            else:
                args.update(desc3d=d3, desc3d_bstride=s3, leaves=db, leaves_bstride=sl)
                # (an older A/B build named by ONEPOSE_LIB has only the fp32 entry point, which
                # would read fp16 descriptors as fp32)
                if hasattr(lib, "onepose_match_dt"):
                    _lib.run("onepose_match_dt", desc_dtype=dt, **args)
                elif dt == _lib.DT_F16:
                    raise _lib.OnePoseError("this libonepose_hip build (ABI < 4) has no fp16 "
                                            "descriptor entry point (onepose_match_dt)")
                else:
                    _lib.run("onepose_match_ex", **args)
        pred = {"matches0": m0[0], "matches1": m1[0],
                "matching_scores0": ms0[0], "matching_scores1": ms1[0]}
        return pred, conf


def from_state_dict(state_dict, hparams=None) -> GATsSuperGlue:
    """Build the matcher from a reference-format state dict (numpy arrays or tensors)."""
    from .synthetic import DEFAULT_HPARAMS
    m = GATsSuperGlue(dict(hparams or DEFAULT_HPARAMS))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in state_dict.items()})
    return m.eval()

"""One object made ready for the matcher, and its life cycle in one place.

The leaves go point-major once (``onepose_prepare_leaves_dt``); with ``cache`` the object-only
prefix of the forward -- GAT layer 0 and the 3D half of self-attention 1 -- runs once too
(``onepose_object_prepare_dt``), and every frame starts from it (``onepose_match_cached*``).
The library keeps a host-side record per cache address, so the record has to go
(``onepose_object_release``) before the memory returns to the allocator: ``release()``.
"""
from __future__ import annotations

import torch

from . import _lib


class PreparedObject:
    """``desc3d [256, n3]`` and ``leaves [256, n3*L]`` (device, dense, both fp32 or both fp16;
    a leading batch dimension of 1 is fine) prepared on the current stream with the packed
    ``weights``.  Holds ``leaves_pm``, ``cache`` (None without ``cache``), ``n3``, ``num_leaf``,
    ``precision``, ``flags`` (ONEPOSE_OBJ_*) and ``desc_dt`` (DT_F32 / DT_F16)."""

    def __init__(self, weights, desc3d, leaves, precision, flags=0, cache=True):
        if desc3d.dtype != leaves.dtype or desc3d.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"object descriptors of {desc3d.dtype} / {leaves.dtype}: both fp32 "
                             "or both fp16")
        for x in (desc3d, leaves):
            if x.shape[-2] != 256 or x.stride(-1) != 1 or x.stride(-2) != x.shape[-1]:
                raise ValueError(f"object descriptors must be dense [256, n], not "
                                 f"{tuple(x.shape)} with strides {x.stride()}")
        self.n3 = n3 = desc3d.shape[-1]
        self.num_leaf = L = leaves.shape[-1] // n3
        if L * n3 != leaves.shape[-1]:
            raise ValueError(f"{leaves.shape[-1]} leaves for {n3} points")
        self.precision, self.flags = int(precision), int(flags)
        self.desc_dt = _lib.DT_F16 if desc3d.dtype == torch.float16 else _lib.DT_F32
        lib = _lib.load()
        dev = desc3d.device
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev)
            s = self.stream.cuda_stream
            self.leaves_pm = torch.empty(n3 * L * 256, dtype=torch.float32, device=dev)
            _lib.run("onepose_prepare_leaves_dt", leaves=leaves, dtype=self.desc_dt,
                     leaves_bstride=0, batch=1, n3=n3, num_leaf=L, out=self.leaves_pm, stream=s)
            self.cache = None
            if cache:
                nbytes = _lib.object_cache_bytes(lib, n3, L, self.flags, self.precision)
                self.cache = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                wsb = lib.onepose_object_prepare_workspace_bytes(n3, L)
                # (freed behind the prepare: the allocator is stream-ordered)
                ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
                _lib.run("onepose_object_prepare_dt", packed_weights=weights, desc3d=desc3d,
                         desc_dtype=self.desc_dt, leaves_prepared=self.leaves_pm, n3=n3,
                         num_leaf=L, precision=self.precision, flags=self.flags,
                         cache=self.cache, workspace=ws, workspace_bytes=wsb, stream=s)
            self.ready = torch.cuda.Event()
            self.ready.record(self.stream)

    def use_on(self, stream) -> None:
        """Order `stream` behind the prepare and tell the allocator the object is in use
        there too (nothing to do on the stream it was built on)."""
        if stream != self.stream:
            stream.wait_event(self.ready)
            self.leaves_pm.record_stream(stream)
            if self.cache is not None:
                self.cache.record_stream(stream)

    _released = False

    def release(self) -> None:
        """Drop the library's record of the cache; the tensors stay until the object goes.
        A cached forward on a released object is refused."""
        if not self._released and self.__dict__.get("cache") is not None:
            self._released = True
            _lib.load().onepose_object_release(self.cache.data_ptr())

    def __del__(self):
        try:   # before the cache's memory goes back to the allocator
            self.release()
        except Exception:   # (interpreter exit)
            pass

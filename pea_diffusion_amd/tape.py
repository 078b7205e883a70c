"""`HipTape`: what every wrapper around an op-tape handle of libpea_hip.so shares -- the device guard, the handle and its
release, the weight table and the state-dict loader.  `HipUNet`, `HipControlNet`, the VAE halves, `HipTextEncoder`,
`HipImageEncoder` and `ip_adapter.HipResampler` derive from it and add their own create call and forward."""
from __future__ import annotations

import ctypes
from typing import Dict

import torch

from ._lib import PeaError, check, lib, ptr, stream_ptr


def _staged(device, k, shape, t):
    """weight `k` of a state dict as contiguous fp32 on the device, size-checked against the table's shape"""
    n = 1
    for s in shape:
        n *= s
    if t.numel() != n:
        raise PeaError(f"load_state_dict: {k} has shape {tuple(t.shape)}, expected {shape} (or 1x1 conv)")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class HipTape:
    def _open(self):
        """first thing a subclass's __init__ does: refuse to run without a device, then `self.device` and the empty handle
        `self._h` its create call fills"""
        if not torch.cuda.is_available():
            raise PeaError(f"{type(self).__name__} needs a MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                lib().pea_unet_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def weight_table(self) -> Dict[str, tuple]:
        """{state-dict key: torch shape}"""
        out = {}
        name = ctypes.create_string_buffer(256)
        numel, kind, d0, d1 = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        for i in range(lib().pea_unet_num_weights(self._h)):
            check(lib().pea_unet_weight_info(self._h, i, name, 256, ctypes.byref(numel), ctypes.byref(kind),
                                             ctypes.byref(d0), ctypes.byref(d1)))
            k = kind.value
            if k == 0:
                shape = (d0.value,)
            elif k == 1:
                shape = (d0.value, d1.value)
            else:
                shape = (d0.value, d1.value, 3, 3)
            out[name.value.decode()] = shape
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        table = self.weight_table()
        missing = [k for k in table if k not in sd]
        unexpected = [k for k in sd if k not in table]
        if strict and (missing or unexpected):
            raise PeaError(f"load_state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
        for k, shape in table.items():
            if k not in sd:
                continue
            t = _staged(self.device, k, shape, sd[k])
            check(lib().pea_unet_load_weight(self._h, k.encode(), ptr(t), t.numel(), stream_ptr()))
        torch.cuda.current_stream().synchronize()      # staging tensors above are freed after this call
        return missing, unexpected

    def init_random(self, seed: int = 0):
        check(lib().pea_unet_init_random(self._h, seed, stream_ptr()))

    def memory(self):
        w, a, g, n = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int()
        check(lib().pea_unet_memory(self._h, ctypes.byref(w), ctypes.byref(a), ctypes.byref(g), ctypes.byref(n)))
        return {"weight_bytes": w.value, "activation_bytes": a.value, "grad_bytes": g.value, "n_ops": n.value}

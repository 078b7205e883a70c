"""CPU restatement of FreeU as diffusers 0.23 applies it (`utils/torch_utils.py`: `fourier_filter`, `apply_freeu`; the call in
front of every `torch.cat([hidden_states, res_hidden_states], dim=1)` of `UpBlock2D` / `CrossAttnUpBlock2D`), bound onto the
oracle UNet without touching oracle/: `freeu_unet` rebinds `forward` on the first two `UpBlock`s of a `UNet2DConditionRef`.
Also the closed form of the filter that the HIP kernels evaluate, in the caller's precision, for the tests that compare the two.
diffusers cannot be installed where this was written: a restatement from its source, unpinned like the rest of the UNet
arithmetic.  Test infrastructure only (tests/test_freeu_*.py)."""
import math
import types

import torch
import torch.fft as fft

from oracle.bf16_store import st


def fourier_filter(x_in, threshold, scale):
    """`fourier_filter` of diffusers 0.23: scale the centred 2 threshold x 2 threshold block of the shifted spectrum, keep the
    real part.  (diffusers casts a half-precision map with a non-power-of-two side to fp32 first; the oracle is fp32 or fp64.)"""
    x = x_in
    B, C, H, W = x.shape
    x_freq = fft.fftn(x, dim=(-2, -1))
    x_freq = fft.fftshift(x_freq, dim=(-2, -1))
    mask = torch.ones((B, C, H, W), device=x.device, dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = fft.ifftshift(x_freq, dim=(-2, -1))
    x_filtered = fft.ifftn(x_freq, dim=(-2, -1)).real
    return x_filtered.to(x_in.dtype)


def apply_freeu(resolution_idx, hidden_states, res_hidden_states, s1, s2, b1, b2):
    """`apply_freeu` of diffusers 0.23 (out of place: the caller's tensors stay as they are).  The two tensors that change are
    stored anew by the fused concat, hence `st`: a bf16 rounding in storage mode, the identity otherwise."""
    if resolution_idx not in (0, 1):
        return hidden_states, res_hidden_states
    s, b = (s1, b1) if resolution_idx == 0 else (s2, b2)
    h = hidden_states.shape[1] // 2
    hidden_states = torch.cat([st(hidden_states[:, :h] * b), hidden_states[:, h:]], dim=1)
    res_hidden_states = st(fourier_filter(res_hidden_states, threshold=1, scale=s))
    return hidden_states, res_hidden_states


def freeu_unet(unet, s1, s2, b1, b2):
    """`unet.enable_freeu(s1, s2, b1, b2)` on a `UNet2DConditionRef`: up_blocks[0] / [1] (diffusers' resolution_idx 0 / 1) run
    `apply_freeu` in front of every concat.  Returns the same module; `unfreeu_unet` undoes it."""
    def forward(self, x, res_samples, temb, ctx):
        for j, r in enumerate(self.resnets):
            x, skip = apply_freeu(self._freeu_idx, x, res_samples[-1 - j], s1, s2, b1, b2)
            x = torch.cat([x, skip], dim=1)
            x = r(x, temb)
            if self.attentions is not None:
                x = self.attentions[j](x, ctx)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x
    for i, blk in enumerate(unet.up_blocks[:2]):
        blk._freeu_idx = i
        blk.forward = types.MethodType(forward, blk)
    return unet


def unfreeu_unet(unet):
    for blk in unet.up_blocks[:2]:
        blk.__dict__.pop("forward", None)
    return unet


def freeu_sums(x):
    """x [B, C, H, W] -> [B, 7, C]: S00, C10, S10, C01, S01, C11, S11 of every channel map, in x's precision (the layout of
    pea_op_freeu_coef)"""
    B, C, H, W = x.shape
    ty = (2.0 * math.pi / H) * torch.arange(H, dtype=x.dtype)[:, None]
    tx = (2.0 * math.pi / W) * torch.arange(W, dtype=x.dtype)[None, :]
    basis = torch.stack([torch.ones(H, W, dtype=x.dtype), torch.cos(ty).expand(H, W), torch.sin(ty).expand(H, W),
                         torch.cos(tx).expand(H, W), torch.sin(tx).expand(H, W), torch.cos(ty + tx), torch.sin(ty + tx)])
    return torch.einsum("bchw,khw->bkc", x, basis), basis


def fourier_filter_closed(x, scale):
    """the filter with threshold 1 in closed form: x + (scale - 1) / (H W) * sum_k coef_k basis_k"""
    B, C, H, W = x.shape
    coef, basis = freeu_sums(x)
    return x + (scale - 1.0) / (H * W) * torch.einsum("bkc,khw->bchw", coef, basis)

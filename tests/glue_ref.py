"""Shared pieces of the glue-kernel parity tests (tests/test_glue_ops_gpu.py): sentinel-filled outputs, bit views and
float64 references of the small operations."""
import math

import torch

BF = torch.bfloat16
SENT16 = 0x5A5A                      # bf16 1.53e16: finite, never produced by a test's data
SENT32 = 0x5A5A5A5A                  # fp32 1.54e16, and the same for int32 outputs


def bfr(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF)


def f32r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def sentinel(n, dtype=BF):
    """n elements of `dtype` on the device, every one the sentinel bit pattern"""
    if dtype == BF:
        return torch.full((n,), SENT16, dtype=torch.int16, device="cuda").view(BF)
    return torch.full((n,), SENT32, dtype=torch.int32, device="cuda").view(dtype)


def bits(t):
    """the raw bits of a tensor as integers on the CPU (bf16 -> int16, fp32 / int32 -> int32)"""
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def untouched(t):
    """every element still carries the sentinel pattern, bit for bit"""
    b = bits(t)
    want = SENT16 if t.element_size() == 2 else SENT32
    return bool((b == want).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def rnd(x64):
    """float64 result -> the bf16 the kernel stores (one rounding)"""
    return x64.to(torch.float32).to(BF)


# ---- float64 forms of the maps
def silu64(x):
    return x * torch.sigmoid(x)


def silu_grad64(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def t5_dist_table(L, num_buckets, max_distance):
    """|key - query| -> sub-bucket, as the text encoder's tape builds it on the host (fp32 arithmetic in the reference's order)"""
    import numpy as np
    nb = num_buckets // 2
    max_exact = nb // 2
    tab = []
    for d in range(L):
        if d < max_exact:
            tab.append(d)
            continue
        lg = np.float32(np.log(np.float32(d) / np.float32(max_exact), dtype=np.float32)) \
            / np.float32(math.log(max_distance / max_exact)) * np.float32(nb - max_exact)
        tab.append(min(max_exact + int(np.float32(lg)), nb - 1))
    return torch.tensor(tab, dtype=torch.int32)


def hf_t5_bucket(rel_pos, num_buckets, max_distance):
    """transformers T5Attention._relative_position_bucket, bidirectional; rel_pos = key - query (int64 tensor)"""
    nb = num_buckets // 2
    ret = (rel_pos > 0).to(torch.long) * nb
    n = rel_pos.abs()
    max_exact = nb // 2
    is_small = n < max_exact
    large = max_exact + (torch.log(n.clamp(min=1).float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(is_small, n, large)

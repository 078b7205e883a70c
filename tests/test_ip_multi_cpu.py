"""Several image prompts at once, the host side (no GPU): refusals of pea_op_attention_fwd_ipn and of the pea_unet_ip_*_set
entry points, the per-block scale dict, the mask reduction, list / scalar arguments of HipUNet's methods with the library
stubbed, and the restatement of tests/ip_multi_ref.py against a per-query loop."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from ip_multi_ref import combine, downsample_ref, grid_of, multi_ip_terms, rect_mask
from pea_diffusion_amd import _lib
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd._lib import PeaError


# ---------------------------------------------------------------------------------------------- the op, without a device
def _ipn(sets, Sq=128, Skv=77, ld2=128, causal=0, mask_stride=None, H=2, nullk2=False):
    """rc and error text of pea_op_attention_fwd_ipn on pointers that are never followed: every case is refused first"""
    from pea_diffusion_amd import ops
    fake = C.c_void_p(4096)
    st = ops.ip_sets(sets, [0.5] * len(sets))
    if mask_stride is not None:
        st.mask[0], st.mask_stride[0] = 4096, mask_stride
    L = _lib.lib()
    rc = L.pea_op_attention_fwd_ipn(fake, 64 * H, fake, 64 * H, fake, 64 * H, None if nullk2 else fake, ld2, fake, ld2, fake, 64 * H,
                                    None, 1, H, Sq, Skv, C.byref(st), 0.125, 0, causal, None, None)
    return rc, L.pea_last_error().decode()


@pytest.mark.parametrize("what,kw,text", [
    ("J = 0", dict(sets=[]), "1..4 image key sets"),
    ("J = 5", dict(sets=[2] * 5), "1..4 image key sets"),
    ("an empty set", dict(sets=[4, 0, 4]), "set 1 holds 0 keys"),
    ("sum n = 33", dict(sets=[16, 17]), "33 keys together"),
    ("causal", dict(sets=[4, 16], causal=1), "causal"),
    ("129 text keys", dict(sets=[4, 16], Skv=129), "128 text keys"),
    ("mask batch stride 1", dict(sets=[4, 16], mask_stride=1), "batch stride 1"),
    ("mask batch stride Sq - 1", dict(sets=[4, 16], mask_stride=127), "batch stride 127"),
    ("ldk2 = 132", dict(sets=[4, 16], ld2=132), "multiples of 8"),
    ("ldk2 narrower than the heads", dict(sets=[4, 16], ld2=64), "hold every head"),
    ("no K2", dict(sets=[4, 16], nullk2=True), "no image keys"),
])
def test_ipn_refusals_need_no_device(what, kw, text):
    rc, msg = _ipn(**kw)
    assert rc == -3 and text in msg, (what, rc, msg)


def test_ipn_null_table_and_header():
    L = _lib.lib()
    fake = C.c_void_p(4096)
    assert L.pea_op_attention_fwd_ipn(fake, 128, fake, 128, fake, 128, fake, 128, fake, 128, fake, 128, None, 1, 2, 128, 77, None,
                                      0.125, 0, 0, None, None) == -3
    protos = _lib.parse_header()
    for name in ("pea_op_attention_fwd_ipn", "pea_unet_ip_create_sets", "pea_unet_ip_load_weight_set", "pea_unet_ip_set_tokens_set",
                 "pea_unet_ip_set_scale_set", "pea_unet_ip_clear_set", "pea_unet_ip_set_layer_scales", "pea_unet_ip_query_counts",
                 "pea_unet_ip_set_mask"):
        assert name in protos and protos[name][0] is C.c_int, name
    assert protos["pea_op_attention_fwd_ipn"][1][17] is C.c_void_p             # the table travels by pointer
    from pea_diffusion_amd import ops
    assert C.sizeof(ops.IpSets) == 4 + 16 + 16 + 4 + 32 + 32                    # n_sets, n_keys, weight, padding, mask, mask_stride


def test_runtime_entry_points_reject_null_handles():
    L = _lib.lib()
    n = (C.c_int * 2)(4, 16)
    f = (C.c_float * 2)(1.0, 1.0)
    assert L.pea_unet_ip_create_sets(None, 2, n) == -1
    assert L.pea_unet_ip_load_weight_set(None, 0, b"x.to_k_ip.weight", None, 0, None) == -1
    assert L.pea_unet_ip_set_tokens_set(None, 0, None, None) == -1
    assert L.pea_unet_ip_set_scale_set(None, 1, 0.5) == -1
    assert L.pea_unet_ip_clear_set(None, 0) == -1
    assert L.pea_unet_ip_set_layer_scales(None, 0, f, 2) == -1
    assert L.pea_unet_ip_set_mask(None, 0, 64, None, 1, None) == -1
    assert L.pea_unet_ip_query_counts(None, None, 0, None) == -1
    assert b"pea_unet_ip_query_counts" in L.pea_last_error()


# ---------------------------------------------------------------------------------------------- per-block scales
@pytest.mark.parametrize("cfg", [pc.sdxl_config(), pc.sd15_config()], ids=["sdxl", "sd15"])
def test_block_scale_dict_to_layer_vector(cfg):
    keys = ipa.layer_keys(cfg)
    names = [pfx for _, pfx in keys]
    assert ipa.resolve_layer_scales(cfg, 0.7) == [0.7] * len(keys)
    group = lambda n: "down" if n.startswith("down_blocks") else "up" if n.startswith("up_blocks") else "mid"
    coarse = ipa.resolve_layer_scales(cfg, {"down": 0.25, "up": 0.5, "mid": 1.0})
    assert coarse == [{"down": 0.25, "up": 0.5, "mid": 1.0}[group(n)] for n in names]
    # InstantStyle: one attention block of one up block, everything else off; the longest key wins; `default`
    block = next(n for n in names if n.startswith("up_blocks.")).split(".transformer_blocks")[0]       # up_blocks.<i>.attentions.0
    up_i = ".".join(block.split(".")[:2])
    fine = ipa.resolve_layer_scales(cfg, {block: 1.0})
    assert fine == [1.0 if n.startswith(block + ".") else 0.0 for n in names] and 0 < sum(fine) < len(names)
    mixed = ipa.resolve_layer_scales(cfg, {"up": 0.5, up_i: 0.75, block: 1.0, "default": 0.1})
    want = [1.0 if n.startswith(block + ".") else 0.75 if n.startswith(up_i + ".") else 0.5 if group(n) == "up" else 0.1 for n in names]
    assert mixed == want and {0.1, 0.5, 0.75, 1.0} >= set(mixed) and 1.0 in mixed and 0.1 in mixed
    assert ipa.resolve_layer_scales(cfg, {"mid_block": 0.3}) == [0.3 if group(n) == "mid" else 0.0 for n in names]
    for bad in ("sideways", "up_blocks.9", "up_blocks", "down_blocks.1.attn"):
        if bad == "up_blocks":                                       # a whole group by its module name is a prefix like any other
            assert ipa.resolve_layer_scales(cfg, {bad: 1.0}) == [1.0 if group(n) == "up" else 0.0 for n in names]
            continue
        with pytest.raises(PeaError, match="names no cross-attention layer"):
            ipa.resolve_layer_scales(cfg, {bad: 1.0})


# ---------------------------------------------------------------------------------------------- the mask rule
@pytest.mark.parametrize("h,w,h_l,w_l", [(128, 128, 16, 16), (96, 160, 12, 20), (100, 60, 13, 8), (64, 64, 64, 64), (8, 8, 16, 32)])
def test_downsample_mask_is_bicubic_interpolate(h, w, h_l, w_l):
    g = torch.Generator().manual_seed(h * w + h_l)
    m = (torch.rand(2, h, w, generator=g) > 0.5)
    want = F.interpolate(m[:, None].float(), size=(h_l, w_l), mode="bicubic", align_corners=False)[:, 0].reshape(2, h_l * w_l)
    got = ipa.downsample_mask(m, h_l, w_l)
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want)
    assert torch.equal(ipa.downsample_mask(m[0].float(), h_l, w_l), want[:1])               # [h, w] -> [1, h_l w_l]
    assert torch.equal(got, downsample_ref(m.float(), h_l, w_l))                            # the restatement the GPU tests use
    with pytest.raises(PeaError):
        ipa.downsample_mask(torch.zeros(1, 1, 8, 8), 4, 4)


def test_rect_mask_leaves_the_unit_interval():
    for h_l, w_l in ((4, 4), (8, 8), (13, 20), (64, 64)):
        for variant in range(4):
            m = ipa.downsample_mask(rect_mask(h_l, w_l, variant), h_l, w_l)
            assert m.min() < -0.05 and m.max() > 1.05 and tuple(m.shape) == (1, h_l * w_l)
    assert grid_of(1024, 128, 128) == (32, 32) and grid_of(364, 52, 28) == (26, 14) and grid_of(117, 17, 25) == (9, 13)


# ---------------------------------------------------------------------------------------------- HipUNet's methods, library stubbed
class _StubLib:
    """records (name, args) of every pea_* call and answers 0; query_counts answers [64, 16]"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name == "pea_unet_ip_query_counts":
                h, counts, cap, n = args
                n._obj.value = 2
                if counts is not None:
                    counts[0], counts[1] = 64, 16
            return 0
        return call

    def names(self):
        return [n for n, _ in self.calls]


class _Ad(ipa._LayerMap):
    def __init__(self, n_tokens, cfg):
        self.n_tokens, self.cfg = n_tokens, cfg
        self.layers = {"a.to_k_ip.weight": torch.zeros(2, 2), "a.to_v_ip.weight": torch.zeros(2, 2)}


@pytest.fixture
def stub_unet(monkeypatch):
    from pea_diffusion_amd import unet as pu
    stub = _StubLib()
    monkeypatch.setattr(pu, "lib", lambda: stub)
    monkeypatch.setattr(pu, "ptr", lambda t: None if t is None else ("ptr", tuple(t.shape)))
    monkeypatch.setattr(pu, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: type("S", (), {"synchronize": lambda self: None})())
    u = object.__new__(pu.HipUNet)
    u._h, u.cfg, u.B, u.H, u.W, u.device = C.c_void_p(1), pc.tiny_config(), 2, 16, 16, torch.device("cpu")
    yield u, stub
    u._h = C.c_void_p()                                              # nothing for HipTape.__del__ to destroy


def test_list_and_scalar_forms(stub_unet):
    u, stub = stub_unet
    cfg = u.cfg
    a4, a16 = _Ad(4, cfg), _Ad(16, cfg)
    # scalar form: the entry points of one adapter, as before
    assert u.load_ip_adapter(a4) is a4
    assert stub.names() == ["pea_unet_ip_create", "pea_unet_ip_load_weight", "pea_unet_ip_load_weight"]
    assert stub.calls[0][1][1] == 4
    stub.calls.clear()
    u.set_ip_tokens(torch.zeros(2, 4, 128))
    u.set_ip_adapter_scale(0.7)
    assert stub.names() == ["pea_unet_ip_set_tokens", "pea_unet_ip_set_layer_scales", "pea_unet_ip_set_scale_set"]
    assert stub.calls[1][1][1:] == (0, None, 0) and stub.calls[2][1][1:] == (0, 0.7)
    with pytest.raises(PeaError):
        u.set_ip_tokens(torch.zeros(2, 5, 128))
    with pytest.raises(PeaError, match="2 entries for 1 adapters"):
        u.set_ip_adapter_scale([0.5, 0.5])
    u.unload_ip_adapter()
    with pytest.raises(PeaError, match="load_ip_adapter first"):
        u.set_ip_tokens(torch.zeros(2, 4, 128))
    # list form
    stub.calls.clear()
    got = u.load_ip_adapter([a4, a16])
    assert got == [a4, a16] and stub.names()[0] == "pea_unet_ip_create_sets" and stub.names().count("pea_unet_ip_load_weight_set") == 4
    assert stub.calls[0][1][1] == 2 and list(stub.calls[0][1][2]) == [4, 16]
    assert [c[1][1] for c in stub.calls if c[0] == "pea_unet_ip_load_weight_set"] == [0, 0, 1, 1]
    stub.calls.clear()
    u.set_ip_tokens([torch.zeros(2, 4, 128), torch.zeros(2, 16, 128)])
    assert [(n, a[1]) for n, a in stub.calls] == [("pea_unet_ip_set_tokens_set", 0), ("pea_unet_ip_set_tokens_set", 1)]
    stub.calls.clear()
    u.set_ip_tokens([None, torch.zeros(2, 16, 128)])                 # None: that adapter's tokens stay
    assert [(n, a[1]) for n, a in stub.calls] == [("pea_unet_ip_set_tokens_set", 1)]
    with pytest.raises(PeaError, match="one entry per adapter"):
        u.set_ip_tokens(torch.zeros(2, 4, 128))
    with pytest.raises(PeaError, match="adapter 1"):
        u.set_ip_tokens([torch.zeros(2, 4, 128), torch.zeros(2, 4, 128)])
    # scales: a number goes to every adapter; a list entry may be a per-block dict
    stub.calls.clear()
    u.set_ip_adapter_scale(0.5)
    assert [(n, a[1:]) for n, a in stub.calls if n == "pea_unet_ip_set_scale_set"] == [("pea_unet_ip_set_scale_set", (0, 0.5)),
                                                                                      ("pea_unet_ip_set_scale_set", (1, 0.5))]
    stub.calls.clear()
    u.set_ip_adapter_scale([{"down": 0.7, "mid": 0.2}, 0.4])
    (_, a0), (_, s0), (_, a1), (_, s1) = stub.calls
    want = ipa.resolve_layer_scales(cfg, {"down": 0.7, "mid": 0.2})
    assert a0[1] == 0 and a0[3] == len(want) == len(ipa.layer_keys(cfg)) and list(a0[2]) == pytest.approx(want) and s0[1:] == (0, 1.0)
    assert a1[1:] == (1, None, 0) and s1[1:] == (1, 0.4)
    # masks: None or a tensor per adapter, one reduced mask per query count
    stub.calls.clear()
    u.set_ip_adapter_masks([None, torch.ones(1, 128, 128)])
    sets = [(a[1], a[2], a[3], a[4]) for n, a in stub.calls if n == "pea_unet_ip_set_mask"]
    assert sets == [(0, 0, None, 0), (1, 64, ("ptr", (1, 64)), 1), (1, 16, ("ptr", (1, 16)), 1)]
    stub.calls.clear()
    u.set_ip_adapter_masks([torch.ones(2, 32, 32), torch.ones(24, 24)])
    sets = [(a[1], a[2], a[3], a[4]) for n, a in stub.calls if n == "pea_unet_ip_set_mask"]
    assert sets == [(0, 64, ("ptr", (2, 64)), 2), (0, 16, ("ptr", (2, 16)), 2), (1, 64, ("ptr", (1, 64)), 1), (1, 16, ("ptr", (1, 16)), 1)]
    with pytest.raises(PeaError, match="expected"):
        u.set_ip_adapter_masks([torch.ones(3, 8, 8), None])
    # clear / unload: everything, or one adapter
    stub.calls.clear()
    u.clear_ip_tokens(1)
    u.clear_ip_tokens()
    assert [(n, a[1:]) for n, a in stub.calls] == [("pea_unet_ip_clear_set", (1,)), ("pea_unet_ip_clear", ())]
    stub.calls.clear()
    u.unload_ip_adapter(0)                                           # the rest is loaded again as a list of one
    assert stub.names()[:2] == ["pea_unet_ip_destroy", "pea_unet_ip_create_sets"] and list(stub.calls[1][1][2])[:1] == [16]
    assert u._ip == [a16]
    u.unload_ip_adapter()
    assert u._ip is None and stub.names()[-1] == "pea_unet_ip_destroy"


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_against_a_per_query_loop():
    B, H, Sq, Skv, sets, w = 2, 2, 6, 5, (2, 1, 3), [0.6, -1.0, 0.8]
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, n, H * 64, generator=g) for n in (Sq, Skv, Skv))
    k2, v2 = (torch.randn(B, sum(sets), H * 64, generator=g) for _ in range(2))
    masks = [None, torch.randn(1, Sq, generator=g), torch.randn(B, Sq, generator=g)]
    kv_len = [5, 3]
    o1, lse, terms = multi_ip_terms(q, k, v, k2, v2, H, sets, kv_len)
    ref, mag = combine(o1, terms, w, masks)
    want, want_mag, want_lse = torch.zeros_like(q), torch.zeros_like(q), torch.zeros(B, H, Sq)
    for b in range(B):
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            for i in range(Sq):
                def attend(keys, vals):
                    s = [float(q[b, i, c] @ kk[c]) * 0.125 for kk in keys]
                    mx = max(s)
                    e = [math.exp(x - mx) for x in s]
                    return sum(p * vv[c] for p, vv in zip(e, vals)) / sum(e), mx + math.log(sum(e))
                o, l = attend(k[b, :kv_len[b]], v[b, :kv_len[b]])
                m, off = o.abs(), 0
                for j, n in enumerate(sets):
                    oj, _ = attend(k2[b, off:off + n], v2[b, off:off + n])
                    f = w[j] * (1.0 if masks[j] is None else float(masks[j][b if masks[j].shape[0] > 1 else 0, i]))
                    o, m, off = o + f * oj, m + abs(f) * oj.abs(), off + n
                want[b, i, c], want_mag[b, i, c], want_lse[b, h, i] = o, m, l
    torch.testing.assert_close(ref, want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(mag, want_mag, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse, want_lse, rtol=1e-5, atol=1e-5)

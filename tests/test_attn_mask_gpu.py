"""-m gpu: the key-length, causal and bias masks of every attention kernel (csrc/attention.hip) against the fp32 reference of
tests/attn_mask_ref.py, through pea_op_attention_fwd_text / pea_op_attention_bwd_masked.

Forward: O within 2 bf16 ulps, lse within rtol 1e-3 / atol 2e-3 -- the numbers of tests/test_ops_gpu.py::test_attention_fwd_bwd, at
the same logit sizes (tests/test_attn_mask_cpu.py checks the score spread of every case).
Backward: O and lse come from the library's own masked forward; dQ / dK / dV within 4 ulps PER SAMPLE (a short sample's dK / dV
are larger and must not set the scale for the others), rows >= kv_len[b] of dK / dV exactly zero (write form) or bit-identical
to what was there (accumulate form), nothing written around the destinations, two launches equal bit for bit.
Ill-conditioned rows (test_attention_softmax_spike's rule and numbers): a query with reference max P > 0.9 is held to
|err| < 0.25 x rms(dQ of the sample's other rows), a key that captures such a query to 0.5 x rms(dK of the sample's other keys);
where a sample has no other rows (kv_len = 1: P = 1 on every row, every gradient of a score is an exact 0) the smallest such rms
among the case's other samples is the scale.  tests/test_attn_mask_cpu.py bounds the share of such rows per case (30 %).
Which kernel form a case reaches is read from the dispatch code and listed beside the cases in tests/attn_mask_ref.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from attn_mask_ref import (BWD_CASES, BWD_PARAMS, FWD_CASES, attn_mask_ref, bwd_inputs, case_scale, fwd_inputs, hard_rows,  # noqa: E402
                           padded_log2_bias)
from test_layouts_gpu import Canvas, vp  # noqa: E402
from test_ops_gpu import ALPHA, BF, bfr, close_bf16, close_f32, ops  # noqa: E402,F401


def _lens(kv_len):
    return None if kv_len is None else torch.tensor(kv_len, dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=None)
def _fwd_ref(case_id, prescaled):
    """inputs and the fp32 reference of a forward case, computed once"""
    case = next(c for c in FWD_CASES if c["id"] == case_id)
    q, k, v, q_ref, bias_nat = fwd_inputs(case, prescaled)
    oref, lref = attn_mask_ref(q_ref, k.float(), v.float(), case["H"], case_scale(case), case.get("causal", False),
                               case.get("kv_len"), bias_nat)
    return (q, k, v, bias_nat), oref, lref


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c["id"])
def test_attention_fwd_masks(ops, case, prescaled):
    (q, k, v, bias_nat), oref, lref = _fwd_ref(case["id"], prescaled)
    H, causal = case["H"], case.get("causal", False)
    bias = None if bias_nat is None else padded_log2_bias(bias_nat).cuda()
    args = dict(scale=case_scale(case), q_prescaled=prescaled, causal=causal, kv_len=_lens(case.get("kv_len")), bias=bias)
    o, lse = ops.attention_fwd_text(q.cuda(), k.cuda(), v.cuda(), H, **args)
    tag = f"attn-mask fwd {case['id']} pre{int(prescaled)}"
    assert torch.isfinite(lse).all(), tag
    close_bf16(tag + " O", o, oref, ulps=2.0)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)
    o2, lse2 = ops.attention_fwd_text(q.cuda(), k.cuda(), v.cuda(), H, **args)
    assert torch.equal(o, o2) and torch.equal(lse, lse2), tag + ": two launches differ"
    if bias is None and not prescaled:
        # pea_op_attention_fwd_masked is the same launch; O alone (lse = NULL) is the same O
        om, lm = ops.attention_fwd_masked(q.cuda(), k.cuda(), v.cuda(), H, causal=causal, kv_len=_lens(case.get("kv_len")),
                                          want_lse=True)
        assert torch.equal(om, o) and torch.equal(lm, lse), tag + ": _masked and _text entries differ"
        assert torch.equal(ops.attention_fwd_masked(q.cuda(), k.cuda(), v.cuda(), H, causal=causal, kv_len=_lens(case.get("kv_len"))), o)


# ---------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_ref(case_id, prescaled):
    """inputs, fp32 gradients (autograd through the masked reference) and the ill-conditioned rows of a backward case, once"""
    case = next(c for c in BWD_CASES if c["id"] == case_id)
    q, k, v, do, q_ref = bwd_inputs(case, prescaled)
    qr = q_ref.clone().requires_grad_(True)
    kr, vr = [t.float().requires_grad_(True) for t in (k, v)]
    oref, _ = attn_mask_ref(qr, kr, vr, case["H"], 0.125, False, case["kv_len"])
    oref.backward(do.float())
    hard, captured = hard_rows(case, prescaled)
    return (q, k, v, do), (qr.grad, kr.grad, vr.grad), hard, captured


def _rms(t):
    return t.pow(2).mean().sqrt().item() if t.numel() else None


def _check_grads(tag, case, got, ref, base, hard, captured):
    """got / ref: {name: [B, S, H*64]} (cpu; ref fp32 = base + gradient, base = None in the write form).  Per sample: 4 ulps on
    the well-conditioned part, the absolute bounds of the module docstring on the rest; dV whole."""
    B, H, kv_len = case["B"], case["H"], case["kv_len"]
    grad = {n: (ref[n] if base is None else ref[n] - base[n]) for n in ref}          # the pure gradients: they set the loose scales
    if "dQ" in got:
        easy_rms = [_rms(grad["dQ"][b].view(-1, H, 64)[~hard[b].T]) for b in range(B)]
        for b in range(B):
            e = ~hard[b].T                                                               # [Sq, H]
            g, r = got["dQ"][b].float().view(-1, H, 64), ref["dQ"][b].view(-1, H, 64)
            if e.any():
                close_bf16(f"{tag} dQ sample {b} ({int(e.sum())} rows)", g[e], r[e], ulps=4.0)
            if (~e).any():
                scale = easy_rms[b] if easy_rms[b] is not None else min(x for x in easy_rms if x is not None)
                worst = (g[~e] - r[~e]).abs().max().item()
                print(f"[{tag} dQ sample {b}, {int((~e).sum())} concentrated rows] max_abs={worst:.3e} rms(other rows)={scale:.3e}")
                assert worst < 0.25 * scale, f"{tag} dQ sample {b}: {worst} vs 0.25 x {scale}"
    if "dK" in got:
        free_rms = [_rms(grad["dK"][b, :kv_len[b]].view(-1, H, 64)[~captured[b, :, :kv_len[b]].T]) for b in range(B)]
        for b in range(B):
            n = kv_len[b]
            f = ~captured[b, :, :n].T                                                    # [n, H]
            g, r = got["dK"][b, :n].float().view(n, H, 64), ref["dK"][b, :n].view(n, H, 64)
            if f.any():
                close_bf16(f"{tag} dK sample {b} ({n} keys)", g[f], r[f], ulps=4.0)
            if (~f).any():
                scale = free_rms[b] if free_rms[b] is not None else min(x for x in free_rms if x is not None)
                worst = (g[~f] - r[~f]).abs().max().item()
                print(f"[{tag} dK sample {b}, {int((~f).sum())} capturing keys] max_abs={worst:.3e} rms(other keys)={scale:.3e}")
                assert worst < 0.5 * scale, f"{tag} dK sample {b}: {worst} vs 0.5 x {scale}"
            close_bf16(f"{tag} dV sample {b} ({n} keys)", got["dV"][b, :n], ref["dV"][b, :n], ulps=4.0)


def _run_bwd(L, case, form, prescaled, dev, o, lse, kv, accum, fill=None):
    """one launch of pea_op_attention_bwd_masked into fresh canvases (rows and columns of sentinel around every destination)
    -> {name: canvas}; fill: {name: [B*S, C]} to accumulate onto"""
    from pea_diffusion_amd._lib import check, stream_ptr
    B, H, Sq, Skv = case["B"], case["H"], case["Sq"], case["Skv"]
    C = H * 64
    q, k, v, do = dev
    names = {"all": ("dQ", "dK", "dV"), "dkv": ("dK", "dV"), "dq": ("dQ",)}[form["grads"]]
    cv = {n: Canvas(B * (Sq if n == "dQ" else Skv), C + 32, [(16, C)]) for n in names}
    if fill is not None:
        for n in names:
            cv[n].win().copy_(fill[n])
    scratch = None
    if form["scratch"]:
        nb = L.pea_op_attention_bwd_scratch_bytes(B, H, Sq, Skv, 1)
        assert nb > 0, "the scratch is passed but this shape would run unsplit"
        scratch = torch.empty(nb, device="cuda", dtype=torch.uint8)
    delta = torch.empty(2, B, H, Sq, device="cuda", dtype=torch.float32)
    win = lambda n: vp(cv[n].win()) if n in cv else None
    check(L.pea_op_attention_bwd_masked(vp(q), C, vp(k), C, vp(v), C, vp(o), C, vp(do), C, vp(lse), vp(delta), win("dQ"), C + 32,
                                        win("dK"), C + 32, win("dV"), C + 32, B, H, Sq, Skv, 0.125, accum, accum, 1, vp(scratch),
                                        int(prescaled), vp(kv), stream_ptr()))
    torch.cuda.synchronize()
    return cv


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case,form", BWD_PARAMS, ids=lambda x: x["id"])
def test_attention_bwd_kv_len(ops, case, form, prescaled):
    from pea_diffusion_amd._lib import lib
    L = lib()
    B, H, Sq, Skv, kv_len = case["B"], case["H"], case["Sq"], case["Skv"], case["kv_len"]
    C = H * 64
    (q, k, v, do), grads, hard, captured = _bwd_ref(case["id"], prescaled)
    ref = dict(zip(("dQ", "dK", "dV"), grads))
    dev = tuple(t.cuda() for t in (q, k, v, do))
    kv = _lens(kv_len)
    o, lse = ops.attention_fwd_text(dev[0], dev[1], dev[2], H, q_prescaled=prescaled, kv_len=kv)    # the library's own masked forward
    tag = f"attn-mask bwd {case['id']} {form['id']} pre{int(prescaled)}"
    shape = lambda n: (B, Sq if n == "dQ" else Skv, C)
    try:
        if form["ver"] is not None:
            L.pea_debug_set_xattn_bwd_v2(form["ver"])
        L.pea_debug_set_attn_fused_bwd(form["fused"])
        L.pea_debug_set_attn_tr(form["tr"])
        # ---- write form, twice
        cv = _run_bwd(L, case, form, prescaled, dev, o, lse, kv, accum=0)
        cv2 = _run_bwd(L, case, form, prescaled, dev, o, lse, kv, accum=0)
        got = {}
        for n, c in cv.items():
            c.check(f"{tag} {n}")
            assert torch.equal(c.win().view(torch.int16), cv2[n].win().view(torch.int16)), f"{tag} {n}: two launches differ"
            got[n] = c.win().cpu().view(shape(n))
            assert torch.isfinite(got[n].float()).all(), f"{tag} {n}"
        for n in ("dK", "dV"):
            if n in got:
                for b in range(B):
                    if kv_len[b] < Skv:
                        assert (got[n][b, kv_len[b]:] == 0).all(), f"{tag} {n} sample {b}: rows behind kv_len={kv_len[b]} are not zero"
        _check_grads(tag, case, got, {n: ref[n] for n in got}, None, hard, captured)
        # ---- accumulate form: the destinations already hold another consumer's share
        x0 = {n: bfr(*shape(n), seed=20 + i) for i, n in enumerate(("dQ", "dK", "dV")) if n in got}
        ca = _run_bwd(L, case, form, prescaled, dev, o, lse, kv, accum=1, fill={n: t.view(-1, C).cuda() for n, t in x0.items()})
        acc = {}
        for n, c in ca.items():
            c.check(f"{tag} {n} accumulate")
            acc[n] = c.win().cpu().view(shape(n))
        for n in ("dK", "dV"):
            if n in acc:
                for b in range(B):
                    if kv_len[b] < Skv:
                        same = torch.equal(acc[n][b, kv_len[b]:].view(torch.int16), x0[n][b, kv_len[b]:].view(torch.int16))
                        assert same, f"{tag} {n} sample {b} accumulate: rows behind kv_len={kv_len[b]} changed"
        base = {n: t.float() for n, t in x0.items()}
        _check_grads(tag + " accumulate", case, acc, {n: base[n] + ref[n] for n in acc}, base, hard, captured)
    finally:
        L.pea_debug_set_xattn_bwd_v2(3)
        L.pea_debug_set_attn_fused_bwd(1)
        L.pea_debug_set_attn_tr(1)


@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_bwd_masked_without_kv_len_is_the_plain_backward(ops, prescaled):
    """kv_len = NULL: the new entry gives the bits of pea_op_attention_bwd / _prescaled"""
    B, H, Sq, Skv = 2, 2, 260, 77
    q, k, v, do = bfr(B, Sq, H * 64, seed=1), bfr(B, Skv, H * 64, seed=2), bfr(B, Skv, H * 64, seed=3), bfr(B, Sq, H * 64, seed=4)
    if prescaled:
        q = (q.float() * ALPHA).to(BF)
    q, k, v, do = q.cuda(), k.cuda(), v.cuda(), do.cuda()
    o, lse = ops.attention_fwd(q, k, v, H, q_prescaled=prescaled)
    plain = ops.attention_bwd(q, k, v, o, do, lse, H, q_prescaled=prescaled)
    masked = ops.attention_bwd_masked(q, k, v, o, do, lse, H, q_prescaled=prescaled, kv_len=None)
    full = ops.attention_bwd_masked(q, k, v, o, do, lse, H, q_prescaled=prescaled, kv_len=_lens([Skv] * B))
    for n, a, b_, c in zip(("dQ", "dK", "dV"), plain, masked, full):
        assert torch.equal(a, b_), f"{n}: kv_len = NULL differs from pea_op_attention_bwd"
        assert torch.equal(a, c), f"{n}: kv_len = Skv for every sample differs from no mask"

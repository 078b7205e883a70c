"""No GPU: the masked-attention reference of tests/attn_mask_ref.py against torch's SDPA in float64, and the conditions the
cases of tests/test_attn_mask_gpu.py rely on -- so that a case which stopped reaching its kernel form, or whose inputs drifted
into the ill-conditioned regime, fails here and not silently there."""
import pytest
import torch
import torch.nn.functional as F

from attn_mask_ref import (BIAS_PAD, BWD_CASES, BWD_PARAMS, FWD_CASES, HARD_SHARE, additive_mask, attn_mask_ref, bias_pitch,
                           bwd_inputs, case_scale, fwd_inputs, hard_rows, one_pass_kernel, padded_log2_bias)


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c["id"])
def test_reference_matches_sdpa_in_float64(case):
    """O of the reference = F.scaled_dot_product_attention(attn_mask=...) on the same float64 inputs; lse = logsumexp of the
    masked scores computed here a second way (log of the explicit sum)"""
    B, H, Sq, Skv = case["B"], case["H"], case["Sq"], case["Skv"]
    q, k, v, q_ref, bias = fwd_inputs(case, prescaled=False)
    scale, causal, kv_len = case_scale(case), case.get("causal", False), case.get("kv_len")
    q64, k64, v64 = q_ref.double(), k.double(), v.double()
    b64 = None if bias is None else bias.double()
    o, lse = attn_mask_ref(q64, k64, v64, H, scale, causal, kv_len, b64)
    sp = lambda t: t.view(B, -1, H, 64).transpose(1, 2)
    m = additive_mask(Sq, Skv, causal, kv_len, b64, dtype=torch.float64)
    ref = F.scaled_dot_product_attention(sp(q64), sp(k64), sp(v64), attn_mask=m, scale=scale).transpose(1, 2).reshape(B, Sq, H * 64)
    torch.testing.assert_close(o, ref, rtol=1e-12, atol=1e-12)
    s = sp(q64) @ sp(k64).transpose(-1, -2) * scale + (0 if m is None else m)
    torch.testing.assert_close(lse, s.exp().sum(-1).log(), rtol=1e-12, atol=1e-12)
    # the fp32 run the GPU tests compare with is the same function: it agrees with float64 far inside their tolerances
    o32, lse32 = attn_mask_ref(q_ref, k.float(), v.float(), H, scale, causal, kv_len, bias)
    torch.testing.assert_close(o32.double(), o, rtol=0, atol=2e-5)
    torch.testing.assert_close(lse32.double(), lse, rtol=0, atol=2e-5)


def test_reference_gradients_of_cut_keys_are_exact_zeros():
    case = BWD_CASES[0]
    q, k, v, do, q_ref = bwd_inputs(case, prescaled=False)
    qr, kr, vr = [t.float().requires_grad_(True) for t in (q, k, v)]
    o, _ = attn_mask_ref(qr, kr, vr, case["H"], 0.125, False, case["kv_len"])
    o.backward(do.float())
    for b, n in enumerate(case["kv_len"]):
        if n < case["Skv"]:
            assert kr.grad[b, n:].abs().max().item() == 0 and vr.grad[b, n:].abs().max().item() == 0
        assert vr.grad[b, :n].abs().min().item() > 0


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c["id"])
def test_forward_case_conditions(case):
    B, H, Sq, Skv = case["B"], case["H"], case["Sq"], case["Skv"]
    kv_len, causal, bias = case.get("kv_len"), case.get("causal", False), case.get("bias", False)
    assert kv_len is not None or causal or bias, "a case without any mask or bias tests nothing here"
    if kv_len is not None:
        assert len(kv_len) == B and all(1 <= n <= Skv for n in kv_len)      # every row keeps a valid key; 0 is outside the contract
    # launch_attention_fwd's choice (attn_fwd_nd): resident keys need no causal mask, no bias, Sq >= 128 and Skv <= 128
    resident = not causal and not bias and Sq >= 128 and Skv <= 128
    assert case["kernel"] == ("xattn" if resident else "text")
    for prescaled in (False, True):
        q, k, v, q_ref, bias_nat = fwd_inputs(case, prescaled)
        assert q.dtype == k.dtype == v.dtype == torch.bfloat16
        assert (bias_nat is not None) == bool(bias)
        # logit size the tolerances (O 2 ulps, lse 1e-3 / 2e-3) were set for: unit inputs at scale 1/8, i.e. scores of variance ~1
        s = (q_ref.view(B, Sq, H, 64).transpose(1, 2) @ k.float().view(B, Skv, H, 64).transpose(1, 2).transpose(-1, -2)) * case_scale(case)
        assert 0.8 < s.std().item() < 1.25, s.std().item()
        if bias_nat is not None:
            assert 1.4 < bias_nat.std().item() < 1.6
            pb = padded_log2_bias(bias_nat)
            assert pb.shape == (H, Sq, bias_pitch(Skv)) and pb.is_contiguous() and torch.isfinite(pb).all()
            assert bias_pitch(Skv) % 64 == 0 and 0 <= bias_pitch(Skv) - Skv < 64
            if bias_pitch(Skv) > Skv:
                assert (pb[..., Skv:] == BIAS_PAD).all()


def test_forward_cases_cover_the_edges():
    ids = {c["id"]: c for c in FWD_CASES}
    assert {32, 33} <= set(ids["xattn-3blocks"]["kv_len"])                                  # a count on a 32-key edge, one past it
    assert {n % 32 for n in ids["xattn-4blocks"]["kv_len"]} == {0, 1}
    assert {n - 64 for n in ids["text-200keys"]["kv_len"]} == {1, 0, -1}                    # around the 64-key tile edge
    assert any(n <= 64 for n in ids["text-trailing-tiles"]["kv_len"]) and ids["text-trailing-tiles"]["Skv"] > 128   # tiles masked whole
    assert bias_pitch(ids["bias-nopad"]["Skv"]) == ids["bias-nopad"]["Skv"]
    assert bias_pitch(ids["bias-pitch128"]["Skv"]) == 128 and bias_pitch(ids["bias-pitch192"]["Skv"]) == 192


@pytest.mark.parametrize("case,form", BWD_PARAMS, ids=lambda x: x["id"])
def test_backward_case_conditions(case, form):
    from pea_diffusion_amd._lib import lib
    L = lib()
    B, H, Sq, Skv, kv_len = case["B"], case["H"], case["Sq"], case["Skv"], case["kv_len"]
    assert len(kv_len) == B and all(1 <= n <= Skv for n in kv_len) and kv_len[0] == Skv
    assert Sq % 4 == 0                                                       # launch_attention_bwd's own condition
    try:
        if form["ver"] is not None:
            L.pea_debug_set_xattn_bwd_v2(form["ver"])
        nb = L.pea_op_attention_bwd_scratch_bytes(B, H, Sq, Skv, 1)            # host only: the split rule of the selected kernel
    finally:
        L.pea_debug_set_xattn_bwd_v2(3)
    if form["scratch"]:
        assert nb > 0 and Sq >= 512 and Skv <= 128, "a case that passes the scratch must run split"
    if form["grads"] == "all" and Skv <= 128:
        assert form["ver"] is not None and form["kernel"] == one_pass_kernel(form["ver"], Skv)
    elif form["grads"] == "all":
        assert form["kernel"] == ("general-fused" if form["fused"] else "general-split")
        assert sum(n <= 128 for n in kv_len) >= 2, "two samples whose second 128-key workgroup is all padding"
    else:
        assert form["kernel"] == form["grads"]


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c["id"])
def test_backward_cases_are_mostly_well_conditioned(case, prescaled):
    """the loose rule for query rows with max P > 0.9 is a condition, not a licence: at most 30 % of a case's rows"""
    hard, captured = hard_rows(case, prescaled)
    share = hard.float().mean().item()
    print(f"[{case['id']} pre{int(prescaled)}] ill-conditioned query rows {share:.4f}, captured keys {int(captured.sum())}")
    assert share <= HARD_SHARE, share
    for b, n in enumerate(case["kv_len"]):
        assert not captured[b, :, n:].any()                                  # a cut key captures nothing
        if n == 1:
            assert hard[b].all()                                             # one key: P = 1 exactly

"""CPU checks of the LoRA weight path: key resolution (pea_diffusion_amd/lora.py) against the full SDXL, SSD-1B and SD1.5 key
sets, and the argument checks of the two C entry points, which answer without a device.

The kohya, diffusers and PEFT spellings below are BUILT from the naming conventions stated in lora.py's docstring, not read
from a published LCM-LoRA file: none is available offline."""
import ctypes

import pytest
import torch

from pea_diffusion_amd import _lib
from pea_diffusion_amd.lora import (check_factors, kohya_names, load_lora_state_dict, merged_weight, resolve_lora)


def key_table(name):
    """{state-dict key: shape} of the oracle UNet of that size, built on the meta device (no memory, no init)"""
    from oracle import unet_ref as ou
    with torch.device("meta"):
        m = ou.UNet2DConditionRef(getattr(ou, name)())
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def targets(table):
    return [k for k, s in table.items() if k.endswith(".weight") and len(s) in (2, 4)]


def factors(shape, rank, tag):
    """(down, up) of the right sizes; down[0, ..., 0] carries `tag` so a resolved pair can be told from every other"""
    if len(shape) == 4:
        down, up = torch.zeros(rank, *shape[1:]), torch.zeros(shape[0], rank, 1, 1)
    else:
        down, up = torch.zeros(rank, shape[1]), torch.zeros(shape[0], rank)
    down.view(-1)[0] = float(tag)
    return down, up


def spell(style, key, down, up, alpha=None):
    mod = key[:-len(".weight")]
    if style == "kohya":
        base = "lora_unet_" + mod.replace(".", "_")
        d = {base + ".lora_down.weight": down, base + ".lora_up.weight": up}
        if alpha is not None:
            d[base + ".alpha"] = torch.tensor(float(alpha))
        return d
    if style == "diffusers":
        return {f"unet.{mod}.lora.down.weight": down, f"unet.{mod}.lora.up.weight": up}
    if style == "peft":
        return {f"base_model.model.{mod}.lora_A.weight": down, f"base_model.model.{mod}.lora_B.weight": up}
    if style == "peft_unet":
        return {f"unet.{mod}.lora_A.default.weight": down, f"unet.{mod}.lora_B.default.weight": up}
    raise ValueError(style)


@pytest.mark.parametrize("cfg_name,n_min", [("sdxl_config", 700), ("ssd1b_config", 300), ("sd15_config", 200)])
def test_every_matrix_key_resolves_one_to_one_in_every_spelling(cfg_name, n_min):
    table = key_table(cfg_name)
    keys = targets(table)
    assert len(keys) >= n_min and len(kohya_names(table)) == sum(k.endswith(".weight") for k in table)
    for style in ("kohya", "diffusers", "peft", "peft_unet"):
        sd = {}
        for i, k in enumerate(keys):
            sd.update(spell(style, k, *factors(table[k], 2, i + 1)))
        got, skipped = resolve_lora(sd, table)
        assert not skipped and set(got) == set(keys), style
        for i, k in enumerate(keys):
            down, up, alpha = got[k]
            assert down.shape == (2, int(torch.tensor(table[k][1:]).prod())) and up.shape == (table[k][0], 2)
            assert float(down[0, 0]) == i + 1 and alpha == 2.0, (style, k)


def test_processor_spelling_alpha_text_encoder_keys_and_errors():
    table = key_table("tiny_config")
    q = next(k for k in table if k.endswith("attn1.to_q.weight"))
    o = next(k for k in table if k.endswith("attn1.to_out.0.weight"))
    conv = next(k for k in table if k.endswith("conv1.weight"))
    attn = q[:-len(".to_q.weight")]
    dq, uq = factors(table[q], 4, 7)
    do, uo = factors(table[o], 4, 8)
    sd = {f"unet.{attn}.processor.to_q_lora.down.weight": dq, f"unet.{attn}.processor.to_q_lora.up.weight": uq,
          f"unet.{attn}.processor.to_out_lora.down.weight": do, f"unet.{attn}.processor.to_out_lora.up.weight": uo}
    sd.update(spell("kohya", conv, *factors(table[conv], 8, 9), alpha=2.0))
    sd["lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = torch.zeros(4, 8)
    sd["lora_te2_text_model_encoder_layers_0_mlp_fc1.alpha"] = torch.tensor(4.0)
    sd["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora.down.weight"] = torch.zeros(4, 8)
    got, skipped = resolve_lora(sd, table)
    assert set(got) == {q, o, conv} and len(skipped) == 3
    assert got[q][2] == 4.0 and float(got[q][0][0, 0]) == 7 and float(got[o][0][0, 0]) == 8      # alpha = rank without one
    assert got[conv][2] == 2.0 and got[conv][0].shape == (8, table[conv][1] * 9) and got[conv][1].shape == (table[conv][0], 8)
    # a UNet key that names nothing is an error that lists it, never a silent skip
    with pytest.raises(_lib.PeaError, match="lora_unet_no_such_module"):
        resolve_lora(dict(sd, **{"lora_unet_no_such_module.lora_down.weight": torch.zeros(4, 8)}), table)
    with pytest.raises(_lib.PeaError, match="no_such.module"):
        resolve_lora({"unet.no_such.module.lora.down.weight": torch.zeros(4, 8)}, table)
    with pytest.raises(_lib.PeaError, match="both down and up"):
        resolve_lora({f"unet.{q[:-7]}.lora.down.weight": dq}, table)
    # factor sizes against the weight's shape, rank range, vector targets
    with pytest.raises(_lib.PeaError, match="does not give"):
        resolve_lora(spell("peft", q, dq[:, :-1].contiguous(), uq), table)
    with pytest.raises(_lib.PeaError, match="does not give"):
        resolve_lora(spell("peft", q, dq, uq[:-1].contiguous()), table)
    with pytest.raises(_lib.PeaError, match="does not give"):
        resolve_lora(spell("peft", q, dq, torch.zeros(table[q][0], 5)), table)
    with pytest.raises(_lib.PeaError, match="rank 300"):
        resolve_lora(spell("peft", q, *factors(table[q], 300, 1)), table)
    with pytest.raises(_lib.PeaError, match="vector"):
        check_factors("x.bias", (8,), torch.zeros(2, 1), torch.zeros(8, 2))


def test_safetensors_and_pickle_round_trip(tmp_path):
    from safetensors.torch import save_file
    table = key_table("tiny_config")
    g = torch.Generator().manual_seed(0)
    sd = {}
    for k in targets(table)[:6]:
        d, u = factors(table[k], 3, 1)
        sd.update(spell("kohya", k, torch.randn(d.shape, generator=g), torch.randn(u.shape, generator=g), alpha=1.5))
    save_file(sd, str(tmp_path / "lora.safetensors"))
    torch.save(sd, str(tmp_path / "lora.bin"))
    want, _ = resolve_lora(sd, table)
    for name in ("lora.safetensors", "lora.bin"):
        back = load_lora_state_dict(str(tmp_path / name))
        assert set(back) == set(sd)
        got, _ = resolve_lora(back, table)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]) and got[k][2] == 1.5
    assert load_lora_state_dict(sd) is sd


def test_merged_weight_is_the_conv_product():
    g = torch.Generator().manual_seed(1)
    W = torch.randn(6, 5, 3, 3, generator=g)
    down, up = torch.randn(2, 5, 3, 3, generator=g), torch.randn(6, 2, 1, 1, generator=g)
    want = W.double() + 0.5 * torch.einsum("or,rikl->oikl", up[:, :, 0, 0].double(), down.double())
    got = merged_weight(W, [(down, up, 0.5)])
    assert got.shape == W.shape and got.dtype == W.dtype and torch.allclose(got.double(), want, rtol=0, atol=1e-6)
    # ... which is what the composed convolution computes
    x = torch.randn(1, 5, 8, 8, generator=g)
    F = torch.nn.functional
    y = F.conv2d(x, W, padding=1) + 0.5 * F.conv2d(F.conv2d(x, down, padding=1), up)
    assert torch.allclose(F.conv2d(x, got, padding=1), y, rtol=1e-4, atol=1e-4)


def test_c_entry_points_report_argument_errors_without_a_device():
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused before any device work
    assert L.pea_op_lora_compose(one, one, one, one, 8, 8, 0, 1.0, None) == -3 and b"rank=0" in L.pea_last_error()
    assert L.pea_op_lora_compose(one, one, one, one, 8, 8, 257, 1.0, None) == -3 and b"rank=257" in L.pea_last_error()
    assert L.pea_op_lora_compose(one, one, one, one, 0, 8, 4, 1.0, None) == -3 and b"M=0" in L.pea_last_error()
    assert L.pea_op_lora_compose(one, None, one, one, 8, 8, 4, 1.0, None) == -1
    ptrs = (ctypes.c_void_p * 2)(16, 16)
    scales = (ctypes.c_float * 2)(1.0, 1.0)
    bad, good = (ctypes.c_int * 2)(4, 0), (ctypes.c_int * 2)(4, 4)
    call = lambda h, n, ranks, ups=ptrs: L.pea_unet_load_weight_lora(h, b"w", one, 64, n, ptrs, ups, ranks, scales, None)
    assert call(None, 2, bad) == -3 and b"adapter 1 has rank=0" in L.pea_last_error()
    assert call(None, 0, good) == -1 and b"n_adapters=0" in L.pea_last_error()
    assert call(None, 2, good, (ctypes.c_void_p * 2)(16, None)) == -1 and b"null factor" in L.pea_last_error()
    assert call(None, 2, good) == -1 and b"null handle" in L.pea_last_error()
    assert L.pea_op_lcm_update(one, one, None, None, 0, 1.0, 1.0, 1.0, 0.0, None) == -3 and b"n=0" in L.pea_last_error()
    assert L.pea_op_lcm_update(None, one, None, None, 8, 1.0, 1.0, 1.0, 0.0, None) == -1

"""Which combinations of the UNet's attention features a context takes, and what they compute: one JSON line.

One tiny UNet (inference, B = 2, 16 x 16 latents, a context of 96 rows = two prompts of 48, so regions, an edit and heat maps are
each admissible alone; weights and inputs from fixed seeds) and six features: a live image prompt, regional prompts (R = 2), heat
maps, a prompt edit, StyleAligned sharing (ref = (-1, 0)) and self-attention guidance on the default layer.  For each feature alone
and each of the 30 ordered pairs: clear everything, set A, then B, run one forward, clear everything, run a plain forward.  Per
case: the call that refused ("set:<feature>", "forward" or "ok"), its return code and the full text of pea_last_error (the outcome,
tests/golden/feature_combos.json, tests/test_feature_combos_gpu.py); for an accepted case the SHA-256 of eps and, where they are
there, of the heat-map accumulators and the column sums; and whether the plain forward afterwards has the bits of the first one.
Two builds of the library that print the same line refuse the same calls with the same words and compute the same bits:
python scripts/lib_ab.py 1 scripts/feature_digest.py  (profiles/feature_digest.json is the line of the committed sources on an MI355X.)"""
import hashlib, json, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd._lib import PeaError
from pea_diffusion_amd.prompt2prompt import PromptEdit, equalizer, refine_mapper
from pea_diffusion_amd.unet import HipUNet

B, HW, L, N_TOK, T = 2, 16, 96, 4, 2
FEATURES = ("ip", "regions", "maps", "edit", "style", "sag")
SRC_IDS = list(range(200, 230))
TGT_IDS = SRC_IDS[:4] + [901, 902] + SRC_IDS[4:11] + [903] + SRC_IDS[11:]


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _adapter_file(cfg, seed=5):
    """a base IP-Adapter file of N_TOK tokens for `cfg`, every tensor seeded"""
    cross = cfg.cross_attention_dim
    proj = {"proj.weight": _rnd(N_TOK * cross, 64, seed=seed, scale=0.1), "proj.bias": torch.zeros(N_TOK * cross),
            "norm.weight": torch.ones(cross), "norm.bias": torch.zeros(cross)}
    layers = {}
    for (idx, _), (_, C) in zip(ipa.layer_keys(cfg), ipa._cross_layers(cfg)):
        for j, nm in enumerate(("to_k_ip", "to_v_ip")):
            layers[f"{idx}.{nm}.weight"] = _rnd(C, cross, seed=seed + 2 * idx + j, scale=cross ** -0.5)
    return {"image_proj": proj, "ip_adapter": layers}


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _refusal(where, err):
    m = re.match(r"pea error (-?\d+): (.*)", str(err), re.S)
    return {"refused": where, "rc": int(m.group(1)) if m else None, "message": m.group(2) if m else str(err)}


def walk():
    """-> {case: {"refused", "rc", "message", "eps", "maps", "colsum", "plain_restored"}}, case = "A" or "A+B" (A set first)"""
    cfg = pc.tiny_config()
    hip = HipUNet(cfg, B, HW, HW, L, needs_grad=False)
    hip.init_random(3)
    hip.load_ip_adapter(_adapter_file(cfg))                  # an adapter without tokens is no image prompt
    x, t = _rnd(B, 4, HW, HW, seed=1).cuda(), torch.tensor([250, 500]).cuda()
    ehs = _rnd(B, L, cfg.cross_attention_dim, seed=2).cuda()
    added = {"text_embeds": _rnd(B, cfg.pooled_dim, seed=3).cuda(),
             "time_ids": torch.tensor([[HW * 8, HW * 8, 0, 0, HW * 8, HW * 8]] * B).cuda()}
    tokens = _rnd(B, N_TOK, cfg.cross_attention_dim, seed=4)
    left = torch.zeros(8 * HW, 8 * HW)
    left[:, : 4 * HW] = 1.0
    edit = PromptEdit.compose(L, T, [None, dict(source=0, refine=refine_mapper(SRC_IDS, TGT_IDS, L), equalizer=equalizer(L, {2: 2.0}))],
                              cross_replace_steps=0.5, self_replace_steps=0.5, self_max_tokens=64)

    def set_edit():
        hip.set_prompt_edit(edit)
        hip.set_prompt_edit_step(0)

    setters = {"ip": lambda: hip.set_ip_tokens(tokens), "regions": lambda: hip.set_prompt_regions([left, 1.0 - left]),
               "maps": hip.enable_attention_maps, "edit": set_edit, "style": lambda: hip.set_style_aligned(ref=[-1, 0]),
               "sag": hip.enable_sag}

    def clear_all():
        hip.clear_ip_tokens()
        hip.clear_prompt_regions()
        hip.disable_attention_maps()
        hip.clear_prompt_edit()
        hip.clear_style_aligned()
        hip.disable_sag()

    run = lambda: hip(x, t, ehs, added_cond_kwargs=added)[0].clone()
    clear_all()
    plain = _sha(run())
    out = {}
    for case in [(a,) for a in FEATURES] + [(a, b) for a in FEATURES for b in FEATURES if a != b]:
        clear_all()
        rec = {"refused": "ok", "rc": 0, "message": "", "eps": None, "maps": None, "colsum": None}
        try:
            where = None
            for f in case:
                where = "set:" + f
                setters[f]()
            where = "forward"
            eps = run()
            rec["eps"] = _sha(eps)
            if "maps" in case:
                rec["maps"] = _sha(*[m for _, (m, _) in sorted(hip.attention_maps().items())])
            if "sag" in case:
                rec["colsum"] = _sha(hip.sag_colsum())
        except PeaError as e:
            rec.update(_refusal(where, e))
        clear_all()
        rec["plain_restored"] = _sha(run()) == plain
        out["+".join(case)] = rec
    return out


if __name__ == "__main__":
    print(json.dumps(walk(), sort_keys=True))

#!/usr/bin/env python3
"""Records tests/golden/attn_dispatch.json: what the attention launchers launch (pea_debug_attn_dispatch) over a fixed case list.

    python scripts/record_attn_dispatch.py [--rev REV] [--work DIR] [--lib PATH] [--out PATH] [--coverage]

The fixture pins behaviour, so it is recorded from the commit that HAS the behaviour to keep: REV (default HEAD~1, the parent of
the commit that changes the rules), never the tree under test.  REV's csrc is checked out into DIR, and in that scratch copy of
attention.hip every launch site RECORDS its instantiation, grid, LDS bytes and scalar arguments instead of launching (PATCHES
below: launch_lds, the two LDS-less launches, the device query behind the launchers); an entry point appended to the copy builds
the AttnP of a case and calls REV's own launch_attention_fwd / _bwd / _fwd_fewq.  The copy is built with its own Makefile and is
never committed.  The enumerators of include/pea_hip.h go in as a table of kernel addresses (instantiations()).  Afterwards the tree's own
library (--lib) is asked the same cases and every difference is printed: the recording must be reproduced record for record.
--coverage prints, per enumerator, the first GPU test case of gpu_tests() that launches it (profiles/EXPERIMENTS.md).  Needs no GPU.

Case = [direction, B, H, Sq, Skv, nd, features, Skv2, sets, set mask bits, xattn_ver, use_tr, xattn, fused_bwd]; see
include/pea_hip.h.  Expectation = [error code] or [launches, nsplit, then per launch: enumerator, grid x, y, z, LDS bytes, a0, a1].
The file stores each problem once, each distinct expectation once and each list of switch values once (pack()).
Sections: "default" plus one per environment switch, which tests/test_attn_dispatch_cpu.py replays in a child process.
"""
import argparse
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAUSAL, KVLEN, BIAS, PRE, K2, ZEROW, DQ, DK, DV, SCRATCH, ACCUM = (1 << i for i in range(11))
ALL = DQ | DK | DV
FWD, BWD, FEWQ = 0, 1, 2
N_ENUMERATORS = 52
ENV_SECTIONS = {"PEA_XATTN_BWD_VER=0": ("PEA_XATTN_BWD_VER", "0"), "PEA_XATTN_BWD_VER=2": ("PEA_XATTN_BWD_VER", "2"),
                "PEA_XATTN_OFF=1": ("PEA_XATTN_OFF", "1"), "PEA_ATTN_BWD_SPLIT=1": ("PEA_ATTN_BWD_SPLIT", "1")}
ENV_NAMES = sorted({k for k, _ in ENV_SECTIONS.values()})
OWN = (-1, -1, -1, -1)                                         # the process's own switches
ENVS_FWD = [(3, tr, x, 1) for tr in (1, 0) for x in (1, 0)]    # what the forward reads
ENVS_ALL = [(ver, tr, x, f) for ver in (3, 0, 2) for tr in (1, 0) for x in (1, 0) for f in (1, 0)] + [(1, 1, 1, 1)]
ENVS_VER = [(ver, 1, 1, 1) for ver in (3, 0, 2)]
ENVS_EACH = ENVS_VER + [(3, 0, 1, 1), (3, 1, 0, 1), (3, 1, 1, 0), (3, 0, 0, 0), (0, 1, 0, 0), (2, 1, 0, 1)]   # every value of every switch
ENVS_GENERAL = [(3, tr, 1, f) for tr in (1, 0) for f in (1, 0)]


def case(direction, B, H, Sq, Skv, nd=1, feat=0, Skv2=0, sets=0, masks=0, env=OWN):
    return [direction, B, H, Sq, Skv, nd, feat, Skv2, sets, masks, *env]


# ---------------------------------------------------------------------------------------------- the case list
def graph_shapes():
    """(B, H, Sq, Skv, nd) of the attention ops of every graph in tests/test_attn_census_cpu.py, at the benchmark's and the tests'
    batch sizes (levels without a transformer included: a superset)"""
    sys.path.insert(0, ROOT)
    from pea_diffusion_amd import config as pc
    out = set()
    for name, hw, L in [("sdxl_config", 128, 77), ("sdxl_config", 64, 52), ("sd15_config", 64, 77), ("ssd1b_config", 128, 77),
                        ("ssd1b_uniform_config", 64, 77), ("tiny_config", 16, 12), ("tiny15_config", 16, 12)]:
        cfg = getattr(pc, name)()
        for lvl, (C, heads) in enumerate(zip(cfg.block_out_channels, cfg.num_attention_heads)):
            tokens, nd = (hw >> lvl) ** 2, -(-(C // heads) // 64)
            for B in (1, 2, 4, 8):
                out.add((B, heads, tokens, tokens, nd))
                out.add((B, heads, tokens, L, nd))
    return sorted(out)


def text_shapes():
    """(B, H, S, features) of the text towers: CLIP-L / bigG causal, the BERT family with key counts, mT5 with a score bias"""
    out = []
    for heads, S, feat in [(12, 77, CAUSAL), (20, 77, CAUSAL), (16, 52, KVLEN), (16, 77, KVLEN), (32, 77, KVLEN | BIAS), (2, 12, CAUSAL),
                           (2, 12, KVLEN), (3, 12, KVLEN | BIAS)]:
        out += [(B, heads, S, feat) for B in (1, 2, 4)]
    return out


# (test id, case) of the GPU attention tests: their shapes as the Python wrappers hand them to the library (ops.attention_bwd
# always passes the split scratch, attention_bwd_masked on request)
def gpu_tests():
    t = []
    for use_tr, pre in ((1, 1), (1, 0), (0, 0)):
        for (B, H, Sq, Skv) in [(2, 2, 256, 256), (1, 3, 128, 77), (2, 2, 16, 16), (1, 2, 1024, 200), (1, 1, 64, 7), (2, 2, 1024, 77),
                                (1, 2, 576, 77), (1, 2, 364, 77), (2, 3, 1456, 77), (1, 2, 640, 128), (1, 2, 512, 100), (1, 2, 260, 33)]:
            tid = f"test_ops_gpu.py::test_attention_fwd_bwd[{B}-{H}-{Sq}-{Skv}-{use_tr}-{bool(pre)}]"
            env = (3, use_tr, 1, 1)
            t.append((tid, case(FWD, B, H, Sq, Skv, feat=PRE * pre, env=env)))
            t.append((tid, case(BWD, B, H, Sq, Skv, feat=PRE * pre | ALL | SCRATCH, env=env)))
    for pre in (1, 0):
        for (B, H, Sq, Skv) in [(2, 3, 1024, 77), (1, 2, 4096, 77), (2, 2, 1000, 52), (1, 2, 2048, 64), (1, 1, 192, 77), (1, 2, 576, 96),
                                (3, 2, 640, 40)]:
            tid = f"test_ops_gpu.py::test_cross_attention_bwd_specialised_waves[{B}-{H}-{Sq}-{Skv}-{bool(pre)}]"
            t.append((tid, case(FWD, B, H, Sq, Skv, feat=PRE * pre, env=(3, 1, 1, 1))))
            for ver in (3, 0, 2):
                t.append((tid, case(BWD, B, H, Sq, Skv, feat=PRE * pre | ALL | SCRATCH, env=(ver, 1, 1, 1))))
            t.append((tid, case(BWD, B, H, Sq, Skv, feat=PRE * pre | ALL | ACCUM, env=(3, 1, 1, 1))))
    for (d, H, Sq, Skv, tr) in [(40, 8, 256, 256, 1), (80, 4, 128, 77, 1), (160, 2, 64, 64, 1), (128, 2, 192, 200, 1), (16, 8, 64, 20, 1),
                                (80, 2, 192, 200, 0), (160, 1, 192, 200, 0)]:
        tid = f"test_ops_gpu.py::test_attention_padded_heads[{d}-{H}-{Sq}-{Skv}{'' if tr else '-gather'}]"
        t.append((tid, case(FWD, 2, H, Sq, Skv, nd=-(-d // 64), env=(3, tr, 1, 1))))
        t += [(tid, case(BWD, 2, H, Sq, Skv, nd=-(-d // 64), feat=ALL | SCRATCH, env=(3, tr, 1, f))) for f in ((1,) if tr else (1, 0))]
    for (B, H, S, causal, padded) in [(2, 2, 77, True, False), (3, 4, 52, False, True), (2, 3, 200, True, True), (1, 2, 130, True, False),
                                      (2, 2, 64, False, True)]:
        t.append((f"test_ops_gpu.py::test_attention_text_masks[{B}-{H}-{S}-{causal}-{padded}]",
                  case(FWD, B, H, S, S, feat=CAUSAL * causal | KVLEN * padded)))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from attn_mask_ref import BWD_PARAMS, FWD_CASES
    for c in FWD_CASES:
        for pre in (0, 1):
            feat = PRE * pre | CAUSAL * bool(c.get("causal")) | KVLEN * (c.get("kv_len") is not None) | BIAS * bool(c.get("bias"))
            t.append((f"test_attn_mask_gpu.py::test_attention_fwd_masks[{c['id']}-{bool(pre)}]", case(FWD, c["B"], c["H"], c["Sq"], c["Skv"], feat=feat)))
    for c, f in BWD_PARAMS:
        for pre in (0, 1):
            tid = f"test_attn_mask_gpu.py::test_attention_bwd_kv_len[{c['id']}-{f['id']}-{bool(pre)}]"
            t.append((tid, case(FWD, c["B"], c["H"], c["Sq"], c["Skv"], feat=PRE * pre | KVLEN)))          # (its own masked forward)
            grads = {"all": ALL, "dkv": DK | DV, "dq": DQ}[f["grads"]]
            env = (3 if f["ver"] is None else f["ver"], f["tr"], 1, f["fused"])
            t.append((tid, case(BWD, c["B"], c["H"], c["Sq"], c["Skv"], feat=PRE * pre | KVLEN | grads | SCRATCH * f["scratch"], env=env)))
    for (B, H, Sq, Skv, N) in [(1, 1, 64, 7, 1), (2, 2, 16, 16, 4), (1, 3, 128, 77, 4), (1, 2, 364, 77, 16), (1, 2, 260, 33, 5), (1, 2, 512, 100, 17),
                               (1, 2, 640, 128, 32), (2, 10, 4096, 77, 4), (2, 2, 256, 77, 4), (1, 2, 364, 100, 16)]:
        for pre in (0, 1):
            t.append((f"test_ip_adapter_gpu.py::test_attention_fwd_ip*[{B}-{H}-{Sq}-{Skv}-{N}-{bool(pre)}]", case(FWD, B, H, Sq, Skv, feat=PRE * pre | K2, Skv2=N)))
    for (B, H, Sq, Skv, sets) in [(1, 1, 64, 7, (1, 1)), (2, 2, 16, 16, (4, 4)), (1, 3, 128, 77, (4, 16)), (1, 2, 364, 77, (16, 16)),
                                  (1, 2, 260, 33, (5, 3, 7)), (1, 2, 200, 128, (4, 16, 4, 8)), (2, 2, 300, 77, (3, 29)), (2, 10, 4096, 77, (4, 16)),
                                  (2, 2, 256, 77, (4, 16)), (1, 2, 364, 100, (5, 3, 7))]:
        for masks in (0, (1 << len(sets)) - 1):
            t.append((f"test_ip_multi_gpu.py::test_attention_fwd_ipn*[{B}-{H}-{Sq}-{Skv}-{sets}-masks{masks}]",
                      case(FWD, B, H, Sq, Skv, feat=K2, Skv2=sum(sets), sets=len(sets), masks=masks)))
    for (B, H, Sq, S1, S2) in [(1, 1, 1, 1, 0), (1, 2, 16, 3, 1), (2, 2, 16, 31, 16), (1, 2, 17, 32, 32), (1, 3, 32, 33, 1), (1, 2, 5, 50, 5),
                               (2, 20, 16, 257, 16), (1, 12, 16, 577, 16), (1, 2, 8, 1025, 0)]:
        t.append((f"test_ip_adapter_plus_gpu.py::test_attention_fwd_fewq_vs_fp32[{B}-{H}-{Sq}-{S1}-{S2}]", case(FEWQ, B, H, Sq, S1, feat=K2 * bool(S2), Skv2=S2)))
    # tests/test_layouts_gpu.py: self-attention in a fused Q|K|V buffer (all gradients with the scratch, plain and accumulating; dQ
    # only; dK and dV only), cross-attention on the stacked K|V buffer (every one-pass form, with and without the scratch)
    for (B, H, S, d, pre) in [(1, 10, 1584, 64, 1), (1, 10, 1456, 64, 0), (2, 20, 392, 64, 1), (1, 20, 364, 64, 0), (1, 20, 396, 64, 1),
                              (1, 10, 1568, 64, 1), (1, 8, 1456, 80, 1), (1, 8, 364, 160, 0)]:
        nd, tid = -(-d // 64), f"test_layouts_gpu.py::test_self_attention_fused_qkv_layout[{B}-{H}-{S}-{d}-{bool(pre)}]"
        t.append((tid, case(FWD, B, H, S, S, nd, PRE * pre)))
        t += [(tid, case(BWD, B, H, S, S, nd, PRE * pre | f)) for f in (ALL | SCRATCH, ALL | SCRATCH | ACCUM, DQ, DK | DV)]
        tid = f"test_layouts_gpu.py::test_cross_attention_stacked_kv_layout[{B}-{H}-{S}-{d}-{bool(pre)}]"
        t.append((tid, case(FWD, B, H, S, 77, nd, PRE * pre)))
        for ver in ((3, 2, 0) if nd == 1 else (3,)):
            t += [(tid, case(BWD, B, H, S, 77, nd, PRE * pre | ALL | f, env=(ver, 1, 1, 1))) for f in (SCRATCH, 0, SCRATCH | ACCUM, ACCUM)]
    # the three aspect-ratio buckets of tests/test_buckets_gpu.py at the tiny and the SDXL head counts
    for (h, w) in [(56, 104), (72, 88), (112, 56)]:
        for lvl, heads in ((0, 1), (1, 2), (2, 2), (1, 10), (2, 20)):
            tokens = (h >> lvl) * (w >> lvl)
            for Skv in (tokens, 77, 12):
                t.append((f"test_buckets_gpu.py[{h}x{w}]", case(FWD, 2, heads, tokens, Skv, feat=PRE)))
                t.append((f"test_buckets_gpu.py[{h}x{w}]", case(BWD, 2, heads, tokens, Skv, feat=PRE | ALL | SCRATCH)))
    return t


def default_cases():
    c = []
    # 1. what the graphs launch: forward, the adapter-training backward (all gradients, scratch); at the benchmark's batch under
    #    every value of every switch (their full cross product: section 3), and the first layer's dK / dV-only and the dQ-only forms
    for (B, H, Sq, Skv, nd) in graph_shapes():
        c += [case(FWD, B, H, Sq, Skv, nd, PRE, env=e) for e in (ENVS_FWD if B == 4 else ENVS_FWD[:1])]
        if Sq % 4 == 0:
            c += [case(BWD, B, H, Sq, Skv, nd, PRE | ALL | SCRATCH, env=e) for e in (ENVS_EACH if B == 4 else ENVS_VER if B == 2 else ENVS_VER[:1])]
            c += [case(BWD, B, H, Sq, Skv, nd, PRE | g | sc) for g in (DQ, DK | DV) for sc in (SCRATCH, 0) if B == 4]
    for (B, H, S, feat) in text_shapes():
        c += [case(FWD, B, H, S, S, 1, PRE | feat, env=e) for e in ENVS_FWD]
    # 2. the GPU tests' shapes
    c += [q for _, q in gpu_tests()]
    # 3. the rule boundaries.  Keys x queries, forward: every switch the forward reads, plain and with image keys
    keys, queries = (32, 33, 64, 65, 80, 81, 96, 97, 128, 129), (31, 32, 33, 127, 128, 129, 511, 512)
    for Skv, Sq in itertools.product(keys, queries):
        c += [case(FWD, 2, 10, Sq, Skv, env=e) for e in ENVS_FWD]
        c += [case(FWD, 2, 10, Sq, Skv, feat=f, env=(3, 1, 1, 1)) for f in ((KVLEN, CAUSAL, BIAS) if Sq in (127, 128, 512) else (KVLEN,))]
        c += [case(FWD, 2, 10, Sq, Skv, feat=K2, Skv2=16, sets=s, masks=m) for s, m in ((0, 0), (2, 1))]
    for Skv, Sq, nd in itertools.product((77, 128, 129), (127, 128, 512), (2, 3)):
        c += [case(FWD, 2, 10, Sq, Skv, nd, env=e) for e in ENVS_FWD]
    #    backward: all gradients under every switch combination, with and without the scratch; dQ only / dK and dV only
    for Skv, Sq in itertools.product(keys, (32, 128, 512, 1024)):
        c += [case(BWD, 2, 10, Sq - 4, Skv, feat=ALL | SCRATCH, env=e) for e in ENVS_VER]
        c += [case(BWD, 2, 10, Sq, Skv, feat=ALL | SCRATCH | pre, env=e) for e in ENVS_ALL for pre in ((0, PRE) if e[1:] == (1, 1, 1) else (PRE,))]
        c += [case(BWD, 2, 10, Sq, Skv, feat=ALL, env=e) for e in ENVS_VER]
        if Sq in (128, 512):
            c += [case(BWD, 2, 10, Sq, Skv, feat=g | sc | KVLEN, env=e) for g in (DQ, DK | DV) for sc in (SCRATCH, 0) for e in ENVS_GENERAL]
            c += [case(BWD, 2, 10, Sq, Skv, feat=g | SCRATCH) for g in (DQ | DK, DV, 0)]
    for Sq in (31, 33, 127, 129, 511):                                     # refused: the backward wants Sq % 4 == 0
        c.append(case(BWD, 2, 10, Sq, 77, feat=ALL))
    for Skv, Sq, nd in itertools.product((77, 128, 129, 300), (128, 1024), (1, 2, 3)):
        c += [case(BWD, 2, 4, Sq, Skv, nd, ALL | sc, env=e) for sc in (SCRATCH, 0) for e in ENVS_GENERAL + [(3, 1, 0, 1), (3, 1, 0, 0)]]
        c += [case(BWD, 2, 4, Sq, Skv, nd, g | SCRATCH, env=e) for g in (DQ, DK | DV) for e in ENVS_GENERAL]
    #    units per workgroup of the resident-K/V forward: B * H * units either side of multiples of 512
    for Sq, bhs in ((4096, (15, 16, 17, 31, 32, 33, 47, 48, 49)), (1024, (63, 64, 65, 127, 128, 129, 191, 192, 193)), (16384, (3, 4, 5, 8, 9)),
                    (1000, (64, 65, 128, 129)), (128, (511, 512, 513, 1024, 1025))):
        for bh in bhs:
            c.append(case(FWD, 1, bh, Sq, 77, feat=PRE))
            c.append(case(FWD, 1, bh, Sq, 77, feat=PRE | K2, Skv2=4))
    #    the query-split cost rule
    for bh, Sq, Skv in itertools.product((1, 40, 80, 160, 511, 512, 513), (512, 1000, 1024, 1456, 4096, 16384), (32, 77, 96, 128)):
        B = 8 if bh % 8 == 0 else 1
        c += [case(BWD, B, bh // B, Sq, Skv, feat=PRE | ALL | SCRATCH, env=e) for e in ENVS_VER]
        if Skv == 77:
            c += [case(BWD, B, bh // B, Sq, Skv, nd, feat=ALL | SCRATCH) for nd in (2, 3)]
            c.append(case(BWD, B, bh // B, Sq, Skv, feat=DK | DV | SCRATCH))
    # 4. image key sets: one, several, masks, all-zero weights, per-sample key counts; few queries
    for Skv, Sq, Skv2 in itertools.product((7, 33, 77, 128), (16, 1000), (4, 32)):
        for sets, masks in ((0, 0), (1, 0), (1, 1), (2, 0), (3, 5), (4, 15)):
            c += [case(FWD, 2, 10, Sq, Skv, feat=K2 | z | kl, Skv2=Skv2, sets=sets, masks=masks) for z, kl in ((0, 0), (ZEROW, 0), (0, KVLEN))
                  if not (z and sets == 0)]
    for Sq, Skv, Skv2 in itertools.product((1, 16, 32), (1, 77, 257, 1000), (0, 16, 32)):
        c.append(case(FEWQ, 2, 20, Sq, Skv, feat=K2 * bool(Skv2) | PRE, Skv2=Skv2))
    # 5. what the launchers refuse
    c += [case(BWD, 2, 2, 128, 77, feat=ALL | f) for f in (CAUSAL, BIAS, CAUSAL | BIAS)]
    c += [case(BWD, 2, 2, 128, 77, nd, feat=ALL | KVLEN) for nd in (2, 3)]
    c += [case(FWD, 2, 2, 128, Skv, nd, feat=f) for Skv in (77, 200) for nd in (2, 3) for f in (CAUSAL, KVLEN, BIAS)]
    c += [case(FWD, 2, 2, 128, 77, nd, feat=K2, Skv2=4) for nd in (2, 3)]
    c += [case(FWD, 2, 2, 128, Skv, feat=K2, Skv2=4) for Skv in (128, 129, 200)]
    c += [case(FWD, 2, 2, 128, 77, feat=K2 | f, Skv2=4) for f in (CAUSAL, BIAS)]
    c += [case(FWD, 2, 2, 128, 77, feat=K2, Skv2=n, sets=s) for n, s in ((0, 0), (33, 0), (8, 5), (2, 3))]
    c += [case(FWD, 2, 2, 128, 77, nd) for nd in (0, 4)] + [case(FWD, 0, 2, 128, 77), case(BWD, 2, 2, 128, 0, feat=ALL)]
    c += [case(FEWQ, 2, 2, 33, 77), case(FEWQ, 2, 2, 16, 77, nd=2), case(FEWQ, 2, 2, 16, 77, feat=K2, Skv2=33), case(FEWQ, 2, 2, 16, 77, feat=KVLEN),
          case(FEWQ, 70000, 2, 16, 77)]
    seen, out = set(), []
    for q in c:
        if tuple(q) not in seen:
            seen.add(tuple(q))
            out.append(q)
    return out


def env_cases(name):
    """the process's own switches (-1): what the variable changes, around the rules it touches"""
    c = []
    for Skv, Sq in itertools.product((32, 33, 77, 80, 81, 96, 97, 128, 129), (128, 1024)):
        c.append(case(FWD, 2, 10, Sq, Skv, feat=PRE))
        c += [case(BWD, 2, 10, Sq, Skv, feat=PRE | ALL | sc) for sc in (SCRATCH, 0)]
        c.append(case(BWD, 2, 10, Sq, Skv, feat=PRE | DK | DV | SCRATCH))
    for Skv, nd in itertools.product((77, 300), (2, 3)):
        c.append(case(BWD, 2, 4, 1024, Skv, nd, feat=ALL | SCRATCH))
    return c


# ---------------------------------------------------------------------------------------------- recording from REV
def instantiations():
    """enumerator -> instantiation, as include/pea_hip.h numbers them"""
    tf, k = ("false", "true"), {24: "attn_q_kernel<0, true, 1, true>", 49: "attn_fewq_kernel", 50: "attn_delta_kernel", 51: "attn_dkv_reduce_kernel"}
    for kb in (1, 2, 3, 4):
        for f, (ip, ms) in enumerate(((0, 0), (1, 0), (1, 1))):
            k[4 * f + kb - 1] = f"xattn_fwd_kernel<{kb}, {tf[ip]}, {tf[ms]}>"
        k[37 + kb - 1] = f"xattn_bwd_kernel<{kb}>"
    for tr, nd in itertools.product((0, 1), (1, 2, 3)):
        for mode in (0, 1):
            k[12 + 6 * mode + 3 * tr + nd - 1] = f"attn_q_kernel<{mode}, {tf[tr]}, {nd}>"
        k[25 + 3 * tr + nd - 1] = f"attn_dkv_kernel<{tf[tr]}, {nd}>"
        k[31 + 3 * tr + nd - 1] = f"attn_bwd_fused_kernel<{tf[tr]}, {nd}>"
    for kb, pre in itertools.product((2, 3), (0, 1)):
        k[41 + 2 * (kb - 2) + pre] = f"xattn_bwd2_kernel<{kb}, {tf[pre]}>"
        k[45 + 2 * (kb - 2) + pre] = f"xattn_bwd3_kernel<{kb}, {tf[pre]}>"
    assert sorted(k) == list(range(N_ENUMERATORS))
    return k


RECORDER = r"""
#include <stdio.h>
#include <string>
static std::string g_rec;
static int rec_enumerator(const void* kernel);                     // (the table of instantiations: behind the last kernel)
static void rec_push(const void* k, dim3 g, int lds, const AttnP&, int a0 = 0, int a1 = 0) {
  char buf[160];
  snprintf(buf, sizeof(buf), "|%d;%u;%u;%u;%d;%d;%d", rec_enumerator(k), g.x, g.y, g.z, lds, a0, a1);
  g_rec += buf;
}
"""
LAUNCH_LDS = RECORDER + """template <auto K, typename... Args>
static int launch_lds(dim3 grid, int bytes, hipStream_t, const Args&... args) {
  rec_push((const void*)K, grid, bytes, args...);
  return PEA_OK;
}
"""
PATCHES = [      # (pattern, replacement, how often it must apply)
    # every LDS kernel: launch_lds<K> records K instead of raising the attribute and launching
    (r"(?s)template <auto K, typename\.\.\. Args>\nstatic int launch_lds\(.*?\n\}\n", lambda m: LAUNCH_LDS, 1),
    # the two kernels without dynamic LDS (their call sites come after launch_lds in the file)
    (r"hipLaunchKernelGGL\((attn_delta_kernel|attn_dkv_reduce_kernel), (.*), dim3\(256\), 0, s, p\);", r"rec_push((const void*)\1, \2, 0, p);", 2),
    (r"HIPCHK\(hipGetLastError\(\)\);", ";", 3),          # no device: the launchers' closing query
]
ENTRY = r"""
static int rec_enumerator(const void* kernel) {
  static const struct { const void* k; int e; } table[] = {
TABLE  };
  for (const auto& t : table)
    if (t.k == kernel) return t.e;
  return -1;
}
// the case -> REV's AttnP -> REV's launcher; the switches go through REV's own setters
extern "C" int pea_record_attn(const int* q, char* out, int cap) {
  const int dir = q[0], feat = q[6];
  const int env[4] = {g_xattn_v2, g_attn_use_tr, g_attn_xattn, g_attn_fused_bwd};
  if (q[10] >= 0) g_xattn_v2 = q[10];
  if (q[11] >= 0) g_attn_use_tr = q[11];
  if (q[12] >= 0) g_attn_xattn = q[12];
  if (q[13] >= 0) g_attn_fused_bwd = q[13];
  static float page[64];
  bf16* const any = (bf16*)page;
  AttnP p = AttnP();
  p.Q = p.K = p.V = p.dO = any; p.O = any; p.lse = p.delta = page; p.scale = 0.125f;
  p.B = q[1]; p.H = q[2]; p.Sq = q[3]; p.Skv = q[4]; p.nd = q[5];
  p.ldq = p.ldk = p.ldv = p.ldo = p.lddo = p.lddq = p.lddk = p.lddv = p.ldk2 = p.ldv2 = 64 * p.H * (p.nd > 0 ? p.nd : 1);
  p.causal = feat & 1; p.kv_len = feat & 2 ? (const int*)page : nullptr; p.bias = feat & 4 ? page : nullptr; p.q_prescaled = feat >> 3 & 1;
  if (feat & 16) { p.K2 = p.V2 = any; p.Skv2 = q[7]; p.scale2 = 1.f; p.nset = dir == 2 ? 0 : q[8]; }
  for (int j = 0; j < p.nset && j < 4; ++j) {
    p.set_end[j] = (int)((long long)(j + 1) * p.Skv2 / p.nset);
    p.set_w[j] = feat & 32 ? 0.f : 1.f;
    p.set_mask[j] = q[9] >> j & 1 ? page : nullptr;
  }
  p.dQ = feat & 64 ? any : nullptr; p.dK = feat & 128 ? any : nullptr; p.dV = feat & 256 ? any : nullptr;
  p.dkv_part = feat & 512 ? page : nullptr; p.accum_dq = p.accum_dkv = feat >> 10 & 1;
  g_rec.clear();
  const int rc = dir == 0 ? launch_attention_fwd(p, 0) : dir == 1 ? launch_attention_bwd(p, 0) : launch_attention_fwd_fewq(p, 0);
  const int nsplit = dir == 1 && p.dkv_part ? attention_bwd_nsplit(p.B, p.H, p.Sq, p.Skv) : 1;
  g_xattn_v2 = env[0]; g_attn_use_tr = env[1]; g_attn_xattn = env[2]; g_attn_fused_bwd = env[3];
  snprintf(out, cap, "%d%s", nsplit, g_rec.c_str());
  return rc;
}
"""


def build_recorder(rev, work):
    """REV's csrc + include in `work` (files rewritten only when they differ, so a kept directory rebuilds one object), attention.hip
    patched; -> path of the recording library"""
    files = subprocess.run(["git", "ls-tree", "-r", "--name-only", rev, "pea_diffusion_amd/csrc", "include"], cwd=ROOT, check=True,
                           capture_output=True, text=True).stdout.split()
    for f in files:
        text = subprocess.run(["git", "show", f"{rev}:{f}"], cwd=ROOT, check=True, capture_output=True).stdout
        if f.endswith("csrc/attention.hip"):
            s = text.decode()
            for pat, repl, count in PATCHES:
                s, n = re.subn(pat, repl, s)
                assert n == count, f"{rev}: patch {pat[:40]!r} applied {n} times, expected {count}"
            table = "".join(f"    {{(const void*){k}, {e}}},\n" for e, k in sorted(instantiations().items()))
            text = (s + ENTRY.replace("TABLE", table)).encode()
        dst = os.path.join(work, f)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        if not os.path.exists(dst) or open(dst, "rb").read() != text:
            with open(dst, "wb") as out:
                out.write(text)
    subprocess.run(["make", f"-j{min(16, os.cpu_count() or 1)}"], cwd=os.path.join(work, "pea_diffusion_amd", "csrc"), check=True,
                   stdout=subprocess.DEVNULL)
    return os.path.join(work, "pea_diffusion_amd", "libpea_hip.so")


def record(lib_path, cases):
    fn = ctypes.CDLL(lib_path).pea_record_attn
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(1024)
    out = []
    for q in cases:
        rc = fn((ctypes.c_int * 14)(*q), buf, 1024)
        if rc:
            out.append([rc])
            continue
        nsplit, *launches = buf.value.decode().split("|")
        e = [len(launches), int(nsplit)]
        for l in launches:
            e += [int(x) for x in l.split(";")]
            assert e[-7] >= 0, f"{q}: a kernel outside instantiations()"
        out.append(e)
    return out


def evaluate(lib_path, cases):
    """the same expectations from a library that has pea_debug_attn_dispatch"""
    fn = ctypes.CDLL(lib_path).pea_debug_attn_dispatch
    fn.restype = ctypes.c_int
    out = []
    for q in cases:
        buf = (ctypes.c_int * 23)()
        rc = fn((ctypes.c_int * 14)(*q), buf)
        out.append([rc] if rc else list(buf[:2 + 7 * buf[0]]))
    return out


def pack(sections):
    """{name: (env, cases, expectations)} -> the fixture: a problem (a case's first ten numbers) is stored once with the index of
    its list of switch values (`switches`) and, per entry of that list, the index of its expectation in `plans`"""
    out = {"enumerators": N_ENUMERATORS, "switches": [], "plans": [], "sections": {}}
    plan_ix = {}
    for name, (env, cases, got) in sections.items():
        problems = {}
        for q, e in zip(cases, got):
            problems.setdefault(tuple(q[:10]), []).append((q[10:], plan_ix.setdefault(tuple(e), len(plan_ix))))
        rows = []
        for prob, runs in problems.items():
            sw = [r[0] for r in runs]
            if sw not in out["switches"]:
                out["switches"].append(sw)
            rows.append([*prob, out["switches"].index(sw), [r[1] for r in runs]])
        out["sections"][name] = {"env": env, "problems": rows}
    out["plans"] = [list(e) for e in plan_ix]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD~1", help="the commit whose behaviour is recorded")
    ap.add_argument("--work", help="directory for REV's patched copy (default: a temporary one)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "pea_diffusion_amd", "libpea_hip.so"), help="the tree's library, compared afterwards")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attn_dispatch.json"))
    ap.add_argument("--coverage", action="store_true", help="print enumerator -> first GPU test case that launches it (uses --lib)")
    ap.add_argument("--child", nargs=2, metavar=("MODE", "LIB"), help="internal: record / evaluate the cases on stdin")
    a = ap.parse_args()
    if a.child:
        print(json.dumps((record if a.child[0] == "record" else evaluate)(a.child[1], json.load(sys.stdin))))
        return
    if a.coverage:
        first = {}
        for tid, q in gpu_tests():
            e = evaluate(a.lib, [q])[0]
            for i in range(e[0] if len(e) > 1 else 0):
                first.setdefault(e[2 + 7 * i], tid)
        for k in range(N_ENUMERATORS):
            print(f"| {k} | {first.get(k, '-- none --')} |")
        return

    def run(mode, lib, name, cases):
        env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
        if name in ENV_SECTIONS:
            env[ENV_SECTIONS[name][0]] = ENV_SECTIONS[name][1]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, lib], input=json.dumps(cases), capture_output=True,
                           text=True, env=env, check=True)
        return json.loads(r.stdout)

    with tempfile.TemporaryDirectory() as tmp:
        rec_lib = build_recorder(a.rev, a.work or tmp)
        sections = {"default": default_cases(), **{name: env_cases(name) for name in ENV_SECTIONS}}
        out, seen, bad = {}, set(), 0
        for name, cases in sections.items():
            got = run("record", rec_lib, name, cases)
            for e in got:
                seen.update(e[2 + 7 * i] for i in range(e[0] if len(e) > 1 else 0))
            out[name] = (dict([ENV_SECTIONS[name]]) if name in ENV_SECTIONS else {}, cases, got)
            print(f"{name}: {len(cases)} cases, {sum(len(e) == 1 for e in got)} refused")
            if os.path.exists(a.lib):
                for q, e, g in zip(cases, got, run("evaluate", a.lib, name, cases)):
                    if e != g:
                        bad += 1
                        if bad <= 20:
                            print(f"  DIFFERS {q}: {a.rev} {e}, tree {g}")
    print(f"{a.rev} against {a.lib}: {bad} records differ")
    unreached = sorted(set(range(N_ENUMERATORS)) - seen)
    print("instantiations no case reaches:", unreached or "none")
    with open(a.out, "w") as f:
        json.dump(pack(out), f, separators=(",", ":"))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

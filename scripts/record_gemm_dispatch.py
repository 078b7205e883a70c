#!/usr/bin/env python3
"""Records tests/golden/gemm_dispatch.json: the GEMM launcher's decision (pea_debug_gemm_dispatch) over a fixed case list.

    python scripts/record_gemm_dispatch.py [--lib PATH] [--out PATH]

The fixture pins behaviour, so it is recorded from the library that HAS the behaviour to keep -- for a change to the dispatch
rules that is the parent commit's library, never the tree under test (--lib).  The first recording predates the export: it
came from the parent with the same entry point patched over its launch sites.  Needs no GPU.

Case = [M, N, K, mode, rows_per_batch, features, cus, forced]; feature bits as documented in include/pea_hip.h.
Sections: "default" plus one per environment switch, which tests/test_gemm_dispatch_cpu.py replays in a child process.
"""
import argparse
import csv
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, ROWVEC, F32, ACT, PREACT, GEGLU, GBWD, LN, QSCALE, SPLITK, ALIGNED = (1 << i for i in range(11))
CUS = (256, 128, 64)                       # the device, and what PEA_CU_LIMIT=128 / 64 leaves a chain
TABLE_IDS = [18, 19, 20, 22, 23, 24, 25, 27, 28, 29, 30, 31, 33, 34, 35, 36, 37, 39, 40, 41]
INSTANTIATIONS = TABLE_IDS + [127, 128, 131] + [224, 225, 227, 228, 231]
ENV_SECTIONS = {"PEA_GEMM_DEFER": "1", "PEA_GEMM_KSW_MINK": "1280", "PEA_GEMM_SLOW_EPILOGUE": "1"}
# epilogues of the step's plain GEMMs (residual / row vector come from the case itself where it has them)
MODE0_FEATURES = [ALIGNED, ALIGNED | RES, ALIGNED | LN | QSCALE, ALIGNED | GBWD, ALIGNED | GEGLU | PREACT, 0]
# every feature that makes the launcher leave a pinned variant, one at a time (forced-id sweep)
FIXUP_FEATURES = [(ALIGNED, 0), (ALIGNED | QSCALE, 0), (ALIGNED | GEGLU, 0), (ALIGNED | GEGLU | PREACT, 0), (ALIGNED | GBWD, 0),
                  (ALIGNED | LN, 0), (ALIGNED | ROWVEC, 64), (ALIGNED | ROWVEC, 77), (ALIGNED | F32 | SPLITK, 0), (0, 0),
                  (ALIGNED | F32, 0), (ALIGNED | ACT, 0), (ALIGNED | RES, 0), (ALIGNED | PREACT, 0)]


def profile_tags():
    """distinct (M, N, K, flags) of the GEMM launches in the round-6 per-launch profile; flags: 1 residual, 2 bias, 4 row vector"""
    tags = set()
    with open(os.path.join(ROOT, "profiles", "r06_per_launch_profile.csv")) as f:
        for r in csv.DictReader(f):
            if r["family"].startswith("gemm_lc"):
                tags.add((int(r["t0"]), int(r["t1"]), int(r["t2"]), 1 if "conv" in r["family"] else 0, int(r["t3"])))
    return sorted(tags)


def default_cases():
    c = []

    def add(M, N, K, mode=0, rpb=0, feat=ALIGNED, cus=CUS, forced=-1):
        for cu in cus:
            c.append([M, N, K, mode, rpb, feat, cu, forced])

    # 1. what the step launches
    for (M, N, K, mode, fl) in profile_tags():
        own = ALIGNED | (RES if fl & 1 else 0) | (ROWVEC if fl & 4 else 0)
        rpb = M // 8 if fl & 4 else 0
        add(M, N, K, mode, rpb, own)
        if mode == 0:
            for f in MODE0_FEATURES:
                if f != own:
                    add(M, N, K, 0, 0, f, cus=(256,))
    # 2. tests/test_layouts_gpu.py: ragged GEMMs, GEGLU / GEGLU-backward / LN shapes, the conv cases; tests/test_buckets_gpu.py:
    #    the three non-square buckets' token counts at the SDXL widths
    for (M, N, K) in [(308, 640, 128), (1000, 104, 192), (4100, 1288, 256), (130, 3840, 64), (33000, 336, 128), (64, 160, 640), (256, 320, 128)]:
        for f in (ALIGNED, ALIGNED | RES, ALIGNED | F32, 0):
            add(M, N, K, feat=f)
    for (M, N, K) in [(308, 2560, 320), (1000, 1288, 192), (1456, 2560, 320)]:
        for f in (ALIGNED | GEGLU, ALIGNED | GEGLU | PREACT):
            add(M, N, K, feat=f)
    for (M, N, K) in [(308, 1296, 256), (1000, 2560, 320), (392, 5120, 1280)]:
        add(M, N, K, feat=ALIGNED | GBWD)
    for (M, N, K) in [(308, 1296, 256), (1000, 1920, 640), (392, 3840, 1280)]:
        for f in (ALIGNED | LN, ALIGNED | LN | GEGLU, ALIGNED | LN | QSCALE):
            add(M, N, K, feat=f)
    for (B, Hs, Ws, Cin, Cout, stride, ups) in [(1, 56, 112, 320, 320, 1, False), (2, 36, 44, 640, 640, 1, False), (1, 26, 14, 1280, 1280, 1, False),
                                                (1, 28, 56, 960, 640, 1, False), (1, 14, 28, 2560, 1280, 1, False), (1, 18, 22, 1920, 1280, 1, False),
                                                (1, 56, 112, 320, 320, 2, False), (2, 52, 28, 640, 640, 2, False), (1, 36, 44, 640, 640, 2, False),
                                                (1, 9, 11, 1280, 1280, 1, True), (1, 26, 14, 640, 640, 1, True), (2, 13, 19, 320, 320, 1, False),
                                                (2, 13, 19, 320, 320, 2, False)]:
        Ho, Wo = ((Hs + 1) // 2, (Ws + 1) // 2) if stride == 2 else ((2 * Hs, 2 * Ws) if ups else (Hs, Ws))
        add(B * Ho * Wo, Cout, 9 * Cin, mode=1)
        add(B * Ho * Wo, Cout, 9 * Cin, mode=1, rpb=Ho * Wo, feat=ALIGNED | ROWVEC | RES)
    for (h, w) in [(56, 104), (72, 88), (112, 56)]:
        for B in (1, 2, 4):
            for lvl, C in ((1, 640), (2, 1280)):
                M = B * (h >> lvl) * (w >> lvl)
                add(M, 3 * C, C, feat=ALIGNED | LN | QSCALE)
                add(M, C, C, feat=ALIGNED | RES)
                add(M, 8 * C, C, feat=ALIGNED | LN | GEGLU | PREACT)
                add(M, C, 4 * C, feat=ALIGNED | RES)
                add(M, 4 * C, C, feat=ALIGNED | GBWD)
                add(M, C, 9 * C, mode=1, rpb=M // B, feat=ALIGNED | ROWVEC)
    # 3. the rule boundaries
    for cu in CUS:
        for N in (640, 1280, 5120):
            nbn = -(-N // 160)
            for num, den in ((5, 8), (3, 4), (1, 1), (3, 2), (51, 20)):              # rounds of CUs (2.55: the 85 % rule)
                for tile in (128, 256):
                    mt = max(1, cu * num // (den * nbn))
                    for dm in (-1, 0, 1):
                        if mt + dm > 0:
                            for f in (ALIGNED, ALIGNED | LN, ALIGNED | GBWD, 0):
                                add((mt + dm) * tile, N, 1280, feat=f, cus=(cu,))
    for M in (154, 616, 1000, 1023, 1024, 1025, 2048):                               # M below and above 1024
        for N in (320, 1280, 3840, 10240):
            for f in (ALIGNED, ALIGNED | LN, 0):
                add(M, N, 1280, feat=f)
    for M in (1000, 1024, 16384, 65536, 1048576):                     # N divisible by 128, not by 160 (VAE widths)
        for N in (128, 256, 384, 512):
            for mode in (0, 1):
                for f in (ALIGNED | RES, 0):
                    add(M, N, 1152, mode=mode, feat=f)
    for N in (320, 1280, 2560, 3840, 10240):                                        # M = 6144: the 192-row rule
        for M in (6144, 3072, 12288):
            for f, rpb in ((ALIGNED, 0), (ALIGNED | RES, 0), (ALIGNED | ROWVEC, 1024), (ALIGNED | LN, 0), (ALIGNED | GBWD, 0), (ALIGNED | GEGLU, 0), (0, 0)):
                add(M, N, 1280, rpb=rpb, feat=f)
    for M in (154, 308, 616, 1232):                                                 # stacked cross-attention K|V projection
        for N in (166400, 83200):
            add(M, N, 2048)
    for rpb in (64, 77, 1000, 4096):                                                # row vector inside / across wave tiles
        add(8192, 1280, 1280, rpb=rpb, feat=ALIGNED | ROWVEC)
        add(8192, 1280, 11520, mode=1, rpb=rpb, feat=ALIGNED | ROWVEC | RES)
    # 4. every pinned id (and ids outside the table) x every feature that makes the launcher leave it
    for forced in TABLE_IDS + [0, 21, 26, 32, 38, 99]:
        for (M, N, K, modes) in ((4096, 1280, 1280, (0, 1)), (308, 640, 128, (0,))):
            for mode in modes:
                for f, rpb in FIXUP_FEATURES:
                    add(M, N, K * (9 if mode else 1), mode=mode, rpb=rpb, feat=f, cus=(256,), forced=forced)
    return c


def env_cases(name):
    c = []
    for cu in CUS:
        for N in (640, 1280):
            nbn = -(-N // 160)
            for num, den in ((5, 8), (3, 4), (1, 1), (3, 2), (51, 20)):
                for dm in (0, 1):
                    M = (max(1, cu * num // (den * nbn)) + dm) * 128
                    for K in (640, 1280, 1344):                                      # (1344 / 64 is odd: no K-split form)
                        for f in (ALIGNED, ALIGNED | RES, ALIGNED | LN, ALIGNED | GEGLU, 0):
                            c.append([M, N, K, 0, 0, f, cu, -1])
    for forced in (27, 33, 35, 40, 41):
        for f in (ALIGNED, ALIGNED | RES, ALIGNED | LN, ALIGNED | GBWD):
            c.append([4096, 1280, 1280, 0, 0, f, 256, forced])
    return c


def evaluate(lib_path, cases):
    L = ctypes.CDLL(lib_path)
    fn = L.pea_debug_gemm_dispatch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 8
    return [fn(*case) for case in cases]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "pea_diffusion_amd", "libpea_hip.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json"))
    ap.add_argument("--child", help="internal: evaluate this section's cases (JSON on stdin) and print the results")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(evaluate(a.lib, json.load(sys.stdin))))
        return
    sections = {"default": default_cases()}
    for name in ENV_SECTIONS:
        sections[name] = env_cases(name)
    out = {"instantiations": INSTANTIATIONS, "sections": {}}
    seen = set()
    for name, cases in sections.items():
        env = dict(os.environ)
        for k in ENV_SECTIONS:
            env.pop(k, None)
        if name in ENV_SECTIONS:
            env[name] = ENV_SECTIONS[name]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", a.lib, "--child", name], input=json.dumps(cases),
                           capture_output=True, text=True, env=env, check=True)
        got = json.loads(r.stdout)
        seen.update(got)
        out["sections"][name] = {"env": {name: ENV_SECTIONS[name]} if name in ENV_SECTIONS else {}, "cases": cases, "expect": got}
        print(f"{name}: {len(cases)} cases, {len(set(got))} distinct instantiations")
    missing = sorted(set(INSTANTIATIONS) - seen)
    extra = sorted(seen - set(INSTANTIATIONS))
    assert not missing and not extra, f"case list does not cover {missing}; unknown results {extra}"
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()

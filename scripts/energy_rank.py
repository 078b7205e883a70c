"""Round-5/6 switches ranked by ENERGY per step: the chip is power-bound under this workload, so a change is judged by
J/step (mean board power over the timed region x mean step time), not by ms at whatever clock the box held.  Every switch is
run against the default build / default environment in alternating processes on ONE box (2 rounds), bench.py's own timed region.
usage: python scripts/energy_rank.py [rounds]"""
import json, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
SWITCHES = [  # (label, env that turns the NON-default state on)
    ("next-op weight prefetch OFF", {"PEA_GEMM_PF": "0"}),
    ("upsampler convs folded (not sub-pixel)", {"PEA_UPCONV_SUBPIXEL": "0"}),
    ("intra-workgroup K split, K >= 1280 (variant 41)", {"PEA_GEMM_KSW_MINK": "1280"}),
    ("LayerNorm folded into the consuming GEMM", {"PEA_LN_FOLD": "1"}),
    ("cross-attention backward: round-3 kernel", {"PEA_XATTN_BWD_VER": "0"}),
    ("cross-attention backward: v2 (7 products)", {"PEA_XATTN_BWD_VER": "2"}),
    ("GroupNorm three-kernel path everywhere", {"PEA_GN_UNFUSED": "1"}),
    ("kernel arguments in host memory", {"HIP_FORCE_DEV_KERNARG": "0"}),
]
def run(env):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--no-cpu-baseline", "--no-roofline", "--steps", "16", "--warmup", "3",
                        "--no-dead-row-line"], capture_output=True, text=True, env=e)
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return d["ms_per_step"], d["gpu"]["power_w_mean"], d["energy_j_per_step"], d["gpu"]["sclk_mhz_median"]
print(f"{'switch (non-default state)':52s} {'ms':>7s} {'W':>7s} {'J/step':>8s} {'MHz':>5s}   | default: ms, W, J/step, MHz  | d ms, d J/step")
for label, env in SWITCHES:
    a, b = [], []
    for _ in range(rounds):
        b.append(run({}))
        a.append(run(env))
    m = lambda v, i: sum(x[i] for x in v) / len(v)
    print(f"{label:52s} {m(a,0):7.2f} {m(a,1):7.1f} {m(a,2):8.2f} {m(a,3):5.0f}   | {m(b,0):7.2f} {m(b,1):7.1f} {m(b,2):8.2f} {m(b,3):5.0f} | "
          f"{m(a,0)-m(b,0):+6.2f} ms {m(a,2)-m(b,2):+6.2f} J ({(m(a,2)/m(b,2)-1)*100:+5.2f} %)", flush=True)

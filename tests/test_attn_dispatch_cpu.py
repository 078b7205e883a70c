"""What launch_attention_fwd / _bwd / _fwd_fewq launch for which problem, pinned without a GPU.

tests/golden/attn_dispatch.json holds ~6000 records (the attention ops of every UNet / text-tower graph at the benchmark's and
the tests' batch sizes, the shapes of the GPU attention tests, a grid around every boundary of the rules -- key blocks, query
counts, units per workgroup, the query-split cost rule, head widths -- crossed with the four run-time switches, with dQ-only /
dK-and-dV-only calls, with and without the split scratch, masks, bias, one / several / all-zero image key sets, what the launchers
refuse, and four sections replayed under an environment switch) with the plan each one had at the commit BEFORE the decision
moved into attn_decide_fwd / attn_decide_bwd: every launch's instantiation, grid, LDS bytes and scalar arguments, in order, and
the query-split count, recorded there by launch sites patched to record instead of launching (scripts/record_attn_dispatch.py).
A change to the rules re-records it from its own parent and shows up as a diff of this file's fixture."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from pea_diffusion_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_dispatch.json")
VARIABLES = ["PEA_XATTN_BWD_VER", "PEA_XATTN_OFF", "PEA_ATTN_BWD_SPLIT"]
SECTIONS = ["PEA_XATTN_BWD_VER=0", "PEA_XATTN_BWD_VER=2", "PEA_XATTN_OFF=1", "PEA_ATTN_BWD_SPLIT=1"]
CHILD = r"""
import ctypes, json, sys
fn = ctypes.CDLL(sys.argv[1]).pea_debug_attn_dispatch
fn.restype = ctypes.c_int
out = []
for q in json.load(sys.stdin):
    buf = (ctypes.c_int * 23)()
    rc = fn((ctypes.c_int * 14)(*q), buf)
    out.append([rc] if rc else list(buf[:2 + 7 * buf[0]]))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def golden():
    """the fixture with its sections written out: "cases" (14 numbers each) and "expect", one entry per (problem, switch values).
    The file holds each problem, each list of switch values and each distinct expectation once."""
    with open(FIXTURE) as f:
        g = json.load(f)
    for sec in g["sections"].values():
        sec["cases"], sec["expect"] = [], []
        for *problem, sw, plans in sec["problems"]:
            assert len(g["switches"][sw]) == len(plans)
            sec["cases"] += [problem + env for env in g["switches"][sw]]
            sec["expect"] += [g["plans"][i] for i in plans]
    return g


def dispatch(q):
    """-> [error code] or [launches, nsplit, (enumerator, grid x, y, z, LDS bytes, a0, a1) per launch]"""
    fn = _lib.lib().pea_debug_attn_dispatch
    buf = (ctypes.c_int * 23)()
    rc = fn((ctypes.c_int * 14)(*q), buf)
    return [rc] if rc else list(buf[:2 + 7 * buf[0]])


def describe(q):
    d, B, H, Sq, Skv, nd, feat, Skv2, sets, masks, *env = q
    names = ["causal", "kv_len", "bias", "prescaled", "K2", "zero-weights", "dQ", "dK", "dV", "scratch", "accumulate"]
    return (f"{('fwd', 'bwd', 'fewq')[d]} B={B} H={H} Sq={Sq} Skv={Skv} nd={nd} Skv2={Skv2} sets={sets} masks={masks:#x} "
            f"switches(ver,tr,xattn,fused)={env} features={'|'.join(n for i, n in enumerate(names) if feat >> i & 1) or '0'}")


def mismatches(cases, expect, got):
    assert len(cases) == len(expect) == len(got)
    return [f"{describe(q)}: plan {g}, recorded {e}" for q, e, g in zip(cases, expect, got) if e != g]


def enumerators_of(expect):
    return {e[2 + 7 * i] for e in expect if len(e) > 1 for i in range(e[0])}


def test_default_environment(golden):
    env_set = [k for k in VARIABLES if k in os.environ]
    assert not env_set, f"unset {env_set}: the default section is recorded without them"
    sec = golden["sections"]["default"]
    bad = mismatches(sec["cases"], sec["expect"], [dispatch(q) for q in sec["cases"]])
    assert not bad, f"{len(bad)} of {len(sec['cases'])} problems have another plan:\n" + "\n".join(bad[:20])
    assert sum(len(e) == 1 for e in sec["expect"]) >= 40          # the refused combinations are part of the record


@pytest.mark.parametrize("section", SECTIONS)
def test_environment_switch(golden, section):
    """the variables are read once per process: each section is replayed in a child (plain ctypes, no device, no torch)"""
    sec = golden["sections"][section]
    assert [f"{k}={v}" for k, v in sec["env"].items()] == [section]
    env = {k: v for k, v in os.environ.items() if k not in VARIABLES}
    env.update(sec["env"])
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH], input=json.dumps(sec["cases"]), capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    bad = mismatches(sec["cases"], sec["expect"], json.loads(r.stdout))
    assert not bad, f"{len(bad)} of {len(sec['cases'])} problems have another plan under {sec['env']}:\n" + "\n".join(bad[:20])
    # the section exists because the variable changes something: it must differ from the same problems' plans without it
    assert [dispatch(q) for q in sec["cases"]] != sec["expect"]


def test_every_instantiation_has_a_case(golden):
    """an instantiation added to attn_launch without a problem that reaches it fails here"""
    enumerators = []
    while (e := dispatch([-1, len(enumerators)] + [0] * 12)[0]) >= 0:
        enumerators.append(e)
    assert len(enumerators) == len(set(enumerators)) == golden["enumerators"], enumerators
    recorded = set()
    for sec in golden["sections"].values():
        recorded |= enumerators_of(sec["expect"])
    assert recorded == set(enumerators), f"no case for {sorted(set(enumerators) - recorded)}; unknown {sorted(recorded - set(enumerators))}"


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 512 * 1024

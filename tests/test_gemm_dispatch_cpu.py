"""Which kernel instantiation launch_gemm launches for which problem, pinned without a GPU.

tests/golden/gemm_dispatch.json holds ~7000 problems (the step's launches, the shapes of the layout / bucket tests, a grid around
every boundary of the shape rule at 256 / 128 / 64 CUs, every pinned variant id crossed with every feature that makes the launcher
leave it, and three sections replayed under an environment switch) with the instantiation each one launched at the commit BEFORE
the launcher's decision moved into gemm_decide: recorded there through the same entry point patched over the old launch sites
(scripts/record_gemm_dispatch.py).  A change to the dispatch rules re-records it from its own parent and shows up as a diff of
this file's fixture."""
import json
import os
import subprocess
import sys

import pytest

from pea_diffusion_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch.json")
SWITCHES = ["PEA_GEMM_DEFER", "PEA_GEMM_KSW_MINK", "PEA_GEMM_SLOW_EPILOGUE"]
CHILD = r"""
import ctypes, json, sys
fn = ctypes.CDLL(sys.argv[1]).pea_debug_gemm_dispatch
fn.restype = ctypes.c_int
fn.argtypes = [ctypes.c_int] * 8
print(json.dumps([fn(*c) for c in json.load(sys.stdin)]))
"""


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def describe(case):
    M, N, K, mode, rpb, feat, cus, forced = case
    names = ["res", "rowvec", "f32", "act", "preact", "geglu", "gbwd", "ln", "qscale", "splitk", "aligned"]
    return (f"M={M} N={N} K={K} mode={mode} rows_per_batch={rpb} cus={cus} forced={forced} "
            f"features={'|'.join(n for i, n in enumerate(names) if feat >> i & 1) or '0'}")


def mismatches(cases, expect, got):
    assert len(cases) == len(expect) == len(got)
    return [f"{describe(c)}: launched {g}, recorded {e}" for c, e, g in zip(cases, expect, got) if e != g]


def test_default_environment(golden):
    env_set = [k for k in SWITCHES if k in os.environ]
    assert not env_set, f"unset {env_set}: the default section is recorded without them"
    fn = _lib.lib().pea_debug_gemm_dispatch
    sec = golden["sections"]["default"]
    bad = mismatches(sec["cases"], sec["expect"], [fn(*c) for c in sec["cases"]])
    assert not bad, f"{len(bad)} of {len(sec['cases'])} problems launch another instantiation:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("switch", SWITCHES)
def test_environment_switch(golden, switch):
    """the switches are read once per process: each section is replayed in a child (plain ctypes, no device, no torch)"""
    sec = golden["sections"][switch]
    assert list(sec["env"]) == [switch]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(sec["env"])
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH], input=json.dumps(sec["cases"]), capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    bad = mismatches(sec["cases"], sec["expect"], json.loads(r.stdout))
    assert not bad, f"{len(bad)} of {len(sec['cases'])} problems launch another instantiation under {sec['env']}:\n" + "\n".join(bad[:20])
    # the section exists because the switch changes something: it must differ from what the same problems launch without it
    fn = _lib.lib().pea_debug_gemm_dispatch
    assert [fn(*c) for c in sec["cases"]] != sec["expect"]


def test_every_instantiation_has_a_case(golden):
    """a variant added to the launcher without a problem that reaches it fails here"""
    fn = _lib.lib().pea_debug_gemm_dispatch
    enumerators = []
    while (e := fn(0, len(enumerators), 0, 0, 0, 0, 0, -1)) >= 0:
        enumerators.append(e)
    assert len(enumerators) == len(set(enumerators)), enumerators
    assert sorted(enumerators) == sorted(golden["instantiations"])
    recorded = set()
    for sec in golden["sections"].values():
        recorded.update(sec["expect"])
    assert recorded == set(enumerators), f"no case for {sorted(set(enumerators) - recorded)}; unknown {sorted(recorded - set(enumerators))}"


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) < 512 * 1024

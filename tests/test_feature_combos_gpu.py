"""-m gpu: which combinations of the UNet's attention features a context takes.  The walk of scripts/feature_digest.py -- six
features alone and their 30 ordered pairs on one tiny UNet (B = 2, 16 x 16 latents, a context of 96 rows) -- against the recorded
outcomes of tests/golden/feature_combos.json: the call that refuses (a setter, the forward, or none), its return code and the full
text of pea_last_error.  Every refusal is a host-side error return in front of the first launch; an accepted case runs its
forward, and in every case the plain forward afterwards has the bits of the first one.  The digests of eps stay out of the
fixture (profiles/feature_digest.json has them): a numeric change does not re-record a refusal table."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
from test_model_gpu import gpu  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _walk():
    spec = importlib.util.spec_from_file_location("feature_digest", os.path.join(ROOT, "scripts", "feature_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.walk()


def test_feature_combinations_refuse_as_recorded(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "feature_combos.json")) as f:
        want = json.load(f)
    got = _walk()
    assert sorted(got) == sorted(want) and len(want) == 36
    for case, w in sorted(want.items()):
        g = got[case]
        assert (g["refused"], g["rc"], g["message"]) == (w["refused"], w["rc"], w["message"]), case
        assert (g["eps"] is not None) == (w["refused"] == "ok"), case
        assert g["plain_restored"], case

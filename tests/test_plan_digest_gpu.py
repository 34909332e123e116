"""The lowering emits, for a fixed set of networks, shapes and switch settings, exactly the op lists recorded in
tests/plan_digests.json (see tests/plan_digest.py for what the digest pins and how to re-record it on purpose)."""
import json
import os

import pytest
import torch

import plan_digest
from crossloc_amd import switches

pytestmark = pytest.mark.gpu

_PRESET = sorted(name for name, _, _, _ in switches.LOWERING if name in os.environ)

with open(plan_digest.RECORD) as _f:
    RECORDED = json.load(_f)


def test_every_configuration_is_recorded():
    assert sorted(RECORDED) == sorted(plan_digest.CONFIGS)


@pytest.mark.skipif(bool(_PRESET), reason="the environment already sets lowering switches: %s" % ", ".join(_PRESET))
@pytest.mark.parametrize("name", sorted(plan_digest.CONFIGS))
def test_plan_digest(name):
    got = plan_digest.plan_digest(plan_digest.build_plan(plan_digest.CONFIGS[name], torch.device("cuda:0")))
    want = RECORDED[name]
    assert got["fwd"] == want["fwd"], "forward op types differ"
    assert got["bwd"] == want["bwd"], "backward op types differ"
    assert got["digest"] == want["digest"], "same op types, but a field, a flag or the buffer aliasing of some op differs"

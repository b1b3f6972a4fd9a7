"""The seeds of the whole-pipeline collision sweep (tests/collide_sweep_scenes.py) meet the conditions under which the device comparison of
tests/test_collide_sweep_gpu.py is exact equality with nothing left out."""
import json

import numpy as np
import pytest

from tests import collide_sweep_scenes as S


@pytest.mark.parametrize("agent,furniture", S.MODELS)
def test_sweep_envs_meet_the_three_conditions(agent, furniture):
    sel = S.select(agent, furniture)
    assert json.load(open(S.GOLDEN))["%s/%s" % (agent, furniture)] == sel["keep"], "tests/golden/collide_sweep_envs.json is stale: python -m tests.collide_sweep_scenes"
    assert len(sel["keep"]) == S.N_ENVS
    n = np.array([len(x) for x in sel["expected"]])
    assert n.min() > 0 and n.max() <= S.MAX_CONTACTS          # the checker alone: no overflow path
    assert not any(sel["closed_borderline"])                  # closed-form pairs: same per-pair result at margin -+ 1e-4
    assert sel["portal_gap_min"].min() > S.EDGE               # portal pairs: the reference gap is not within 1e-4 of 0
    assert sel["fp32"] == sel["expected"]                     # the fp32 control build lists the same multiset
    print("%s + %s: %d..%d contacts per env (mean %.1f), smallest |portal gap| %.2e" % (agent, furniture, n.min(), n.max(), n.mean(), sel["portal_gap_min"].min()))

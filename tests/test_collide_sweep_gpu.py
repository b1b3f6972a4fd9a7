"""Whole-pipeline pose sweep through the C-ABI: collision masks, both broadphase stages, the narrow phase's early-outs and its dispatch, in
place in the step kernels.  Per model 64 envs with the parts thrown into a 0.3 m cube around the gripper (tests/collide_sweep_scenes.py), one
fsim_physics_forward, and the multiset of contact geom pairs must EQUAL the fp64 checker's: the envs are chosen (tests/test_collide_sweep.py)
so that no pair is near its threshold and fp32 alone changes nothing."""
import pytest

from tests import collide_sweep_scenes as S
from tests.abi_session import GPU_LIB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("agent,furniture", S.MODELS)
def test_device_lists_the_checkers_contact_pairs(agent, furniture):
    sc = S.scene(agent, furniture)
    got, ncon = S.abi_multisets(GPU_LIB, sc["m"], sc["qpos"], sc["masked"], device="cuda:0")
    bad = [e for e in range(S.N_ENVS) if got[e] != sc["expected"][e]]
    assert not bad, "%s + %s: envs %s list other contact pairs than the checker; first: device-only %s, checker-only %s" % (
        agent, furniture, bad[:8], sorted(set(got[bad[0]]) - set(sc["expected"][bad[0]])), sorted(set(sc["expected"][bad[0]]) - set(got[bad[0]])))
    assert [len(g) for g in got] == ncon.tolist()

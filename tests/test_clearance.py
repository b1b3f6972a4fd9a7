"""What-if clearance queries, the parts that run without a GPU: ClearanceSet validation and caps, the sides of the two helper sensors on
Sawyer and Baxter, the Cursor refusal, the refusals of the wrappers, the C-ABI of include/fsim_clearance.h, and the float64 reference gap
of every pair of robot_clearance_sensors at the reset state of the three GPU models (tests/test_clearance_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.clearance import (MAX_CANDIDATES, MAX_CARRY, MAX_DOFS, ClearanceSet, carried_sensor, check, clearance_tables,
                                     robot_clearance_sensors)
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.pairs import PairSensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_MODELS = [("Sawyer", "table_lack_0825"), ("Baxter", "table_liden_0921"), ("Sawyer", "chair_agne_0010")]  # (chair_agne_0010: a convex-mesh collider)


def _sensor():
    return PairSensor("right_hand", "0_part0")


def _names(m, ids):
    A = m.arrays
    return sorted(set(m.meta["body_names"][int(A["geom_bodyid"][g])] for g in ids))


# ---- ClearanceSet ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,text", [
    (dict(dofs=[]), "no dofs listed"), (dict(dofs=3), "list of dof indices"), (dict(dofs=[0.5]), "list of dof indices"), (dict(dofs=[True]), "list of dof indices"),
    (dict(dofs=[1, 2, 1]), "listed twice"), (dict(dofs=list(range(MAX_DOFS + 1))), "33 dofs"),
    (dict(sensors=[]), "0 sensors"), (dict(sensors=[_sensor()] * 65), "65 sensors"),
    (dict(carry=[("0_part0",)]), "a carry rule is"), (dict(carry=[("0_part0", 3)]), "a carry rule is"), (dict(carry=5), "carry is a list"),
    (dict(carry=[("0_part0", "right_hand"), ("0_part0", "right_l6")]), "carried by two rules"),
    (dict(carry=[("%d_part%d" % (i, i), "right_hand") for i in range(MAX_CARRY + 1)]), "9 carry rules"),
    (dict(max_candidates=0), "max_candidates"), (dict(max_candidates=MAX_CANDIDATES + 1), "max_candidates"), (dict(max_candidates=2.0), "max_candidates"),
    (dict(max_candidates=8, scratch_rows=7), "scratch_rows"), (dict(scratch_rows=-1), "scratch_rows"), (dict(fromto=1), "fromto is a boolean"),
    (dict(normal="yes"), "normal is a boolean")])
def test_set_validation(kw, text):
    base = dict(dofs=[0, 1, 2], sensors=[_sensor()])
    base.update(kw)
    with pytest.raises(ValueError, match=text):
        ClearanceSet(**base)


def test_set_accepts_and_shapes():
    with pytest.raises(TypeError, match="PairSensor"):
        ClearanceSet([0], ["right_hand"])
    with pytest.raises(TypeError, match="ClearanceSet"):
        check([_sensor()])
    s = ClearanceSet(np.arange(7), _sensor(), carry=[("1_part1", "right_hand")], max_candidates=MAX_CANDIDATES, scratch_rows=MAX_CANDIDATES)
    assert s.n_dofs == 7 and s.n_sensors == 1 and s.dofs == list(range(7)) and s.carry == [("1_part1", "right_hand")]
    assert s.shapes(5) == {"clearance_distance": ((5, 1), "float32"), "clearance_geoms": ((5, 1, 2), "int32"), "clearance_valid": ((5,), "uint8")}
    s = ClearanceSet(range(MAX_DOFS), [_sensor(), _sensor()], fromto=True, normal=True)
    assert s.max_candidates == 64 and s.scratch_rows == 0
    assert list(s.shapes(2)) == ["clearance_distance", "clearance_geoms", "clearance_valid", "clearance_fromto", "clearance_normal"]
    assert s.shapes(2)["clearance_fromto"] == ((2, 2, 6), "float32") and s.shapes(2)["clearance_normal"] == ((2, 2, 3), "float32")
    check(s)


def test_tables_against_the_model():
    m = load_compiled("Sawyer", "table_lack_0825")
    arm, grip = list(np.asarray(m.arm_dofadr).reshape(-1)), list(np.asarray(m.arrays["grip_dofadr"]).reshape(-1))
    dofs, tab, carry = clearance_tables(m, ClearanceSet(arm + grip, [_sensor(), carried_sensor(m, "1_part1")], carry=[("1_part1", "right_hand")]))
    assert dofs.dtype == np.int32 and dofs.tolist() == arm + grip and len(tab) == 2 and len(carry) == 1
    names = m.meta["body_names"]
    assert (carry[0].part_body, carry[0].carrier_body) == (names.index("1_part1"), names.index("right_hand"))
    assert clearance_tables(m, ClearanceSet(arm, _sensor()))[2] is None
    nv = len(m.arrays["dof_bodyid"])
    for bad, text in (([nv], "out of range"), ([-1], "out of range"), ([int(m.arrays["part_dofadr"][0])], "not the dof of a hinge or slide joint"),
                      ([0, nv - 1], "free joint")):
        with pytest.raises(ValueError, match=text):
            clearance_tables(m, ClearanceSet(bad, _sensor()))
    for rule, text in ((("right_hand", "right_l6"), "is not a furniture part"), (("0_part0", "nobody"), "unknown carrier body"),
                       (("0_part0", "0_part0"), "belongs to the part it carries")):
        with pytest.raises(ValueError, match=text):
            clearance_tables(m, ClearanceSet(arm, _sensor(), carry=[rule]))
    with pytest.raises(ValueError, match="unknown body"):  # the sensors are checked as a PairSet's are
        clearance_tables(m, ClearanceSet(arm, PairSensor("right_hand", "9_part9")))


# ---- the helpers ------------------------------------------------------------------------------------------------------------------------
def test_helper_sides_on_sawyer():
    m = load_compiled("Sawyer", "table_lack_0825")
    s = robot_clearance_sensors(m, dmax=0.5)
    assert isinstance(s, PairSensor) and s.dmax == 0.5 and s.a[0] == "geoms" and s.b[0] == "geoms"
    # side a: every link that moves, with what is folded into it (the head on right_l0), not the pedestal or the arm base
    assert _names(m, s.a[1]) == sorted(["right_l0", "head", "screen", "right_l1", "right_l1_2", "right_l2", "right_l2_2", "right_l3", "right_l4", "right_l4_2", "right_l5",
                                        "right_l6", "right_gripper_base", "r_gripper_l_finger", "r_gripper_l_finger_tip", "r_gripper_r_finger", "r_gripper_r_finger_tip"])
    assert _names(m, s.b[1]) == sorted(["world"] + list(m.meta["part_names"]))
    assert not set(s.a[1]) & set(s.b[1]) and len(s.pairs(m)) == len(s.a[1]) * len(s.b[1]) == 19 * 6
    c = carried_sensor(m, "1_part1", dmax=0.3)
    assert _names(m, c.a[1]) == ["1_part1"] and _names(m, c.b[1]) == sorted(["world", "0_part0", "2_part2", "3_part3", "4_part4"]) and c.dmax == 0.3
    with pytest.raises(ValueError, match="is not a furniture part"):
        carried_sensor(m, "right_hand")


def test_helper_sides_on_baxter():
    m = load_compiled("Baxter", "table_liden_0921")
    s = robot_clearance_sensors(m)
    a, b = _names(m, s.a[1]), _names(m, s.b[1])
    assert "right_wrist" in a and "left_wrist" in a and "l_gripper_l_finger_tip" in a and "r_gripper_r_finger" in a and "right_upper_shoulder" in a
    assert not {"pedestal", "collision_head_link_1", "collision_head_link_2", "world"} & set(a) and not any(n in m.meta["part_names"] for n in a)
    assert b == sorted(["world"] + list(m.meta["part_names"]))  # the floor and every part (3_part11 and 2_part10 with three geoms each), not the pedestal
    assert len(s.b[1]) == 1 + 16 and len(s.a[1]) == 28 and len(s.pairs(m)) == 28 * 17
    c = carried_sensor(m, "3_part11")
    assert len(c.a[1]) == 3 and len(c.b[1]) == 1 + 13


def test_cursor_is_refused():
    m = load_compiled("Cursor", "toy_table")
    with pytest.raises(ValueError, match="no jointed robot body .*Cursor"):
        robot_clearance_sensors(m)
    with pytest.raises(ValueError, match="no dofs listed .*Cursor agent has none"):
        ClearanceSet(list(np.asarray(m.arm_dofadr).reshape(-1)), PairSensor("cursor0", "0_part0"))
    with pytest.raises(ValueError, match="not the dof of a hinge or slide joint"):  # every dof of the model is a free joint's
        clearance_tables(m, ClearanceSet([0], PairSensor("cursor0", "0_part0")))


# ---- the helper's pairs are apart at reset: none of them is in permanent contact -----------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", GPU_MODELS)
def test_robot_pairs_are_apart_at_the_reset_state(agent, furniture):
    from oracle.oracle_sim import OracleSim
    from tests import clearance_reference as clr
    from tests.test_pairs_gpu import _reference_gaps
    m = load_compiled(agent, furniture)
    s = robot_clearance_sensors(m)
    q0 = np.asarray(m.arrays["qpos0"], dtype=np.float64)
    osim = OracleSim(m)
    geoms = clr.geoms_at(osim, m, q0, [], [])
    osim.close()
    gaps = _reference_gaps(geoms, s.pairs(m))
    worst = min(gaps, key=gaps.get)
    print("%s + %s: %d pairs, the smallest gap %.4f m (colliding geoms %s)" % (agent, furniture, len(gaps), gaps[worst], worst))
    assert gaps[worst] > 0.0


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import ALL_SENSOR_FAMILIES, FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = ClearanceSet(range(7), _sensor())
    with pytest.raises(TypeError, match="ClearanceSet"):
        FurnitureBatchEnv("Sawyer", 1, clearance=[_sensor()])
    with pytest.raises(NotImplementedError, match="clearance= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, clearance=spec)
    with pytest.raises(NotImplementedError, match="clearance= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(clearance=spec))
    assert not any(f.kw == "clearance" for f in ALL_SENSOR_FAMILIES)  # not an observation family

    class _Handle:  # a handle with a clearance set and nothing else
        clearance_set = spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="clearance queries are not part of the multi-GPU gather"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_clearance_header_symbols_are_exported():
    assert sim.CLEARANCE_SYMBOLS == ["fsim_set_clearance", "fsim_clearance"]
    assert sorted(_declared("fsim_clearance.h")) == sorted(sim.CLEARANCE_SYMBOLS)
    assert not set(sim.CLEARANCE_SYMBOLS) & (set(sim.EXPORTED_SYMBOLS) | set(sim.PAIR_SYMBOLS) | _declared("fsim.h") | _declared("fsim_pairs.h"))
    lib = ctypes.CDLL(sim.build())
    for n in sim.CLEARANCE_SYMBOLS + sim.PAIR_SYMBOLS:
        assert hasattr(lib, n), n


def test_clearance_header_is_plain_c11_and_the_struct_matches(tmp_path):
    fields = [n for n, _ in sim.FsimClrCarry._fields_]
    src = tmp_path / "use_clearance.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsim_clearance.h"\n'
                   "int use(fsim_t *s, const int32_t *d, const fsim_pair_sensor_t *k, const fsim_clr_carry_t *c, const float *q, const uint8_t *m, float *o, uint8_t *v) {\n"
                   "  return fsim_set_clearance(s, 7, d, 1, k, 1, c, 64, 0) + fsim_clearance(s, 16, q, m, o, 0, 0, 0, v); }\n"
                   'int main(void) { printf("%zu %d %d %d", sizeof(fsim_clr_carry_t), FSIM_CLR_MAX_DOFS, FSIM_CLR_MAX_CANDIDATES, FSIM_CLR_MAX_CARRY);\n' +
                   "".join('  printf(" %%zu", offsetof(fsim_clr_carry_t, %s));\n' % f for f in fields) + "  return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_clearance.o")])
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_clearance.h"\n'
                    "int fsim_set_clearance(fsim_t *s, int a, const int32_t *d, int b, const fsim_pair_sensor_t *k, int c, const fsim_clr_carry_t *r, int e, int f) {\n"
                    "  (void)s; (void)d; (void)k; (void)r; return a + b + c + e + f; }\n"
                    "int fsim_clearance(fsim_t *s, int K, const float *q, const uint8_t *m, float *a, int32_t *b, float *c, float *d, uint8_t *v) {\n"
                    "  (void)s; (void)q; (void)m; (void)a; (void)b; (void)c; (void)d; (void)v; return K; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [ctypes.sizeof(sim.FsimClrCarry), MAX_DOFS, MAX_CANDIDATES, MAX_CARRY] and got[0] == 8
    assert got[4:] == [getattr(sim.FsimClrCarry, f).offset for f in fields]


def test_clearance_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_clearance.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())
    for s in ("Joint ranges are NOT applied", "valid = 0", "the env's own value in place of each such value", "X_part' = X_carrier(candidate) o X_carrier(record)^-1 o X_part(record)",
              "every colliding geom folded into the part's reduced body moves with it", "need rules of their own", "rules do not chain",
              "writes no state, RNG draw, look-ahead shadow or counter", "nothing but its outputs and a pose scratch the clearance set owns",
              "not on K, on the other candidates, on the other envs or on how the rows were split over launches", "coexist and know nothing of each other",
              "chunks of floor(scratch_rows / K) envs", "A refused call leaves the previous set in place", "K > max_candidates"):
        assert s in flat, s

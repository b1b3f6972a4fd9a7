"""Geom-pair distance sensors, the parts that run without a GPU: PairSensor / PairSet validation, the caps, the body-to-geoms rule, the pair
order, the refusals and the C-ABI of include/fsim_pairs.h (tests/test_pairs_tool_gpu.py and tests/test_pairs_gpu.py run the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.pairs import MAX_PAIRS, MAX_SENSORS, MAX_TOTAL_PAIRS, PairSensor, PairSet, body_geoms, check, gripper_bodies, sensor_table
from furniture_amd.probes import ProbeSensor
from furniture_amd.rays import exclude_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(words):
    v = sum(int(words[j]) << (32 * j) for j in range(3))
    return [k for k in range(96) if v >> k & 1]


# ---- PairSensor / PairSet ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dmax=0.0), dict(dmax=-1.0), dict(dmax=float("inf")), dict(dmax=float("nan")), dict(a=[]), dict(b=[]), dict(a=3), dict(b=None),
                                dict(a=[1.5]), dict(a=["right_hand", 3]), dict(b=[True])])
def test_sensor_validation(kw):
    args = dict(a="right_hand", b=[22, 23])
    args.update(kw)
    with pytest.raises(ValueError):
        PairSensor(**args)


def test_sensor_accepts():
    s = PairSensor("right_hand", ["0_part0", "1_part1"], dmax=0.5)
    assert s.a == ("bodies", ["right_hand"]) and s.b == ("bodies", ["0_part0", "1_part1"]) and s.dmax == 0.5 and "dmax 0.5" in repr(s)
    s = PairSensor(np.array([3, 4]), (5,))
    assert s.a == ("geoms", [3, 4]) and s.b == ("geoms", [5]) and s.dmax == 1.0


def test_pair_set_validation():
    one = PairSensor("right_hand", "0_part0")
    with pytest.raises(ValueError, match="0 sensors"):
        PairSet([])
    with pytest.raises(ValueError, match="65 sensors"):
        PairSet([one] * (MAX_SENSORS + 1))
    with pytest.raises(TypeError, match="PairSensor"):
        PairSet([one, "gripper"])
    with pytest.raises(ValueError, match="boolean"):
        PairSet([one], fromto=1)
    with pytest.raises(ValueError, match="boolean"):
        PairSet([one], normal="yes")
    with pytest.raises(TypeError, match="PairSet"):
        check([one])
    ps = PairSet([one, one], fromto=True)
    assert ps.n_sensors == 2 and ps.fromto and not ps.normal and "2 sensors" in repr(ps)
    assert PairSet(one).n_sensors == 1  # a single sensor is a set of one
    PairSet([one] * MAX_SENSORS)


def test_model_checks_and_caps():
    m = load_compiled("Sawyer", "table_lack_0825")
    cg = np.asarray(m.arrays["cg_orig"])
    with pytest.raises(ValueError, match="unknown body"):
        sensor_table(m, PairSet(PairSensor("no_such_body", "0_part0")))
    with pytest.raises(ValueError, match="names geom 10000"):
        sensor_table(m, PairSet(PairSensor([10000], "0_part0")))
    free = sorted(set(range(len(m.arrays["geom_bodyid"]))) - set(cg.tolist()))
    if free:
        with pytest.raises(ValueError, match="does not collide"):
            sensor_table(m, PairSet(PairSensor("0_part0", [free[0]])))
    with pytest.raises(ValueError, match="no colliding geom"):
        sensor_table(m, PairSet(PairSensor("base", "0_part0")))  # (a world-welded body without a collider of its own)
    with pytest.raises(ValueError, match="no valid pair"):
        sensor_table(m, PairSet(PairSensor([int(cg[0])], [int(cg[0])])))  # the floor with itself
    # the caps need many geoms: Cursor + toy_table has 52 colliding geoms, 52 * 51 = 2652 pairs all against all
    mc = load_compiled("Cursor", "toy_table")
    allg = [int(g) for g in np.asarray(mc.arrays["cg_orig"])]
    every = PairSensor(allg, allg)
    n = len(every.pairs(mc))
    assert n == len(allg) * (len(allg) - 1) <= MAX_PAIRS
    sensor_table(mc, PairSet([every] * (MAX_TOTAL_PAIRS // n)))
    with pytest.raises(ValueError, match="more than 16384 pairs over the set"):
        sensor_table(mc, PairSet([every] * (MAX_TOTAL_PAIRS // n + 1)))


def test_per_sensor_cap_is_checked():
    """no shipped model has 4097 pairs in one sensor (96 geoms at most give 9120, but the largest model here has 52): a model stand-in
    with 70 box geoms on 70 bodies"""
    class _M:
        meta = dict(body_names=["b%d" % i for i in range(70)], agent="x", furniture_name="y")
        arrays = dict(cg_orig=np.arange(70), geom_bodyid=np.arange(70), body_red=np.arange(70), geom_type=np.full(70, 6))
    allg = list(range(70))
    with pytest.raises(ValueError, match="4830 pairs .at most 4096 per sensor"):
        sensor_table(_M, PairSet(PairSensor(allg, allg)))
    assert len(sensor_table(_M, PairSet(PairSensor(allg[:64], allg[:64])))) == 1 and MAX_PAIRS == 4096  # 64 * 63 = 4032


# ---- a body stands for its colliding geoms by the rule of the sensors' "body" exclusion ------------------------------------------------------
def test_body_rule_on_sawyer_and_cursor():
    m = load_compiled("Sawyer", "table_lack_0825")
    cg = np.asarray(m.arrays["cg_orig"])
    gbody = np.asarray(m.arrays["geom_bodyid"])[cg]
    names = m.meta["body_names"]
    hand = body_geoms(m, "right_hand")
    assert np.array_equal(hand, np.isin(gbody, [names.index("right_l6"), names.index("right_gripper_base")])) and hand.sum() >= 2
    assert np.array_equal(hand, exclude_mask(m, ProbeSensor((0, 0, 0), [(0, 0, 0)], body="right_hand")))  # the same rule, not a copy that can drift
    for b in ("r_gripper_l_finger", "0_part0", "pedestal", "world"):
        assert np.array_equal(body_geoms(m, b), exclude_mask(m, ProbeSensor((0, 0, 0), [(0, 0, 0)], body=b))), b
    assert [names[b] for b in gbody[body_geoms(m, "world")]] == ["world"]  # the floor alone: not everything welded to the world
    assert gripper_bodies(m) == ["right_gripper_base", "r_gripper_l_finger", "r_gripper_l_finger_tip", "r_gripper_r_finger", "r_gripper_r_finger_tip"]
    grip = PairSensor(gripper_bodies(m), ["0_part0", "2_part2"], dmax=0.7)
    ma, mb = grip.side_masks(m)
    assert sorted(set(names[b] for b in gbody[ma])) == sorted(["right_l6", "right_gripper_base", "r_gripper_l_finger", "r_gripper_l_finger_tip", "r_gripper_r_finger", "r_gripper_r_finger_tip"])
    assert [names[b] for b in gbody[mb]] == ["0_part0", "2_part2"]
    pairs = grip.pairs(m)
    assert pairs == [(int(g1), int(g2)) for g1 in np.nonzero(ma)[0] for g2 in np.nonzero(mb)[0]] and pairs == sorted(pairs)  # A-major
    tab = sensor_table(m, PairSet([grip, PairSensor("world", gripper_bodies(m), dmax=2.0)]))
    assert _bits(tab[0].a) == np.nonzero(ma)[0].tolist() and _bits(tab[0].b) == np.nonzero(mb)[0].tolist() and abs(tab[0].dmax - 0.7) < 1e-7
    assert _bits(tab[1].a) == [0] and _bits(tab[1].b) == np.nonzero(ma)[0].tolist() and tab[1].dmax == 2.0
    # explicit geom ids; a geom on both sides pairs with everything but itself
    ids = [int(cg[22]), int(cg[23]), int(cg[24])]
    assert PairSensor(ids, ids).pairs(m) == [(22, 23), (22, 24), (23, 22), (23, 24), (24, 22), (24, 23)]
    # a cursor is welded to the world: only its own geom, not the floor
    mc = load_compiled("Cursor", "toy_table")
    cgc = np.asarray(mc.arrays["cg_orig"])
    assert int(mc.arrays["body_red"][mc.meta["body_names"].index("cursor0")]) == 0
    assert [mc.meta["body_names"][int(mc.arrays["geom_bodyid"][int(g)])] for g in cgc[body_geoms(mc, "cursor0")]] == ["cursor0"]
    assert gripper_bodies(mc) == ["cursor0", "cursor1"]
    mb_ = load_compiled("Baxter", "desk_mikael_1064")
    assert len(gripper_bodies(mb_)) == 10 and len(gripper_bodies(mb_, "left")) == 5 and all(n.startswith(("l_", "left_")) for n in gripper_bodies(mb_, "left"))
    with pytest.raises(ValueError, match="no gripper"):
        gripper_bodies(m, "left")


# ---- refusals (before any device work) ----------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = PairSet(PairSensor("right_hand", "0_part0"))
    with pytest.raises(TypeError, match="PairSet"):
        FurnitureBatchEnv("Sawyer", 1, pairs=[PairSensor("right_hand", "0_part0")])
    with pytest.raises(NotImplementedError, match="pairs= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, pairs=spec)
    with pytest.raises(NotImplementedError, match="pairs= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(pairs=spec))

    class _Handle:  # a handle with a pair set and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs = None, None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="pair-distance outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_pairs_header_symbols_are_exported():
    assert sim.PAIR_SYMBOLS == ["fsim_set_pairs", "fsim_pair_distance"]
    assert sorted(_declared("fsim_pairs.h")) == sorted(sim.PAIR_SYMBOLS)
    others = (set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS) | set(sim.VOXELS_SYMBOLS) | set(sim.NORMALS_SYMBOLS) | set(sim.FLOW_SYMBOLS) |
              set(sim.RAY_SYMBOLS) | set(sim.PROBE_SYMBOLS))
    assert not set(sim.PAIR_SYMBOLS) & others
    assert not set(sim.PAIR_SYMBOLS) & set().union(*[_declared(h) for h in ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h", "fsim_rays.h",
                                                                              "fsim_probes.h")])
    lib = ctypes.CDLL(sim.build())
    for n in sim.PAIR_SYMBOLS:
        assert hasattr(lib, n), n


def test_pairs_header_is_plain_c11_and_the_struct_matches(tmp_path):
    fields = [n for n, _ in sim.FsimPairSensor._fields_]
    src = tmp_path / "use_pairs.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsim_pairs.h"\n'
                   "int use(fsim_t *s, const fsim_pair_sensor_t *k, float *o) { return fsim_set_pairs(s, 1, k) + fsim_pair_distance(s, o, 0, 0, 0); }\n"
                   'int main(void) { printf("%zu %d %d %d", sizeof(fsim_pair_sensor_t), FSIM_PAIR_MAX_SENSORS, FSIM_PAIR_MAX_PAIRS, FSIM_PAIR_MAX_TOTAL);\n' +
                   "".join('  printf(" %%zu", offsetof(fsim_pair_sensor_t, %s));\n' % f for f in fields) + "  return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_pairs.o")])
    # the layout: a program that defines the two entry points itself prints sizeof and every offsetof
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_pairs.h"\nint fsim_set_pairs(fsim_t *s, int a, const fsim_pair_sensor_t *k) { (void)s; (void)k; return a; }\n'
                    "int fsim_pair_distance(fsim_t *s, float *a, int32_t *b, float *c, float *d) { (void)s; (void)a; (void)b; (void)c; (void)d; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [ctypes.sizeof(sim.FsimPairSensor), MAX_SENSORS, MAX_PAIRS, MAX_TOTAL_PAIRS] and got[0] == 28
    assert got[4:] == [getattr(sim.FsimPairSensor, f).offset for f in fields]


def test_pairs_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_pairs.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("collision masks (contype / conaffinity) are ignored", "geoms of one body or of welded bodies are NOT skipped", "a geom may be on both sides",
              "g1 != g2 and not both planes", "ordered A-major", "d = -h_X(-n_p) - n_p . p_plane", "exact for either sign",
              "A sphere is its centre plus a radius, a capsule its axis segment plus a radius",
              "While the two cores are disjoint, d is the Euclidean distance of the cores minus the two radii", "exact also when that is negative",
              "never a normalised to - from", "to - from = d * n",
              # the portal bound
              "d is MINUS THE PORTAL DEPTH", "d <= the true signed gap", "the face of the Minkowski difference that the line through the two centres leaves through",
              "never reports a shallower overlap than the true one and may report a deeper one", "PORTAL_OVER_FP64 of tests/test_narrowphase.py",
              "NOT the depth the step's closed-form box-box routine (np_box_box) uses", "moved by -d / 2 and +d / 2 along n",
              # the tie rule
              "the smallest d wins; a strict < in pair order (A-major) settles ties: of equal distances the first pair wins",
              # the dmax convention
              "accepted when d <= dmax", "dist = dmax, geoms = (-1, -1) and the vectors are (0, 0, 0)",
              "in the numbering of the segmentation image", "writes no state, RNG draw, look-ahead shadow or counter", "depends only on its own record and the pair set",
              "does not depend on the other sensors of the set", "Without a pair set, nothing is allocated or launched", "n_sensors == 0 clears",
              "The hull vertices of convex-mesh colliders come from the model, so no plane tables are passed", "a side without a geom", "a sensor with no valid pair",
              "a mask bit at or beyond the number of colliding geoms", "a dmax that is not 0 < dmax < inf", "more than 96 colliding geoms",
              "waits for the handle's stream before it replaces the tables", "any may be NULL, not all", "settled exactly as fsim_probe_distance settles it",
              "returns without waiting"):
        assert s in flat, s

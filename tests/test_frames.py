"""Body and site frame sensors, the parts that run without a GPU: Frame / FrameSensor / FrameSet validation, the frame table, the refusals,
the C-ABI of include/fsim_frames.h, connector_pairs, and the float64 reference tests/frames_reference.py against central differences of the
oracle's kinematics (tests/test_frames_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.frames import MAX_NV, MAX_SENSORS, Frame, FrameSensor, FrameSet, check, connector_pairs, sensor_table
from furniture_amd.mjcf.model import load_compiled
from oracle.oracle_sim import OracleSim
from tests import frames_reference as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_TOL = 1e-7  # the FD_TOL of tests/test_flow.py: central differences at h = 1e-4 measured 5.2e-9 (linear) and 2.2e-8 (angular) of the scale S
FD_H = 1e-4


# ---- Frame / FrameSensor / FrameSet ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(body="right_hand", site="grip_site"), dict(body=3), dict(site=5), dict(pos=(0, 0)), dict(quat=(1, 0, 0)), dict(pos=(0, float("nan"), 0)),
                                dict(quat=(float("inf"), 0, 0, 0)), dict(quat=(0, 0, 0, 0)), dict(pos="abc")])
def test_frame_validation(kw):
    with pytest.raises(ValueError):
        Frame(**kw)


def test_frame_accepts_and_normalises():
    f = Frame(body="right_hand", pos=(0.1, 0, 0), quat=(2, 0, 0, 0))
    assert f.body == "right_hand" and f.site is None and np.array_equal(f.quat, [1, 0, 0, 0]) and "right_hand" in repr(f)
    w = Frame()
    assert w.body is None and w.site is None and repr(w) == "Frame(world)"
    assert repr(Frame(site="grip_site")) == "Frame(site='grip_site')"
    s = FrameSensor(f)
    assert s.ref.body is None and s.ref.site is None and not s.ref.pos.any() and "ref=Frame(world)" in repr(s)
    with pytest.raises(TypeError, match="Frame"):
        FrameSensor("right_hand")
    with pytest.raises(TypeError, match="Frame"):
        FrameSensor(f, ref="world")


def test_frame_set_validation():
    one = FrameSensor(Frame(body="right_hand"))
    with pytest.raises(ValueError, match="0 sensors"):
        FrameSet([])
    with pytest.raises(ValueError, match="65 sensors"):
        FrameSet([one] * (MAX_SENSORS + 1))
    with pytest.raises(TypeError, match="FrameSensor"):
        FrameSet([one, Frame()])
    with pytest.raises(ValueError, match="boolean"):
        FrameSet([one], velocity=1)
    with pytest.raises(ValueError, match="boolean"):
        FrameSet([one], jacobian="yes")
    with pytest.raises(TypeError, match="FrameSet"):
        check([one])
    fs = FrameSet([one, one], velocity=True)
    assert fs.n_sensors == 2 and fs.velocity and not fs.jacobian and "2 sensors" in repr(fs)
    check(fs)
    fs.sensors.append("junk")  # check() looks again
    with pytest.raises(TypeError, match="FrameSensor"):
        check(fs)
    assert FrameSet(one).n_sensors == 1  # a single sensor is a set of one
    FrameSet([one] * MAX_SENSORS)


def test_sensor_table_resolves_names_and_sites():
    m = load_compiled("Sawyer", "table_lack_0825")
    names, sites = m.meta["body_names"], m.meta["site_names"]
    with pytest.raises(ValueError, match="unknown body"):
        sensor_table(m, FrameSet(FrameSensor(Frame(body="no_such_body"))))
    with pytest.raises(ValueError, match="unknown site"):
        sensor_table(m, FrameSet(FrameSensor(Frame(), ref=Frame(site="no_such_site"))))
    with pytest.raises(ValueError, match="unknown body"):
        sensor_table(m, FrameSet(FrameSensor(Frame(body="grip_site"))))  # a site name is no body name
    # "0_part0" is both a body and a site: the keyword decides
    k = sites.index("0_part0")
    tab = sensor_table(m, FrameSet([FrameSensor(Frame(body="0_part0"), ref=Frame(site="0_part0")), FrameSensor(Frame(pos=(1, 2, 3)))]))
    assert ctypes.sizeof(tab) == 2 * ctypes.sizeof(sim.FsimFrameSensor)
    assert tab[0].frame.body == names.index("0_part0") and list(tab[0].frame.pos) == [0, 0, 0] and list(tab[0].frame.quat) == [1, 0, 0, 0]
    assert tab[0].ref.body == int(m.arrays["site_bodyid"][k]) == names.index("0_part0")
    assert np.allclose(list(tab[0].ref.pos), np.asarray(m.arrays["site_pos"]).reshape(-1, 3)[k], atol=1e-7)
    assert tab[1].frame.body == -1 and list(tab[1].frame.pos) == [1, 2, 3] and tab[1].ref.body == -1 and list(tab[1].ref.quat) == [1, 0, 0, 0]
    # a site with an offset: site pose (x) offset, in float64
    g = sites.index("grip_site")
    sp, sq = np.asarray(m.arrays["site_pos"], dtype=np.float64).reshape(-1, 3)[g], np.asarray(m.arrays["site_quat"], dtype=np.float64).reshape(-1, 4)[g]
    off_q = np.array([np.cos(0.3), np.sin(0.3), 0.0, 0.0])
    b, p, q = Frame(site="grip_site", pos=(0.0, 0.1, 0.2), quat=off_q).resolve(m)
    assert b == int(m.arrays["site_bodyid"][g])
    assert np.allclose(p, sp + fref.q2m(sq / np.linalg.norm(sq)) @ [0.0, 0.1, 0.2], atol=1e-14) and np.allclose(q, fref.qmul(sq / np.linalg.norm(sq), off_q), atol=1e-14)

    class _Big:  # the caps: no shipped model is beyond them (32 reduced bodies and nv = 93 are the catalogue's largest)
        nv = MAX_NV + 1
        arrays = dict(rdims=np.array([20]))
        meta = m.meta
    with pytest.raises(ValueError, match="nv = 129"):
        sensor_table(_Big, FrameSet(FrameSensor(Frame())))
    _Big.nv, _Big.arrays = 30, dict(rdims=np.array([33]))
    with pytest.raises(ValueError, match="33 reduced bodies"):
        sensor_table(_Big, FrameSet(FrameSensor(Frame())))


def test_connector_pairs():
    m = load_compiled("Sawyer", "table_lack_0825")
    pairs = connector_pairs(m)
    assert len(pairs) == 4  # four leg-to-table pairs
    sites, sbody, names = m.meta["site_names"], np.asarray(m.arrays["site_bodyid"]), m.meta["body_names"]
    assert all(a.startswith("leg-table") and b.startswith("table-leg") for a, b in pairs)
    assert len({a for a, _ in pairs}) == 4 and len({b for _, b in pairs}) == 4  # every connector site once
    assert sorted(names[int(sbody[sites.index(a)])] for a, _ in pairs) == ["0_part0", "1_part1", "2_part2", "3_part3"]
    assert {names[int(sbody[sites.index(b)])] for _, b in pairs} == {"4_part4"}
    fs = FrameSet([FrameSensor(Frame(site=a), ref=Frame(site=b)) for a, b in pairs])
    assert fs.n_sensors == 4 and len(sensor_table(m, fs)) == 4
    # keys decide: every pair of another furniture matches a-b against b-a and joins two parts
    md = load_compiled("Baxter", "desk_mikael_1064")
    for a, b in connector_pairs(md):
        ka, kb = a.split(",")[0].split("-"), b.split(",")[0].split("-")
        assert ka == kb[::-1]
        assert md.arrays["site_bodyid"][md.meta["site_names"].index(a)] != md.arrays["site_bodyid"][md.meta["site_names"].index(b)]


# ---- refusals (before any device work) ----------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = FrameSet(FrameSensor(Frame(body="right_hand")))
    with pytest.raises(TypeError, match="FrameSet"):
        FurnitureBatchEnv("Sawyer", 1, frames=[FrameSensor(Frame(body="right_hand"))])
    with pytest.raises(NotImplementedError, match="frames= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, frames=spec)
    with pytest.raises(NotImplementedError, match="frames= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(frames=spec))

    class _Handle:  # a handle with a frame set and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs, frames = None, None, None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="frame-sensor outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
OTHER_HEADERS = ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h", "fsim_rays.h", "fsim_probes.h", "fsim_pairs.h")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_frames_header_symbols_are_exported():
    assert sim.FRAME_SYMBOLS == ["fsim_set_frames", "fsim_frame_state"]
    assert sorted(_declared("fsim_frames.h")) == sorted(sim.FRAME_SYMBOLS)
    lists = [n for n in dir(sim) if n.endswith("_SYMBOLS") and n != "FRAME_SYMBOLS"]
    assert len(lists) >= 9 and {"EXPORTED_SYMBOLS", "PAIR_SYMBOLS", "FLOW_SYMBOLS"} <= set(lists)
    assert not set(sim.FRAME_SYMBOLS) & set().union(*[set(getattr(sim, n)) for n in lists])
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h") and h != "fsim_frames.h"]  # every other header, later ones too
    assert set(OTHER_HEADERS) <= set(others)
    assert not set(sim.FRAME_SYMBOLS) & set().union(*[_declared(h) for h in others])
    lib = ctypes.CDLL(sim.build())
    for n in sim.FRAME_SYMBOLS:
        assert hasattr(lib, n), n


def test_frames_header_is_plain_c11_and_the_structs_match(tmp_path):
    src = tmp_path / "use_frames.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsim_frames.h"\n'
                   "int use(fsim_t *s, const fsim_frame_sensor_t *k, float *o) { return fsim_set_frames(s, 1, k) + fsim_frame_state(s, o, 0, 0, 0); }\n"
                   'int main(void) { printf("%zu %zu %d %d", sizeof(fsim_frame_t), sizeof(fsim_frame_sensor_t), FSIM_FRAME_MAX_SENSORS, FSIM_FRAME_MAX_NV);\n' +
                   "".join('  printf(" %%zu", offsetof(fsim_frame_t, %s));\n' % f for f, _ in sim.FsimFrame._fields_) +
                   "".join('  printf(" %%zu", offsetof(fsim_frame_sensor_t, %s));\n' % f for f, _ in sim.FsimFrameSensor._fields_) + "  return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_frames.o")])
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_frames.h"\nint fsim_set_frames(fsim_t *s, int a, const fsim_frame_sensor_t *k) { (void)s; (void)k; return a; }\n'
                    "int fsim_frame_state(fsim_t *s, float *a, float *b, float *c, float *d) { (void)s; (void)a; (void)b; (void)c; (void)d; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [ctypes.sizeof(sim.FsimFrame), ctypes.sizeof(sim.FsimFrameSensor), MAX_SENSORS, MAX_NV] and got[:2] == [32, 64]
    assert got[4:] == [getattr(sim.FsimFrame, f).offset for f, _ in sim.FsimFrame._fields_] + [getattr(sim.FsimFrameSensor, f).offset for f, _ in sim.FsimFrameSensor._fields_]
    assert got[4:] == [0, 4, 16, 0, 32]


def test_frames_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_frames.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("body is a model body id before reduction, -1 means the world", "quaternion wxyz, normalised by the library in double",
              "folds the body into its reduced body with body_relpos / body_relquat in double at set time, as fsim_set_cameras does for mounts",
              "(p, R, q) is the world pose of F", "the world-frame linear velocity of the material point at p and the angular velocity of F's body",
              "A world reference has p_g = 0, R_g = I, v_g = w_g = 0", "r = p - p_g", "pos = R_g^T r", "quat = qnormalized(conj(q_g) (x) q), wxyz, not sign-canonicalised",
              "vel[0:3] = R_g^T (v - v_g - w_g x r)", "This is the exact time derivative of pos", "vel[3:6] = R_g^T (w - w_g)",
              "d quat / dt = 1/2 (0, vel[3:6]) (x) quat", "jac is [6][nv], linear rows first, such that vel = jac @ qvel in real arithmetic",
              "linear rows = R_g^T (jp - jp_g + [r]x jr_g)", "angular rows = R_g^T (jr - jr_g)", "Body twists follow fsim_flow.h's rule exactly",
              "a hinge turns about its anchor, a slide moves along its axis", "v(x_b) = qvel[0:3] and its angular qvel[3:6] in the body's own frame",
              "reduced body 0 has twist 0", "that dof's unit twist about the world origin, taken at p",
              "hinge (anchor x a, a); slide (a, 0); free translation (e_i, 0); free rotation (x_b x R_b e_i, R_b e_i)",
              "The column is zero unless the dof's reduced body is an ancestor-or-self of the frame's",
              "follows the env's cursor position exactly as a camera on a cursor body does", "It has no velocity and no Jacobian columns, because the offset is a teleport",
              "writes no state, RNG draw, look-ahead shadow or counter", "depends only on its own record and the frame set", "does not depend on the other sensors of the set",
              "Without a frame set, nothing is allocated or launched", "n_sensors == 0 clears", "waits for the handle's stream before it replaces the tables",
              "more than 64 sensors", "a body unknown to the model", "a non-finite pose or a zero quaternion", "a model with more than 32 reduced bodies", "nv above 128",
              "A refused set leaves the previous set in place", "any may be NULL, not all", "settled exactly as fsim_pair_distance settles it", "returns without waiting",
              "null handle, no frame set, all four pointers NULL"):
        assert s in flat, s


# ---- the reference against central differences of the oracle's kinematics ---------------------------------------------------------------
def _random_state(m, seed):
    """qpos0 with every part turned by a random unit quaternion and shifted, the arm joints moved, qvel uniform(-1, 1) on every dof"""
    rng = np.random.RandomState(seed)
    q = np.asarray(m.arrays["qpos0"], dtype=np.float64).copy()
    for a in np.asarray(m.part_qposadr, dtype=np.int64):
        q[a:a + 3] += rng.uniform(-0.2, 0.2, 3)
        u = rng.normal(size=4)
        q[a + 3:a + 7] = u / np.linalg.norm(u)
    adr = np.asarray(m.arm_qposadr, dtype=np.int64).reshape(-1)
    q[adr] += rng.uniform(-0.25, 0.25, len(adr))
    return q, rng.uniform(-1.0, 1.0, m.nv)


def _liden_sensors(m):
    pairs = connector_pairs(m)
    sites, sbody = m.meta["site_names"], np.asarray(m.arrays["site_bodyid"])
    assert all(sbody[sites.index(a)] != sbody[sites.index(b)] for a, b in pairs)
    (a0, b0), (a1, b1) = pairs[0], pairs[-1]
    return [FrameSensor(Frame(site=a0), ref=Frame(site=b0)), FrameSensor(Frame(site=b1), ref=Frame(site=a1)),  # site to site across two parts
            FrameSensor(Frame(site="grip_site"), ref=Frame(site=a0)), FrameSensor(Frame(site="l_g_grip_site"), ref=Frame(site=b1)),  # grip site to a connector site
            FrameSensor(Frame(site=a1), ref=Frame(site="grip_site")), FrameSensor(Frame(site=b0), ref=Frame(site="l_g_grip_site"))]  # a connector site to the grip site


@pytest.fixture(scope="module")
def liden():
    m = load_compiled("Baxter", "table_liden_0921")
    osim = OracleSim(m)
    qpos, qvel = _random_state(m, 7)
    sensors = _liden_sensors(m)
    fref.set_state(osim, m, qpos, qvel)
    ref = fref.evaluate_set(osim, m, sensors)
    side = {}
    for sgn in (-1, 1):
        fref.set_state(osim, m, fref.advance(m, qpos, qvel, sgn * FD_H), qvel)
        side[sgn] = fref.evaluate_set(osim, m, sensors)
    osim.close()
    return m, qvel, sensors, ref, side


def test_reference_velocity_is_the_derivative_of_the_reference_pose(liden):
    """independent of body_jac: the relative position differenced at h = 1e-4 for vel[0:3], the axial vector of R_rel(t + h) R_rel(t - h)^T /
    (4 h) for vel[3:6]"""
    m, qvel, sensors, ref, side = liden
    assert m.nv == 91 and len(sensors) == 6
    worst = [0.0, 0.0]
    for i, s in enumerate(sensors):
        lin = (side[1]["pos"][i] - side[-1]["pos"][i]) / (2 * FD_H)
        M = side[1]["R_rel"][i] @ side[-1]["R_rel"][i].T
        ang = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / (4 * FD_H)
        el = np.linalg.norm(lin - ref["vel"][i, :3]) / ref["scale_lin"][i]
        ea = np.linalg.norm(ang - ref["vel"][i, 3:]) / ref["scale_ang"][i]
        print("sensor %d %r: linear %.2e of S = %.3f, angular %.2e of S = %.3f" % (i, s, el, ref["scale_lin"][i], ea, ref["scale_ang"][i]))
        assert ref["scale_lin"][i] > 0.1 and ref["scale_ang"][i] > 0.1
        assert el <= FD_TOL and ea <= FD_TOL, (i, el, ea)
        worst = [max(worst[0], el), max(worst[1], ea)]
    print("worst ratio to S: linear %.2e, angular %.2e" % tuple(worst))


def test_reference_velocity_is_jacobian_times_qvel(liden):
    m, qvel, sensors, ref, _ = liden
    for i in range(len(sensors)):
        assert ref["jac"][i].shape == (6, m.nv)
        assert np.abs(ref["jac"][i] @ qvel - ref["vel"][i]).max() <= 1e-12, i
        cols = int((np.abs(ref["jac"][i]).max(axis=0) > 0).sum())
        assert cols == 12 if i < 2 else cols >= 7 + 6, (i, cols)  # two parts' free joints; an arm's dofs and a part's free joint, at least
    # the quaternion is that of the relative rotation
    for i in range(len(sensors)):
        assert np.abs(fref.q2m(ref["quat"][i]) - ref["R_rel"][i]).max() <= 1e-12

"""Force-torque, accelerometer and joint-load sensors, host side (furniture_amd/wrench.py, include/fsim_wrench.h) and their float64
reference (tests/wrench_reference.py): validation and refusals on the three agents, the header as plain C11 with exported and disjoint
symbols, and the reference held to facts it did not use -- the joint-axis identity against the oracle's M qacc + bias, Newton's law of
the free parts, the accelerations by finite difference of the positions -- on the states tests/test_wrench_gpu.py uses, each checked for
the conditions it is used under; and what fp32 alone does to the GPU test's measures (wref.WRENCH_FLOOR, WRIST_FLOOR, WRENCH_FLOOR_ABS, QACC_FLOOR).  The device:
tests/test_wrench_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.frames import Frame
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.wrench import MAX_SENSORS, MAX_SLOTS, WrenchSensor, WrenchSet, check, cut_body, part_sensors, sensor_table, wrist_sensor
from oracle.oracle_sim import OracleSim
from tests import contacts_reference as cref
from tests import wrench_reference as wref
from tests.abi_session import CPU_LIB, Abi, Session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The joint-axis identity and Newton's law of the free parts hold in the reference up to the oracle's rounding and the solve's tolerance:
# 4 x the largest residual measured over every state of this file, over the env's largest |qfrc_constraint| -- and, for the envs where
# that is zero, a bound of its own on the absolute residual in newtons / newton metres.  Measured: joint axis 6.435e-14 relative (sweep, table_lack_0825) and 4.583e-13 N m absolute (moving,
# desk_mikael_1064, where no constraint force exists); free parts 6.435e-14 relative (sweep, table_lack_0825) and 2.271e-15 absolute
# (moving, desk_mikael_1064).  The identity needs one term the issue's statement of it leaves out: the rotor inertia armature[d] qacc[d]
# (Baxter: 0.01 kg m^2 per joint), which is in M and in no body; without it Baxter's residual is 5 N m.
AXIS_MEASURED = dict(rel=6.435e-14, abs=4.583e-13)
FREE_MEASURED = dict(rel=6.435e-14, abs=2.271e-15)
AXIS_TOL, FREE_TOL = {k: 4.0 * v for k, v in AXIS_MEASURED.items()}, {k: 4.0 * v for k, v in FREE_MEASURED.items()}
# d2p/dt2 of the reference against Jp qacc + ((Jp(q+) - Jp(q-)) / 2h) qvel with the oracle's body Jacobians at the moved origin: the
# central difference's error falls as h^2 until rounding (1e-16 / h per unit of Jp) takes over; between h = 1e-5 and h = 1e-6 the
# difference is flat -- 3.506e-10 and 3.632e-10 m/s^2 in the moving state of desk_mikael_1064, where |d2p/dt2| reaches 3.4e3 m/s^2 (1e-13
# of it); 7.5e-11 and 1.4e-10 for table_lack_0825; below 1e-12 in the states with qvel = 0, where the second term vanishes
FD_H = 1e-5
FD_MEASURED = 3.506e-10
FD_TOL = 4.0 * FD_MEASURED


# ---- validation -----------------------------------------------------------------------------------------------------------------------
def test_sensor_and_set_validation():
    with pytest.raises(TypeError, match="Frame"):
        WrenchSensor("0_part0")
    with pytest.raises(ValueError, match="fixed in the world"):
        WrenchSensor(Frame())
    s = WrenchSensor(Frame(body="0_part0"))
    assert "WrenchSensor" in repr(s) and s.cut is None
    for kw in (dict(external=1), dict(joint="yes")):
        with pytest.raises(ValueError, match="boolean"):
            WrenchSet([s], **kw)
    with pytest.raises(TypeError, match="WrenchSensor"):
        WrenchSet([s, "0_part0"])
    with pytest.raises(ValueError, match="0 sensors"):
        WrenchSet([])
    with pytest.raises(ValueError, match="%d sensors" % (MAX_SENSORS + 1)):
        WrenchSet([s] * (MAX_SENSORS + 1))
    with pytest.raises(TypeError, match="WrenchSet"):
        check([s])
    assert WrenchSet(s).n_sensors == 1 and WrenchSet([s] * MAX_SENSORS).n_sensors == MAX_SENSORS
    assert WrenchSet(s).keys() == ["wrench_force", "wrench_torque", "wrench_accel", "wrench_angacc", "wrench_status"]
    assert WrenchSet(s, external=True, joint=True).keys() == ["wrench_force", "wrench_torque", "wrench_accel", "wrench_angacc", "wrench_external", "wrench_qacc",
                                                             "wrench_qfrc_constraint", "wrench_status"]
    assert ["wrench_" + f for f in sim.WRENCH_OUT_FIELDS] == WrenchSet(s, external=True, joint=True).keys()  # the order of fsim_wrench_out_t


@pytest.mark.parametrize("agent,furniture", [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table")])
def test_sensor_table_on_the_three_agents(agent, furniture):
    m = load_compiled(agent, furniture)
    A = m.arrays
    names, red = m.meta["body_names"], np.asarray(A["body_red"])
    wrist, parts = wrist_sensor(m), part_sensors(m)
    assert len(wrist) == len(np.asarray(A["eef_siteid"])) == {"Sawyer": 1, "Baxter": 2, "Cursor": 0}[agent] and len(parts) == m.nparts
    ws = WrenchSet(wrist + parts + [WrenchSensor(Frame(body=m.meta["part_names"][0], pos=(0.1, 0.0, -0.2), quat=(0.0, 2.0, 0.0, 0.0)))], external=True)
    tab = sensor_table(m, ws)
    assert len(tab) == ws.n_sensors
    for i, k in enumerate(wrist):  # the grip site sits on a body without a joint of its own: the cut is at the last arm joint, and repr says so
        site = int(np.asarray(A["eef_siteid"])[i])
        body = int(np.asarray(A["site_bodyid"])[site])
        assert tab[i].body == body and np.asarray(A["body_jntnum"])[body] == 0
        cut = names.index(k.cut)
        assert np.asarray(A["body_jntnum"])[cut] == 1 and red[cut] == red[body] and cut == wref.cut_of(m, body)[0] and "cut at the joint of %r" % k.cut in repr(k)
        assert np.allclose(list(tab[i].pos), np.asarray(A["site_pos"]).reshape(-1, 3)[site], atol=1e-7)
    for i, p in enumerate(m.meta["part_names"]):
        t = tab[len(wrist) + i]
        assert names[t.body] == p == parts[i].cut and list(t.pos) == [0.0, 0.0, 0.0] and list(t.quat) == [1.0, 0.0, 0.0, 0.0]
    last = tab[len(tab) - 1]
    assert np.allclose(list(last.pos), (0.1, 0.0, -0.2)) and np.allclose(list(last.quat), (0.0, 1.0, 0.0, 0.0))  # normalised
    # refusals that need the model: unknown names, a body fixed in the world
    fixed = [names[b] for b in range(1, m.nbody) if red[b] == 0]
    assert cut_body(m, 0) is None
    for fr, msg in [(Frame(body="no_such_body"), "unknown body"), (Frame(site="no_such_site"), "unknown site"), (Frame(body="world"), "does not move")] + \
                   ([(Frame(body=fixed[0]), "does not move")] if fixed else []):
        with pytest.raises(ValueError, match=msg):
            sensor_table(m, WrenchSet([WrenchSensor(fr)]))


def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = WrenchSet([WrenchSensor(Frame(body="0_part0"))])
    with pytest.raises(TypeError, match="WrenchSet"):
        FurnitureBatchEnv("Sawyer", 1, wrenches=[WrenchSensor(Frame(body="0_part0"))])
    with pytest.raises(NotImplementedError, match="wrenches= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, wrenches=spec)
    with pytest.raises(NotImplementedError, match="wrenches= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(wrenches=spec))

    class _Handle:  # a handle with a wrench set and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs, frames, dyn, contacts, wrench_set = None, None, None, None, None, None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="wrench-sensor outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_wrench_header_symbols_are_exported():
    assert sim.WRENCH_SYMBOLS == ["fsim_set_wrenches", "fsim_wrenches"]
    assert sorted(_declared("fsim_wrench.h")) == sorted(sim.WRENCH_SYMBOLS)
    lists = [n for n in dir(sim) if n.endswith("_SYMBOLS") and n != "WRENCH_SYMBOLS"]
    assert len(lists) >= 12 and {"EXPORTED_SYMBOLS", "DYN_SYMBOLS", "CONTACT_SYMBOLS"} <= set(lists)
    assert not set(sim.WRENCH_SYMBOLS) & set().union(*[set(getattr(sim, n)) for n in lists])
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h") and h != "fsim_wrench.h"]
    assert {"fsim.h", "fsim_frames.h", "fsim_contacts.h"} <= set(others)
    assert not set(sim.WRENCH_SYMBOLS) & set().union(*[_declared(h) for h in others])
    lib = ctypes.CDLL(sim.build())
    for n in sim.WRENCH_SYMBOLS:
        assert hasattr(lib, n), n


def test_wrench_header_is_plain_c11(tmp_path):
    src = tmp_path / "use_wrench.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsim_wrench.h"\n'
                   "int use(fsim_t *s, const fsim_wrench_sensor_t *k, float *f) { fsim_wrench_out_t o = {0}; o.force = f; return fsim_set_wrenches(s, 1, k) + fsim_wrenches(s, &o); }\n"
                   'int main(void) { printf("%d %d %d %d %d %d", FSIM_WRENCH_MAX_SENSORS, FSIM_WRENCH_MAX_SLOTS, (int)sizeof(fsim_wrench_sensor_t), (int)sizeof(fsim_wrench_out_t), '
                   "(int)offsetof(fsim_wrench_sensor_t, quat), (int)offsetof(fsim_wrench_out_t, status)); return 0; }\n")
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_wrench.h"\nint fsim_set_wrenches(fsim_t *s, int a, const fsim_wrench_sensor_t *k) { (void)s; (void)k; return a; }\n'
                    "int fsim_wrenches(fsim_t *s, const fsim_wrench_out_t *o) { (void)s; (void)o; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [MAX_SENSORS, MAX_SLOTS, ctypes.sizeof(sim.FsimWrenchSensor), ctypes.sizeof(sim.FsimWrenchOut), sim.FsimWrenchSensor.quat.offset, sim.FsimWrenchOut.status.offset]
    assert len(sim.WRENCH_OUT_FIELDS) == 8 and ctypes.sizeof(sim.FsimWrenchOut) == 8 * ctypes.sizeof(ctypes.c_void_p) and ctypes.sizeof(sim.FsimWrenchSensor) == 32


# ---- the reference on its own ---------------------------------------------------------------------------------------------------------
def session_state(agent, furniture, n, steps, pre=None):
    """the state the CPU build of the library reaches after a reset (pre: started preassembled) and ``steps`` zero-action steps"""
    from furniture_amd.envs import ResetTableSampler, make_config
    m = load_compiled(agent, furniture)
    ecfg = make_config(unity=False, record_vid=False, furniture_name=furniture, max_episode_steps=150, seed=11)
    p, nz = ResetTableSampler(m, ecfg, 11, 0, n).draw()
    ses = Session(Abi(CPU_LIB), m.to_blob(), n, auto_reset=0, max_episode_steps=150)
    if pre is not None:
        ses.set_preassembled(m, pre)
    if agent == "Cursor":  # (no robot joints: no noise table)
        ses.set_reset_tables(p, np.zeros((n, 1), np.float32), n_noise=0)
    else:
        nz = np.asarray(nz, dtype=np.float32).reshape(n, -1)
        ses.set_reset_tables(np.asarray(p).reshape(n, -1), nz, n_noise=nz.shape[1] // len(m.arm_qposadr))
    ses.reset()
    for _ in range(steps):
        ses.step(np.zeros((n, ses.dof), np.float32))
    st = cref.state_of_session(ses, m)
    ses.close()
    return m, st


def _rest(agent, furniture):
    return session_state(agent, furniture, cref.N_REST, cref.REST_STEPS)


def _weld(agent, furniture):
    return session_state(agent, furniture, wref.N_WELD, wref.WELD_STEPS, pre=[0])


STATES = [("sweep", a, f) for a, f in cref.SWEEP_MODELS] + [("rest", a, f) for a, f in cref.REST_MODELS] + [("lifted", "Sawyer", "table_lack_0825")] + \
         [("moving", a, f) for a, f in wref.MOVING_MODELS] + [("weld", "Sawyer", "table_lack_0825")]
MAKERS = {"sweep": cref.sweep_state, "rest": _rest, "lifted": cref.lifted_state, "moving": wref.moving_states, "weld": _weld}


def sensors_of(m):
    """the sensors the GPU test compares: the wrist, every moving robot body, the parts"""
    return wref.robot_sensors(m) + part_sensors(m)


@pytest.fixture(scope="module", params=STATES, ids=["%s-%s" % (k, f) for k, _, f in STATES])
def state(request):
    kind, agent, furniture = request.param
    m, st = MAKERS[kind](agent, furniture)
    osim = OracleSim(m)
    refs = []
    for e in range(len(st["qpos"])):
        ref = cref.evaluate(osim, m, st, e)
        ref["flags"] = cref.only_contacts(osim, m, st, e)
        d = osim.data
        ref["joint"] = np.array(d.qfrc_passive) + np.array(d.qfrc_actuator) + np.array(d.qfrc_applied) - np.asarray(m.arrays["dof_armature"], dtype=np.float64) * ref["qacc"]
        kin = wref.kinematics(osim, m)
        ref["kin"], ref["ine"] = kin, wref.inertial(osim, m, kin)
        ref["wrench"] = wref.evaluate(osim, m, sensors_of(m))
        refs.append(ref)
    yield dict(kind=kind, m=m, st=st, refs=refs, osim=osim, tag="%s %s" % (kind, furniture))
    osim.close()


def test_states_meet_their_conditions(state):
    """no limit is active anywhere (the identities need it), ncon <= 64, no Cartesian force; no weld except in the weld state, where at
    least one is active in every env; nothing touches a part in the lifted and the moving states, and the moving states move"""
    kind, m, st = state["kind"], state["m"], state["st"]
    part = np.asarray(m.arrays["body_partid"])[np.asarray(m.arrays["geom_bodyid"])] >= 0
    for e, ref in enumerate(state["refs"]):
        no_weld, inside, no_xfrc = ref["flags"]
        assert inside and no_xfrc and len(ref["contacts"]) <= 64
        assert no_weld == (kind != "weld")
        if kind in ("lifted", "moving"):
            assert not any(part[g1] or part[g2] for g1, g2 in ref["contacts"])
        if kind == "moving":
            assert len(ref["contacts"]) == 0 and np.abs(st["qvel"][e]).max() > 0.5
    print("%s: contacts per env %s, active welds per env %s" % (state["tag"], [len(r["contacts"]) for r in state["refs"]], np.asarray(st["eq_active"]).sum(1).tolist()))
    assert len(st["qpos"]) == {"sweep": cref.N_SWEEP, "rest": cref.N_REST, "lifted": 2, "moving": wref.N_MOVING, "weld": wref.N_WELD}[kind]


def _worse(worst, err, ref):
    """err into worst["rel"] over the env's largest |qfrc_constraint|, or into worst["abs"] where that is zero"""
    scale = np.abs(ref["qfrc_constraint"]).max()
    kind = "rel" if scale > 0 else "abs"
    worst[kind] = max(worst[kind], err / scale if scale > 0 else err)


def test_joint_axis_identity(state):
    """for every dof d of every jointed body b, S_d . cfrc_int[b] -- the subtree's inertial wrench minus the constraint force through d,
    qfrc_constraint[d]: with no limit active that is the contacts and welds on the subtree alone -- equals what acts along the joint:
    qfrc_passive + qfrc_actuator + qfrc_applied, minus the rotor inertia armature[d] qacc[d], which M carries and no body does.  S_d is a
    column of the oracle's body Jacobian; the right side is the oracle's M qacc + bias bookkeeping, which the reference did not use."""
    m, osim = state["m"], state["osim"]
    A = m.arrays
    jb, jd, jt = np.asarray(A["jnt_bodyid"]), np.asarray(A["jnt_dofadr"]), np.asarray(A["jnt_type"])
    worst = dict(rel=0.0, abs=0.0)
    for e, ref in enumerate(state["refs"]):
        cref.set_state(osim, m, state["st"], e)
        for j, b in enumerate(jb):
            _, below = wref.cut_of(m, int(b))
            org = ref["kin"]["xpos"][b]
            F, T = wref.subtree_wrench(ref["ine"], below, org)
            jp, jr = osim.body_jac(int(b), org)
            for d in range(jd[j], jd[j] + (6 if jt[j] == wref.JT_FREE else 1)):
                _worse(worst, abs(jp[:, d] @ F + jr[:, d] @ T - ref["qfrc_constraint"][d] - ref["joint"][d]), ref)
    print("%s measured: joint-axis identity %.3e relative, %.3e absolute" % (state["tag"], worst["rel"], worst["abs"]))
    assert worst["rel"] <= AXIS_TOL["rel"] and worst["abs"] <= AXIS_TOL["abs"]


def test_free_parts_obey_newton(state):
    """for every free part, I a + v x* I v with gravity in a, minus the constraint force on its six dofs (contacts and welds; no
    xfrc_applied on these states), is zero: the world-frame force on the three translational dofs, the body-frame torque about the body
    origin on the three rotational ones -- written without the Jacobian"""
    m = state["m"]
    pb, pd = np.asarray(m.arrays["part_bodyid"], dtype=np.int64), np.asarray(m.arrays["part_dofadr"], dtype=np.int64)
    worst = dict(rel=0.0, abs=0.0)
    for ref in state["refs"]:
        for b, d in zip(pb, pd):
            below = np.zeros(m.nbody, dtype=bool)
            below[b] = True
            F, T = wref.subtree_wrench(ref["ine"], below, ref["kin"]["xpos"][b])
            res = np.r_[F - ref["qfrc_constraint"][d:d + 3], ref["kin"]["xmat"][b].T @ T - ref["qfrc_constraint"][d + 3:d + 6]] - ref["joint"][d:d + 6]
            _worse(worst, np.abs(res).max(), ref)
    print("%s measured: free parts %.3e relative, %.3e absolute" % (state["tag"], worst["rel"], worst["abs"]))
    assert worst["rel"] <= FREE_TOL["rel"] and worst["abs"] <= FREE_TOL["abs"]


def _advance(m, qpos, qvel, h):
    """qpos advanced by h qvel, with the quaternion exponential for free joints"""
    A = m.arrays
    q = np.array(qpos, dtype=np.float64)
    for j, t in enumerate(np.asarray(A["jnt_type"])):
        qa, da = int(np.asarray(A["jnt_qposadr"])[j]), int(np.asarray(A["jnt_dofadr"])[j])
        if t != wref.JT_FREE:
            q[qa] += h * qvel[da]
            continue
        q[qa:qa + 3] += h * qvel[da:da + 3]
        w = qvel[da + 3:da + 6] * h  # body frame: q <- q * exp(w / 2)
        ang = np.linalg.norm(w)
        dq = np.r_[np.cos(ang / 2), (np.sin(ang / 2) / ang) * w] if ang > 0 else np.array([1.0, 0.0, 0.0, 0.0])
        a, b = q[qa + 3:qa + 7].copy(), dq
        q[qa + 3:qa + 7] = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
    return q


def test_accelerations_by_finite_difference(state):
    """d2p/dt2 of every sensor origin (accel with g added back, in the world frame) against Jp qacc + ((Jp(q+) - Jp(q-)) / 2h) qvel,
    Jp the oracle's body Jacobian at the origin moved with its body; first env of every state, two step sizes"""
    m, osim, st = state["m"], state["osim"], state["st"]
    sensors = sensors_of(m)
    g = np.asarray(m.arrays["gravity"], dtype=np.float64).reshape(3)
    e, ref = 0, state["refs"][0]
    W = ref["wrench"]
    have = np.einsum("sij,sj->si", W["R"], W["accel"]) + g
    res = {}
    for h in (FD_H, 0.1 * FD_H):
        jps = []
        for sgn in (+1.0, -1.0):
            moved = dict(st, qpos=st["qpos"].copy())
            moved["qpos"][e] = _advance(m, st["qpos"][e], st["qvel"][e], sgn * h)
            cref.set_state(osim, m, moved, e)
            rows = []
            for s in sensors:
                body, org, _ = wref.sensor_frame(osim, m, s)
                rows.append(osim.body_jac(body, org)[0])
            jps.append(np.array(rows))
        cref.set_state(osim, m, st, e)
        jp0 = np.array([osim.body_jac(wref.sensor_frame(osim, m, s)[0], W["origin"][i])[0] for i, s in enumerate(sensors)])
        want = jp0 @ ref["qacc"] + ((jps[0] - jps[1]) / (2.0 * h)) @ st["qvel"][e]
        res[h] = np.abs(have - want).max()
    print("%s measured: d2p/dt2 against the finite difference %.3e (h = %g), %.3e (h = %g); largest |d2p/dt2| %.3g" % (state["tag"], res[FD_H], FD_H, res[0.1 * FD_H], 0.1 * FD_H, np.abs(have).max()))
    assert res[FD_H] <= FD_TOL


def test_what_fp32_alone_does(state):
    """qacc of the checker's float32 build through the C-ABI, pushed through the float64 reference, against the oracle's: force and torque
    of every compared sensor by the GPU test's per-sensor measure (wref.WRENCH_FLOOR, WRIST_FLOOR, WRENCH_FLOOR_ABS), and qacc itself
    (wref.QACC_FLOOR)"""
    m, st, osim = state["m"], state["st"], state["osim"]
    n = len(st["qpos"])
    ses = Session(Abi(os.path.join(ROOT, "oracle", "libfsim_cpu32.so")), m.to_blob(), n, auto_reset=0)
    ses.set_state(m, qacc_warmstart=np.zeros((n, m.nv)), **{k: v for k, v in st.items() if v is not None and v.shape[1] > 0})
    ses.forward()
    buf, sp = np.zeros((n, m.nv), np.float32), sim.StatePtrs()  # (qacc is not among the fields Session.get_state knows)
    sp.qacc = buf.ctypes.data
    ses.abi.check(ses.abi.L.fsim_get_state(ses.h, ctypes.byref(sp)))
    ses.abi.check(ses.abi.L.fsim_sync(ses.h))
    qacc = buf.astype(np.float64)
    ses.close()
    sensors = sensors_of(m)
    vals, vabs, qv, wrist = [], [], [], []
    for e, ref in enumerate(state["refs"]):
        cref.set_state(osim, m, st, e)
        got, W = wref.evaluate(osim, m, sensors, qacc=qacc[e]), ref["wrench"]
        rf, af, pf = wref.wrench_measure(got["force"], W["force"], W["iforce"])
        rt, at, pt = wref.wrench_measure(got["torque"], W["torque"], W["itorque"])
        vals.append(max(rf, rt))
        vabs.append(max(af, at))
        wrist.append(max([max(pf[k], pt[k]) for k in range(len(wrist_sensor(m)))], default=0.0))
        qv.append(wref.qacc_measure(qacc[e], ref["qacc"], m))
    print("%s measured: fp32 floor of force / torque, each sensor over its own reading %.3e (per env %s; the wrist alone %.3e), where the reading is zero %.3e N or N m, "
          "of qacc %.3e (per env %s)" % (state["tag"], max(vals), " ".join("%.1e" % v for v in vals), max(wrist), max(vabs), max(qv), " ".join("%.1e" % v for v in qv)))
    assert max(vals) <= wref.WRENCH_FLOOR and max(wrist) <= wref.WRIST_FLOOR and max(vabs) <= wref.WRENCH_FLOOR_ABS and max(qv) <= wref.QACC_FLOOR

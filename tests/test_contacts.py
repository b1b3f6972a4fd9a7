"""Contact-force sensors, host side (furniture_amd/contacts.py, include/fsim_contacts.h) and their float64 reference
(tests/contacts_reference.py): validation and refusals on the three agents, the header as plain C11 with exported and disjoint symbols,
the reference validated on its own -- on the states tests/test_contacts_gpu.py uses, the oracle's qfrc_constraint is M qacc + qfrc_bias -
qfrc_passive - qfrc_actuator - qfrc_applied, no weld is active and every limited joint is inside its range --, and what fp32 alone does to
the GPU test's measure (cref.FORCE_FLOOR).  The device: tests/test_contacts_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.contacts import MAX_SENSORS, MAX_SLOTS, ContactSensor, ContactSet, check, part_sensors, sensor_table
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.pairs import body_geoms, gripper_bodies
from oracle.oracle_sim import OracleSim
from tests import contacts_reference as cref
from tests.abi_session import CPU_LIB, Abi, Session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The identity M qacc - smooth == qfrc_constraint holds in the oracle up to its own rounding and the solve's tolerance: 4 x the largest
# residual measured over every state of this file, over the env's largest |qfrc_constraint| (force_measure).  Measured 6.354e-14, in the
# sweep scene of table_lack_0825.
IDENTITY_MEASURED = 6.354e-14
IDENTITY_TOL = 4.0 * IDENTITY_MEASURED


# ---- validation -----------------------------------------------------------------------------------------------------------------------
def test_sensor_and_set_validation():
    for a, b, msg in [([], None, "empty"), ("0_part0", [], "empty"), (3.5, None, "body name"), ([1, "x"], None, "body name"), ([True], None, "body name")]:
        with pytest.raises(ValueError, match=msg):
            ContactSensor(a, b)
    s = ContactSensor("0_part0")
    assert s.b is None and "ContactSensor" in repr(s)
    with pytest.raises(ValueError, match="boolean"):
        ContactSet([s], contacts=1)
    with pytest.raises(TypeError, match="ContactSensor"):
        ContactSet([s, "0_part0"])
    with pytest.raises(ValueError, match="0 sensors"):
        ContactSet([])
    with pytest.raises(ValueError, match="%d sensors" % (MAX_SENSORS + 1)):
        ContactSet([s] * (MAX_SENSORS + 1))
    with pytest.raises(TypeError, match="ContactSet"):
        check([s])
    assert ContactSet(s).n_sensors == 1 and ContactSet([s] * MAX_SENSORS).n_sensors == MAX_SENSORS
    assert ContactSet(s).keys() == ["contact_force", "contact_touch", "contact_count", "contact_status"]
    assert ContactSet(s, contacts=True).keys()[4:] == ["con_geoms", "con_pos", "con_normal", "con_dist", "con_force", "con_fn"]


@pytest.mark.parametrize("agent,furniture", [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table")])
def test_sensor_table_on_the_three_agents(agent, furniture):
    m = load_compiled(agent, furniture)
    cg_orig = np.asarray(m.arrays["cg_orig"]).astype(np.int64)
    parts = m.meta["part_names"]
    grip = gripper_bodies(m)
    cs = ContactSet(part_sensors(m) + [ContactSensor(grip, parts[0]), ContactSensor(parts[0], grip), ContactSensor([int(cg_orig[0])], [int(cg_orig[1]), int(cg_orig[2])])], contacts=True)
    tab = sensor_table(m, cs)
    assert len(tab) == m.nparts + 3 == cs.n_sensors
    for i, p in enumerate(parts):  # one sensor per part against everything else: side b is left to the library (nb = 0)
        ids = [tab[i].a[k] for k in range(tab[i].na)]
        assert ids == cg_orig[body_geoms(m, p)].tolist() and tab[i].nb == 0 and len(ids) >= 1
        ma, mb = cs.sensors[i].side_masks(m)
        assert (ma ^ mb).all()
    g, h = tab[m.nparts], tab[m.nparts + 1]  # a pair of sensors with the sides swapped
    assert [g.a[k] for k in range(g.na)] == [h.b[k] for k in range(h.nb)] and [g.b[k] for k in range(g.nb)] == [h.a[k] for k in range(h.na)]
    last = tab[m.nparts + 2]
    assert (last.na, last.nb, last.a[0], last.b[1]) == (1, 2, cg_orig[0], cg_orig[2])
    # refusals that need the model
    ngeom = len(m.arrays["geom_bodyid"])
    free = [g for g in range(ngeom) if g not in set(cg_orig.tolist())]
    for a, b, msg in [("no_such_body", None, "unknown body"), ([ngeom], None, "names geom %d" % ngeom), ([-1], None, "names geom -1"),
                      ([int(cg_orig[0]), int(cg_orig[0])], None, "twice"), (parts[0], [parts[0], parts[1]], "on side a and on side b"),
                      ([int(cg_orig[0])], [int(cg_orig[1]), int(cg_orig[0])], "geom %d is on side a and on side b" % cg_orig[0]),
                      ([int(g) for g in cg_orig], None, "nothing is left for side b")] + ([([free[0]], None, "does not collide")] if free else []):
        with pytest.raises(ValueError, match=msg):
            sensor_table(m, ContactSet([ContactSensor(a, b)]))


def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = ContactSet([ContactSensor("0_part0")])
    with pytest.raises(TypeError, match="ContactSet"):
        FurnitureBatchEnv("Sawyer", 1, contacts=[ContactSensor("0_part0")])
    with pytest.raises(NotImplementedError, match="contacts= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, contacts=spec)
    with pytest.raises(NotImplementedError, match="contacts= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(contacts=spec))

    class _Handle:  # a handle with a contact set and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs, frames, dyn, contacts = None, None, None, None, None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="contact-force outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_contacts_header_symbols_are_exported():
    assert sim.CONTACT_SYMBOLS == ["fsim_set_contacts", "fsim_contact_forces"]
    assert sorted(_declared("fsim_contacts.h")) == sorted(sim.CONTACT_SYMBOLS)
    lists = [n for n in dir(sim) if n.endswith("_SYMBOLS") and n != "CONTACT_SYMBOLS"]
    assert len(lists) >= 11 and {"EXPORTED_SYMBOLS", "DYN_SYMBOLS", "PAIR_SYMBOLS"} <= set(lists)
    assert not set(sim.CONTACT_SYMBOLS) & set().union(*[set(getattr(sim, n)) for n in lists])
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h") and h != "fsim_contacts.h"]
    assert {"fsim.h", "fsim_pairs.h", "fsim_dynamics.h"} <= set(others)
    assert not set(sim.CONTACT_SYMBOLS) & set().union(*[_declared(h) for h in others])
    lib = ctypes.CDLL(sim.build())
    for n in sim.CONTACT_SYMBOLS:
        assert hasattr(lib, n), n


def test_contacts_header_is_plain_c11(tmp_path):
    src = tmp_path / "use_contacts.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsim_contacts.h"\n'
                   "int use(fsim_t *s, const fsim_contact_sensor_t *k, float *f) { fsim_contact_out_t o = {0}; o.force = f; return fsim_set_contacts(s, 1, k) + fsim_contact_forces(s, &o); }\n"
                   'int main(void) { printf("%d %d %d %d %d", FSIM_CON_MAX_SENSORS, FSIM_CON_MAX_SLOTS, (int)sizeof(fsim_contact_sensor_t), (int)sizeof(fsim_contact_out_t), (int)offsetof(fsim_contact_sensor_t, na)); return 0; }\n')
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_contacts.h"\nint fsim_set_contacts(fsim_t *s, int a, const fsim_contact_sensor_t *k) { (void)s; (void)k; return a; }\n'
                    "int fsim_contact_forces(fsim_t *s, const fsim_contact_out_t *o) { (void)s; (void)o; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [MAX_SENSORS, MAX_SLOTS, ctypes.sizeof(sim.FsimContactSensor), ctypes.sizeof(sim.FsimContactOut), sim.FsimContactSensor.na.offset]
    assert len(sim.CONTACT_OUT_FIELDS) == 10 and ctypes.sizeof(sim.FsimContactOut) == 10 * ctypes.sizeof(ctypes.c_void_p)


# ---- the reference on its own ---------------------------------------------------------------------------------------------------------
def _rest_state(agent, furniture):
    """the resting state as the CPU build of the library reaches it: a reset and REST_STEPS zero-action steps"""
    from furniture_amd.envs import ResetTableSampler, make_config
    m = load_compiled(agent, furniture)
    n = cref.N_REST
    ecfg = make_config(unity=False, record_vid=False, furniture_name=furniture, max_episode_steps=150, seed=11)
    p, nz = ResetTableSampler(m, ecfg, 11, 0, n).draw()
    ses = Session(Abi(CPU_LIB), m.to_blob(), n, auto_reset=0, max_episode_steps=150)
    if agent == "Cursor":  # (no robot joints: no noise table)
        ses.set_reset_tables(p, np.zeros((n, 1), np.float32), n_noise=0)
    else:
        nz = np.asarray(nz, dtype=np.float32).reshape(n, -1)
        ses.set_reset_tables(np.asarray(p).reshape(n, -1), nz, n_noise=nz.shape[1] // len(m.arm_qposadr))
    ses.reset()
    for _ in range(cref.REST_STEPS):
        ses.step(np.zeros((n, ses.dof), np.float32))
    st = cref.state_of_session(ses, m)
    ses.close()
    return m, st


STATES = [("sweep", a, f) for a, f in cref.SWEEP_MODELS] + [("rest", a, f) for a, f in cref.REST_MODELS] + [("lifted", "Sawyer", "table_lack_0825")]


@pytest.fixture(scope="module", params=STATES, ids=["%s-%s" % (k, f) for k, _, f in STATES])
def state(request):
    kind, agent, furniture = request.param
    m, st = {"sweep": cref.sweep_state, "rest": _rest_state, "lifted": cref.lifted_state}[kind](agent, furniture)
    osim = OracleSim(m)
    refs = []
    for e in range(len(st["qpos"])):
        ref = cref.evaluate(osim, m, st, e)
        ref["flags"] = cref.only_contacts(osim, m, st, e)
        refs.append(ref)
    yield dict(kind=kind, m=m, st=st, refs=refs, tag="%s %s" % (kind, furniture))
    osim.close()


def test_states_have_contacts_only(state):
    """no active weld, every limited joint inside its range by more than its margin, no Cartesian force: qfrc_constraint is the contacts' alone"""
    for ref in state["refs"]:
        assert ref["flags"] == (True, True, True)
    ncon = [len(r["contacts"]) for r in state["refs"]]
    print("%s: contacts per env %s" % (state["tag"], ncon))
    if state["kind"] == "sweep":
        assert len(ncon) == cref.N_SWEEP and all(0 < k <= 32 for k in ncon)
    if state["kind"] == "rest":
        assert all(k >= 4 for k in ncon)  # the parts rest on the floor
    if state["kind"] == "lifted":  # no contact on any part
        part = np.asarray(state["m"].arrays["body_partid"])[np.asarray(state["m"].arrays["geom_bodyid"])] >= 0
        assert not any(part[g1] or part[g2] for r in state["refs"] for g1, g2 in r["contacts"])


def test_constraint_force_is_mass_times_acceleration_minus_smooth(state):
    worst = 0.0
    for ref in state["refs"]:
        worst = max(worst, cref.force_measure(ref["M"] @ ref["qacc"] - ref["smooth"], ref["qfrc_constraint"]))
    print("%s measured: identity residual %.3e" % (state["tag"], worst))
    assert worst <= IDENTITY_TOL


def test_what_fp32_alone_does(state):
    """qacc of the checker's float32 build through the C-ABI, as a generalised constraint force with the float64 M and smooth forces,
    against the oracle's qfrc_constraint, by the GPU test's measure.  cref.FORCE_FLOOR is the largest over the states of this file."""
    m, st = state["m"], state["st"]
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
    vals = [cref.force_measure(ref["M"] @ qacc[e] - ref["smooth"], ref["qfrc_constraint"]) for e, ref in enumerate(state["refs"])]
    print("%s measured: fp32 floor %.3e (per env %s)" % (state["tag"], max(vals), " ".join("%.1e" % v for v in vals)))
    assert max(vals) <= cref.FORCE_FLOOR


def test_projection_of_the_constraint_force_itself(state):
    """project() against the oracle: a unit force at a part's origin on one of its geoms, against the world, is that part's three
    translational dofs"""
    m = state["m"]
    osim = OracleSim(m)
    cref.set_state(osim, m, state["st"], 0)
    gb, pb = np.asarray(m.arrays["geom_bodyid"]), np.asarray(m.arrays["part_bodyid"])
    floor = int(np.asarray(m.arrays["floor_geomid"]).reshape(-1)[0])
    for i, dofs in enumerate(cref.part_dofs(m)):
        g = int(np.nonzero(gb == pb[i])[0][0])
        F = np.array([0.3, -1.0, 2.0])
        q = cref.project(osim, m, [(floor, g), (-1, -1)], [osim.data.xpos[pb[i]], np.zeros(3)], [F, F])
        assert np.allclose(q[dofs], F, atol=1e-12) and np.abs(np.delete(q, np.r_[dofs, dofs + 3])).max() <= 1e-12
        assert np.allclose(cref.project(osim, m, [(g, floor)], [osim.data.xpos[pb[i]]], [F])[dofs], -F, atol=1e-12)
    osim.close()

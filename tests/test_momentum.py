"""Centre-of-mass, momentum and energy sensors, the parts that run without a GPU: the float64 reference tests/momentum_reference.py against
the mass matrix, finite differences of the potential and of the centre of mass, its own Jacobian and the generalised-momentum identity
p = M qvel; what fp32 alone does to its formulas about the world origin and about a set's own reference point (the floors
tests/test_momentum_gpu.py measures the device against); MomentumSensor / MomentumSet validation, the sensor table, the helpers, the
refusals and the C-ABI of include/fsim_momentum.h (tests/test_momentum_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.momentum import (MAX_SENSORS, MomentumSensor, MomentumSet, all_parts_sensor, body_masks, check, masses, part_sensors, robot_sensor,
                                    sensor_table)
from oracle.oracle_sim import OracleSim
from tests import dynamics_reference as dref
from tests import momentum_reference as mref
from tests.flow_reference import advance, set_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = mref.MODELS
# Central differences in float64.  Steps and tolerances were picked here, on the CPU, each tolerance about 10 x the residual measured over
# the four models, near and far states (every test prints its own):
KINETIC_TOL = 5e-14   # |energy[1] - 1/2 qvel^T full_M qvel| / energy[1]: measured 4.7e-15 (toy_table): two float64 evaluations of one quantity
FD_H = 1e-5           # step of d energy[0] / dq: a hinge angle in rad, a slide or a free translation in m
POTENTIAL_TOL = 1e-9  # |gravity - d energy[0] / dq| / max|gravity|: measured 1.1e-10 (table_liden_0921); truncation h^2 / 6 = 2e-11, the rest is the rounding of the potential over h
COM_H = 1e-4          # time step of d com / dt along advance(qpos, qvel, +-h)
LINVEL_TOL = 2e-8     # |linvel - d com / dt| / max|linvel|: measured 1.6e-9 (table_lack_0825): truncation h^2 |x'''| / 6 = 2e-9 |x'''|
JAC_TOL = 3e-15       # |jac @ qvel - linvel| / max|linvel|: measured 2.2e-16 (toy_table)
MOMENTUM_TOL = 5e-14  # the generalised-momentum identity, |p - formula| / max|p| of the env: measured 5.4e-15 (table_lack_0825)
FLOOR_RATIO = 10.0    # FLOOR_ORIGIN's angmom over FLOOR's in the far states is at least this (measured 20)


@pytest.fixture(scope="module", params=MODELS, ids=[f for _, f in MODELS])
def case(request):
    """the reference of every state of the GPU file's cases (the float32-rounded states the device holds), near and far"""
    agent, furniture = request.param
    m = load_compiled(agent, furniture)
    sensors = mref.sensor_sets(m)
    osim = OracleSim(m)
    groups = {}
    for g in mref.GROUPS:
        qpos, qvel = mref.states(m, furniture, g)
        groups[g] = dict(qpos=qpos, qvel=qvel, refs=[mref.evaluate(osim, m, sensors, qpos[e], qvel[e]) for e in range(len(qpos))])
    yield dict(m=m, tag=furniture, sensors=sensors, groups=groups, osim=osim)
    osim.close()


def _envs(case):
    for g in mref.GROUPS:
        G = case["groups"][g]
        for e in range(len(G["qpos"])):
            yield g, e, G["qpos"][e], G["qvel"][e], G["refs"][e]


def test_the_cases_are_what_the_issue_names(case):
    m, sensors = case["m"], case["sensors"]
    nparts = len(m.meta["part_names"])
    assert len(case["groups"]["near"]["qpos"]) == dref.n_envs(case["tag"]) and len(sensors) == nparts + (2 if robot_sensor(m) is None else 4)
    near, far = case["groups"]["near"]["qpos"], case["groups"]["far"]["qpos"]
    for a in np.asarray(m.part_qposadr, dtype=np.int64):
        assert np.allclose(far[:, a:a + 3] - near[:, a:a + 3], mref.FAR, atol=1e-6) and np.linalg.norm(mref.FAR) == pytest.approx(8.0)
    if case["tag"] == "table_liden_0921":  # nv = 91 and a body on bit 31 of the masks
        assert m.nv == 91 and body_masks(m, sensor_table(m, MomentumSet(sensors)))[nparts - 1] == 1 << 31


def test_kinetic_energy_is_the_mass_matrix_form(case):
    """(a) energy[1] == 1/2 qvel^T full_M qvel, armature included"""
    worst = 0.0
    for g, e, qpos, qvel, ref in _envs(case):
        set_state(case["osim"], case["m"], qpos, qvel)
        worst = max(worst, abs(ref["energy"][1] - 0.5 * qvel @ case["osim"].full_M() @ qvel) / ref["energy"][1])
    print("%s measured: kinetic energy against 1/2 v^T M v: %.3e" % (case["tag"], worst))
    assert worst <= KINETIC_TOL


def test_gravity_is_the_gradient_of_the_potential_energy(case):
    """(b) d energy[0] / dq == gravity of dynamics_reference.evaluate, along each hinge and slide dof and the translations of each free joint"""
    m, osim = case["m"], case["osim"]
    A = m.arrays
    worst, n = 0.0, 0
    G = case["groups"]["near"]
    for e in range(len(G["qpos"])):
        qpos = G["qpos"][e]
        grav = dref.evaluate(osim, m, qpos, G["qvel"][e])["gravity"]
        for jt, qa, da in zip(np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"]), np.asarray(A["jnt_dofadr"])):
            for k in range(3 if jt == 0 else 1):
                qp, qm = qpos.copy(), qpos.copy()
                qp[int(qa) + k] += FD_H
                qm[int(qa) + k] -= FD_H
                fd = (mref.centres(osim, m, [], qp)[1] - mref.centres(osim, m, [], qm)[1]) / (2 * FD_H)
                worst = max(worst, abs(fd - grav[int(da) + k]) / np.abs(grav).max())
                n += 1
    print("%s measured: gravity against d energy[0] / dq over %d dofs: %.3e" % (case["tag"], n, worst))
    assert n >= 2 * 12 and worst <= POTENTIAL_TOL


def test_linvel_is_the_rate_of_com(case):
    """(c) linvel == the central difference of com along advance(qpos, qvel, +-h)"""
    m, osim, sensors = case["m"], case["osim"], case["sensors"]
    worst = 0.0
    for g, e, qpos, qvel, ref in _envs(case):
        cp, cm = mref.centres(osim, m, sensors, advance(m, qpos, qvel, COM_H))[0], mref.centres(osim, m, sensors, advance(m, qpos, qvel, -COM_H))[0]
        worst = max(worst, np.abs((cp - cm) / (2 * COM_H) - ref["linvel"]).max() / np.abs(ref["linvel"]).max())
    print("%s measured: linvel against d com / dt: %.3e" % (case["tag"], worst))
    assert worst <= LINVEL_TOL


def test_jacobian_times_qvel_is_linvel(case):
    """(d) jac @ qvel == linvel; the columns of dofs that move none of a set's bodies are exact zeros"""
    m = case["m"]
    worst = 0.0
    moved = _moved_columns(m, case["sensors"])
    for g, e, qpos, qvel, ref in _envs(case):
        worst = max(worst, np.abs(ref["jac"] @ qvel - ref["linvel"]).max() / np.abs(ref["linvel"]).max())
        for i in range(len(case["sensors"])):
            assert (ref["jac"][i][:, ~moved[i]] == 0).all() and np.abs(ref["jac"][i][:, moved[i]]).max() > 0  # (a part's rotation about its own centre of mass: a zero too)
    print("%s measured: jac @ qvel against linvel: %.3e" % (case["tag"], worst))
    assert worst <= JAC_TOL and all((~mv).any() for mv in moved[:m.nparts])  # (every part leaves the other dofs alone)


def _moved_columns(m, sensors):
    """[S][nv] bool: dof d moves a body of the set -- a body of the set is the dof's body or below it (tests/test_momentum_gpu.py too)"""
    A = m.arrays
    parent, dof_body = np.asarray(A["body_parentid"]).astype(np.int64), np.asarray(A["dof_bodyid"]).astype(np.int64)
    out = []
    for s in sensors:
        above = set()
        for b in mref.model_bodies(m, s):
            while b > 0:
                above.add(b)
                b = int(parent[b])
        out.append(np.array([int(dof_body[d]) in above for d in range(m.nv)]))
    return out


def test_generalised_momentum_identity(case):
    """(e) p = full_M @ qvel ties linvel and angmom to a mass matrix that tests/test_dynamics.py validates by finite differences: for a
    part's sensor p[translation] = m linvel and p[rotation] = R^T (angmom + m (c - x0) x linvel) with x0, R the part's frame; for a hinge d
    of the arm and the sensor of its body's subtree p_d = axis_d . (angmom + m (c - anchor_d) x linvel) + armature_d qvel_d."""
    m, osim = case["m"], case["osim"]
    A = m.arrays
    names = m.meta["body_names"]
    parts = [names.index(p) for p in m.meta["part_names"]]
    dof_body, dof_jnt = np.asarray(A["dof_bodyid"]).astype(np.int64), np.asarray(A["dof_jntid"]).astype(np.int64)
    jtype, jaxis, jpos = np.asarray(A["jnt_type"]), np.asarray(A["jnt_axis"], dtype=np.float64).reshape(-1, 3), np.asarray(A["jnt_pos"], dtype=np.float64).reshape(-1, 3)
    arm = np.asarray(A["dof_armature"], dtype=np.float64)
    hinges = [d for d in range(m.nv) if int(dof_body[d]) not in parts and jtype[dof_jnt[d]] == 3]
    sensors = part_sensors(m) + [MomentumSensor(int(dof_body[d]), subtree=True) for d in hinges]
    mass = mref.set_masses(m, sensors)
    assert np.abs(mass - masses(m, MomentumSet(sensors[:MAX_SENSORS]))[:len(mass)]).max() <= 1e-12 * mass.max()
    worst, n = 0.0, 0
    for g, e, qpos, qvel, _ in _envs(case):
        ref = mref.evaluate(osim, m, sensors, qpos, qvel)
        p = osim.full_M() @ qvel
        scale = np.abs(p).max()
        xpos, xmat = np.array(osim.data.xpos, dtype=np.float64), np.array(osim.data.xmat, dtype=np.float64).reshape(-1, 3, 3)
        for i, b in enumerate(parts):
            da = int(np.asarray(m.part_dofadr)[i])
            c, v, L = ref["com"][i], ref["linvel"][i], ref["angmom"][i]
            worst = max(worst, np.abs(p[da:da + 3] - mass[i] * v).max() / scale,
                        np.abs(p[da + 3:da + 6] - xmat[b].T @ (L + mass[i] * np.cross(c - xpos[b], v))).max() / scale)
            n += 2
        for k, d in enumerate(hinges):
            i, b, j = len(parts) + k, int(dof_body[d]), int(dof_jnt[d])
            axis, anchor = xmat[b] @ jaxis[j], xpos[b] + xmat[b] @ jpos[j]
            c, v, L = ref["com"][i], ref["linvel"][i], ref["angmom"][i]
            worst = max(worst, abs(p[d] - (axis @ (L + mass[i] * np.cross(c - anchor, v)) + arm[d] * qvel[d])) / scale)
            n += 1
    print("%s measured: the generalised-momentum identity over %d rows: %.3e" % (case["tag"], n, worst))
    assert worst <= MOMENTUM_TOL and n >= 2 * 2 * len(parts) and (case["tag"] == "toy_table" or len(hinges) >= 7)


def test_what_fp32_alone_does(case):
    """(f) the reference's formulas in float32, about the world origin and about the set's reference point: the floors of the device's
    measures.  mref.FLOOR / FLOOR_ORIGIN hold the largest over the four models; far from the origin the first way loses angmom."""
    m, osim, sensors = case["m"], case["osim"], case["sensors"]
    got = {g: {a: {k: 0.0 for k in mref.KEYS} for a in ("ref", "origin")} for g in mref.GROUPS}
    for g, e, qpos, qvel, ref in _envs(case):
        for a in ("ref", "origin"):
            ms = mref.measures(ref, mref.evaluate_f32(osim, m, sensors, qpos, qvel, a))
            got[g][a] = {k: max(got[g][a][k], ms[k]) for k in mref.KEYS}
    for g in mref.GROUPS:
        print("%s measured: fp32 floor, %s: %s" % (case["tag"], g, "  ".join("%s %.3e (origin %.3e)" % (k, got[g]["ref"][k], got[g]["origin"][k]) for k in mref.KEYS)))
        for k in mref.KEYS:  # (BLAS builds may differ in what they round: the recorded floors bound every model's, and one model reaches them)
            assert got[g]["ref"][k] <= 1.25 * mref.FLOOR[g][k] and got[g]["origin"][k] <= 1.25 * mref.FLOOR_ORIGIN[g][k], (g, k)
    if case["tag"] == "toy_table":  # the model that sets the far angmom floors
        assert got["far"]["origin"]["angmom"] >= FLOOR_RATIO * got["far"]["ref"]["angmom"]
        assert got["far"]["ref"]["angmom"] == pytest.approx(mref.FLOOR["far"]["angmom"], rel=0.25) and got["far"]["origin"]["angmom"] == pytest.approx(mref.FLOOR_ORIGIN["far"]["angmom"], rel=0.25)
    assert mref.FLOOR_ORIGIN["far"]["angmom"] >= FLOOR_RATIO * mref.FLOOR["far"]["angmom"]


# ---- MomentumSensor, MomentumSet, the sensor table and the helpers ---------------------------------------------------------------------
def test_sensor_and_set_validation():
    """(g)"""
    for args, kw, exc, msg in [(([],), {}, ValueError, "empty set"), ((1.5,), {}, TypeError, "a body name"), (([1.5],), {}, TypeError, "a name or a model body id"),
                               (([True],), {}, TypeError, "a name or a model body id"), (([-1],), {}, ValueError, "negative body id"),
                               ((["a", "b"],), dict(subtree=[True]), ValueError, "one boolean per body"), (("a",), dict(subtree=1), ValueError, "one boolean per body"),
                               (("a",), dict(subtree=[1]), ValueError, "one boolean per body")]:
        with pytest.raises(exc, match=msg):
            MomentumSensor(*args, **kw)
    s = MomentumSensor("0_part0")
    assert s.bodies == ["0_part0"] and s.subtree == [True] and "subtree=True" in repr(s)
    s2 = MomentumSensor([3, "x"], subtree=[False, True])
    assert s2.bodies == [3, "x"] and s2.subtree == [False, True] and MomentumSensor(np.int32(4), subtree=False).bodies == [4]
    for kw, msg in [(dict(jacobian=1), "jacobian is a boolean"), (dict(energy="yes"), "energy is a boolean")]:
        with pytest.raises(ValueError, match=msg):
            MomentumSet([s], **kw)
    with pytest.raises(ValueError, match="0 sensors"):
        MomentumSet([])
    with pytest.raises(ValueError, match="65 sensors"):
        MomentumSet([s] * (MAX_SENSORS + 1))
    with pytest.raises(TypeError, match="MomentumSensor"):
        MomentumSet(["0_part0"])
    with pytest.raises(TypeError, match="MomentumSet"):
        check([s])
    ms = MomentumSet(s)
    assert ms.n_sensors == 1 and MomentumSet([s] * MAX_SENSORS).n_sensors == MAX_SENSORS == 64 and not ms.jacobian and not ms.energy
    assert ms.keys() == ["mom_com", "mom_linvel", "mom_angmom"] and "1 sensors" in repr(ms)
    full = MomentumSet(s, jacobian=True, energy=True)
    assert full.keys() == ["mom_com", "mom_linvel", "mom_angmom", "mom_jac", "mom_energy"] == ["mom_" + f for f in sim.MOMENTUM_OUT_FIELDS]  # the order of fsim_momentum_out_t
    assert MomentumSet(s, energy=True).keys() == ["mom_com", "mom_linvel", "mom_angmom", "mom_energy"]
    ms.sensors.append("x")  # check() looks again
    with pytest.raises(TypeError, match="MomentumSensor"):
        check(ms)


@pytest.mark.parametrize("agent,furniture", [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table")])
def test_sensor_table_on_the_three_agents(agent, furniture):
    """(h) the tables, the masks and the masses; (i) the refusals that need the model"""
    m = load_compiled(agent, furniture)
    A = m.arrays
    names, red = m.meta["body_names"], np.asarray(A["body_red"]).astype(np.int64)
    parts, robot = part_sensors(m), robot_sensor(m)
    assert len(parts) == m.nparts and (robot is None) == (agent == "Cursor")
    sensors = mref.sensor_sets(m)
    ms = MomentumSet(sensors, jacobian=True)
    adr, bodies, subtree = tab = sensor_table(m, ms)
    assert all(a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] for a in tab) and len(adr) == len(sensors) + 1 and adr[0] == 0 and adr[-1] == len(bodies) == len(subtree)
    for i, p in enumerate(m.meta["part_names"]):
        assert bodies[adr[i]:adr[i + 1]].tolist() == [names.index(p)] and subtree[adr[i]] == 0
    masks = body_masks(m, tab)
    for i, s in enumerate(sensors):  # the masks are the compiled bodies of the reference's own resolution
        assert masks[i] == sum(1 << r for r in set(int(red[b]) for b in mref.model_bodies(m, s))), i
    assert masks[m.nparts - 1 + (1 if robot is None else 3)] == sum(masks[:m.nparts])  # all parts together
    mass = masses(m, ms)
    assert mass.dtype == np.float64 and np.allclose(mass, mref.set_masses(m, sensors), rtol=1e-13, atol=0) and np.allclose(mass[:m.nparts], np.asarray(A["body_mass"])[[names.index(p) for p in m.meta["part_names"]]])
    if robot is not None:
        rmask = masks[m.nparts]
        assert rmask & sum(masks[:m.nparts]) == 0 and rmask | sum(masks[:m.nparts]) == (1 << int(np.asarray(A["rdims"])[0])) - 2  # the robot and the parts: everything that moves
        # a body without a joint of its own stands for the compiled body it was folded into; listed with that body, it counts once
        folded = [b for b in range(1, m.nbody) if red[b] > 0 and np.asarray(A["body_jntnum"])[b] == 0]
        owner = [b for b in range(1, m.nbody) if red[b] == red[folded[0]] and np.asarray(A["body_jntnum"])[b] == 1][0]
        twice = MomentumSet([MomentumSensor(folded[0], subtree=False), MomentumSensor(owner, subtree=False), MomentumSensor([owner, folded[0], owner], subtree=[False, True, True])])
        mk = body_masks(m, sensor_table(m, twice))
        assert mk[0] == mk[1] == 1 << int(red[owner]) and mk[2] & mk[0] and masses(m, twice)[0] == masses(m, twice)[1] > 0
        # a subtree is the set of bodies below: the arm link's holds the hand and the fingers, not the links above it
        link = names.index(mref.arm_link(m))
        sub = body_masks(m, sensor_table(m, MomentumSet(MomentumSensor(link))))[0]
        assert sub & (1 << int(red[link])) and sub & rmask == sub and bin(sub).count("1") >= 4 and sub < rmask and masks[m.nparts + 1] == sub
    fixed = [names[b] for b in range(1, m.nbody) if red[b] == 0]
    for s, msg in [(MomentumSensor("no_such_body"), "unknown body"), (MomentumSensor("world"), "does not move"), (MomentumSensor(0), "does not move"),
                   (MomentumSensor(m.nbody), "out of range"), (MomentumSensor([names.index(m.meta["part_names"][0]), m.nbody + 3]), "out of range")] + \
                  ([(MomentumSensor(fixed[0]), "does not move"), (MomentumSensor([m.meta["part_names"][0], fixed[0]], subtree=False), "does not move")] if fixed else []):
        with pytest.raises(ValueError, match=msg):
            sensor_table(m, MomentumSet([s]))
    with pytest.raises(TypeError, match="MomentumSet"):
        sensor_table(m, [parts[0]])


def test_host_refusals_of_the_caps_and_of_a_set_without_mass():
    """(i) the caps (no shipped model is beyond them) and a set whose bodies weigh nothing"""
    m = load_compiled("Sawyer", "table_lack_0825")

    class _Big:
        nv = 30
        meta = m.meta
        arrays = dict(m.arrays, rdims=np.array([33]))
    with pytest.raises(ValueError, match="33 reduced bodies"):
        sensor_table(_Big, MomentumSet(part_sensors(m)))
    _Big.nv, _Big.arrays = 129, dict(m.arrays)
    with pytest.raises(ValueError, match="nv = 129"):
        sensor_table(_Big, MomentumSet(part_sensors(m)))
    part = m.meta["body_names"].index(m.meta["part_names"][1])
    rmass = np.array(m.arrays["r_mass"], dtype=np.float64)
    rmass[int(m.arrays["body_red"][part])] = 0.0
    _Big.nv, _Big.arrays = m.nv, dict(m.arrays, r_mass=rmass)
    with pytest.raises(ValueError, match="sensor 1 .* zero total mass"):
        sensor_table(_Big, MomentumSet(part_sensors(m)))
    assert len(sensor_table(_Big, MomentumSet([all_parts_sensor(m)]))[1]) == m.nparts  # with the others it weighs something


def test_wrapper_refusals():
    """(k) the VecEnv wrapper, the mixed batch and the multi-GPU gather refuse momenta= in the words of the other seven families"""
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import ALL_SENSOR_FAMILIES, SENSOR_FAMILIES, FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    assert len(SENSOR_FAMILIES) == 7 and ALL_SENSOR_FAMILIES[:7] == SENSOR_FAMILIES and [f.kw for f in ALL_SENSOR_FAMILIES[7:]] == ["momenta"]
    f = ALL_SENSOR_FAMILIES[7]
    assert (f.module, f.cls, f.attr, f.set, f.shapes, f.call) == ("momentum", "MomentumSet", "momenta_set", "set_momenta", "momentum_shapes", "momenta")
    assert all(hasattr(sim.FSim, n) for n in (f.attr, f.set, f.shapes, f.call)) and sim.FSim.momenta_set is None and FurnitureBatchEnv.momenta is None
    spec = MomentumSet([MomentumSensor("0_part0")])
    with pytest.raises(TypeError, match="MomentumSet"):
        FurnitureBatchEnv("Sawyer", 1, momenta=[MomentumSensor("0_part0")])
    with pytest.raises(NotImplementedError, match=r"momenta= is not supported by the mixed-furniture batch \(one momentum set per FurnitureBatchEnv\)"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, momenta=spec)
    with pytest.raises(NotImplementedError, match=r"momenta= is not supported by the VecEnv wrapper .*FurnitureBatchEnv\(\.\.\., momenta=MomentumSet\(\.\.\.\)\), whose momentum outputs stay on the device"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(momenta=spec))

    class _Handle:  # a handle with a momentum set and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs, frames, dyn, contacts, wrench_set, momenta_set = (None,) * 12 + (spec,)

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="momentum-sensor outputs are not part of the multi-GPU gather; compute them on each rank instead"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_momentum_header_symbols_are_exported():
    """(j)"""
    assert sim.MOMENTUM_SYMBOLS == ["fsim_set_momenta", "fsim_momenta"]
    assert sorted(_declared("fsim_momentum.h")) == sorted(sim.MOMENTUM_SYMBOLS)
    lists = [n for n in dir(sim) if n.endswith("_SYMBOLS") and n != "MOMENTUM_SYMBOLS"]
    assert len(lists) >= 13 and {"EXPORTED_SYMBOLS", "DYN_SYMBOLS", "WRENCH_SYMBOLS"} <= set(lists)
    assert not set(sim.MOMENTUM_SYMBOLS) & set().union(*[set(getattr(sim, n)) for n in lists])
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h") and h != "fsim_momentum.h"]
    assert {"fsim.h", "fsim_dynamics.h", "fsim_wrench.h"} <= set(others)
    assert not set(sim.MOMENTUM_SYMBOLS) & set().union(*[_declared(h) for h in others])
    lib = ctypes.CDLL(sim.build())
    for n in sim.MOMENTUM_SYMBOLS:
        assert hasattr(lib, n), n


def test_momentum_header_is_plain_c11(tmp_path):
    """(j)"""
    src = tmp_path / "use_momentum.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsim_momentum.h"\n'
                   "int use(fsim_t *s, const int32_t *t, float *f) { fsim_momentum_out_t o = {0}; o.energy = f; return fsim_set_momenta(s, 1, t, t, t) + fsim_momenta(s, &o); }\n"
                   'int main(void) { printf("%d %d %d %d", FSIM_MOM_MAX_SENSORS, (int)sizeof(fsim_momentum_out_t), (int)offsetof(fsim_momentum_out_t, jac), '
                   "(int)offsetof(fsim_momentum_out_t, energy)); return 0; }\n")
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_momentum.h"\nint fsim_set_momenta(fsim_t *s, int a, const int32_t *x, const int32_t *y, const int32_t *z) { (void)s; (void)x; (void)y; (void)z; return a; }\n'
                    "int fsim_momenta(fsim_t *s, const fsim_momentum_out_t *o) { (void)s; (void)o; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [MAX_SENSORS, ctypes.sizeof(sim.FsimMomentumOut), sim.FsimMomentumOut.jac.offset, sim.FsimMomentumOut.energy.offset]
    assert len(sim.MOMENTUM_OUT_FIELDS) == 5 and ctypes.sizeof(sim.FsimMomentumOut) == 5 * ctypes.sizeof(ctypes.c_void_p)

"""Reference centre of mass, momentum and energy for the device's momentum sensors (include/fsim_momentum.h), in float64.

It builds on the oracle (oracle/oracle_sim.py) and shares no code with the device path: from an OracleSim set to a given qpos / qvel with
tests.flow_reference.set_state it takes every MODEL body's inertial origin data.xipos, its orientation data.xmat and its Jacobians
body_jac(b, xipos_b), and the UNREDUCED model tables body_mass, body_inertia and body_iquat -- so it also checks what folding jointless
bodies into their moving ancestors did to the masses and inertias the device works with.  A sensor's set of model bodies is resolved here,
from body_parentid and body_red, not with furniture_amd.momentum's tables.  tests/test_momentum.py validates the outputs against the mass
matrix, finite differences and the generalised-momentum identity before tests/test_momentum_gpu.py uses them as a yardstick.
"""

import numpy as np

from furniture_amd import momentum as mom
from tests import dynamics_reference as dref
from tests.flow_reference import set_state

MODELS = dref.MODELS
SEED = dref.SEED
FAR = np.array([4.8, -6.4, 0.0])  # the shift of every free part in the far states: 8 m from where it was
GROUPS = ("near", "far")
KEYS = ("com", "linvel", "angmom", "jac", "energy")
# What fp32 alone does: the measures of the reference's own formulas evaluated in float32 on float32-rounded body terms (inertial origins,
# frames, Jacobians, masses, inertias), against the float64 reference, the largest over the four models' cases of each group (computed and
# checked by tests/test_momentum.py::test_what_fp32_alone_does; rounded up in the last digit).  FLOOR sums positions relative to the inertial
# origin of the set's lowest-numbered body and forms angmom from (x_b - c) and (v_b - v_c), as the device does; FLOOR_ORIGIN sums about
# the world origin and forms angmom as the difference of two moments about it.  In the far states the second loses angmom: 1.95e-5 against
# 9.51e-7, a factor of 20 (toy_table, whose parts are the lightest); what is left in FLOOR there is the rounding of the world positions
# themselves, 5e-7 m at 8 m against lever arms of centimetres.
FLOOR = dict(near=dict(com=7.92e-8, linvel=1.05e-7, angmom=2.47e-7, jac=8.14e-8, energy=3.61e-7),
             far=dict(com=5.83e-8, linvel=1.05e-7, angmom=9.51e-7, jac=8.14e-8, energy=3.61e-7))
FLOOR_ORIGIN = dict(near=dict(com=2.83e-7, linvel=1.05e-7, angmom=9.89e-7, jac=8.14e-8, energy=3.61e-7),
                    far=dict(com=9.20e-8, linvel=1.05e-7, angmom=1.95e-5, jac=8.14e-8, energy=3.61e-7))


def n_envs(furniture):
    return dref.n_envs(furniture)


def states(model, furniture, group):
    """[n, nq], [n, nv] float64 holding float32 values: dynamics_reference.random_states, and for "far" the same with every free part
    shifted by FAR"""
    qpos, qvel = dref.random_states(model, n_envs(furniture))
    if group == "far":
        for a in np.asarray(model.part_qposadr, dtype=np.int64):
            qpos[:, a:a + 3] += FAR
        qpos = qpos.astype(np.float32).astype(np.float64)
    return qpos, qvel


def arm_link(model):
    """the name of an arm link in the middle of the (first) arm: the body of the arm's fourth dof; None for the Cursor agent"""
    robot = mom.robot_sensor(model)
    if robot is None:
        return None
    return model.meta["body_names"][robot.bodies[3]]


def sensor_sets(model):
    """[MomentumSensor]: every part, the robot, an arm link with its subtree, all parts together, a robot link with a part (the last two
    without the robot for the Cursor agent, where a set of two parts takes the mixed one's place)"""
    parts = list(model.meta["part_names"])
    sensors = mom.part_sensors(model)
    link = arm_link(model)
    if link is not None:
        sensors += [mom.robot_sensor(model), mom.MomentumSensor(link, subtree=True)]
    sensors.append(mom.all_parts_sensor(model))
    sensors.append(mom.MomentumSensor([link, parts[-1]], subtree=[True, False]) if link is not None else mom.MomentumSensor([parts[0], parts[-1]], subtree=False))
    return sensors


def model_bodies(model, sensor):
    """the model bodies of a sensor's set, ascending: the listed bodies, with subtree every model body below them, and with each of those
    every body of the same compiled body (a folded body stands for the compiled body with everything folded into it)"""
    A = model.arrays
    names = model.meta["body_names"]
    parent = np.asarray(A["body_parentid"]).astype(np.int64)
    red = np.asarray(A["body_red"]).astype(np.int64)
    picked = set()
    for b, sub in zip(sensor.bodies, sensor.subtree):
        b = names.index(b) if isinstance(b, str) else int(b)
        picked.add(b)
        if sub:
            for d in range(b + 1, len(parent)):
                chain = d
                while chain > b:
                    chain = int(parent[chain])
                if chain == b:
                    picked.add(d)
    compiled = set(int(red[b]) for b in picked)
    assert 0 not in compiled and -1 not in compiled
    return [b for b in range(1, len(red)) if int(red[b]) in compiled]


def set_masses(model, sensors):
    """[S] float64: the mass of every set, from the unreduced body_mass"""
    mass = np.asarray(model.arrays["body_mass"], dtype=np.float64)
    return np.array([mass[model_bodies(model, s)].sum() for s in sensors])


def body_terms(osim, model):
    """per MODEL body at the oracle's current state: x [nb, 3] inertial origins, R [nb, 3, 3] the inertial frames, jp, jr [nb, 3, nv] the
    Jacobians of the inertial origin and of the orientation, m [nb], I [nb, 3] the principal inertias"""
    A = model.arrays
    nb = model.nbody
    mass, inertia = np.asarray(A["body_mass"], dtype=np.float64), np.asarray(A["body_inertia"], dtype=np.float64).reshape(-1, 3)
    iquat = np.asarray(A["body_iquat"], dtype=np.float64).reshape(-1, 4)
    x = np.array(osim.data.xipos, dtype=np.float64).reshape(nb, 3)
    R = np.stack([np.asarray(osim.data.xmat[b], dtype=np.float64).reshape(3, 3) @ dref.q2m(iquat[b]) for b in range(nb)])
    jp, jr = np.zeros((nb, 3, model.nv)), np.zeros((nb, 3, model.nv))
    for b in range(1, nb):
        jp[b], jr[b] = osim.body_jac(b, x[b])
    return dict(x=x, R=R, jp=jp, jr=jr, m=mass, I=inertia)


def moving(model):
    """the model bodies that move: those of a compiled body other than the world"""
    return np.nonzero(np.asarray(model.arrays["body_red"]).astype(np.int64) > 0)[0]


def gravity(model):
    return np.asarray(model.arrays["opt"], dtype=np.float64)[1:4]


def formulas(model, sensors, T, qvel, dtype=np.float64, about="ref"):
    """The header's formulas on the body terms T in the arithmetic of ``dtype``.  about="ref": positions relative to the inertial origin
    of the set's lowest-numbered body, angmom from (x_b - c) and (v_b - v_c); about="origin": sums about the world origin, angmom as the
    moment about the origin minus that of the centre of mass."""
    f = dtype
    x, R, jp, jr, m, I = (np.asarray(T[k], dtype=f) for k in ("x", "R", "jp", "jr", "m", "I"))
    qv = np.asarray(qvel, dtype=f)
    v, w = jp @ qv, jr @ qv  # [nb, 3]
    h = np.einsum("bij,bj->bi", R, I * np.einsum("bji,bj->bi", R, w))  # R (I (R^T w)): the product in the body frame, then turned
    S = len(sensors)
    out = dict(com=np.zeros((S, 3), f), linvel=np.zeros((S, 3), f), angmom=np.zeros((S, 3), f), jac=np.zeros((S, 3, model.nv), f))
    for i, s in enumerate(sensors):
        B = model_bodies(model, s)
        M = f(0)
        for b in B:
            M = M + m[b]
        x0 = x[B[0]] if about == "ref" else np.zeros(3, f)
        sx, sv, sj = np.zeros(3, f), np.zeros(3, f), np.zeros((3, model.nv), f)
        for b in B:
            sx = sx + m[b] * (x[b] - x0)
            sv = sv + m[b] * v[b]
            sj = sj + m[b] * jp[b]
        c, vc = sx / M, sv / M
        L = np.zeros(3, f)
        if about == "ref":
            for b in B:
                L = L + (h[b] + m[b] * np.cross((x[b] - x0) - c, v[b] - vc))
        else:
            for b in B:
                L = L + (h[b] + m[b] * np.cross(x[b], v[b]))
            L = L - M * np.cross(c, vc)
        out["com"][i], out["linvel"][i], out["angmom"][i], out["jac"][i] = x0 + c, vc, L, sj / M
    g = gravity(model).astype(f)
    pot, kin = f(0), f(0)
    for b in moving(model):
        pot = pot - m[b] * (g @ x[b])
        kin = kin + f(0.5) * (m[b] * (v[b] @ v[b]) + w[b] @ h[b])
    arm = np.asarray(model.arrays["dof_armature"], dtype=f)
    for d in range(model.nv):
        kin = kin + f(0.5) * arm[d] * qv[d] * qv[d]
    out["energy"] = np.array([pot, kin], dtype=f)
    return out


def evaluate(osim, model, sensors, qpos, qvel, cursor=None):
    """dict of com, linvel, angmom [S, 3], jac [S, 3, nv], energy [2] at (qpos, qvel), float64; the oracle is left at (qpos, qvel)"""
    qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    set_state(osim, model, qpos, qvel, cursor)
    return formulas(model, sensors, body_terms(osim, model), qvel)


def centres(osim, model, sensors, qpos):
    """com [S, 3] and the potential energy at qpos alone (for finite differences): from data.xipos and body_mass"""
    set_state(osim, model, np.asarray(qpos, dtype=np.float64), np.zeros(model.nv))
    m = np.asarray(model.arrays["body_mass"], dtype=np.float64)
    x = np.array(osim.data.xipos, dtype=np.float64).reshape(model.nbody, 3)
    com = np.array([(m[B][:, None] * x[B]).sum(axis=0) / m[B].sum() for B in (model_bodies(model, s) for s in sensors)]).reshape(-1, 3)
    mv = moving(model)
    return com, -float((m[mv][:, None] * x[mv] * gravity(model)[None, :]).sum())


def evaluate_f32(osim, model, sensors, qpos, qvel, about):
    """the same formulas in float32 on float32-rounded body terms: what fp32 alone does"""
    qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    set_state(osim, model, qpos, qvel)
    return formulas(model, sensors, body_terms(osim, model), qvel, dtype=np.float32, about=about)


def measures(ref, got):
    """The error measures of one env: for every key of ``got`` (com, linvel, angmom, jac, energy) the largest absolute error over the env's
    sensors divided by the largest reference magnitude of that quantity in the env (the convention of dynamics_reference.measures)."""
    return {k: np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-300) for k in got}

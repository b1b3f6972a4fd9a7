"""Reference for the device's force-torque, accelerometer and joint-load sensors (include/fsim_wrench.h), in float64.

From an OracleSim at a state, after forward() with the solver at 1e-14 (contacts_reference.set_state): a plain recursive Newton-Euler pass
on the UNFOLDED model -- every model body, jointed or not -- with the oracle's qacc, qvel, xpos / xmat / xipos and the model's masses,
inertias and joint tables: angular velocity and acceleration and the classical acceleration of every body's centre of mass down the tree
(kinematics), then per body the inertial wrench m (a_c - g), I alpha + w x I w about its centre of mass (inertial), and sums over the bodies
below a cut about any origin (subtree_wrench).  The oracle's own cvel / cacc are not used: the pass stands on positions and joint tables
alone, and tests/test_wrench.py holds it to facts it did not use (the joint-axis identity against M qacc + bias, Newton's law of the free
parts, the accelerations by finite difference of the positions).

oracle/ exposes no per-contact or weld force, so the external part of a wrench comes from the device's own contact list through
fsim_contact_forces, as contacts_reference.project takes it: external_rows turns con_geoms / con_pos / con_force into (body, point, force)
rows, and evaluate() subtracts those that cross the cut.  That pins force and torque wherever the subtree below the cut has no weld to a
body outside it.  One kind of cut needs no row at all: the six dofs of a FREE joint span the wrench, so for a sensor on a free body the
oracle's qfrc_constraint on those dofs is the external part, contacts and welds alike, and evaluate() takes it from there.

The measure (wrench_measure) is per sensor, as the issue sets it: the largest error of the sensor's vector over the largest |component| of
that sensor's own reference reading, and the error itself, in N or N m, where that reading is a zero (a free part).  On the CPU the
reference reading of a robot sensor has no contact part (the oracle gives none, and the joint's one dof does not span six): the floors
below are therefore over the sensor's own inertial part, which is its whole reading wherever nothing touches the bodies below the cut.
"""

import numpy as np

from tests.contacts_reference import f32, set_state  # noqa: F401  (set_state: the states are written as the contact tests write them)

# What fp32 alone does to the measures of tests/test_wrench_gpu.py: qacc of the checker's float32 build (oracle/libfsim_cpu32.so through
# the C-ABI) pushed through this reference against the oracle's own qacc, force and torque of the wrist sensor, of a sensor on every moving
# robot body and of the part sensors; the largest over the states of tests/test_wrench.py (test_what_fp32_alone_does prints and checks
# them), rounded up in the last digit.  WRENCH_FLOOR, each sensor over its own reading: 5.011e-2 in env 4 of the sweep scene of
# desk_mikael_1064 (table_lack_0825: 5.1e-3; moving 6.0e-3 and 9.7e-3; lifted 1.6e-3; at rest and welded below 1e-4).  WRIST_FLOOR, the
# wrist sensor(s) alone: 3.427e-3 in the same scene (table_lack_0825 3.2e-3, lifted 1.6e-3, elsewhere below 1e-5).  WRENCH_FLOOR_ABS,
# the parts, whose reading is a zero, in N or N m: 1.074 in that scene (table_lack_0825 0.15; elsewhere below 1e-5) -- m (a - g) minus
# the constraint force, with a float32 qacc of a part that sits centimetres deep in another.  QACC_FLOOR, qacc itself by qacc_measure:
# 5.31752e-3 in env 7 of the sweep scene of table_lack_0825 (desk_mikael_1064: 7.8e-4; at rest 1.3e-5 and 5.5e-5; welded 4.9e-4).
WRENCH_FLOOR = 5.012e-2
WRIST_FLOOR = 3.428e-3
WRENCH_FLOOR_ABS = 1.075
QACC_FLOOR = 5.3176e-3
JT_FREE, JT_SLIDE, JT_HINGE = 0, 2, 3


def _q2m(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def kinematics(osim, m, qacc=None):
    """dict of [nbody, 3] arrays at the oracle's current state: w, alpha (angular velocity, acceleration), v, a (velocity and classical
    acceleration of the body ORIGIN), xpos, xmat [nbody, 3, 3]; qacc: the oracle's unless given"""
    A, d = m.arrays, osim.data
    nb = m.nbody
    parent = np.asarray(A["body_parentid"], dtype=np.int64)
    jadr, jnum = np.asarray(A["body_jntadr"], dtype=np.int64), np.asarray(A["body_jntnum"], dtype=np.int64)
    jtype, jax, jpos = np.asarray(A["jnt_type"]), np.asarray(A["jnt_axis"], dtype=np.float64).reshape(-1, 3), np.asarray(A["jnt_pos"], dtype=np.float64).reshape(-1, 3)
    jdof = np.asarray(A["jnt_dofadr"], dtype=np.int64)
    qvel = np.array(d.qvel, dtype=np.float64)
    qacc = np.array(d.qacc if qacc is None else qacc, dtype=np.float64)
    xpos, xmat = np.array(d.xpos, dtype=np.float64), np.array(d.xmat, dtype=np.float64).reshape(nb, 3, 3)
    w, al, v, a = (np.zeros((nb, 3)) for _ in range(4))
    for b in range(1, nb):
        p = int(parent[b])
        assert p < b and jnum[b] <= 1, "bodies in tree order with at most one joint each"
        if jnum[b] == 0 or jtype[jadr[b]] == JT_SLIDE:
            r = xpos[b] - xpos[p]
            w[b], al[b] = w[p], al[p]
            v[b] = v[p] + np.cross(w[p], r)
            a[b] = a[p] + np.cross(al[p], r) + np.cross(w[p], np.cross(w[p], r))
            if jnum[b]:
                j = int(jadr[b])
                ax = xmat[b] @ jax[j]
                v[b] += ax * qvel[jdof[j]]
                a[b] += ax * qacc[jdof[j]] + 2.0 * np.cross(w[p], ax) * qvel[jdof[j]]
            continue
        j = int(jadr[b])
        k = int(jdof[j])
        if jtype[j] == JT_FREE:
            assert p == 0
            v[b], a[b] = qvel[k:k + 3], qacc[k:k + 3]
            w[b], al[b] = xmat[b] @ qvel[k + 3:k + 6], xmat[b] @ qacc[k + 3:k + 6]
            continue
        assert jtype[j] == JT_HINGE
        ax, anchor = xmat[b] @ jax[j], xpos[b] + xmat[b] @ jpos[j]
        r = anchor - xpos[p]
        va = v[p] + np.cross(w[p], r)
        aa = a[p] + np.cross(al[p], r) + np.cross(w[p], np.cross(w[p], r))
        w[b] = w[p] + ax * qvel[k]
        al[b] = al[p] + ax * qacc[k] + np.cross(w[p], ax) * qvel[k]
        r = xpos[b] - anchor
        v[b] = va + np.cross(w[b], r)
        a[b] = aa + np.cross(al[b], r) + np.cross(w[b], np.cross(w[b], r))
    return dict(w=w, alpha=al, v=v, a=a, xpos=xpos, xmat=xmat)


def point_motion(kin, body, point):
    """(velocity, classical acceleration) of the material point of ``body`` now at the world position ``point``"""
    r = np.asarray(point, dtype=np.float64) - kin["xpos"][body]
    w, al = kin["w"][body], kin["alpha"][body]
    return kin["v"][body] + np.cross(w, r), kin["a"][body] + np.cross(al, r) + np.cross(w, np.cross(w, r))


def inertial(osim, m, kin):
    """per model body: F [nbody, 3] = m (a_c - g), N [nbody, 3] = I alpha + w x I w about the body's centre of mass c [nbody, 3]"""
    A = m.arrays
    nb = m.nbody
    mass = np.asarray(A["body_mass"], dtype=np.float64)
    inertia = np.asarray(A["body_inertia"], dtype=np.float64).reshape(nb, 3)
    iquat = np.asarray(A["body_iquat"], dtype=np.float64).reshape(nb, 4)
    g = np.asarray(A["gravity"], dtype=np.float64).reshape(3)
    c = np.array(osim.data.xipos, dtype=np.float64)
    F, N = np.zeros((nb, 3)), np.zeros((nb, 3))
    for b in range(1, nb):
        _, ac = point_motion(kin, b, c[b])
        Ri = kin["xmat"][b] @ _q2m(iquat[b] / np.linalg.norm(iquat[b]))
        Iw = Ri @ np.diag(inertia[b]) @ Ri.T
        F[b] = mass[b] * (ac - g)
        N[b] = Iw @ kin["alpha"][b] + np.cross(kin["w"][b], Iw @ kin["w"][b])
    return dict(F=F, N=N, c=c)


def cut_of(m, body):
    """(model body id of the cut: the body itself or the moving ancestor it is folded into, [nbody] bool: the bodies below the cut)"""
    A = m.arrays
    parent = np.asarray(A["body_parentid"], dtype=np.int64)
    jnum = np.asarray(A["body_jntnum"], dtype=np.int64)
    cut = int(body)
    while cut > 0 and jnum[cut] == 0:
        cut = int(parent[cut])
    assert cut > 0, "a body fixed in the world"
    below = np.zeros(m.nbody, dtype=bool)
    below[cut] = True
    for b in range(cut + 1, m.nbody):
        below[b] = below[parent[b]]
    return cut, below


def subtree_wrench(ine, below, origin):
    """(force, torque about origin), world frame: the inertial wrench summed over the bodies below the cut"""
    origin = np.asarray(origin, dtype=np.float64)
    F = ine["F"][below].sum(0)
    T = (ine["N"][below] + np.cross(ine["c"][below] - origin, ine["F"][below])).sum(0)
    return F, T


def external_rows(m, con_geoms, con_pos, con_force):
    """[(model body, point, force)] of a contact list as fsim_contact_forces gives it: +force on geom 2's body, -force on geom 1's"""
    gb = np.asarray(m.arrays["geom_bodyid"], dtype=np.int64)
    rows = []
    for (g1, g2), p, F in zip(np.asarray(con_geoms), np.asarray(con_pos, dtype=np.float64), np.asarray(con_force, dtype=np.float64)):
        if g1 < 0:
            continue
        rows += [(int(gb[g2]), p, F), (int(gb[g1]), p, -F)]
    return rows


def external_wrench(rows, on, origin):
    """(force, torque about origin) of the rows acting on the bodies ``on`` ([nbody] bool)"""
    origin = np.asarray(origin, dtype=np.float64)
    F, T = np.zeros(3), np.zeros(3)
    for b, p, f in rows:
        if on[b]:
            F += f
            T += np.cross(p - origin, f)
    return F, T


def sensor_frame(osim, m, sensor):
    """(model body, origin [3], R [3, 3] sensor -> world) of a furniture_amd.wrench.WrenchSensor at the oracle's current state"""
    body, pos, quat = sensor.resolve(m)
    R = np.array(osim.data.xmat, dtype=np.float64).reshape(-1, 3, 3)[body]
    return body, np.array(osim.data.xpos, dtype=np.float64)[body] + R @ pos, R @ _q2m(quat)


def evaluate(osim, m, sensors, rows=(), qacc=None):
    """dict of [S, 3] arrays at the oracle's current state (after forward()): force, torque, accel, angacc in the sensor frame, the
    world-frame inertial parts iforce / itorque (torque about the sensor origin) the measure is scaled by, and the frames"""
    kin = kinematics(osim, m, qacc)
    ine = inertial(osim, m, kin)
    g = np.asarray(m.arrays["gravity"], dtype=np.float64).reshape(3)
    out = {k: np.zeros((len(sensors), 3)) for k in ("force", "torque", "accel", "angacc", "iforce", "itorque", "origin")}
    out["R"] = np.zeros((len(sensors), 3, 3))
    A = m.arrays
    jadr, jtype, jdof = np.asarray(A["body_jntadr"], dtype=np.int64), np.asarray(A["jnt_type"]), np.asarray(A["jnt_dofadr"], dtype=np.int64)
    qc = np.array(osim.data.qfrc_constraint, dtype=np.float64)
    for i, s in enumerate(sensors):
        body, org, R = sensor_frame(osim, m, s)
        cut, below = cut_of(m, body)
        F, T = subtree_wrench(ine, below, org)
        if jtype[jadr[cut]] == JT_FREE:
            # the six dofs of a free joint span the wrench, so here -- and only here -- the oracle's qfrc_constraint IS the external part
            # below the cut (contacts and welds alike): the world force on the translational dofs, the body-frame torque about the body
            # origin on the rotational ones.  No row of the device's is used.
            d = int(jdof[jadr[cut]])
            Fe = qc[d:d + 3]
            Te = kin["xmat"][cut] @ qc[d + 3:d + 6] - np.cross(org - kin["xpos"][cut], Fe)
        else:
            Fe, Te = external_wrench(rows, below, org)
        _, a = point_motion(kin, body, org)
        out["iforce"][i], out["itorque"][i], out["origin"][i], out["R"][i] = F, T, org, R
        out["force"][i], out["torque"][i] = R.T @ (F - Fe), R.T @ (T - Te)
        out["accel"][i], out["angacc"][i] = R.T @ (a - g), R.T @ kin["alpha"][body]
    return out


ZERO = 1e-9  # a reference reading below this share of its own inertial part is a zero: what float64 leaves of a sum that cancels


def wrench_measure(got, ref, iref):
    """(relative, absolute, per-sensor [S]) of [S, 3] vectors, sensor by sensor: the largest error of the sensor's vector over the
    largest |component| of the sensor's own reference reading; where that reading is a zero -- a body on a free joint, through which
    nothing passes: the reference's own value is its inertial part cancelling against the constraint forces to 1e-12 -- the error
    itself, in newtons or newton metres.  relative / absolute: the largest over the sensors of each kind (0.0 where there is none);
    per-sensor: each sensor's own figure, of whichever kind."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max(axis=1)
    scale, iscale = np.abs(ref).max(axis=1), np.abs(iref).max(axis=1)
    zero = scale <= ZERO * np.maximum(iscale, 1.0)  # (1.0: a part in free fall has no inertial part either)
    per = np.where(zero, err, err / np.where(zero, 1.0, scale))
    return (per[~zero].max() if (~zero).any() else 0.0), (per[zero].max() if zero.any() else 0.0), per


def qacc_measure(got, ref, m):
    """the largest absolute error of qacc over the env's largest |qacc|, or over |g| where that is larger: a scene at rest has
    accelerations of 1e-4, and what an error there is to be compared with is the 9.81 the contacts hold up"""
    g = np.linalg.norm(np.asarray(m.arrays["gravity"], dtype=np.float64))
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), g)


def robot_sensors(m):
    """the wrist sensor(s), then one sensor at the body frame of every robot body with a joint of its own"""
    from furniture_amd.frames import Frame
    from furniture_amd.wrench import WrenchSensor, wrist_sensor
    A = m.arrays
    names = m.meta["body_names"]
    partid = np.asarray(A["body_partid"])
    jointed = [b for b in range(1, m.nbody) if np.asarray(A["body_jntnum"])[b] > 0 and partid[b] < 0]
    return wrist_sensor(m) + [WrenchSensor(Frame(body=names[b])) for b in jointed]


MOVING_MODELS = (("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"))
N_MOVING, N_WELD, WELD_STEPS = 4, 4, 20


def moving_states(agent, furniture, n=N_MOVING, pool=16):
    """n envs of dynamics_reference.random_states -- every part turned by a random unit quaternion, every joint uniform within its limits,
    qvel uniform(-1, 1) -- with the parts lifted and spaced apart as contacts_reference.lifted_state places them: the velocity-product
    terms are the whole signal.  A random arm pose may touch itself or the floor, so the envs are the first n of a pool of 16 in which
    the oracle lists no contact at all (decided by the oracle alone)."""
    from oracle.oracle_sim import OracleSim
    from tests.contacts_reference import lifted_state
    from tests.dynamics_reference import random_states
    m, st = lifted_state(agent, furniture, pool)
    qpos, qvel = random_states(m, pool)
    for a in np.asarray(m.part_qposadr, dtype=np.int64):
        qpos[:, a:a + 3] = st["qpos"][:, a:a + 3]
    st["qpos"], st["qvel"] = f32(qpos), f32(qvel)
    osim = OracleSim(m)
    keep = []
    for e in range(pool):
        set_state(osim, m, st, e)
        if osim.ncon == 0 and len(keep) < n:
            keep.append(e)
    osim.close()
    assert len(keep) == n, "the pool holds %d envs without a contact" % len(keep)
    return m, {k: (v[keep] if v is not None else None) for k, v in st.items()}

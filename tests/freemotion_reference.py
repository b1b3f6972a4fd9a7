"""The free-motion dynamics and the integrator of the step kernels against float64: what runs before the Newton solve (fs_kinematics,
fs_com_inertia, fs_crb_factor, fs_velocity_bias, fs_smooth of csrc/fsim_physics.hpp) and after it (the unconstrained exit of fs_solve and
fs_integrate_body of csrc/fsim_solver.hpp).  The states, the float64 reference of one forward pass, of one substep and of 100 substeps, a
numpy restatement of the free-motion step that shares no code with the oracle or the device, the measures, and what fp32 alone does to them.
Shared by tests/test_freemotion.py (CPU) and tests/test_freemotion_gpu.py (the device).  Pure numpy + oracle/.

Every state switches every geom off (geom_contype = geom_conaffinity = 0, state on both sides) and no weld is active: no contact, no
constraint row, so qacc is the smooth acceleration and one substep is the damped integrator alone.  N = 8 envs per model, float32 values
held in float64 arrays, from the recipe of tests/test_frames_gpu.py::_random_states with every limited joint at least JOINT_INSET inside
its range (no limit row sits on a threshold):

  env  families                        what it sets
  0    rest                            qvel = 0
  1    fast (tumble)                   parts: |w| in [10, 30] rad/s, |v| in [1, 5] m/s; arm and gripper dofs uniform(-3, 3)
  2    fast, far (tumble)              the same with every part 8 m from the origin
  3    unnormalised, wrench            part quaternions scaled by factors in [0.5, 2]; xfrc_applied alone, a force of 2 N square to the part's centre-of-mass offset
                                       (beside qfrc_applied of 5 on every dof, the moment of that force about the centre of mass would not show)
  4    still-spin                      part 0 with w exactly 0, part 1 with |w| = 1e-18
  5    ctrl                            ctrl below, inside and above actuator_ctrlrange; gripper ctrl so that the force is clamped low, high, not at all
  6    applied                         qfrc_applied uniform(-5, 5) on every dof; xfrc_applied (|F| <= 2 N, |T| <= 0.2 N m) on every other part, a lone z torque on one
  7    ctrl, applied, unnormalised     all three at once

The measures, per env (measures()):
  pose      the larger of max |xpos error| / max(1, max |xpos|) and the largest xquat error with the sign taken out
  bias      max |qfrc_bias error| / max |qfrc_bias|
  force     |M64 qacc - f_smooth64| per dof over the largest |f_smooth64| of the dof's tree (a gripper finger accelerates at 1.6e4: a raw qacc measure sees nothing else)
  acc       |qacc error| per dof over the largest |qacc64| of the dof's tree
            (a tree that nothing drives -- Baxter's head, 1e-16 N m -- is judged against gravity: the scale of an acceleration is at least |g|, that of a force at
            least |g| times the tree's largest diagonal entry of M; a free part at rest has exactly these)
  actuator  the actuator force the output implies, M64 qacc + bias64 + D v - applied64, against qfrc_actuator on the actuated dofs, over max |qfrc_actuator|
  step      (qvel' - qvel) / h against the oracle's, per dof over the largest of the dof's tree
  move      (qpos' - qpos) / h on scalar and translation entries over max(1, |v'|); for a free joint the angle between the new orientations over h max(1, |w'|)
  tumble_pos / tumble_ang / tumble_norm   after 100 substeps from the fast envs: part position error (m), orientation angle (rad), ||q| - 1|
"""
import ctypes

import numpy as np

MODELS = {
    "lack": ("Sawyer", "table_lack_0825", "impedance"),
    "lack_torque": ("Sawyer", "table_lack_0825", "torque"),
    "billy": ("Sawyer", "bookcase_billy_0191", "impedance"),  # nv = 75: the second row pass of the kernels with two and eight slot sets
    "desk": ("Baxter", "desk_mikael_1064", "impedance"),
    "toy": ("Cursor", "toy_table", "impedance"),
    "liden": ("Baxter", "table_liden_0921", "impedance"),  # nv = 91, a reduced body on bit 31 of the masks
}
N, SEED = 8, 33
JOINT_INSET = 1e-3
FAMILY = {"rest": (0,), "fast": (1, 2), "far": (2,), "unnormalised": (3, 7), "wrench": (3,), "still-spin": (4,), "ctrl": (5, 7), "applied": (6, 7)}
GROUPS = ("near", "far")  # FLOOR and the device's tolerances are kept apart for the envs 8 m out: there fp32 loses 100 x more, and one bound for all would be theirs
TUMBLE_ENVS, TUMBLE_STEPS = (1, 2), 100
FAR = 8.0
FIELDS = ("qpos", "qvel", "ctrl", "qfrc_applied", "xfrc_applied", "eq_active", "geom_contype", "geom_conaffinity", "qacc_warmstart", "cursor")
MEASURES = ("pose", "bias", "force", "acc", "actuator", "step", "move")
TUMBLE = ("tumble_pos", "tumble_ang", "tumble_norm")
# The oracle against the restatement, relative; the closed forms
RESTATE_TOL, CLOSED_TOL = 1e-10, 1e-10
# A deliberate defect of the restatement must exceed this many fp32 floors in some measure on some env (tests/test_freemotion.py)
CAN_TELL = 100.0
# What fp32 alone does, per model: the measures of the checker's float32 build (oracle/libfsim_cpu32.so through the C-ABI: one
# fsim_physics_forward, one fsim_physics_step, 100 more for the tumble) against the float64 reference on the same states, the largest over
# envs of each group (the one env 8 m out apart from the others); tests/test_freemotion.py::test_what_fp32_alone_does prints them and checks
# that they still hold.  Rounded up in the last digit.  The checker works about the world origin, so 8 m out its float32 build loses far more than
# the device, which works about each tree's centre of mass.
FLOOR = {
    "lack": dict(
        near=dict(pose=2.424e-07, bias=1.022e-06, force=1.625e-04, acc=2.216e-04, actuator=1.084e-05, step=1.024e-04, move=2.876e-04, tumble_pos=3.166e-07, tumble_ang=3.185e-06, tumble_norm=5.695e-08),
        far=dict(pose=1.274e-07, bias=3.494e-06, force=2.140e-03, acc=2.573e-02, actuator=1.404e-05, step=1.507e-02, move=3.374e-03, tumble_pos=2.282e-06, tumble_ang=3.962e-04, tumble_norm=6.395e-08),
    ),
    "lack_torque": dict(
        near=dict(pose=2.424e-07, bias=1.022e-06, force=1.625e-04, acc=2.216e-04, actuator=8.841e-06, step=1.024e-04, move=2.876e-04, tumble_pos=3.166e-07, tumble_ang=3.201e-06, tumble_norm=5.695e-08),
        far=dict(pose=1.274e-07, bias=3.494e-06, force=2.140e-03, acc=2.573e-02, actuator=1.372e-05, step=1.507e-02, move=3.374e-03, tumble_pos=2.282e-06, tumble_ang=3.962e-04, tumble_norm=6.395e-08),
    ),
    "billy": dict(
        near=dict(pose=2.047e-07, bias=9.997e-07, force=9.073e-05, acc=2.945e-04, actuator=3.614e-05, step=2.308e-04, move=1.503e-04, tumble_pos=1.721e-06, tumble_ang=9.367e-06, tumble_norm=8.419e-08),
        far=dict(pose=1.188e-07, bias=2.651e-06, force=1.280e-04, acc=1.633e-02, actuator=3.829e-06, step=1.362e-02, move=8.003e-04, tumble_pos=3.695e-06, tumble_ang=3.083e-03, tumble_norm=8.718e-08),
    ),
    "desk": dict(
        near=dict(pose=2.732e-07, bias=4.462e-07, force=8.119e-06, acc=2.340e-05, actuator=7.086e-06, step=2.339e-05, move=6.440e-05, tumble_pos=8.648e-07, tumble_ang=2.024e-05, tumble_norm=3.027e-08),
        far=dict(pose=1.373e-07, bias=9.278e-06, force=1.427e-04, acc=1.991e-02, actuator=2.949e-06, step=1.976e-02, move=2.330e-04, tumble_pos=1.342e-05, tumble_ang=1.286e-03, tumble_norm=4.010e-08),
    ),
    "toy": dict(
        near=dict(pose=6.795e-08, bias=5.853e-07, force=1.462e-04, acc=2.809e-04, step=2.715e-04, move=1.357e-04, tumble_pos=2.293e-07, tumble_ang=8.587e-06, tumble_norm=5.130e-08),
        far=dict(pose=1.625e-08, bias=2.850e-04, force=1.859e-03, acc=3.281e-01, step=3.146e-01, move=6.429e-03, tumble_pos=1.089e-06, tumble_ang=4.151e-03, tumble_norm=5.473e-08),
    ),
    "liden": dict(
        near=dict(pose=1.745e-07, bias=4.680e-07, force=2.927e-04, acc=2.208e-04, actuator=1.072e-05, step=1.363e-04, move=4.814e-04, tumble_pos=2.059e-07, tumble_ang=4.222e-06, tumble_norm=7.892e-08),
        far=dict(pose=1.904e-07, bias=2.492e-06, force=2.395e-03, acc=9.801e-02, actuator=2.506e-06, step=5.227e-02, move=1.308e-02, tumble_pos=4.656e-06, tumble_ang=1.129e-03, tumble_norm=8.998e-08),
    ),
}

_models = {}
JT_FREE, JT_SLIDE, JT_HINGE = 0, 2, 3


def model(name):
    from furniture_amd.mjcf.model import load_compiled
    if name not in _models:
        _models[name] = load_compiled(*MODELS[name])
    return _models[name]


def group(e):
    return "far" if e in FAMILY["far"] else "near"


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _unit(rng, k=3):
    u = rng.normal(size=k)
    return u / np.linalg.norm(u)


# ---- the states ----------------------------------------------------------------------------------------------------------------------------
def states(name, seed=SEED):
    """dict of [N, .] arrays (FIELDS; float64 holding float32 values, int32 for the switches; cursor None unless the Cursor agent)"""
    m = model(name)
    A, rng = m.arrays, np.random.RandomState(seed)
    pq, pd = np.asarray(m.part_qposadr, dtype=np.int64), np.asarray(m.part_dofadr, dtype=np.int64)
    robot = np.setdiff1d(np.arange(m.nv), (pd[:, None] + np.arange(6)[None, :]).reshape(-1))
    jt, jq = np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"], dtype=np.int64)
    lim, rg = np.asarray(A["jnt_limited"]).astype(bool), np.asarray(A["jnt_range"], dtype=np.float64).reshape(-1, 2)
    qpos = np.tile(np.asarray(A["qpos0"], dtype=np.float64), (N, 1))
    for e in range(N):
        for a in pq:
            qpos[e, a:a + 3] += rng.uniform(-0.2, 0.2, 3)
            qpos[e, a + 3:a + 7] = _unit(rng, 4)
        for j in range(len(jt)):
            if jt[j] != JT_FREE:
                qpos[e, jq[j]] = rng.uniform(rg[j, 0] + JOINT_INSET, rg[j, 1] - JOINT_INSET) if lim[j] else rng.uniform(-1.0, 1.0)
    qvel = rng.uniform(-1.0, 1.0, (N, m.nv))
    ctrl, qfrc, xfrc = np.zeros((N, m.nu)), np.zeros((N, m.nv)), np.zeros((N, 6 * m.nparts))
    qvel[FAMILY["rest"][0]] = 0.0
    for e in FAMILY["fast"]:
        for d in pd:
            qvel[e, d:d + 3] = _unit(rng) * rng.uniform(1.0, 5.0)
            qvel[e, d + 3:d + 6] = _unit(rng) * rng.uniform(10.0, 30.0)
        qvel[e, robot] = rng.uniform(-3.0, 3.0, len(robot))
    for e in FAMILY["far"]:
        for a in pq:
            u = _unit(rng)
            qpos[e, a:a + 3] = FAR * np.array([u[0], u[1], abs(u[2])])
    for e in FAMILY["unnormalised"]:
        for a in pq:
            qpos[e, a + 3:a + 7] *= rng.uniform(0.5, 2.0)
    e = FAMILY["still-spin"][0]
    qvel[e, pd[0] + 3:pd[0] + 6] = 0.0
    qvel[e, pd[1] + 3:pd[1] + 6] = (0.0, 1e-18, 0.0)
    if m.nu:
        aj = np.asarray(A["actuator_jntid"], dtype=np.int64)
        cr, fl = np.asarray(A["actuator_ctrlrange"], dtype=np.float64).reshape(-1, 2), np.asarray(A["actuator_forcelimited"]).astype(bool)
        gain, fr = np.asarray(A["actuator_gain"], dtype=np.float64), np.asarray(A["actuator_forcerange"], dtype=np.float64).reshape(-1, 2)
        for e in FAMILY["ctrl"]:
            for u in range(m.nu):
                k, lo, hi = (u + e) % 3, cr[u, 0], cr[u, 1]
                if fl[u]:  # a position servo with a force clamp: the joint in the middle of its range, ctrl 2.5 / 2.5 / 0.5 force ranges away
                    q = 0.5 * (rg[aj[u], 0] + rg[aj[u], 1]) + rng.uniform(-2e-3, 2e-3)
                    qpos[e, jq[aj[u]]] = q
                    ctrl[e, u] = q + (2.5 * fr[u, 0], 2.5 * fr[u, 1], 0.5 * fr[u, 1 - u % 2])[k] / gain[u]
                else:
                    ctrl[e, u] = (lo - rng.uniform(0.1, 0.5) * (hi - lo), hi + rng.uniform(0.1, 0.5) * (hi - lo), rng.uniform(lo, hi))[k]
    for e in FAMILY["applied"]:
        qfrc[e] = rng.uniform(-5.0, 5.0, m.nv)
        for i in range(m.nparts):
            if (i + e) % 2 == 0:  # (exactly zero on the other parts: the non-zero test of fs_smooth)
                xfrc[e, 6 * i:6 * i + 3] = _unit(rng) * rng.uniform(0.5, 2.0)
                xfrc[e, 6 * i + 3:6 * i + 6] = _unit(rng) * rng.uniform(0.05, 0.2)
        i = [i for i in range(m.nparts) if (i + e) % 2 == 0][-1]
        xfrc[e, 6 * i:6 * i + 6] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.15)  # a lone z torque
    ipos = np.asarray(A["body_ipos"], dtype=np.float64).reshape(-1, 3)[np.asarray(A["part_bodyid"], dtype=np.int64)]
    for e in FAMILY["wrench"]:
        for i in range(m.nparts):  # a world force square to the world direction of the part's centre-of-mass offset (any direction where that is zero)
            q = qpos[e, pq[i] + 3:pq[i] + 7]
            r = _rot(q) @ ipos[i]
            u = np.cross(r, _unit(rng)) if np.linalg.norm(r) > 0 else _unit(rng)
            xfrc[e, 6 * i:6 * i + 3] = 2.0 * u / np.linalg.norm(u)
    cursor = None
    if m.meta.get("agent") == "Cursor":  # [pos of cursor0, pos of cursor1, selection + 1]: the cursors where the model has them, nothing selected
        # (the device welds the cursor bodies to the world at the model's body_pos and lets the env's cursor move their geoms alone,
        #  csrc/fsim_collide.hpp: its xpos of a cursor body is the model's whatever the cursor, and the dynamics never see it)
        pos0 = np.asarray(A["body_pos"], dtype=np.float64).reshape(-1, 3)[np.asarray(A["cursor_bodyid"], dtype=np.int64)]
        cursor = np.tile(np.concatenate([pos0.reshape(-1), [0.0, 0.0]]), (N, 1))
    zi = lambda k: np.zeros((N, k), dtype=np.int32)
    return dict(qpos=f32(qpos), qvel=f32(qvel), ctrl=f32(ctrl), qfrc_applied=f32(qfrc), xfrc_applied=f32(xfrc), eq_active=zi(m.neq),
                geom_contype=zi(m.ngeom), geom_conaffinity=zi(m.ngeom), qacc_warmstart=np.zeros((N, m.nv)), cursor=None if cursor is None else f32(cursor))


def fields(st):
    """the fields of a state that a handle's set_state takes (those the model has)"""
    return {k: st[k] for k in FIELDS if st[k] is not None and st[k].shape[1] > 0}


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------
def put(osim, m, st, e):
    d, mo = osim.data, osim.model
    osim.reset()
    d.qpos[:], d.qvel[:], d.ctrl[:], d.qfrc_applied[:] = st["qpos"][e], st["qvel"][e], st["ctrl"][e], st["qfrc_applied"][e]
    d.qacc_warmstart[:] = 0.0
    d.xfrc_applied[:] = 0.0
    for i, b in enumerate(np.asarray(m.arrays["part_bodyid"], dtype=np.int64)):
        d.xfrc_applied[int(b)] = st["xfrc_applied"][e][6 * i:6 * i + 6]
    if m.neq:
        mo.eq_active[:] = st["eq_active"][e]
    mo.geom_contype[:], mo.geom_conaffinity[:] = st["geom_contype"][e], st["geom_conaffinity"][e]
    if st["cursor"] is not None:
        for k, b in enumerate(m.arrays["cursor_bodyid"]):
            mo.body_pos[int(b)] = st["cursor"][e][3 * k:3 * k + 3]
    osim.set_solver(100, 1e-10, "newton")


def reference(osim, m, st, e, tumble=None):
    """dict at env e.  Of one forward(): xpos, xquat, bias, qacc, actuator (qfrc_actuator), qpos_fwd (qpos with its quaternions normalised in
    place), M, f_smooth = M qacc_smooth, applied = the generalised force of qfrc_applied and xfrc_applied, ncon, nefc.  Of one step(): qvel1,
    qpos1.  Of TUMBLE_STEPS step()s (tumble: None = for the envs of TUMBLE_ENVS): qpos_tumble."""
    c = lambda a: np.array(a, dtype=np.float64)
    d = osim.data
    put(osim, m, st, e)
    osim.forward()
    M = osim.full_M()
    ref = dict(xpos=c(d.xpos), xquat=c(d.xquat), bias=c(d.qfrc_bias), qacc=c(d.qacc), actuator=c(d.qfrc_actuator), qpos_fwd=c(d.qpos), M=M,
               f_smooth=M @ c(d.qacc_smooth), passive=c(d.qfrc_passive), ncon=osim.ncon, nefc=osim.nefc, qvel=c(st["qvel"][e]), qpos=c(st["qpos"][e]))
    ref["applied"] = ref["f_smooth"] - ref["passive"] + ref["bias"] - ref["actuator"]
    put(osim, m, st, e)
    osim.step()
    ref["qvel1"], ref["qpos1"] = c(d.qvel), c(d.qpos)
    if (e in TUMBLE_ENVS) if tumble is None else tumble:
        for _ in range(TUMBLE_STEPS - 1):
            osim.step()
        ref["qpos_tumble"] = c(d.qpos)
    return ref


# ---- the restatement: numpy, rotation matrices, the mass matrix and the bias force as sums over bodies of J^T (.) ------------------------
DEFECTS = ("gyroscopic", "cc", "parallel_axis", "armature", "explicit_damping", "left_quaternion", "xfrc_arm", "ctrl_clamp", "force_clamp")


def _skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _rot(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    v = np.array([x, y, z])
    return np.eye(3) + 2.0 * w * _skew(v) + 2.0 * _skew(v) @ _skew(v)


def _rodrigues(axis, t):
    K = _skew(axis)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def _qmul(a, b):
    return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])


def _xm(v, s):
    """the spatial cross product of a motion v with a motion s, [angular, linear about the world origin]"""
    return np.concatenate([np.cross(v[:3], s[:3]), np.cross(v[:3], s[3:]) + np.cross(v[3:], s[:3])])


def _xf(v, f):
    """the spatial cross product of a motion v with a force f, [moment about the world origin, force]"""
    return np.concatenate([np.cross(v[:3], f[:3]) + np.cross(v[3:], f[3:]), np.cross(v[:3], f[3:])])


def restate(m, st, e, M=None, defect=None):
    """The free-motion step of env e in plain numpy float64: dict of bias, M (its own, the sum over bodies of J^T I J plus armature), actuator,
    qacc = solve(M, -D v - bias + applied + J^T xfrc + actuator), qvel1 = v + h solve(M + h D, M qacc), qpos1, qpos_fwd.  M: the mass matrix
    to solve with (tests pass the oracle's full_M(); None: its own).  defect: one of DEFECTS, put in on purpose."""
    assert defect is None or defect in DEFECTS
    A = m.arrays
    f = lambda k, *s: np.asarray(A[k], dtype=np.float64).reshape(*s) if s else np.asarray(A[k], dtype=np.float64)
    i_ = lambda k: np.asarray(A[k], dtype=np.int64)
    nb, nv = m.nbody, m.nv
    h, g = float(A["opt"][0]), np.asarray(A["opt"][1:4], dtype=np.float64)
    qpos, v = np.array(st["qpos"][e], dtype=np.float64), np.array(st["qvel"][e], dtype=np.float64)
    parent, jntnum, jntadr = i_("body_parentid"), i_("body_jntnum"), i_("body_jntadr")
    jt, jq, jd = i_("jnt_type"), i_("jnt_qposadr"), i_("jnt_dofadr")
    bpos, bquat = f("body_pos", -1, 3).copy(), f("body_quat", -1, 4)
    if st["cursor"] is not None:
        for k, b in enumerate(i_("cursor_bodyid")):
            bpos[b] = st["cursor"][e][3 * k:3 * k + 3]
    jpos, jaxis, qpos0 = f("jnt_pos", -1, 3), f("jnt_axis", -1, 3), f("qpos0")
    # kinematics, and the motion axis S of every dof with the bodies it moves
    X, R, S = np.zeros((nb, 3)), np.tile(np.eye(3), (nb, 1, 1)), np.zeros((nv, 6))
    chain = [np.zeros(0, dtype=np.int64) for _ in range(nb)]  # the dofs between the world and the body
    for b in range(1, nb):
        p = parent[b]
        own = []
        if jntnum[b] == 1 and jt[jntadr[b]] == JT_FREE:
            a, d = jq[jntadr[b]], jd[jntadr[b]]
            qpos[a + 3:a + 7] /= np.linalg.norm(qpos[a + 3:a + 7])
            X[b], R[b] = qpos[a:a + 3], _rot(qpos[a + 3:a + 7])
            for k in range(3):
                S[d + k, 3 + k] = 1.0
                S[d + 3 + k] = np.concatenate([R[b][:, k], np.cross(X[b], R[b][:, k])])
            own = list(range(d, d + 6))
        else:
            pos, Rb = X[p] + R[p] @ bpos[b], R[p] @ _rot(bquat[b])
            for j in range(jntadr[b], jntadr[b] + jntnum[b]):
                anchor, axis, q = pos + Rb @ jpos[j], Rb @ jaxis[j], qpos[jq[j]] - qpos0[jq[j]]
                if jt[j] == JT_SLIDE:
                    S[jd[j]] = np.concatenate([np.zeros(3), axis])
                    pos = pos + q * axis
                else:
                    assert jt[j] == JT_HINGE
                    S[jd[j]] = np.concatenate([axis, np.cross(anchor, axis)])
                    Rb = Rb @ _rodrigues(jaxis[j], q)
                    pos = anchor - Rb @ jpos[j]
                own.append(jd[j])
            X[b], R[b] = pos, Rb
        chain[b] = np.concatenate([chain[p], np.asarray(own, dtype=np.int64)])
    # body velocities and velocity-product accelerations, joint by joint: a += v_before x (S qdot)
    vel, acc = np.zeros((nb, 6)), np.zeros((nb, 6))
    for b in range(1, nb):
        vb, ab = vel[parent[b]].copy(), acc[parent[b]].copy()
        for j in range(jntadr[b], jntadr[b] + jntnum[b]):
            d = jd[j]
            if jt[j] == JT_FREE:
                vb = vb + S[d:d + 3].T @ v[d:d + 3]
                vj = S[d + 3:d + 6].T @ v[d + 3:d + 6]
                if defect != "cc":
                    ab = ab + _xm(vb, vj)
            else:
                vj = S[d] * v[d]
                ab = ab + _xm(vb, vj)
            vb = vb + vj
        vel[b], acc[b] = vb, ab
    # the spatial inertia of every body about the world origin; M and the bias force as sums over the bodies
    mass, inertia, ipos, iquat = f("body_mass"), f("body_inertia", -1, 3), f("body_ipos", -1, 3), f("body_iquat", -1, 4)
    Mo, bias, ag = np.zeros((nv, nv)), np.zeros(nv), np.concatenate([np.zeros(3), -g])
    com = X + np.einsum("bij,bj->bi", R, ipos)
    for b in range(1, nb):
        if len(chain[b]) == 0 or mass[b] == 0.0:
            continue
        Ri, c, mb = R[b] @ _rot(iquat[b]), com[b], mass[b]
        Io = Ri @ np.diag(inertia[b]) @ Ri.T
        if defect != "parallel_axis":
            Io = Io + mb * ((c @ c) * np.eye(3) - np.outer(c, c))
        I6 = np.block([[Io, mb * _skew(c)], [-mb * _skew(c), mb * np.eye(3)]])
        J = S[chain[b]].T  # [6, k]
        Mo[np.ix_(chain[b], chain[b])] += J.T @ I6 @ J
        fb = I6 @ (acc[b] + ag)
        if defect != "gyroscopic":
            fb = fb + _xf(vel[b], I6 @ vel[b])
        bias[chain[b]] += J.T @ fb
    if defect != "armature":
        Mo += np.diag(f("dof_armature"))
    # actuators, applied forces
    act = np.zeros(nv)
    for u in range(m.nu):
        j = i_("actuator_jntid")[u]
        c, gear, bp = st["ctrl"][e][u], f("actuator_gear")[u], f("actuator_bias", -1, 3)[u]
        if i_("actuator_ctrllimited")[u] and defect != "ctrl_clamp":
            c = min(max(c, f("actuator_ctrlrange", -1, 2)[u, 0]), f("actuator_ctrlrange", -1, 2)[u, 1])
        fu = f("actuator_gain")[u] * c + bp[0] + bp[1] * qpos[jq[j]] * gear + bp[2] * v[jd[j]] * gear
        if i_("actuator_forcelimited")[u] and defect != "force_clamp":
            fu = min(max(fu, f("actuator_forcerange", -1, 2)[u, 0]), f("actuator_forcerange", -1, 2)[u, 1])
        act[jd[j]] += fu * gear
    applied = np.array(st["qfrc_applied"][e], dtype=np.float64)
    for i, b in enumerate(i_("part_bodyid")):
        F, T = st["xfrc_applied"][e][6 * i:6 * i + 3], st["xfrc_applied"][e][6 * i + 3:6 * i + 6]
        at = X[b] if defect == "xfrc_arm" else com[b]
        applied[chain[b]] += S[chain[b]] @ np.concatenate([T + np.cross(at, F), F])
    D = f("dof_damping")
    Ms = Mo if (M is None or defect in ("parallel_axis", "armature")) else M
    qacc = np.linalg.solve(Ms, -D * v - bias + applied + act)
    v1 = v + h * (qacc if defect == "explicit_damping" else np.linalg.solve(Ms + h * np.diag(D), Ms @ qacc))
    q1 = qpos.copy()
    for j in range(len(jt)):
        a, d = jq[j], jd[j]
        if jt[j] == JT_FREE:
            q1[a:a + 3] += h * v1[d:d + 3]
            w = v1[d + 3:d + 6]
            t = np.linalg.norm(w) * h
            if t > 0:
                ax = w / np.linalg.norm(w) if np.linalg.norm(w) >= 1e-15 else np.array([1.0, 0.0, 0.0])
                dq = np.concatenate([[np.cos(0.5 * t)], np.sin(0.5 * t) * ax])
                qn = _qmul(dq, qpos[a + 3:a + 7]) if defect == "left_quaternion" else _qmul(qpos[a + 3:a + 7], dq)
                q1[a + 3:a + 7] = qn / np.linalg.norm(qn)
        else:
            q1[a] += h * v1[d]
    return dict(bias=bias, M=Mo, actuator=act, qacc=qacc, qvel1=v1, qpos1=q1, qpos_fwd=qpos, xpos=X, xmat=R, xipos=com)


# ---- the measures --------------------------------------------------------------------------------------------------------------------------
def _tree_scale(m, x, M=None):
    """[nv]: for every dof the largest |x| of its kinematic tree, and at least |g| (M: times the tree's largest diagonal entry of M)"""
    tree = np.asarray(m.arrays["dof_tree"], dtype=np.int64)
    g = float(np.linalg.norm(np.asarray(m.arrays["opt"][1:4], dtype=np.float64)))
    per = np.array([max(np.abs(x[tree == t]).max(), g * (1.0 if M is None else np.diag(M)[tree == t].max())) for t in range(int(tree.max()) + 1)])
    return per[tree]


def quat_angle(q, r):
    """the angle of the rotation between two orientations given as quaternions (of any length and sign)"""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    q, r = q / np.linalg.norm(q), r / np.linalg.norm(r)
    chord = min(np.linalg.norm(q - r), np.linalg.norm(q + r))  # |q - r| = 2 sin(angle / 4): exact for small angles, where arccos of the dot is not
    return 4.0 * np.arcsin(min(1.0, 0.5 * chord))


def move_errors(m, ref, qpos1):
    """[njnt]: per joint the `move` error of a new qpos against the reference's"""
    A = m.arrays
    h = float(A["opt"][0])
    out = []
    for t, a, d in zip(np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"], dtype=np.int64), np.asarray(A["jnt_dofadr"], dtype=np.int64)):
        if t == JT_FREE:
            lin = np.abs((qpos1[a:a + 3] - ref["qpos1"][a:a + 3]) / h) / np.maximum(1.0, np.abs(ref["qvel1"][d:d + 3]))
            ang = quat_angle(qpos1[a + 3:a + 7], ref["qpos1"][a + 3:a + 7]) / (h * max(1.0, np.linalg.norm(ref["qvel1"][d + 3:d + 6])))
            out.append(max(lin.max(), ang))
        else:
            out.append(abs((qpos1[a] - ref["qpos1"][a]) / h) / max(1.0, abs(ref["qvel1"][d])))
    return np.array(out)


def measures(m, ref, got):
    """the measures of one env: got holds xpos [nbody, 3], xquat [nbody, 4], bias, qacc, qvel1, qpos1 (any subset of the first three may be
    missing: the restatement has no quaternions) and, for the tumble, qpos_tumble"""
    A = m.arrays
    h, D = float(A["opt"][0]), np.asarray(A["dof_damping"], dtype=np.float64)
    g = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    out = {}
    if "xpos" in g:
        out["pose"] = np.abs(g["xpos"].reshape(-1, 3) - ref["xpos"]).max() / max(1.0, np.abs(ref["xpos"]).max())
    if "xquat" in g:
        q, r = g["xquat"].reshape(-1, 4), ref["xquat"]
        out["pose"] = max(out.get("pose", 0.0), np.minimum(np.linalg.norm(q - r, axis=1), np.linalg.norm(q + r, axis=1)).max())
    if "bias" in g:
        out["bias"] = np.abs(g["bias"] - ref["bias"]).max() / np.abs(ref["bias"]).max()
    if "qacc" in g:
        ferr = ref["M"] @ g["qacc"] - ref["f_smooth"]
        out["force"] = (np.abs(ferr) / _tree_scale(m, ref["f_smooth"], ref["M"])).max()
        out["acc"] = (np.abs(g["qacc"] - ref["qacc"]) / _tree_scale(m, ref["qacc"])).max()
        if m.nu:
            dofs = np.unique(np.asarray(A["jnt_dofadr"], dtype=np.int64)[np.asarray(A["actuator_jntid"], dtype=np.int64)])
            implied = ref["M"] @ g["qacc"] + ref["bias"] + D * ref["qvel"] - ref["applied"]
            scale = np.abs(ref["actuator"]).max()
            out["actuator"] = np.abs(implied - ref["actuator"])[dofs].max() / (scale if scale > 0 else 1.0)
    if "qvel1" in g:
        a64 = (ref["qvel1"] - ref["qvel"]) / h
        out["step"] = (np.abs((g["qvel1"] - ref["qvel"]) / h - a64) / _tree_scale(m, a64)).max()
    if "qpos1" in g:
        out["move"] = move_errors(m, ref, g["qpos1"]).max()
    if "qpos_tumble" in g and "qpos_tumble" in ref:
        pq = np.asarray(m.part_qposadr, dtype=np.int64)
        out["tumble_pos"] = max(np.abs(g["qpos_tumble"][a:a + 3] - ref["qpos_tumble"][a:a + 3]).max() for a in pq)
        out["tumble_ang"] = max(quat_angle(g["qpos_tumble"][a + 3:a + 7], ref["qpos_tumble"][a + 3:a + 7]) for a in pq)
        out["tumble_norm"] = max(abs(np.linalg.norm(g["qpos_tumble"][a + 3:a + 7]) - 1.0) for a in pq)
    return out


def worst(rows):
    """the largest value of each measure over a list of measures() dicts"""
    out = {}
    for r in rows:
        for k, v in r.items():
            out[k] = max(out.get(k, 0.0), float(v))
    return out


def normalised_qpos_error(m, ref, qpos_fwd):
    """qpos after a forward pass against the reference's: the largest absolute difference (part quaternions normalised in place, sign kept)"""
    return np.abs(np.asarray(qpos_fwd, dtype=np.float64) - ref["qpos_fwd"]).max()


# ---- the checker's builds through the C-ABI ------------------------------------------------------------------------------------------------
def abi_run(path, m, st):
    """list over the envs of the `got` dict of measures() from the library at `path` (host pointers: oracle/libfsim_cpu.so,
    oracle/libfsim_cpu32.so): one fsim_physics_forward, one fsim_physics_step on the state again, TUMBLE_STEPS on the state again"""
    from furniture_amd import sim
    from tests.abi_session import Abi, Session
    ses = Session(Abi(path), m.to_blob(), N, auto_reset=0)
    L = ses.abi.L
    L.fsim_physics_step.argtypes = [ctypes.c_void_p, ctypes.c_int]
    ses.set_state(m, **fields(st))
    ses.forward()
    qacc, sp = np.zeros((N, m.nv), np.float32), sim.StatePtrs()  # (qacc is not among the fields Session.get_state knows)
    sp.qacc = qacc.ctypes.data
    ses.abi.check(L.fsim_get_state(ses.h, ctypes.byref(sp)))
    fwd = ses.get_state(m, "xpos", "xquat", "qfrc_bias", "qpos", "ncon")
    ses.set_state(m, **fields(st))
    ses.abi.check(L.fsim_physics_step(ses.h, 1))
    one = ses.get_state(m, "qvel", "qpos")
    ses.set_state(m, **fields(st))
    ses.abi.check(L.fsim_physics_step(ses.h, TUMBLE_STEPS))
    far = ses.get_state(m, "qpos")
    ses.close()
    return [dict(xpos=fwd["xpos"][e], xquat=fwd["xquat"][e], bias=fwd["qfrc_bias"][e], qacc=qacc[e], qpos_fwd=fwd["qpos"][e], ncon=int(fwd["ncon"][e]),
                 qvel1=one["qvel"][e], qpos1=one["qpos"][e], qpos_tumble=far["qpos"][e]) for e in range(N)]


def references(name):
    """(model, states, [reference of env e]) of a model"""
    from oracle.oracle_sim import OracleSim
    m, st = model(name), states(name)
    o = OracleSim(m)
    refs = [reference(o, m, st, e) for e in range(N)]
    o.close()
    return m, st, refs


def by_group(m, refs, got):
    """{group: {measure: the largest over the group's envs}} of a list of `got` dicts, one per env"""
    return {g: worst([measures(m, refs[e], got[e]) for e in range(N) if group(e) == g]) for g in GROUPS}


def what_fp32_alone_does(name, refs=None):
    """the value FLOOR[name] must hold: by_group of the checker's float32 build"""
    import os
    m, st = model(name), states(name)
    if refs is None:
        refs = references(name)[2]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "libfsim_cpu32.so")
    return by_group(m, refs, abi_run(path, m, st))

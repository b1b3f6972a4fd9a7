"""Reference for the device's frame sensors (include/fsim_frames.h), in float64 numpy.

It builds on the oracle (oracle/oracle_sim.py) and shares no code with the device path: with an OracleSim set to a given qpos / qvel
(tests.flow_reference.set_state), a frame's world pose comes from xpos / xquat -- or site_xpos / site_xmat for a site -- composed with
the frame's offset, the world Jacobians of its point and rotation from OracleSim.body_jac(body, p), and the header's contract is
evaluated as it is written there.
"""

import numpy as np

from tests.flow_reference import advance, set_state  # noqa: F401  (re-exported: the callers set the oracle's state with them)


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def q2m(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def m2q(R):
    """unit quaternion wxyz of a rotation matrix (the branch with the largest pivot)"""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def frame_world(osim, model, frame):
    """(model body id or -1, p [3], q [4] wxyz) of a furniture_amd.frames.Frame at the oracle's current state"""
    d = osim.data
    off_p, off_q = np.asarray(frame.pos, dtype=np.float64), np.asarray(frame.quat, dtype=np.float64)
    off_q = off_q / np.linalg.norm(off_q)
    if frame.body is not None:
        b = model.meta["body_names"].index(frame.body)
        bp, bq = np.array(d.xpos[b], dtype=np.float64), np.array(d.xquat[b], dtype=np.float64)
    elif frame.site is not None:
        k = model.meta["site_names"].index(frame.site)
        b = int(np.asarray(model.arrays["site_bodyid"])[k])
        bp, bq = np.array(d.site_xpos[k], dtype=np.float64), m2q(np.array(d.site_xmat[k], dtype=np.float64).reshape(3, 3))
    else:
        return -1, off_p.copy(), off_q.copy()
    bq = bq / np.linalg.norm(bq)
    q = qmul(bq, off_q)
    return b, bp + q2m(bq) @ off_p, q / np.linalg.norm(q)


def _jac(osim, model, body, p):
    if body < 0:
        return np.zeros((3, model.nv)), np.zeros((3, model.nv))
    jp, jr = osim.body_jac(body, p)
    return np.array(jp, dtype=np.float64), np.array(jr, dtype=np.float64)


def evaluate(osim, model, sensor):
    """The contract of include/fsim_frames.h for one furniture_amd.frames.FrameSensor at the oracle's current state -> dict of pos [3],
    quat [4], vel [6], jac [6, nv] and the velocity scales: scale_lin = |v| + |v_g| + |w_g| |r|, scale_ang = |w| + |w_g|."""
    qvel = np.asarray(osim.data.qvel, dtype=np.float64)
    b, p, q = frame_world(osim, model, sensor.frame)
    bg, pg, qg = frame_world(osim, model, sensor.ref)
    jp, jr = _jac(osim, model, b, p)
    jpg, jrg = _jac(osim, model, bg, pg)
    Rg = q2m(qg)
    r = p - pg
    v, w, vg, wg = jp @ qvel, jr @ qvel, jpg @ qvel, jrg @ qvel
    rx = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    quat = qmul(qg * np.array([1.0, -1.0, -1.0, -1.0]), q)
    return dict(pos=Rg.T @ r, quat=quat / np.linalg.norm(quat),
                vel=np.concatenate([Rg.T @ (v - vg - np.cross(wg, r)), Rg.T @ (w - wg)]),
                jac=np.concatenate([Rg.T @ (jp - jpg + rx @ jrg), Rg.T @ (jr - jrg)], axis=0),
                scale_lin=np.linalg.norm(v) + np.linalg.norm(vg) + np.linalg.norm(wg) * np.linalg.norm(r),
                scale_ang=np.linalg.norm(w) + np.linalg.norm(wg), R_rel=Rg.T @ q2m(q))


def evaluate_set(osim, model, sensors):
    """evaluate() of every sensor, stacked: pos [S, 3], quat [S, 4], vel [S, 6], jac [S, 6, nv], scale_lin [S], scale_ang [S], R_rel [S, 3, 3]"""
    rows = [evaluate(osim, model, s) for s in sensors]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}

"""Reference optical flow and surface velocity for the device's flow images (include/fsim_flow.h), in float64 numpy.

It builds on tests/camera_reference.py (the pixel rays) and on the oracle (oracle/oracle_sim.py) and shares no code with the device
path: poses come from OracleSim.forward(), twists from OracleSim.body_jac(body, point) @ qvel (linear and angular rows), and the
header's formulas are evaluated per pixel on a depth and a segmentation image that are GIVEN -- the device's own images when the device
is checked, the float64 caster's in the CPU tests.  Besides the two images it returns, per pixel, what the error measures need:
  scale  S = |v_g| + |w_g| |q - pos_g| + |v_c| + |w_c| |q - p_c|, the magnitude of what was added up (m/s);
  cx, cy the pixel's ray slopes, depth and the camera's slope s.
"""

import numpy as np

from tests import camera_reference as cref


def set_state(osim, model, qpos, qvel, cursor=None):
    """qpos / qvel (and, for the Cursor agent, the cursor offsets [6]) into the oracle, then forward kinematics"""
    osim.data.qpos[:] = qpos
    osim.data.qvel[:] = qvel
    if cursor is not None:
        for k, b in enumerate(model.arrays["cursor_bodyid"]):
            osim.model.body_pos[int(b)] = cursor[3 * k:3 * k + 3]
    osim.forward()


def camera_pose(osim, model, cam):
    b = cam.body_id(model)
    p, R = cam.world_pose(osim.data.xpos[b] if b >= 0 else None, osim.data.xquat[b] if b >= 0 else None)
    return b, np.asarray(p, dtype=np.float64), np.asarray(R, dtype=np.float64)


def twist_at(osim, body, point):
    """(v, w) of the body-fixed point `point` (world coordinates) of `body` at the oracle's current state"""
    if body < 0:
        return np.zeros(3), np.zeros(3)
    jp, jr = osim.body_jac(body, point)
    qvel = np.asarray(osim.data.qvel, dtype=np.float64)
    return jp @ qvel, jr @ qvel


def render(osim, model, qpos, qvel, cams, depth, seg, cursor=None):
    """depth, seg: [C, H, W] images of the camera list at this state -> dict of flow [C, H, W, 3], velocity [C, H, W, 3], scale, cx, cy,
    depth [C, H, W] and slope [C]"""
    set_state(osim, model, np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64), cursor)
    depth, seg = np.asarray(depth, dtype=np.float64), np.asarray(seg)
    C, H, W = seg.shape
    flow, vel, scale = np.zeros((C, H, W, 3)), np.zeros((C, H, W, 3)), np.zeros((C, H, W))
    cxs, cys, slope = np.zeros((C, H, W)), np.zeros((C, H, W)), np.zeros(C)
    body_of = np.asarray(model.arrays["geom_bodyid"])
    for c, cam in enumerate(cams):
        b, pc, Rc = camera_pose(osim, model, cam)
        vc, wc = twist_at(osim, b, pc)
        s = np.tan(np.radians(cam.fovy) / 2.0) / (0.5 * H)
        slope[c] = s
        cx = np.broadcast_to(((np.arange(W) + 0.5 - W / 2.0) * s)[None, :], (H, W))
        cy = np.broadcast_to(((H / 2.0 - (np.arange(H) + 0.5)) * s)[:, None], (H, W))
        cxs[c], cys[c] = cx, cy
        q = pc + cref.pixel_rays(Rc, cam.fovy, W, H) * depth[c][..., None]
        for g in np.unique(seg[c][seg[c] >= 0]):
            mask = seg[c] == g
            pos_g = np.array(osim.data.geom_xpos[int(g)], dtype=np.float64)
            vg, wg = twist_at(osim, int(body_of[int(g)]), pos_g)
            rq = q[mask] - pos_g
            u = vg + np.cross(wg, rq)
            rc = q[mask] - pc
            X = (u - vc - np.cross(wc, rc)) @ Rc  # R_c^T (.)
            dd = -X[:, 2]
            d = depth[c][mask]
            flow[c][mask] = np.stack([(X[:, 0] - cx[mask] * dd) / (d * s), -(X[:, 1] - cy[mask] * dd) / (d * s), dd], axis=1)
            vel[c][mask] = u
            scale[c][mask] = (np.linalg.norm(vg) + np.linalg.norm(wg) * np.linalg.norm(rq, axis=1) + np.linalg.norm(vc) +
                              np.linalg.norm(wc) * np.linalg.norm(rc, axis=1))
    return dict(flow=flow, velocity=vel, scale=scale, cx=cxs, cy=cys, depth=depth, slope=slope)


def measures(ref, flow=None, velocity=None, floor=1e-3):
    """The error measures of a flow and / or a velocity image [C, H, W, 3] against the reference `ref`, per pixel [C, H, W]: the velocity
    error |du| / max(S, floor); the image-plane flow error in its metric form, so that near pixels do not dominate,
    |dflow[0:2]| d s / (max(S, floor) (1 + |cx| + |cy|)); and the depth-rate error |dflow[2]| / max(S, floor)."""
    S = np.maximum(ref["scale"], floor)
    out = {}
    if velocity is not None:
        out["velocity"] = np.linalg.norm(np.asarray(velocity, dtype=np.float64) - ref["velocity"], axis=-1) / S
    if flow is not None:
        df = np.asarray(flow, dtype=np.float64) - ref["flow"]
        ds = ref["depth"] * ref["slope"][:, None, None]
        out["flow_xy"] = np.linalg.norm(df[..., :2], axis=-1) * ds / (S * (1.0 + np.abs(ref["cx"]) + np.abs(ref["cy"])))
        out["flow_z"] = np.abs(df[..., 2]) / S
    return out


def advance(model, qpos, qvel, h):
    """qpos moved by h * qvel with MuJoCo's rule: hinge and slide additively, free position additively, free quaternion multiplied on the
    right by exp(h w_local / 2)"""
    A = model.arrays
    out = np.array(qpos, dtype=np.float64)
    for jt, qa, da in zip(np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"]), np.asarray(A["jnt_dofadr"])):
        qa, da = int(qa), int(da)
        if jt != 0:
            out[qa] += h * qvel[da]
            continue
        out[qa:qa + 3] += h * np.asarray(qvel[da:da + 3])
        w = h * np.asarray(qvel[da + 3:da + 6], dtype=np.float64)
        ang = np.linalg.norm(w)
        e = np.array([1.0, 0.0, 0.0, 0.0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * w / ang])
        a = out[qa + 3:qa + 7].copy()
        out[qa + 3:qa + 7] = [a[0] * e[0] - a[1] * e[1] - a[2] * e[2] - a[3] * e[3], a[0] * e[1] + a[1] * e[0] + a[2] * e[3] - a[3] * e[2],
                              a[0] * e[2] - a[1] * e[3] + a[2] * e[0] + a[3] * e[1], a[0] * e[3] + a[1] * e[2] - a[2] * e[1] + a[3] * e[0]]
    return out

"""Body and site frame sensors with their Jacobians, computed on the device (include/fsim_frames.h, csrc/fsim_frames.hpp).

A FrameSensor reports a frame F, optionally relative to a reference frame G: MuJoCo's framepos / framequat / framelinvel / frameangvel
sensors with their reftype / refid reference frame, and mj_jacBody / mj_jacSite.  A Frame is attached to a model body or a site, by name,
or fixed in the world, with an offset pose in that frame.  Per sensor the device gives frame_pos (float32 [3]: F's origin in G's frame,
metres), frame_quat (float32 [4] wxyz: F's orientation in G's frame, not sign-canonicalised) and, when asked for, frame_vel (float32 [6]:
the time derivative of frame_pos, then the relative angular velocity, both in G's frame) and frame_jac (float32 [6, nv]: frame_vel =
frame_jac @ qvel).  Without a reference the frame is reported in the world.  A frame on a cursor body follows the env's cursor and has no
velocity.  The contract is the header's.
"""

import numpy as np

MAX_SENSORS = 64  # FSIM_FRAME_MAX_SENSORS
MAX_NV = 128      # FSIM_FRAME_MAX_NV
MAX_BODIES = 32   # reduced bodies the device pass holds


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _qrot(q, v):
    u = q[1:]
    t = 2.0 * np.cross(u, v)
    return v + q[0] * t + np.cross(u, t)


class Frame:
    """A frame attached to the model body named ``body`` or to the site named ``site`` (at most one of the two; neither: fixed in the
    world), with the offset pose (pos, quat wxyz) in that body's or site's frame.  "0_part0" is both a body and a site name, so the
    keyword decides."""

    def __init__(self, body=None, site=None, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0)):
        if body is not None and site is not None:
            raise ValueError("Frame: give at most one of body= and site= (got %r and %r)" % (body, site))
        for name, v in (("body", body), ("site", site)):
            if v is not None and not isinstance(v, str):
                raise ValueError("Frame: %s is a name (got %r)" % (name, v))
        self.body, self.site = body, site
        try:
            self.pos = np.array(pos, dtype=np.float64).reshape(-1)
            self.quat = np.array(quat, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("Frame: pos is 3 numbers and quat 4 (got %r, %r)" % (pos, quat))
        if self.pos.shape != (3,) or self.quat.shape != (4,):
            raise ValueError("Frame: pos is 3 numbers and quat 4 (got %r, %r)" % (pos, quat))
        if not np.isfinite(self.pos).all() or not np.isfinite(self.quat).all():
            raise ValueError("Frame: a pose that is not finite (%r, %r)" % (pos, quat))
        n = np.linalg.norm(self.quat)
        if not n > 1e-12:
            raise ValueError("Frame: a zero quaternion")
        self.quat = self.quat / n

    def resolve(self, model):
        """(model body id or -1, pos [3], quat [4]) in float64: a site's own pose in its body composed with the offset"""
        if self.body is not None:
            names = model.meta["body_names"]
            if self.body not in names:
                raise ValueError("Frame: unknown body %r (model %s + %s)" % (self.body, model.meta.get("agent"), model.meta.get("furniture_name")))
            return names.index(self.body), self.pos.copy(), self.quat.copy()
        if self.site is not None:
            names = model.meta["site_names"]
            if self.site not in names:
                raise ValueError("Frame: unknown site %r (model %s + %s)" % (self.site, model.meta.get("agent"), model.meta.get("furniture_name")))
            k = names.index(self.site)
            sp = np.asarray(model.arrays["site_pos"], dtype=np.float64).reshape(-1, 3)[k]
            sq = np.asarray(model.arrays["site_quat"], dtype=np.float64).reshape(-1, 4)[k]
            sq = sq / np.linalg.norm(sq)
            q = _qmul(sq, self.quat)
            return int(np.asarray(model.arrays["site_bodyid"])[k]), sp + _qrot(sq, self.pos), q / np.linalg.norm(q)
        return -1, self.pos.copy(), self.quat.copy()

    def __repr__(self):
        where = "body=%r" % self.body if self.body is not None else ("site=%r" % self.site if self.site is not None else "world")
        plain = not self.pos.any() and self.quat[0] == 1.0
        return "Frame(%s)" % where if plain else "Frame(%s, pos=%s, quat=%s)" % (where, tuple(self.pos.tolist()), tuple(self.quat.tolist()))


class FrameSensor:
    """One sensor: the frame ``frame`` as seen from the frame ``ref`` (None: the world)."""

    def __init__(self, frame, ref=None):
        ref = Frame() if ref is None else ref
        for name, f in (("frame", frame), ("ref", ref)):
            if not isinstance(f, Frame):
                raise TypeError("FrameSensor: %s is a furniture_amd.frames.Frame, not %r" % (name, type(f).__name__))
        self.frame, self.ref = frame, ref

    def __repr__(self):
        return "FrameSensor(%r, ref=%r)" % (self.frame, self.ref)


class FrameSet:
    """The frame sensors of a handle or env, in the style of PairSet.  velocity / jacobian: add frame_vel / frame_jac to the outputs."""

    def __init__(self, sensors, velocity=False, jacobian=False):
        self.sensors = [sensors] if isinstance(sensors, FrameSensor) else list(sensors)
        for name, v in (("velocity", velocity), ("jacobian", jacobian)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("FrameSet: %s is a boolean (got %r)" % (name, v))
        self.velocity, self.jacobian = bool(velocity), bool(jacobian)
        self.check()

    def check(self):
        """Host-side check of the frame set, before any device work (the names need the model: sensor_table)."""
        for k in self.sensors:
            if not isinstance(k, FrameSensor):
                raise TypeError("FrameSet: a list of furniture_amd.frames.FrameSensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= MAX_SENSORS:
            raise ValueError("FrameSet: %d sensors (1 .. %d)" % (len(self.sensors), MAX_SENSORS))

    @property
    def n_sensors(self):
        return len(self.sensors)

    def __repr__(self):
        return "FrameSet(%d sensors, velocity=%r, jacobian=%r)" % (len(self.sensors), self.velocity, self.jacobian)


def check(spec):
    """Host-side check of a frames= argument, before any device work."""
    if not isinstance(spec, FrameSet):
        raise TypeError("frames: a furniture_amd.frames.FrameSet, not %r" % type(spec).__name__)
    spec.check()


def sensor_table(model, frame_set):
    """the fsim_frame_sensor_t array of a frame set against a compiled model (checked here first, then again by the library)"""
    from .sim import FsimFrameSensor
    check(frame_set)
    nr = int(np.asarray(model.arrays["rdims"])[0])
    if nr > MAX_BODIES:
        raise ValueError("frames: the model has %d reduced bodies (at most %d)" % (nr, MAX_BODIES))
    if model.nv > MAX_NV:
        raise ValueError("frames: the model has nv = %d (at most %d)" % (model.nv, MAX_NV))
    tab = (FsimFrameSensor * len(frame_set.sensors))()
    for i, k in enumerate(frame_set.sensors):
        for dst, f in ((tab[i].frame, k.frame), (tab[i].ref, k.ref)):
            body, pos, quat = f.resolve(model)
            dst.body = body
            dst.pos[:] = [float(x) for x in pos]
            dst.quat[:] = [float(x) for x in quat]
    return tab


def connector_pairs(model):
    """[(a, b)] site names of connector sites on different parts whose keys match the way the env pairs them (conn_keya / conn_keyb:
    `a-b` against `b-a`; keys without a second half match their equals).  Every connector site is used once: in connector-table order a
    site takes the first counterpart that is still free -- where counterparts are interchangeable (four legs, four holes of a table top)
    the keys name the kind only, and this is one of the equal assignments: four leg-to-table pairs for table_lack_0825.
    FrameSet([FrameSensor(Frame(site=a), ref=Frame(site=b)) for a, b in connector_pairs(model)]) reports every connector in the frame of
    its counterpart -- the error the env's alignment test thresholds."""
    A = model.arrays
    sites = model.meta["site_names"]
    sid, part = np.asarray(A["conn_siteid"]), np.asarray(A["conn_partid"])
    ka, kb = np.asarray(A["conn_keya"]), np.asarray(A["conn_keyb"])
    used = np.zeros(len(sid), dtype=bool)
    out = []
    for k1 in range(len(sid)):
        if used[k1]:
            continue
        for k2 in range(k1 + 1, len(sid)):
            if used[k2] or part[k1] == part[k2]:
                continue
            a1, b1, a2, b2 = int(ka[k1]), int(kb[k1]), int(ka[k2]), int(kb[k2])
            match = (b1 < 0 and b2 < 0 and a1 == a2) if (b1 < 0 or b2 < 0) else (a1 == b2 and b1 == a2)
            if match:
                used[k1] = used[k2] = True
                out.append((sites[int(sid[k1])], sites[int(sid[k2])]))
                break
    return out

"""Ray-cast range sensors and lidar computed on the device (include/fsim_rays.h, csrc/fsim_rays.hpp).

A RaySensor is a frame fixed in the world or mounted on a model body with a set of ray directions in that frame, a range [tmin, tmax]
in metres along the ray and a set of geoms it does not see.  Per ray the device gives ray_distance (float32 metres along the ray, -1
where nothing is hit: MuJoCo's rangefinder convention), ray_geom (int32 model geom id, the numbering of camera_segmentation, so
furniture_amd.camera.geom_labels applies; -1 = nothing) and, when asked for, ray_normal (float32 world-frame outward unit normal at the hit
point, (0, 0, 0) = nothing).  The hit point in the sensor frame is ray_distance * direction.  The sensors see the collision geometry the
cameras see; they need no camera.  The contract is the header's.
"""

import numpy as np

from .camera import MAX_GEOMS

MAX_SENSORS = 16  # FSIM_RAY_MAX_SENSORS
MAX_RAYS = 4096   # FSIM_RAY_MAX_RAYS, per env over all sensors


class RaySensor:
    """One sensor: fixed in the world (body=None) or mounted on the model body named ``body``; pos / quat (wxyz) in that frame.
    directions: [k, 3] in the sensor frame, any nonzero length (normalised here).  tmin, tmax: the range in metres along the ray.
    exclude: "body" (the default: a mounted sensor does not see the geoms that move rigidly with its mount; see exclude_mask), None
    (sees everything) or a list of model geom ids."""

    def __init__(self, pos, directions, quat=None, body=None, tmin=0.0, tmax=10.0, exclude="body"):
        self.pos = np.asarray(pos, dtype=np.float64).reshape(3)
        q = np.asarray((1.0, 0.0, 0.0, 0.0) if quat is None else quat, dtype=np.float64).reshape(4)
        if not np.all(np.isfinite(self.pos)) or not np.all(np.isfinite(q)) or np.linalg.norm(q) < 1e-12:
            raise ValueError("RaySensor: bad pose")
        self.quat = q / np.linalg.norm(q)
        d = np.asarray(directions, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3 or len(d) < 1:
            raise ValueError("RaySensor: directions is a [k, 3] array with k >= 1 (got shape %s)" % (d.shape,))
        ln = np.linalg.norm(d, axis=1)
        if not np.all(np.isfinite(d)) or not np.all(ln > 0):
            raise ValueError("RaySensor: a direction is zero or not finite")
        self.directions = d / ln[:, None]
        self.tmin, self.tmax = float(tmin), float(tmax)
        if not (self.tmin >= 0.0 and self.tmax > self.tmin and np.isfinite(self.tmax)):
            raise ValueError("RaySensor: needs 0 <= tmin < tmax < inf (got %g, %g)" % (self.tmin, self.tmax))
        if not (exclude is None or exclude == "body" or (not isinstance(exclude, str) and all(int(g) == g for g in exclude))):
            raise ValueError("RaySensor: exclude is \"body\", None or a list of model geom ids (got %r)" % (exclude,))
        self.exclude = exclude if exclude is None or isinstance(exclude, str) else [int(g) for g in exclude]
        self.body = body

    @property
    def n_rays(self):
        return len(self.directions)

    def body_id(self, model):
        if self.body is None:
            return -1
        names = model.meta["body_names"]
        if self.body not in names:
            raise ValueError("RaySensor: unknown body %r (model %s + %s)" % (self.body, model.meta.get("agent"), model.meta.get("furniture_name")))
        return names.index(self.body)

    def world_pose(self, body_xpos=None, body_xquat=None):
        """(origin, 3 x 3 sensor -> world rotation) given the world pose of the sensor's body (ignored for a world sensor)."""
        from .camera import quat_to_mat
        if self.body is None:
            return self.pos.copy(), quat_to_mat(self.quat)
        R = quat_to_mat(body_xquat)
        return np.asarray(body_xpos, dtype=np.float64) + R @ self.pos, R @ quat_to_mat(self.quat)

    def __repr__(self):
        return "RaySensor(pos=%s, %d rays, body=%r, range %g .. %g, exclude=%r)" % (self.pos.tolist(), self.n_rays, self.body, self.tmin, self.tmax, self.exclude)


def exclude_mask(model, sensor):
    """[ncg] bool: the colliding geoms (rows of cg_orig) the sensor does not see.  exclude="body": a world sensor excludes nothing; a
    mounted one excludes the colliding geoms whose body mjcf/reduce.py folds into the same reduced body as the mount's body -- they move
    rigidly with the sensor, and a sensor origin usually lies inside one of them (right_hand's lies inside the gripper-base box, which
    belongs to another body of the same reduced body) -- unless that reduced body is 0 (a cursor is welded to the world): then only the
    geoms of the mount's body itself, or the floor would be hidden."""
    A = model.arrays
    cg_orig = np.asarray(A["cg_orig"]).astype(np.int64)
    mask = np.zeros(len(cg_orig), dtype=bool)
    if sensor.exclude is None:
        return mask
    if sensor.exclude == "body":
        b = sensor.body_id(model)
        if b < 0:
            return mask
        gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[cg_orig]
        red = np.asarray(A["body_red"]).astype(np.int64)
        return gbody == b if red[b] == 0 else red[gbody] == red[b]
    ngeom = len(A["geom_bodyid"])
    for g in sensor.exclude:
        if not 0 <= g < ngeom:
            raise ValueError("sensor: exclude names geom %d (the model has %d geoms)" % (g, ngeom))
        mask |= cg_orig == g  # (a geom that does not collide is invisible anyway)
    return mask


def mask_bits(mask):
    """[3] ints: a [ncg <= 96] bool mask of colliding geoms as the 96-bit masks of the C structs hold it, bit g & 31 of word g >> 5"""
    bits = [0, 0, 0]
    for g in np.nonzero(mask)[0]:
        bits[g >> 5] |= 1 << (int(g) & 31)
    return bits


def lidar(n_azimuth, n_elevation=1, elevation=(0.0, 0.0)):
    """[n_elevation * n_azimuth, 3] unit directions of a scanning lidar about the sensor's z axis: elevation outer (n_elevation rings
    from lo to hi degrees inclusive; one ring: their mean), azimuth inner at cell centres (i + 0.5) * 360 / n_azimuth degrees from +x
    towards +y."""
    if int(n_azimuth) != n_azimuth or int(n_elevation) != n_elevation or n_azimuth < 1 or n_elevation < 1:
        raise ValueError("lidar: n_azimuth and n_elevation are positive integers (got %r, %r)" % (n_azimuth, n_elevation))
    lo, hi = float(elevation[0]), float(elevation[1])
    if not (-90.0 <= lo <= hi <= 90.0):
        raise ValueError("lidar: elevation (lo, hi) in degrees with -90 <= lo <= hi <= 90 (got %g, %g)" % (lo, hi))
    el = np.radians(np.linspace(lo, hi, int(n_elevation)) if n_elevation > 1 else np.array([0.5 * (lo + hi)]))
    az = np.radians((np.arange(int(n_azimuth)) + 0.5) * 360.0 / int(n_azimuth))
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    return np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], se * np.ones_like(az)[None, :]], axis=-1).reshape(-1, 3)


def camera_rays(camera, tmin=0.0, tmax=None, exclude="body"):
    """A RaySensor on the camera's mount whose directions are the camera's pixel-centre rays in row-major order: ray j * W + i is pixel
    (i, j).  tmax: the camera's zfar unless given.  (The camera's depth is along its optical axis; ray_distance is along the ray:
    depth = ray_distance * -direction.z.)"""
    f = 0.5 * camera.height / np.tan(np.radians(camera.fovy) / 2.0)
    x = (np.arange(camera.width) + 0.5 - camera.width / 2.0) / f
    y = (camera.height / 2.0 - (np.arange(camera.height) + 0.5)) / f
    d = np.stack(np.broadcast_arrays(x[None, :], y[:, None], -1.0), axis=-1).reshape(-1, 3)
    return RaySensor(camera.pos, d, quat=camera.quat, body=camera.body, tmin=tmin, tmax=camera.zfar if tmax is None else tmax, exclude=exclude)


class RaySet:
    """The ray sensors of a handle or env, in the style of Flow and Normals.  normal: add ray_normal to the outputs."""

    def __init__(self, sensors, normal=False):
        self.sensors = [sensors] if isinstance(sensors, RaySensor) else list(sensors)
        if not isinstance(normal, (bool, np.bool_)):
            raise ValueError("RaySet: normal is a boolean (got %r)" % (normal,))
        self.normal = bool(normal)
        self.check()

    def check(self):
        """Host-side check of the ray set, before any device work."""
        for k in self.sensors:
            if not isinstance(k, RaySensor):
                raise TypeError("RaySet: a list of furniture_amd.rays.RaySensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= MAX_SENSORS:
            raise ValueError("RaySet: %d sensors (1 .. %d)" % (len(self.sensors), MAX_SENSORS))
        if self.n_rays > MAX_RAYS:
            raise ValueError("RaySet: %d rays over all sensors (at most %d)" % (self.n_rays, MAX_RAYS))

    @property
    def n_rays(self):
        return sum(k.n_rays for k in self.sensors)

    def sensor_slices(self):
        """{sensor index: slice of the ray dimension of the outputs}"""
        out, at = {}, 0
        for i, k in enumerate(self.sensors):
            out[i] = slice(at, at + k.n_rays)
            at += k.n_rays
        return out

    def __repr__(self):
        return "RaySet(%d sensors, %d rays, normal=%r)" % (len(self.sensors), self.n_rays, self.normal)


def check(spec):
    """Host-side check of a rays= argument, before any device work."""
    if not isinstance(spec, RaySet):
        raise TypeError("rays: a furniture_amd.rays.RaySet, not %r" % type(spec).__name__)
    spec.check()


def sensor_table(model, ray_set):
    """(fsim_ray_sensor_t array, float32 [R, 3] directions) of a ray set against a compiled model (checked here first, then again by
    the library)."""
    from .sim import FsimRaySensor
    check(ray_set)
    ncg = len(model.arrays["cg_orig"])
    if ncg > MAX_GEOMS:
        raise ValueError("rays: the model has %d colliding geoms (at most %d)" % (ncg, MAX_GEOMS))
    tab = (FsimRaySensor * len(ray_set.sensors))()
    at = 0
    for i, k in enumerate(ray_set.sensors):
        t = tab[i]
        t.body, t.tmin, t.tmax, t.first_ray, t.n_rays = k.body_id(model), k.tmin, k.tmax, at, k.n_rays
        t.pos[:], t.quat[:], t.exclude[:] = k.pos.tolist(), k.quat.tolist(), mask_bits(exclude_mask(model, k))
        at += k.n_rays
    dirs = np.ascontiguousarray(np.concatenate([k.directions for k in ray_set.sensors]), dtype=np.float32)
    return tab, dirs

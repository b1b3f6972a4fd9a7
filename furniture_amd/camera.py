"""Depth / segmentation cameras rendered on the device (include/fsim_camera.h, csrc/fsim_camera.hpp).

The cameras see exactly the collision geometry the solver uses -- planes, spheres, capsules, cylinders, boxes and the convex hulls
of the mesh colliders.  The reference's textured visual meshes are not part of the compiled model, so there is no RGB image: this is
the project's own observation, not pixel parity with the reference's Unity / MuJoCo renders.

Camera model (MuJoCo's): a pinhole camera looking along its own -z with +y up, ``fovy`` the vertical field of view in degrees, pixel
centres at (i + 0.5, j + 0.5), row 0 the top of the image.  Depth is the distance along the optical axis in metres; a pixel that sees
nothing between znear and zfar gets zfar and segmentation -1.  Segmentation is the model geom id; ``geom_labels`` maps it to a part
index (-2 robot, -3 floor / arena).
"""

import numpy as np

MAX_CAMERAS = 8        # FSIM_CAM_MAX
MAX_SIZE = 512         # FSIM_CAM_MAX_SIZE
MAX_GEOMS = 96         # FSIM_CAM_MAX_GEOMS
MAX_PLANES = 1024      # FSIM_CAM_MAX_PLANES
LABEL_ROBOT, LABEL_ARENA = -2, -3

# fsim_camera_t
CAMERA_DTYPE = np.dtype([("body", "<i4"), ("pos", "<f4", (3,)), ("quat", "<f4", (4,)), ("fovy", "<f4"), ("znear", "<f4"), ("zfar", "<f4"),
                         ("width", "<i4"), ("height", "<i4")])
assert CAMERA_DTYPE.itemsize == 52


def quat_from_mat(R):
    """wxyz quaternion of a rotation matrix (Shepperd: the largest of the four squared components first)."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    k = int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        s = 2.0 * np.sqrt(1.0 - R[0, 0] + R[1, 1] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 - R[0, 0] - R[1, 1] + R[2, 2])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q)
    return q if q[0] >= 0 else -q


def quat_to_mat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def lookat_quat(pos, lookat, up=(0.0, 0.0, 1.0)):
    """Orientation (wxyz) of a camera at ``pos`` whose optical axis (-z) points at ``lookat``, +y as close to ``up`` as it gets."""
    z = np.asarray(pos, dtype=np.float64) - np.asarray(lookat, dtype=np.float64)
    if np.linalg.norm(z) < 1e-12:
        raise ValueError("Camera: lookat equals pos")
    z /= np.linalg.norm(z)
    up = np.asarray(up, dtype=np.float64)
    x = np.cross(up, z)
    if np.linalg.norm(x) < 1e-9 * max(np.linalg.norm(up), 1e-300):  # looking along up: any horizontal x will do
        x = np.cross(np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0]), z)
    x /= np.linalg.norm(x)
    return quat_from_mat(np.stack([x, np.cross(z, x), z], axis=1))


class Camera:
    """One camera: fixed in the world (body=None) or attached to the model body named ``body``; pos / quat in that frame.  Give the
    orientation as a wxyz ``quat`` or as a point to ``lookat`` (with ``up``, in the same frame); neither = the frame's own axes."""

    def __init__(self, pos, quat=None, lookat=None, fovy=45.0, width=64, height=64, znear=0.01, zfar=10.0, body=None, up=(0.0, 0.0, 1.0)):
        self.pos = np.asarray(pos, dtype=np.float64).reshape(3)
        if quat is not None and lookat is not None:
            raise ValueError("Camera: give quat or lookat, not both")
        if lookat is not None:
            quat = lookat_quat(self.pos, lookat, up)
        q = np.asarray((1.0, 0.0, 0.0, 0.0) if quat is None else quat, dtype=np.float64).reshape(4)
        if not np.all(np.isfinite(self.pos)) or not np.all(np.isfinite(q)) or np.linalg.norm(q) < 1e-12:
            raise ValueError("Camera: bad pose")
        self.quat = q / np.linalg.norm(q)
        self.fovy, self.znear, self.zfar = float(fovy), float(znear), float(zfar)
        if not 0.0 < self.fovy < 180.0:
            raise ValueError("Camera: fovy %g not in (0, 180) degrees" % self.fovy)
        if not (self.znear > 0.0 and self.zfar > self.znear and np.isfinite(self.zfar)):
            raise ValueError("Camera: needs 0 < znear < zfar (got %g, %g)" % (self.znear, self.zfar))
        if int(width) != width or int(height) != height or not (1 <= width <= MAX_SIZE and 1 <= height <= MAX_SIZE):
            raise ValueError("Camera: size %s x %s (1 .. %d each)" % (width, height, MAX_SIZE))
        self.width, self.height = int(width), int(height)
        self.body = body

    def body_id(self, model):
        if self.body is None:
            return -1
        names = model.meta["body_names"]
        if self.body not in names:
            raise ValueError("Camera: unknown body %r (model %s + %s)" % (self.body, model.meta.get("agent"), model.meta.get("furniture_name")))
        return names.index(self.body)

    def world_pose(self, body_xpos=None, body_xquat=None):
        """(position, 3 x 3 camera -> world rotation) given the world pose of the camera's body (ignored for a world camera)."""
        if self.body is None:
            return self.pos.copy(), quat_to_mat(self.quat)
        R = quat_to_mat(body_xquat)
        return np.asarray(body_xpos, dtype=np.float64) + R @ self.pos, R @ quat_to_mat(self.quat)

    def __repr__(self):
        return "Camera(pos=%s, quat=%s, fovy=%g, %dx%d, body=%r)" % (self.pos.tolist(), self.quat.tolist(), self.fovy, self.width, self.height, self.body)


def reduced_pose(model, cam):
    """(reduced body, position, quaternion) of a camera in the frame of the reduced body its body was folded into
    (mjcf/reduce.py): (body_relpos, body_relquat) (x) the camera pose -- what fsim_set_cameras composes."""
    b = cam.body_id(model)
    if b < 0:
        return 0, cam.pos.copy(), cam.quat.copy()
    A = model.arrays
    rp = np.asarray(A["body_relpos"], dtype=np.float64).reshape(-1, 3)[b]
    rq = np.asarray(A["body_relquat"], dtype=np.float64).reshape(-1, 4)[b]
    return int(A["body_red"][b]), rp + quat_to_mat(rq) @ cam.pos, quat_mul(rq, cam.quat)


def camera_table(model, cams):
    """fsim_camera_t rows of a camera list (checked here first, then again by the library)."""
    if not 1 <= len(cams) <= MAX_CAMERAS:
        raise ValueError("cameras: %d given (1 .. %d)" % (len(cams), MAX_CAMERAS))
    if any((c.width, c.height) != (cams[0].width, cams[0].height) for c in cams):
        raise ValueError("cameras: all cameras of a handle have one size")
    tab = np.zeros(len(cams), dtype=CAMERA_DTYPE)
    for i, c in enumerate(cams):
        tab[i] = (c.body_id(model), c.pos, c.quat, c.fovy, c.znear, c.zfar, c.width, c.height)
    return tab


def hull_planes(vertices, tol=1e-6):
    """Face planes [k, 4] = (n, c), |n| = 1, inside where n . x <= c, of the convex hull of ``vertices``; coplanar facets merged."""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(vertices, dtype=np.float64)).equations  # n . x + d <= 0 inside
    keep = []
    for e in eq:
        if not any(abs(e[:3] @ k[:3] - 1.0) < tol and abs(e[3] - k[3]) < tol for k in keep):
            keep.append(e)
    out = np.asarray(keep, dtype=np.float64)
    out[:, 3] = -out[:, 3]
    return out


def hull_plane_table(model):
    """(planes float32 [P, 4], first plane int32 [ncg], plane count int32 [ncg]) of the model's convex-mesh colliders."""
    A = model.arrays
    ncg = len(A["cg_orig"])
    adr, num = np.zeros(ncg, np.int32), np.zeros(ncg, np.int32)
    rows = []
    if "cg_meshnum" in A:
        verts = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)
        for g in np.nonzero(np.asarray(A["cg_meshnum"]) > 0)[0]:
            a, k = int(A["cg_meshadr"][g]), int(A["cg_meshnum"][g])
            p = hull_planes(verts[a:a + k])
            adr[g], num[g] = sum(len(r) for r in rows), len(p)
            rows.append(p)
    planes = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, 4), np.float32)
    if len(planes) > MAX_PLANES:
        raise ValueError("cameras: the model's hull colliders have %d face planes (at most %d)" % (len(planes), MAX_PLANES))
    return np.ascontiguousarray(planes), adr, num


def geom_labels(model):
    """[ngeom] int32: part index of every furniture geom, -2 for a robot (or cursor) geom, -3 for the floor / arena -- a segmentation
    image (model geom ids, -1 = nothing) becomes a part mask with one gather: labels[seg.clamp(min=0)], masked where seg < 0."""
    A = model.arrays
    body = np.asarray(A["geom_bodyid"])
    part = np.asarray(A["body_partid"])[body]
    robot = (np.asarray(A["geom_is_robot"]) != 0) | (body != 0)
    return np.where(part >= 0, part, np.where(robot, LABEL_ROBOT, LABEL_ARENA)).astype(np.int32)

"""Point-cloud observations built on the device from the cameras (include/fsim_points.h, csrc/fsim_points.hpp).

Per env: the world-frame points of the camera pixels that see a kept geom, fused over all cameras, cropped to a box, labelled with
the model geom id, and either every pixel's point (dense mode, ``n_points=0``) or ``n_points`` of them chosen by farthest-point
sampling.  The contract -- which pixels are kept, how a point is computed, the FPS rule and its padding -- is the header's.
"""

import numpy as np

from .camera import LABEL_ARENA, LABEL_ROBOT, geom_labels

MAX_PIXELS = 16384  # FSIM_PTS_MAX_PIXELS: n_cam * width * height
MAX_POINTS = 4096   # FSIM_PTS_MAX_POINTS
INCLUDE = ("parts", "robot", "floor")  # "floor": the floor and the rest of the arena (camera.geom_labels' -3)


class PointCloud:
    """Settings of a point-cloud observation.  n_points: points per env by farthest-point sampling, 0 = dense mode (the point of every
    pixel).  include: which geoms' pixels are kept -- any of "parts" (the furniture), "robot" (arm, gripper or cursor) and "floor".
    box: ((lo x, y, z), (hi x, y, z)) crop in the world frame, bounds inclusive, or None."""

    def __init__(self, n_points=512, include=("parts", "robot"), box=None):
        if isinstance(n_points, (bool, np.bool_)) or int(n_points) != n_points or not 0 <= n_points <= MAX_POINTS:
            raise ValueError("PointCloud: n_points %r (0 .. %d; 0 = dense mode)" % (n_points, MAX_POINTS))
        if isinstance(include, str):
            include = (include,)
        include = tuple(include)
        if not include or any(k not in INCLUDE for k in include) or len(set(include)) != len(include):
            raise ValueError("PointCloud: include %r (a non-empty set of %s)" % (include, ", ".join(INCLUDE)))
        if box is not None:
            b = np.asarray(box, dtype=np.float64)
            if b.size != 6 or not np.all(np.isfinite(b)):
                raise ValueError("PointCloud: box must be ((lo x, y, z), (hi x, y, z)) of finite values")
            b = b.reshape(2, 3)
            if np.any(b[0] > b[1]):
                raise ValueError("PointCloud: box lo %s above hi %s" % (b[0].tolist(), b[1].tolist()))
            box = b
        self.n_points, self.include, self.box = int(n_points), include, box

    @property
    def dense(self):
        return self.n_points == 0

    def __repr__(self):
        return "PointCloud(n_points=%d, include=%r, box=%s)" % (self.n_points, self.include, None if self.box is None else self.box.tolist())


def geom_keep(model, include):
    """[ngeom] uint8: 1 for the model geoms whose pixels a point cloud with this ``include`` keeps (camera.geom_labels: a part index,
    -2 robot, -3 floor / arena)."""
    lab = geom_labels(model)
    keep = np.zeros(len(lab), dtype=bool)
    if "parts" in include:
        keep |= lab >= 0
    if "robot" in include:
        keep |= lab == LABEL_ROBOT
    if "floor" in include:
        keep |= lab == LABEL_ARENA
    return keep.astype(np.uint8)


def check(spec, cameras):
    """Host-side check of a point cloud against a camera list, before any device work."""
    if not isinstance(spec, PointCloud):
        raise TypeError("point_cloud: a furniture_amd.points.PointCloud, not %r" % type(spec).__name__)
    if not cameras:
        raise ValueError("point_cloud needs cameras: the points are built from their images (cameras=[Camera(...)])")
    npix = len(cameras) * cameras[0].width * cameras[0].height
    if npix > MAX_PIXELS:
        raise ValueError("point_cloud: %d camera(s) of %d x %d = %d pixels per env (at most %d)" %
                         (len(cameras), cameras[0].width, cameras[0].height, npix, MAX_PIXELS))

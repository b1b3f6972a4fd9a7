"""Reference for the device point clouds (include/fsim_points.h), written from the header's definitions in numpy.

- ``fps``: farthest-point sampling in float32, operation by operation as the header states it: dist2 = ((dx*dx + dy*dy) + dz*dz) with
  every product and sum rounded on its own (numpy rounds each float32 operation separately), dmin = min(dmin, dist2), the largest
  dmin wins and the smallest index wins a tie.  It reproduces the device bit for bit, except that the device flushes denormals: a
  squared distance below 2^-126 m^2 is 0 there (the test clouds have none).
- ``back_project``: float64 world points of a depth image from a camera pose (tests/camera_reference.py's rays: optical-axis
  component 1, so t along them is the depth).
"""

import numpy as np

from tests import camera_reference as camref


def fps(xyz, n):
    """xyz [K, 3] float32 candidates -> int64 [n] candidate index of every row (K = 0: all -1)."""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    K = len(p)
    out = np.full(n, -1, dtype=np.int64)
    if K == 0 or n == 0:
        return out
    out[:] = 0  # row 0 is candidate 0; rows K .. n-1 repeat it
    dmin = np.full(K, np.inf, dtype=np.float32)
    prev = 0
    for r in range(1, min(K, n)):
        d = p - p[prev]                                   # float32, rounded per element
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        dmin = np.minimum(dmin, d2)
        prev = int(np.argmax(dmin))                       # the first index of the largest value
        out[r] = prev
    return out


def back_project(depth, cam_pos, cam_R, fovy):
    """depth [H, W] (metres along the optical axis) of a camera at cam_pos with camera -> world rotation cam_R -> world xyz [H, W, 3]
    in float64"""
    H, W = depth.shape
    D = camref.pixel_rays(cam_R, fovy, W, H)
    return np.asarray(cam_pos, dtype=np.float64) + D * np.asarray(depth, dtype=np.float64)[..., None]


def kept(xyz, seg, keep, box=None):
    """the header's kept-pixel test on the device's own fp32 points: seg >= 0, keep[seg], inside box (inclusive)"""
    ok = (seg >= 0) & np.asarray(keep, dtype=bool)[np.maximum(seg, 0)]
    if box is not None:
        b = np.asarray(box, dtype=np.float32).reshape(2, 3)
        ok &= np.all((xyz >= b[0]) & (xyz <= b[1]), axis=-1)
    return ok

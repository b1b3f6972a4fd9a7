"""Reference surface normals for the device's normal images (include/fsim_normals.h), in float64 numpy, from the geometric definition
of every collision shape.

It builds on tests/camera_reference.py (the float64 ray caster) and shares no code with the device path: for each pixel it takes that
caster's hit point (camera centre + pixel ray * depth), brings it into the frame of the geom the caster names, and takes the outward
normal of the face or surface the point lies on -- the face whose supporting plane / surface is nearest to the point from outside,
i.e. has the largest signed distance.  Besides the normal it returns, per pixel,
  margin  the gap between the best and the runner-up face candidate (box: the three axes; cylinder: side against cap; hull: the best
          facet against the best facet that is not parallel to it), +inf for the smooth shapes (plane, sphere, capsule): a pixel with a
          small margin sits on an edge, where a rounding error of the hit point may pick the other face;
  radius  the radius of curvature of the surface there (sphere, capsule, cylinder side), +inf where it is flat.
"""

import numpy as np

from tests import camera_reference as cref

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = cref.PLANE, cref.SPHERE, cref.CAPSULE, cref.CYLINDER, cref.BOX, cref.MESH


def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(n < 1e-20, 0.0, v / np.where(n < 1e-20, 1.0, n))


def local_normal(gtype, size, p, halfspaces=None):
    """Outward normal of the geom's surface at the points p [k, 3] of its frame -> (normal [k, 3], margin [k], radius [k])"""
    k = len(p)
    inf = np.full(k, np.inf)
    if gtype == PLANE:
        return np.tile([0.0, 0.0, 1.0], (k, 1)), inf, inf.copy()
    if gtype == SPHERE:
        return _unit(p), inf, np.full(k, float(size[0]))
    if gtype == CAPSULE:  # the surface at distance r of the segment: the normal points away from the segment's nearest point
        c = np.zeros_like(p)
        c[:, 2] = np.clip(p[:, 2], -size[1], size[1])
        return _unit(p - c), inf, np.full(k, float(size[0]))
    if gtype == CYLINDER:
        rho = np.hypot(p[:, 0], p[:, 1])
        side, cap = rho - size[0], np.abs(p[:, 2]) - size[1]  # signed distances to the tube and to the nearer cap plane
        radial = np.stack([p[:, 0], p[:, 1], np.zeros(k)], 1)
        axial = np.stack([np.zeros(k), np.zeros(k), np.where(p[:, 2] < 0, -1.0, 1.0)], 1)
        on_side = side >= cap
        return np.where(on_side[:, None], _unit(radial), axial), np.abs(side - cap), np.where(on_side, float(size[0]), np.inf)
    if gtype == BOX:
        dist = np.abs(p) - np.asarray(size, dtype=np.float64)[None, :]  # signed distance to the nearer face of every axis
        a = np.argmax(dist, axis=1)  # (the first of equals)
        n = np.zeros((k, 3))
        n[np.arange(k), a] = np.where(p[np.arange(k), a] < 0, -1.0, 1.0)
        srt = np.sort(dist, axis=1)
        return n, srt[:, 2] - srt[:, 1], inf
    if gtype == MESH:
        N = np.stack([h[0] for h in halfspaces])  # facets n . x + off <= 0 inside
        off = np.asarray([h[1] for h in halfspaces])
        dist = p @ N.T + off[None, :]
        best = np.argmax(dist, axis=1)
        n = N[best]
        other = np.where(n @ N.T > 1.0 - 1e-9, -np.inf, dist)  # facets not parallel to the best one (coplanar triangles are one face)
        return n, dist[np.arange(k), best] - other.max(axis=1), inf
    raise ValueError("geom type %d" % gtype)


def render(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms):
    """camera_reference.render plus normals -> dict of depth [H, W], seg [H, W], point [H, W, 3] (world), normal [H, W, 3] (world, unit,
    0 where seg is -1), margin [H, W] and radius [H, W] (+inf where seg is -1)"""
    geoms = list(geoms)
    depth, seg = cref.render(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms)
    point = np.asarray(cam_pos, dtype=np.float64) + cref.pixel_rays(cam_R, fovy, width, height) * depth[..., None]
    normal = np.zeros((height, width, 3))
    margin = np.full((height, width), np.inf)
    radius = np.full((height, width), np.inf)
    for g in geoms:
        mask = seg == g["id"]
        if not mask.any():
            continue
        Rg = np.asarray(g["mat"], dtype=np.float64).reshape(3, 3)
        p = (point[mask] - np.asarray(g["pos"], dtype=np.float64)) @ Rg  # Rg^T (q - pos)
        n, mg, rad = local_normal(g["type"], np.asarray(g["size"], dtype=np.float64), p, g.get("halfspaces"))
        normal[mask], margin[mask], radius[mask] = n @ Rg.T, mg, rad
    return dict(depth=depth, seg=seg, point=point, normal=normal, margin=margin, radius=radius)

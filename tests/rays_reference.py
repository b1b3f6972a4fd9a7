"""Reference for the device's ray sensors (include/fsim_rays.h), in float64 numpy.

It builds on tests/camera_reference.py (solid_interval: the ray / solid interval of every collision shape) and, for the normal, on
tests/normals_reference.py (local_normal); it shares no code with the device path or furniture_amd.rays.  The observation it defines, per
ray o + t d (|d| = 1): over the geoms that are not skipped, t = t0 >= tmin ? t0 : t1 of the solid's interval, accepted when
tmin <= t <= tmax; the smallest t wins, the first geom on a tie; nothing -> distance -1, geom -1, normal 0.
"""

import numpy as np

from tests import camera_reference as cref
from tests import normals_reference as nref

CLIP_BAND = 1e-4  # metres: near_clip
TILT = 1e-3       # radians: ambiguous


def cast(origin, dirs, geoms, tmin, tmax, skip=()):
    """origin [3], dirs [k, 3] (world, normalised here), geoms as camera_reference.model_geoms gives them, skip: model geom ids the
    sensor does not see -> dict of dist [k] (-1: miss), geom [k] (-1: miss), normal [k, 3] (world, 0: miss), margin [k] and radius [k]
    (normals_reference's, +inf on a miss) and near_clip [k] (bool: the entry t0 of the geom the ray hits lies within CLIP_BAND of tmin, or
    its t within CLIP_BAND of tmax: a rounding error may move that surface point across the bound)."""
    o = np.asarray(origin, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    k = len(d)
    best = np.full(k, np.inf)
    label = np.full(k, -1, dtype=np.int32)
    entry = np.full(k, np.inf)
    skip = set(int(g) for g in skip)
    for g in geoms:
        if int(g["id"]) in skip:
            continue
        Rg = np.asarray(g["mat"], dtype=np.float64).reshape(3, 3)
        og = Rg.T @ (o - np.asarray(g["pos"], dtype=np.float64))
        t0, t1, hit = cref.solid_interval(g["type"], np.asarray(g["size"], dtype=np.float64), og, d @ Rg, g.get("halfspaces"))
        t = np.where(t0 >= tmin, t0, t1)
        ok = hit & (t >= tmin) & (t <= tmax) & (t < best)
        best = np.where(ok, t, best)
        entry = np.where(ok, t0, entry)
        label = np.where(ok, g["id"], label)
    normal = np.zeros((k, 3))
    margin = np.full(k, np.inf)
    radius = np.full(k, np.inf)
    for g in geoms:
        mask = label == g["id"]
        if not mask.any():
            continue
        Rg = np.asarray(g["mat"], dtype=np.float64).reshape(3, 3)
        p = (o + d[mask] * best[mask, None] - np.asarray(g["pos"], dtype=np.float64)) @ Rg
        n, mg, rad = nref.local_normal(g["type"], np.asarray(g["size"], dtype=np.float64), p, g.get("halfspaces"))
        normal[mask], margin[mask], radius[mask] = n @ Rg.T, mg, rad
    near = (label >= 0) & ((np.abs(entry - tmin) <= CLIP_BAND) | (np.abs(best - tmax) <= CLIP_BAND))
    return dict(dist=np.where(label >= 0, best, -1.0), geom=label, normal=normal, margin=margin, radius=radius, near_clip=near)


def _perpendicular(d):
    """two unit vectors [k, 3] each, perpendicular to the unit vectors d [k, 3] and to each other"""
    a = np.where((np.abs(d[:, 0]) < 0.9)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    u = np.cross(d, a)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(d, u)


def ambiguous(origin, dirs, geoms, tmin, tmax, skip=()):
    """[k] bool: rays whose label changes under any of the four tilts of TILT radians about two axes perpendicular to the ray (the
    ray grazes a silhouette, or runs along the seam of two geoms)"""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    base = cast(origin, d, geoms, tmin, tmax, skip)["geom"]
    u, v = _perpendicular(d)
    out = np.zeros(len(d), dtype=bool)
    for axis in (u, v):
        for sign in (1.0, -1.0):
            out |= cast(origin, d * np.cos(TILT) + sign * np.sin(TILT) * axis, geoms, tmin, tmax, skip)["geom"] != base
    return out

"""Reference for the device's signed-distance probes (include/fsim_probes.h), in float64 numpy.

Written from the header's definitions; it shares no code with the device path or furniture_amd.probes.  It takes the geoms as
tests/camera_reference.model_geoms gives them (a hull: the half-spaces of scipy's facets, unmerged).  The observation it defines, per
probe point p: over the geoms that are not skipped, the signed distance of the header (a hull: the plane bound); the smallest wins, the
first geom on a tie; a winner beyond dmax -> distance dmax, geom -1, gradient 0.

It also gives the EXACT distance to a hull (hull_exact_distance: the minimum over the hull's triangles of the point-triangle distance,
negated inside), which the plane bound is compared with.
"""

import numpy as np

from tests import camera_reference as cref

OFFSET = 1e-4      # metres: ambiguous and gradient-unstable are judged under the six offsets of +-OFFSET along the world axes
TURN = 1e-2        # radians: gradient-unstable
RANGE_BAND = 1e-4  # metres: near-range
TINY = 1e-12       # a vector shorter than this has no direction: the geom's local +x (the header's degenerate points)


def _unit(v):
    l = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(l < TINY, np.array([1.0, 0.0, 0.0]), v / np.where(l < TINY, 1.0, l))


def _sign(x):
    return np.where(x < 0, -1.0, 1.0)


def local_distance(gtype, size, q, halfspaces=None):
    """q [k, 3] in the geom frame -> (distance [k], local unit gradient [k, 3], flat [k] bool: the gradient is that of a flat feature --
    a plane, a box face, a cylinder cap, a hull face -- and so one of finitely many vectors)"""
    k = len(q)
    ez = np.array([0.0, 0.0, 1.0])
    if gtype == cref.PLANE:
        return q[:, 2].copy(), np.tile(ez, (k, 1)), np.ones(k, dtype=bool)
    if gtype == cref.SPHERE:
        return np.linalg.norm(q, axis=1) - size[0], _unit(q), np.zeros(k, dtype=bool)
    if gtype == cref.CAPSULE:
        v = q - ez * np.clip(q[:, 2], -size[1], size[1])[:, None]
        return np.linalg.norm(v, axis=1) - size[0], _unit(v), np.zeros(k, dtype=bool)
    if gtype == cref.CYLINDER:
        dr, dz = np.hypot(q[:, 0], q[:, 1]) - size[0], np.abs(q[:, 2]) - size[1]
        rad = _unit(q * np.array([1.0, 1.0, 0.0]))
        cap = ez * _sign(q[:, 2])[:, None]
        inside = (dr <= 0) & (dz <= 0)
        a, b = np.maximum(dr, 0.0), np.maximum(dz, 0.0)
        out = np.hypot(a, b)
        g_out = (rad * a[:, None] + cap * b[:, None]) / np.where(out > 0, out, 1.0)[:, None]
        side = dr >= dz  # the side wins a tie
        g_in = np.where(side[:, None], rad, cap)
        flat = np.where(inside, ~side, a == 0)
        return np.where(inside, np.maximum(dr, dz), out), np.where(inside[:, None], g_in, g_out), flat
    if gtype == cref.BOX:
        a = np.abs(q) - size[None, :3]
        inside = (a <= 0).all(axis=1)
        m = np.maximum(a, 0.0)
        out = np.linalg.norm(m, axis=1)
        g_out = _sign(q) * m / np.where(out > 0, out, 1.0)[:, None]
        ax = np.argmax(a, axis=1)  # (the first maximum: the smallest axis wins a tie)
        g_in = np.zeros((k, 3))
        g_in[np.arange(k), ax] = _sign(q[np.arange(k), ax])
        flat = inside | ((m > 0).sum(axis=1) == 1)
        return np.where(inside, a.max(axis=1), out), np.where(inside[:, None], g_in, g_out), flat
    if gtype == cref.MESH:
        n = np.stack([h[0] for h in halfspaces])
        off = np.array([h[1] for h in halfspaces])
        v = q @ n.T + off[None, :]  # n . x + off <= 0 inside
        i = np.argmax(v, axis=1)    # (the first maximum: the smallest plane index wins a tie)
        return v[np.arange(k), i], n[i], np.ones(k, dtype=bool)
    raise ValueError("geom type %d" % gtype)


def distance(points, geoms, dmax, skip=()):
    """points [k, 3] (world), geoms as camera_reference.model_geoms gives them, skip: model geom ids the sensor does not see -> dict of
    dist [k] (dmax: nothing), geom [k] (-1: nothing), grad [k, 3] (world, 0: nothing), flat [k] (bool, see local_distance), type [k]
    (the winner's geom type, -1: nothing), raw [k] (the winner's distance before dmax is applied; +inf without a geom) and near_range [k]
    (bool: raw within RANGE_BAND of dmax, where a rounding error may move the winner across it)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    k = len(p)
    best = np.full(k, np.inf)
    label = np.full(k, -1, dtype=np.int32)
    gtype = np.full(k, -1, dtype=np.int32)
    grad = np.zeros((k, 3))
    flat = np.zeros(k, dtype=bool)
    skip = set(int(g) for g in skip)
    for g in geoms:
        if int(g["id"]) in skip:
            continue
        Rg = np.asarray(g["mat"], dtype=np.float64).reshape(3, 3)
        q = (p - np.asarray(g["pos"], dtype=np.float64)) @ Rg
        d, gl, fl = local_distance(g["type"], np.asarray(g["size"], dtype=np.float64), q, g.get("halfspaces"))
        ok = d < best
        best = np.where(ok, d, best)
        label = np.where(ok, g["id"], label)
        gtype = np.where(ok, g["type"], gtype)
        grad = np.where(ok[:, None], gl @ Rg.T, grad)
        flat = np.where(ok, fl, flat)
    hit = best <= dmax
    return dict(dist=np.where(hit, best, dmax), geom=np.where(hit, label, -1).astype(np.int32), grad=np.where(hit[:, None], grad, 0.0),
                flat=flat & hit, type=np.where(hit, gtype, -1), raw=best, near_range=np.abs(best - dmax) < RANGE_BAND)


def flags(points, geoms, dmax, skip=()):
    """(ambiguous [k], gradient_unstable [k]) bool: under any of the six offsets of +-OFFSET along the world axes the label changes /
    the reference gradient turns by more than TURN radians (within about 1 cm of an edge, a corner or a small sphere)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    base = distance(p, geoms, dmax, skip)
    amb = np.zeros(len(p), dtype=bool)
    uns = np.zeros(len(p), dtype=bool)
    for a in range(3):
        for sgn in (1.0, -1.0):
            off = np.zeros(3)
            off[a] = sgn * OFFSET
            r = distance(p + off, geoms, dmax, skip)
            amb |= r["geom"] != base["geom"]
            chord = np.linalg.norm(r["grad"] - base["grad"], axis=1)
            uns |= 2.0 * np.arcsin(np.minimum(0.5 * chord, 1.0)) > TURN
    return amb, uns


# ---- the exact distance to a hull ---------------------------------------------------------------------------------------------------
def hull_triangles(vertices):
    """[t, 3, 3]: the triangles of scipy's convex hull of the vertices"""
    from scipy.spatial import ConvexHull
    v = np.asarray(vertices, dtype=np.float64)
    return v[ConvexHull(v).simplices]


def _segment_distance(p, a, b):
    ab = b - a
    t = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * ab), axis=1)


def point_triangle(p, tri):
    """p [k, 3], one triangle [3, 3] -> (distance [k], interior [k] bool: the projection onto the triangle's plane falls strictly inside it)"""
    a, b, c = tri
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n)
    h = (p - a) @ n
    proj = p - h[:, None] * n
    # barycentric signs: the projection is inside when it is on the inner side of all three edges
    s = [np.cross(v1 - v0, proj - v0) @ n for v0, v1 in ((a, b), (b, c), (c, a))]
    scale = np.sqrt(np.linalg.norm(np.cross(b - a, c - a)))
    inside = (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)
    interior = (s[0] > 1e-9 * scale) & (s[1] > 1e-9 * scale) & (s[2] > 1e-9 * scale)
    edge = np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
    return np.where(inside, np.abs(h), edge), interior


def hull_exact_distance(points, vertices, halfspaces):
    """points [k, 3] in the hull's frame -> (signed exact distance [k]: the minimum over the hull's triangles of the point-triangle
    distance, negative inside (all half-spaces hold), interior [k] bool: the nearest triangle is reached at its interior)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    best = np.full(len(p), np.inf)
    interior = np.zeros(len(p), dtype=bool)
    for tri in hull_triangles(vertices):
        d, it = point_triangle(p, tri)
        better = d < best
        best = np.where(better, d, best)
        interior = np.where(better, it, interior)
    n = np.stack([h[0] for h in halfspaces])
    off = np.array([h[1] for h in halfspaces])
    inside = ((p @ n.T + off[None, :]) <= 0).all(axis=1)
    return np.where(inside, -best, best), interior

"""Reference ray caster for the device cameras (include/fsim_camera.h), written from the geometric definitions in float64 numpy.

It shares no code with the device path or furniture_amd.camera: its own pixel rays, its own geom-frame transforms, its own
intersection formulas (the textbook quadratics, slabs and the half-spaces of scipy's hull facets, unmerged).  The observation it
defines: for each pixel, the nearest point of a collision surface on the pixel's ray with znear <= depth <= zfar (depth = distance
along the optical axis); planes are infinite; nothing -> (zfar, -1).
"""

import numpy as np

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = 0, 2, 3, 5, 6, 7


def pixel_rays(R, fovy, width, height, dx=0.0, dy=0.0):
    """World directions [H, W, 3] of the pixel rays of a camera with camera -> world rotation R, scaled so that the optical-axis
    component is 1 (t along them = depth).  dx / dy: sub-pixel offset of the sample point (right / down) in pixels."""
    f = 0.5 * height / np.tan(np.radians(fovy) / 2.0)
    i = np.arange(width) + 0.5 + dx
    j = np.arange(height) + 0.5 + dy
    x = (i[None, :] - width / 2.0) / f
    y = (height / 2.0 - j[:, None]) / f
    d_cam = np.stack(np.broadcast_arrays(x, y, -np.ones_like(x + y)), axis=-1)  # camera looks along -z, +y up
    return d_cam @ np.asarray(R).T


def _quad_interval(a, b, c):
    """t with a t^2 + 2 b t + c <= 0 (a > 0): (t0, t1, hit)"""
    disc = b * b - a * c
    hit = (disc >= 0) & (a > 0)
    sq = np.sqrt(np.where(hit, disc, 0.0))
    a_ = np.where(a > 0, a, 1.0)
    return (-b - sq) / a_, (-b + sq) / a_, hit


def _slab(o, d, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-h - o) / d, (h - o) / d
    par = d == 0
    inside = np.abs(o) <= h
    t0 = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    t1 = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    return t0, t1


def solid_interval(gtype, size, o, d, halfspaces=None):
    """Ray o + t d, in the geom's frame (o [3], d [..., 3]) -> (t0, t1, hit) of the solid; a plane: t0 = t1 = its crossing."""
    shape = d.shape[:-1]
    if gtype == PLANE:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[2] / d[..., 2]
        return t, t, d[..., 2] != 0
    if gtype == SPHERE:
        return _quad_interval((d * d).sum(-1), d @ o, np.full(shape, o @ o - size[0] ** 2))
    if gtype in (CYLINDER, CAPSULE):
        r, h = size[0], size[1]
        a = d[..., 0] ** 2 + d[..., 1] ** 2
        b = d[..., 0] * o[0] + d[..., 1] * o[1]
        c = np.full(shape, o[0] ** 2 + o[1] ** 2 - r * r)
        t0, t1, hit = _quad_interval(a, b, c)
        along = a == 0  # ray parallel to the axis
        t0, t1, hit = np.where(along, -np.inf, t0), np.where(along, np.inf, t1), np.where(along, c <= 0, hit)
        z0, z1 = _slab(o[2], d[..., 2], h)
        t0, t1 = np.maximum(t0, z0), np.minimum(t1, z1)
        hit = hit & (t0 <= t1)
        if gtype == CYLINDER:
            return t0, t1, hit
        t0, t1 = np.where(hit, t0, np.inf), np.where(hit, t1, -np.inf)
        for zc in (h, -h):
            oc = o - np.array([0.0, 0.0, zc])
            s0, s1, sh = _quad_interval((d * d).sum(-1), d @ oc, np.full(shape, oc @ oc - r * r))
            t0, t1 = np.where(sh, np.minimum(t0, s0), t0), np.where(sh, np.maximum(t1, s1), t1)
            hit = hit | sh
        return t0, t1, hit
    if gtype == BOX:
        t0, t1 = np.full(shape, -np.inf), np.full(shape, np.inf)
        for k in range(3):
            a0, a1 = _slab(o[k], d[..., k], size[k])
            t0, t1 = np.maximum(t0, a0), np.minimum(t1, a1)
        return t0, t1, t0 <= t1
    if gtype == MESH:
        t0, t1 = np.full(shape, -np.inf), np.full(shape, np.inf)
        for n, off in halfspaces:  # n . x + off <= 0 inside
            nd = d @ n
            rest = -(off + n @ o)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = rest / nd
            t1 = np.where(nd > 0, np.minimum(t1, t), t1)
            t0 = np.where(nd < 0, np.maximum(t0, t), t0)
            t0 = np.where((nd == 0) & (rest < 0), np.inf, t0)
        return t0, t1, t0 <= t1
    raise ValueError("geom type %d" % gtype)


def mesh_halfspaces(vertices):
    from scipy.spatial import ConvexHull
    eq = ConvexHull(np.asarray(vertices, dtype=np.float64)).equations
    return [(e[:3], e[3]) for e in eq]


def render(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms, dx=0.0, dy=0.0):
    """geoms: iterable of dicts {id, type, size, pos, mat (3 x 3 geom -> world), halfspaces (mesh)} -> (depth [H, W], seg [H, W])"""
    D = pixel_rays(cam_R, fovy, width, height, dx, dy)
    depth = np.full((height, width), np.inf)
    seg = np.full((height, width), -1, dtype=np.int32)
    cam_pos = np.asarray(cam_pos, dtype=np.float64)
    for g in geoms:
        Rg = np.asarray(g["mat"], dtype=np.float64).reshape(3, 3)
        o = Rg.T @ (cam_pos - np.asarray(g["pos"], dtype=np.float64))
        d = D @ Rg
        t0, t1, hit = solid_interval(g["type"], np.asarray(g["size"], dtype=np.float64), o, d, g.get("halfspaces"))
        t = np.where(t0 >= znear, t0, t1)
        ok = hit & (t >= znear) & (t <= zfar) & (t < depth)
        depth = np.where(ok, t, depth)
        seg = np.where(ok, g["id"], seg)
    return np.where(seg >= 0, depth, zfar), seg


def model_geoms(model, geom_xpos, geom_xmat, cursor_offsets=None):
    """The colliding geoms of a compiled model at the given world poses (model geom numbering, e.g. OracleSim.data.geom_xpos)."""
    A = model.arrays
    verts = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3) if "mesh_vert" in A else None
    out = []
    for k, g in enumerate(np.asarray(A["cg_orig"])):
        g = int(g)
        ent = dict(id=g, type=int(A["geom_type"][g]), size=np.asarray(A["geom_size"], dtype=np.float64).reshape(-1, 3)[g],
                   pos=np.asarray(geom_xpos[g], dtype=np.float64), mat=np.asarray(geom_xmat[g], dtype=np.float64).reshape(3, 3))
        if ent["type"] == MESH:
            a, n = int(A["geom_meshadr"][g]), int(A["geom_meshnum"][g])
            ent["halfspaces"] = mesh_halfspaces(verts[a:a + n])
        out.append(ent)
    return out


def silhouette(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms):
    """pixels whose label changes when the sample point moves by half a pixel (left, right, up or down)"""
    _, s0 = render(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms)
    edge = np.zeros_like(s0, dtype=bool)
    for dx, dy in ((0.5, 0), (-0.5, 0), (0, 0.5), (0, -0.5)):
        _, s = render(cam_pos, cam_R, fovy, width, height, znear, zfar, geoms, dx, dy)
        edge |= s != s0
    return edge

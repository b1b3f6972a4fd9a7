"""Seeded case sets of the narrow-phase tests (tests/test_narrowphase.py on the CPU, tests/test_narrowphase_gpu.py on the device): per pair
type and pose mode, N pairs of shapes whose TRUE signed gap (tests/collide_reference.py) is known and lies away from the contact threshold.

Sizes (radii / half extents) 0.02 - 0.15 m, centres up to 1 m from the origin.  The second shape is moved along a direction u until the
reference gap meets a target: half of the cases -10 mm .. -BAND (must touch), half +BAND .. +3 mm above the margin (must not touch), the
margin 0 or 0.001 (the two values of the catalogue).  A case whose placed gap misses its range is dropped at generation (more are drawn than
kept), so no case lies within BAND of the threshold and none is left out of an existence assertion.  The "inside" modes are not moved: the
sphere's centre / the whole small box sits inside the other shape, the gap is whatever the reference says (deeply negative).

Sets are built once per process and pair type (functools.lru_cache), from SEED alone."""
import functools

import numpy as np

from tests import collide_reference as cr
from tests.collide_reference import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE, Shapes

SEED = 20260
BAND = 1.7e-4        # no case has |gap - threshold| below this (a condition of the construction, see the module text of test_narrowphase.py)
N_CASES = 256        # per pair type and mode (hull pairs: N_HULL -- 433 hull vertices per support value)
N_HULL = 96
N_SAMPLED = 16       # of each set, the first N_SAMPLED are evaluated with the full 40 000-direction sampling as well
N_SAMPLED_HULL = 6
FLAT = (0.32, 0.12, 0.02)  # the 0.64 x 0.24 x 0.04 table top

# name: (device pair type PT_*, geom type 1, geom type 2, portal pair, modes)
KINDS = {
    "plane_sphere": (0, PLANE, SPHERE, False, ("generic",)),
    "plane_box": (1, PLANE, BOX, False, ("generic", "parallel", "yaw", "flat")),
    "plane_cyl": (2, PLANE, CYLINDER, False, ("generic", "parallel", "on_side")),
    "sphere_sphere": (3, SPHERE, SPHERE, False, ("generic",)),
    "sphere_box": (4, SPHERE, BOX, False, ("generic", "centre_inside", "flat")),
    "sphere_cyl": (5, SPHERE, CYLINDER, False, ("generic", "centre_inside")),
    "box_box": (6, BOX, BOX, False, ("generic", "parallel", "yaw", "edge_edge", "corner_face", "inside", "flat")),
    "cyl_box": (7, CYLINDER, BOX, True, ("generic", "parallel", "rim_on_face", "on_side", "flat")),
    "cyl_cyl": (8, CYLINDER, CYLINDER, True, ("generic", "parallel", "coaxial")),
    "plane_cap": (9, PLANE, CAPSULE, False, ("generic", "parallel")),
    "plane_mesh": (11, PLANE, MESH, False, ("generic", "parallel")),
    "sphere_cap": (10, SPHERE, CAPSULE, True, ("generic",)),
    "cap_cyl": (10, CAPSULE, CYLINDER, True, ("generic", "parallel")),
    "cap_box": (10, CAPSULE, BOX, True, ("generic", "parallel", "flat")),
    "box_hull": (10, BOX, MESH, True, ("generic", "parallel")),
    "cyl_hull": (10, CYLINDER, MESH, True, ("generic", "parallel")),
}


@functools.lru_cache(maxsize=None)
def hull_vertices():
    """the convex-mesh collider of chair_agne_0010, from the compiled model"""
    from furniture_amd.mjcf.model import load_compiled
    m = load_compiled("Sawyer", "chair_agne_0010")
    g = int(np.nonzero(m.geom_meshnum > 0)[0][0])
    return np.ascontiguousarray(m.mesh_vert[m.geom_meshadr[g]:m.geom_meshadr[g] + m.geom_meshnum[g]], dtype=np.float64)


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


def axis_rotation(axis, angle):
    """(N, 3, 3) rotations about the unit axes (N, 3) by the angles (N,) (Rodrigues); exact for angle 0"""
    axis, angle = np.asarray(axis, dtype=np.float64), np.asarray(angle, dtype=np.float64)
    K = np.zeros((len(angle), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    s, c = np.sin(angle)[:, None, None], np.cos(angle)[:, None, None]
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rbound(S):
    """the bounding radius the model compiler gives a geom (furniture_amd/mjcf/compile.py: _rbound; a hull: its farthest vertex)"""
    s = S.size
    if S.type == SPHERE:
        return s[:, 0].copy()
    if S.type == CAPSULE:
        return s[:, 0] + s[:, 1]
    if S.type == CYLINDER:
        return np.hypot(s[:, 0], s[:, 1])
    if S.type == BOX:
        return np.linalg.norm(s, axis=1)
    if S.type == MESH:
        return np.full(len(S), np.linalg.norm(S.verts, axis=1).max())
    return np.zeros(len(S))


def _sizes(rng, t, n):
    s = rng.uniform(0.02, 0.15, size=(n, 3))
    if t in (SPHERE,):
        s[:, 1:] = 0
    elif t in (CAPSULE, CYLINDER):
        s[:, 2] = 0
    elif t in (PLANE, MESH):
        s[:] = 0
    return s


def _draw(name, mode, n, rng):
    """the poses before the second shape is moved: (A, B at a deeply overlapping start, u or None when the mode is not moved)"""
    pt, t1, t2, portal, _ = KINDS[name]
    verts = hull_vertices() if MESH in (t1, t2) else None
    s1, s2 = _sizes(rng, t1, n), _sizes(rng, t2, n)
    R1, R2 = random_rotations(rng, n), random_rotations(rng, n)
    p1 = rng.uniform(-0.55, 0.55, size=(n, 3))
    u = _unit(rng.normal(size=(n, 3)))
    off = rng.uniform(-0.01, 0.01, size=(n, 3))  # start: centre on centre, give or take 1 cm
    z = np.array([0.0, 0.0, 1.0])
    if mode == "flat":
        if t2 == BOX:
            s2[:] = FLAT
        else:
            s1[:] = FLAT
        if name == "box_box":  # either of the two is the table top
            sw = rng.rand(n) < 0.5
            s1[sw], s2[sw] = s2[sw].copy(), s1[sw].copy()
    if mode == "parallel":
        R2 = R1.copy()
    elif mode == "yaw":  # rotation about the shared face normal (local z of both): exactly 0, 45 and 90 degrees, and anything
        ang = np.deg2rad(np.concatenate([[0.0, 45.0, 90.0] * 8, rng.uniform(0, 180, size=n)])[:n])
        ang[rng.permutation(n)] = ang.copy()
        Rz = axis_rotation(np.tile(z, (n, 1)), ang)
        ex = np.isin(np.rad2deg(ang), (0.0, 90.0))  # exact matrices for the exact angles
        Rz[ex] = np.round(Rz[ex])
        R2 = R1 @ Rz
        u = R1[:, :, 2] * np.where(rng.rand(n) < 0.5, 1.0, -1.0)[:, None]
        if t1 != PLANE:
            off = np.einsum("nij,nj->ni", R1, rng.uniform(-1, 1, size=(n, 3)) * s1 * [0.8, 0.8, 0.0])
    elif mode == "edge_edge":
        # A's edge along local x at the (+y, +z) corner, its outward diagonal nA; B's edge x' across it at the angle phi, B's
        # (-y', -z') corner edge facing A: y' + z' = sqrt(2) nA
        nA = np.tile(np.array([0.0, 1.0, 1.0]) / np.sqrt(2), (n, 1))
        w = np.cross(nA, [1.0, 0.0, 0.0])
        phi = np.deg2rad(rng.uniform(20, 160, size=n))
        xb = np.cos(phi)[:, None] * [1.0, 0.0, 0.0] + np.sin(phi)[:, None] * w
        mb = np.cross(nA, xb)
        Q = np.stack([xb, (nA + mb) / np.sqrt(2), (nA - mb) / np.sqrt(2)], axis=2)
        tilt = axis_rotation(_unit(rng.normal(size=(n, 3))), np.deg2rad(rng.uniform(0, 4, size=n)))
        R2 = R1 @ tilt @ Q
        u = np.einsum("nij,nj->ni", R1, nA)
        off = np.einsum("nij,nj->ni", R1, rng.uniform(-0.5, 0.5, size=(n, 3)) * s1 * [1.0, 0.0, 0.0])
    elif mode == "corner_face":  # B's body diagonal along A's face normal, spun about it, tilted a little
        dg = np.ones(3) / np.sqrt(3)
        ax = _unit(np.cross(dg, z))
        Q0 = axis_rotation(ax[None], np.array([np.arccos(dg @ z)]))[0]  # takes the diagonal to z
        spin = axis_rotation(np.tile(z, (n, 1)), rng.uniform(0, 2 * np.pi, size=n))
        tilt = axis_rotation(_unit(rng.normal(size=(n, 3))), np.deg2rad(rng.uniform(0, 8, size=n)))
        R2 = R1 @ tilt @ spin @ Q0[None]
        u = -R1[:, :, 2]  # B's (+,+,+) corner points along A's +z: B sits below A's -z face ... moved along -z
        off = np.einsum("nij,nj->ni", R1, rng.uniform(-0.6, 0.6, size=(n, 3)) * s1 * [1.0, 1.0, 0.0])
    elif mode == "coaxial":
        flip = rng.rand(n) < 0.5
        R2 = R1.copy()
        R2[flip] = R2[flip] * [1.0, -1.0, -1.0]
        u = R1[:, :, 2] * np.where(rng.rand(n) < 0.5, 1.0, -1.0)[:, None]
        off = np.where(rng.rand(n, 1) < 0.5, 0.0, 1.0) * np.einsum("nij,nj->ni", R1, rng.uniform(-0.01, 0.01, size=(n, 3)) * [1.0, 1.0, 0.0])
        same = rng.rand(n) < 0.3
        s2[same, 0] = s1[same, 0]
    elif mode == "rim_on_face":  # the cylinder's axis 10 - 40 degrees off the box's face normal: its rim meets the face
        tilt = axis_rotation(_unit(rng.normal(size=(n, 3)) * [1.0, 1.0, 0.0] + [1e-9, 0, 0]), np.deg2rad(rng.uniform(10, 40, size=n)))
        R1 = R2 @ tilt
        u = R2[:, :, 2] * np.where(rng.rand(n) < 0.5, 1.0, -1.0)[:, None]
        off = np.einsum("nij,nj->ni", R2, rng.uniform(-0.5, 0.5, size=(n, 3)) * s2 * [1.0, 1.0, 0.0])
    elif mode == "on_side":  # the cylinder's axis exactly in the plane / the box's face
        spin = axis_rotation(np.tile(z, (n, 1)), rng.uniform(0, 2 * np.pi, size=n))
        lay = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # local z -> the face's y
        if t1 == PLANE:
            R2 = R1 @ spin @ lay[None]
        else:
            R1 = R2 @ spin @ lay[None]
            u = R2[:, :, 2] * np.where(rng.rand(n) < 0.5, 1.0, -1.0)[:, None]
            off = np.einsum("nij,nj->ni", R2, rng.uniform(-0.5, 0.5, size=(n, 3)) * s2 * [1.0, 1.0, 0.0])
    elif mode == "centre_inside":  # the sphere's centre inside the box / cylinder: anywhere, or exactly on an axis
        f = rng.uniform(-0.98, 0.98, size=(n, 3))
        if t2 == CYLINDER:
            rad, ang = np.sqrt(rng.rand(n)) * 0.98, rng.uniform(0, 2 * np.pi, size=n)
            loc = np.stack([rad * np.cos(ang) * s2[:, 0], rad * np.sin(ang) * s2[:, 0], f[:, 2] * s2[:, 1]], axis=1)
        else:
            loc = f * s2
        # one in four exactly on the local z axis, near enough to an end face that the way out is along the axis (on the axis every
        # sideways way out is as short as any other: a tie, not a case)
        ax = np.arange(n) % 4 == 0
        zlim = s2[:, 2] if t2 == BOX else s2[:, 1]
        short = 0.3 * (s2.min(axis=1) if t2 == BOX else s2[:, :2].min(axis=1))
        loc[ax, :2] = 0.0
        loc[ax, 2] = (np.where(rng.rand(n) < 0.5, 1.0, -1.0) * (zlim - short))[ax]
        p2 = p1 - np.einsum("nij,nj->ni", R2, loc)
        return Shapes(t1, p1, R1, s1, None), Shapes(t2, p2, R2, s2, None), None
    elif mode == "inside":  # the second box wholly inside the first
        s1, s2 = rng.uniform(0.08, 0.15, size=(n, 3)), rng.uniform(0.02, 0.035, size=(n, 3))
        room = s1 - np.linalg.norm(s2, axis=1, keepdims=True)  # (> 0.019: inside whatever its rotation)
        # off centre along every axis by 20 - 90 % of the room: a box centred on an axis can leave either way, a tie and not a case
        loc = np.where(rng.rand(n, 3) < 0.5, 1.0, -1.0) * rng.uniform(0.2, 0.9, size=(n, 3)) * room
        p2 = p1 + np.einsum("nij,nj->ni", R1, loc)
        par = rng.rand(n) < 0.25
        R2[par] = R1[par]
        return Shapes(t1, p1, R1, s1, None), Shapes(t2, p2, R2, s2, None), None
    if t1 == PLANE:
        u = R1[:, :, 2].copy()
        off = np.einsum("nij,nj->ni", R1, rng.uniform(-0.3, 0.3, size=(n, 3)) * [1.0, 1.0, 0.0])
    return Shapes(t1, p1, R1, s1, verts if t1 == MESH else None), Shapes(t2, p1 + off, R2, s2, verts if t2 == MESH else None), u


@functools.lru_cache(maxsize=None)
def case_set(name, mode):
    """dict: name, mode, pt, t1, t2, portal, A, B (Shapes), margin, touch (the construction's intent = gap <= threshold), gap (the reference's,
    at the placed pose), threshold (margin; 0 for portal pairs: the portal routine has no margin), verts"""
    pt, t1, t2, portal, modes = KINDS[name]
    hull = MESH in (t1, t2)
    n = N_HULL if hull else N_CASES
    rng = np.random.RandomState(SEED + 1000 * sorted(KINDS).index(name) + modes.index(mode))
    nd = n + n // 16 + 6
    A, B, u = _draw(name, mode, nd, rng)
    margin = np.where(rng.rand(nd) < 0.5, 0.0, 0.001)
    thr = np.zeros(nd) if portal else margin
    touch = np.arange(nd) % 2 == 0
    if u is None:
        touch[:] = True
        gap = cr.signed_gap(A, B, ndir=2000, chunk=nd)
        ok = gap < -BAND
    else:
        target = np.where(touch, rng.uniform(-0.010, -BAND - 2e-5, size=nd), margin + rng.uniform(BAND + 2e-5, 0.003, size=nd))
        t = cr.place_at_gap(A, B, u, target)
        B = B.moved(t[:, None] * u)
        gap = cr.signed_gap(A, B, ndir=2000, chunk=nd)
        ok = np.where(touch, (gap >= -0.0105) & (gap <= -BAND), (gap >= np.maximum(margin, thr) + BAND) & (gap <= margin + 0.0035))
    idx = np.nonzero(ok)[0][:n]
    assert len(idx) == n, "%s/%s: only %d of %d drawn cases were placed inside their range" % (name, mode, len(idx), nd)
    A, B = A.take(idx), B.take(idx)
    assert np.abs(np.concatenate([A.pos, B.pos])).max() < 1.0
    return dict(name=name, mode=mode, pt=pt, t1=t1, t2=t2, portal=portal, A=A, B=B, margin=margin[idx], touch=touch[idx], gap=gap[idx], threshold=thr[idx],
                verts=hull_vertices() if hull else None, nsampled=N_SAMPLED_HULL if hull else N_SAMPLED)


def all_sets():
    return [(name, mode) for name in KINDS for mode in KINDS[name][4]]

"""Independent float64 reference for the collision narrow phase: plain numpy, no code shared with the checker (oracle/) or the device.

Every convex shape is known through its support value h(d) = max over the shape of d . x.  For two convex shapes A and B
    signed_gap(A, B) = max over unit d of ( -h_A(d) - h_B(-d) )
is their distance when they are apart (d: the separating direction from A to B) and minus their penetration depth when they overlap
(the shortest translation that separates them).  The maximum is found by sampling the unit sphere and refining the best few samples by a
shrinking pattern search; `separation_along` is the same expression at ONE direction, `point_depth` the closed-form signed distance of a
point to a shape.  The closed forms at the end check the reference itself (tests/test_narrowphase.py, part (a)).

All functions are vectorised over N cases: a `Shapes` holds N shapes of one type."""
import numpy as np

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = 0, 2, 3, 5, 6, 7  # MuJoCo's mjtGeom numbers


class Shapes:
    """N shapes of one type: pos (N, 3), R (N, 3, 3) with the local axes as columns, size (N, 3) in MuJoCo's convention (sphere: r;
    capsule / cylinder: r, half length along local z; box: half extents; plane: the half space below local z = 0), verts (V, 3): the hull's
    vertices in the local frame, shared by the N shapes; planes (F, 4): the hull's face planes (outward unit normal, offset)."""

    def __init__(self, type, pos, R, size, verts=None):
        self.type = int(type)
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        n = len(self.pos)
        self.R = np.array(R, dtype=np.float64).reshape(n, 3, 3)
        self.size = np.array(size, dtype=np.float64).reshape(n, 3)
        self.verts = None if verts is None else np.array(verts, dtype=np.float64).reshape(-1, 3)
        self._planes = None

    def __len__(self):
        return len(self.pos)

    def take(self, idx):
        s = Shapes(self.type, self.pos[idx], self.R[idx], self.size[idx], self.verts)
        s._planes = self._planes
        return s

    def moved(self, delta):
        s = Shapes(self.type, self.pos + delta, self.R, self.size, self.verts)
        s._planes = self._planes
        return s

    @property
    def planes(self):
        if self._planes is None:
            from scipy.spatial import ConvexHull
            eq = ConvexHull(self.verts).equations  # (normal, offset): normal . x + offset <= 0 inside
            self._planes = np.unique(np.round(eq, 12), axis=0)
        return self._planes


def rot_local(S, d):
    """world directions d (N, M, 3) in the shapes' local frames"""
    return np.matmul(d, S.R)  # (R^T d)_i = sum_j d_j R_ji


def support_value(S, d):
    """h_S(d) for world directions d (N, M, 3) (need not be unit: h is homogeneous) -> (N, M).  A plane's half space is unbounded: its
    support value is finite along its own normal only (see signed_gap)."""
    dl = rot_local(S, d)
    r, h = S.size[:, None, 0], S.size[:, None, 1]
    if S.type == SPHERE:
        loc = r * np.linalg.norm(dl, axis=2)
    elif S.type == CAPSULE:
        loc = r * np.linalg.norm(dl, axis=2) + h * np.abs(dl[..., 2])
    elif S.type == CYLINDER:
        loc = r * np.sqrt(dl[..., 0] ** 2 + dl[..., 1] ** 2) + h * np.abs(dl[..., 2])
    elif S.type == BOX:
        loc = (S.size[:, None, :] * np.abs(dl)).sum(axis=2)
    elif S.type == MESH:
        loc = np.empty(dl.shape[:2])
        blk = max(1, int(2e7 // (dl.shape[1] * len(S.verts))))  # (bounds the N x M x V intermediate)
        for i in range(0, len(dl), blk):
            loc[i:i + blk] = (dl[i:i + blk] @ S.verts.T).max(axis=2)
    else:
        raise ValueError("no bounded support value for geom type %d" % S.type)
    return loc + np.matmul(d, S.pos[:, :, None])[..., 0]


def support_point(S, d):
    """a point of S farthest along the unit world directions d (N, M, 3) -> (N, M, 3); d . support_point = support_value"""
    dl = rot_local(S, d)
    r, h = S.size[:, None, 0:1], S.size[:, None, 1]
    sg = np.where(dl >= 0, 1.0, -1.0)
    if S.type == SPHERE:
        pl = r * dl
    elif S.type == CAPSULE:
        pl = r * dl
        pl[..., 2] += h * sg[..., 2]
    elif S.type == CYLINDER:
        rho = np.sqrt(dl[..., 0:1] ** 2 + dl[..., 1:2] ** 2)
        pl = np.concatenate([r * dl[..., :2] / np.maximum(rho, 1e-300), (h * sg[..., 2])[..., None]], axis=2)
    elif S.type == BOX:
        pl = S.size[:, None, :] * sg
    elif S.type == MESH:
        pl = np.empty(dl.shape)
        blk = max(1, int(2e7 // (dl.shape[1] * len(S.verts))))
        for i in range(0, len(dl), blk):
            pl[i:i + blk] = S.verts[(dl[i:i + blk] @ S.verts.T).argmax(axis=2)]
    else:
        raise ValueError("no support point for geom type %d" % S.type)
    return np.matmul(pl, np.swapaxes(S.R, 1, 2)) + S.pos[:, None, :]


def separation_along(A, B, n):
    """(min over B of n . x) - (max over A of n . x) for unit n (N, 3) pointing from A to B: the gap the two shapes leave along n (< 0: they
    overlap along n by that much).  A plane as A is its half space, n must then be the plane's normal."""
    n = np.asarray(n, dtype=np.float64).reshape(-1, 1, 3)
    hb = support_value(B, -n)[:, 0]
    if A.type == PLANE:
        return -hb - np.einsum("nj,nj->n", n[:, 0], A.pos)
    return -support_value(A, n)[:, 0] - hb


def fibonacci_sphere(m):
    i = np.arange(m) + 0.5
    z = 1.0 - 2.0 * i / m
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def _f(A, B, d):
    return -support_value(A, d) - support_value(B, -d)


def _norm(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)


def refine(A, B, d0, rho, iters=18, shrink=0.5):
    """local maximisation on the unit sphere from the start directions d0 (N, S, 3), monotone: the best candidate replaces the current
    direction only when it is better, so the result is never below the start and never above the true maximum.

    The objective is -d . p(d), p(d) = support_point(A, d) - support_point(B, -d) a point of the Minkowski difference.  Its maximum sits on
    ridges (a flat face of either shape makes p jump, a kink of the objective), where a plain pattern search stalls.  Wherever p differs
    between the current direction and a neighbour, e = p_j - p_0 is (for polytopes exactly) an edge of the Minkowski difference and the
    ridge between the two is the great circle d . e = 0.  Candidates per step, patch half width rho (halved per step): the 3 x 3 tangent
    patch; for each of its eight e_j the current direction snapped onto d . e_j = 0 and moved along that circle by +-rho; the crossings
    e_i x e_j of two such circles (a face normal of the Minkowski difference).  Returns (value (N, S), direction (N, S, 3))."""
    N, S, _ = d0.shape
    d = _norm(d0)
    best = _f(A, B, d.reshape(N, S, 3))
    gu, gv = [x.reshape(-1) for x in np.meshgrid([0.0, -1.0, 1.0], [0.0, -1.0, 1.0])]  # (the centre first)
    ii, jj = np.triu_indices(8, 1)
    for _ in range(iters):
        e = np.where(np.abs(d[..., 0:1]) < 0.6, [1.0, 0.0, 0.0], [0.0, 1.0, 0.0])
        u = _norm(np.cross(d, e))
        v = np.cross(d, u)
        c = _norm(d[:, :, None, :] + rho * (gu[None, None, :, None] * u[:, :, None, :] + gv[None, None, :, None] * v[:, :, None, :]))
        cf = c.reshape(N, S * 9, 3)
        p = (support_point(A, cf) - support_point(B, -cf)).reshape(N, S, 9, 3)
        ed = p[:, :, 1:, :] - p[:, :, :1, :]                                     # (N, S, 8, 3)
        en = _norm(ed)
        dc = d[:, :, None, :]
        snap = _norm(dc - en * (en * dc).sum(axis=3, keepdims=True))             # d on the circle d . e = 0 (e = 0: d itself)
        along = _norm(np.cross(snap, en))
        cx = _norm(np.cross(ed[:, :, ii, :], ed[:, :, jj, :]))                   # (N, S, 28, 3)
        cx = np.where((cx * dc).sum(axis=3, keepdims=True) < 0, -cx, cx)
        cx = np.where(np.abs(cx).sum(axis=3, keepdims=True) > 0, cx, dc)
        cand = np.concatenate([c, snap, _norm(snap + rho * along), _norm(snap - rho * along), cx], axis=2)  # 9 + 24 + 28
        C = cand.shape[2]
        val = _f(A, B, cand.reshape(N, S * C, 3)).reshape(N, S, C)
        # (a crossing far outside the patch belongs to another maximum: spread_starts gave that one a start of its own)
        val = np.where((cand * dc).sum(axis=3) > np.cos(4.0 * rho), val, -np.inf)
        k = val.argmax(axis=2)
        vb = np.take_along_axis(val, k[..., None], axis=2)[..., 0]
        db = np.take_along_axis(cand, np.broadcast_to(k[..., None, None], (N, S, 1, 3)), axis=2)[:, :, 0, :]
        up = vb > best
        best = np.where(up, vb, best)
        d = np.where(up[..., None], db, d)
        rho *= shrink
    return best, d


def spread_starts(f0, dirs, nstart, apart=0.3):
    """indices (N, nstart) of the best samples that lie at least `apart` radians from one another: the overlap of two polytopes has one
    local maximum per face of their Minkowski difference, and the best few samples by value alone all sit on the same one"""
    f = f0.copy()
    out = np.zeros((len(f), nstart), dtype=np.int64)
    ca = np.cos(apart)
    for k in range(nstart):
        out[:, k] = f.argmax(axis=1)
        f[dirs[out[:, k]] @ dirs.T > ca] = -np.inf
    return out


def signed_gap(A, B, ndir=40000, nstart=5, chunk=None, with_dir=False):
    """the signed gap of N pairs (see the module text): `ndir` sample directions, the best `nstart` (spread_starts) and the best two of the shapes' own axes refined.  A plane as A: its half space
    has one direction of finite extent, the gap is -h_B(-n) - n . p exactly."""
    N = len(A)
    if A.type == PLANE:
        n = A.R[:, :, 2]
        g = separation_along(A, B, n)
        return (g, n) if with_dir else g
    dirs = fibonacci_sphere(ndir)
    rho = max(2.5 * np.sqrt(4.0 * np.pi / ndir), 0.1)  # 2.5 x the sample spacing, and wide enough to straddle the ridges next to a start
    if chunk is None:
        chunk = max(1, int(4e6 // (ndir * (len(B.verts) // 8 + 1 if B.type == MESH else 1) * (len(A.verts) // 8 + 1 if A.type == MESH else 1))))
    gap, dbest = np.zeros(N), np.zeros((N, 3))
    for i0 in range(0, N, chunk):
        a, b = A.take(slice(i0, i0 + chunk)), B.take(slice(i0, i0 + chunk))
        n = len(a)
        f0 = _f(a, b, np.broadcast_to(dirs, (n, ndir, 3)))
        start = dirs[spread_starts(f0, dirs, nstart)]
        # a shape's own axes are where its support value has its sharpest peaks (a cylinder's axis: a cone a coarse sampling steps over
        # while a whole circle of equal maxima takes every start): the best two of the twelve join the starts
        ax = np.concatenate([a.R, -a.R, b.R, -b.R], axis=2).transpose(0, 2, 1)  # (n, 12, 3): +- the local axes
        top = np.argsort(-_f(a, b, ax), axis=1)[:, :2]
        start = np.concatenate([start, np.take_along_axis(ax, np.broadcast_to(top[..., None], (n, 2, 3)), axis=1)], axis=1)
        val, d = refine(a, b, start, rho)
        k = val.argmax(axis=1)
        gap[i0:i0 + n] = val[np.arange(n), k]
        dbest[i0:i0 + n] = d[np.arange(n), k]
    return (gap, dbest) if with_dir else gap


def place_at_gap(A, B, u, target, ndir=2000, lo=0.0, hi=1.0):
    """B moved along the unit directions u (N, 3) so that signed_gap(A, B + t u) comes close to `target` (N,).  Moving B by t u adds t (u . d)
    to the expression under the maximum, so the gap is a convex, piecewise linear function of t and its slope at t is u . d*(t).  A bisection
    on the sampled maximum (one table of `ndir` values per pair) over [lo, hi] -- the caller starts B deep inside A, where the gap is below
    every target, and B leaves A along u -- brackets t; two Newton steps on a locally refined maximum land it.  The gap a caller reports is
    signed_gap of the placed shapes, never a value from here.  Returns t (N,)."""
    N = len(A)
    target = np.broadcast_to(np.asarray(target, dtype=np.float64), (N,))
    if A.type == PLANE:
        n = A.R[:, :, 2]
        return (target - separation_along(A, B, n)) / np.einsum("nj,nj->n", u, n)
    dirs = fibonacci_sphere(ndir)
    f0 = _f(A, B, np.broadcast_to(dirs, (N, ndir, 3)))
    ud = u @ dirs.T
    a, b = np.full(N, lo), np.full(N, hi)
    for _ in range(26):
        t = 0.5 * (a + b)
        g = (f0 + t[:, None] * ud).max(axis=1)
        up = g < target
        a, b = np.where(up, t, a), np.where(up, b, t)
    t = 0.5 * (a + b)
    rho = max(2.5 * np.sqrt(4.0 * np.pi / ndir), 0.1)
    for _ in range(2):
        top = spread_starts(f0 + t[:, None] * ud, dirs, 2)
        val, d = refine(A, B.moved(t[:, None] * u), dirs[top], rho, iters=10)
        k = val.argmax(axis=1)
        g, d = val[np.arange(N), k], d[np.arange(N), k]
        slope = np.einsum("nj,nj->n", u, d)
        t = t + np.where(slope > 0.05, (target - g) / np.maximum(slope, 0.05), 0.0)
    return t


def point_depth(S, x):
    """signed distance of the world points x (N, K, 3) to the shapes (< 0 inside) -> (N, K).  Closed forms; for a hull the maximum over its face
    planes (exact inside, a lower bound outside)."""
    x = np.asarray(x, dtype=np.float64)
    xl = np.einsum("nji,nkj->nki", S.R, x - S.pos[:, None, :])
    r, h = S.size[:, None, 0], S.size[:, None, 1]
    if S.type == PLANE:
        return xl[..., 2]
    if S.type == SPHERE:
        return np.linalg.norm(xl, axis=2) - r
    if S.type == CAPSULE:
        q = xl.copy()
        q[..., 2] -= np.clip(q[..., 2], -h, h)
        return np.linalg.norm(q, axis=2) - r
    if S.type == CYLINDER:
        a, b = np.hypot(xl[..., 0], xl[..., 1]) - r, np.abs(xl[..., 2]) - h
        return np.hypot(np.maximum(a, 0), np.maximum(b, 0)) + np.minimum(np.maximum(a, b), 0)
    if S.type == BOX:
        q = np.abs(xl) - S.size[:, None, :]
        return np.linalg.norm(np.maximum(q, 0), axis=2) + np.minimum(q.max(axis=2), 0)
    if S.type == MESH:
        P = S.planes
        return (xl @ P[:, :3].T + P[:, 3]).max(axis=2)
    raise ValueError(S.type)


# ---- exact closed forms, to check the reference itself ------------------------------------------------------------------------------------
def gap_sphere_sphere(A, B):
    return np.linalg.norm(B.pos - A.pos, axis=1) - A.size[:, 0] - B.size[:, 0]


def gap_sphere_box(A, B):
    """sphere A, box B; the centre outside the box (distance to it) or inside (minus the way out through the nearest face), minus the radius"""
    return point_depth(B, A.pos[:, None, :])[:, 0] - A.size[:, 0]


def gap_plane(A, B):
    """plane A against any bounded shape B: the lowest point of B over the plane"""
    n = A.R[:, :, 2]
    return -support_value(B, -n[:, None, :])[:, 0] - np.einsum("nj,nj->n", n, A.pos)


def gap_box_box_shared_axis(A, B, k):
    """two boxes with the SAME rotation whose centres differ along their shared axis k only, overlapping in the other two: |d_k| - a_k - b_k"""
    d = np.einsum("nj,nj->n", B.pos - A.pos, A.R[:, :, k])
    return np.abs(d) - A.size[:, k] - B.size[:, k]

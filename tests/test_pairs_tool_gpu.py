"""The per-pair distance routine of the device (furniture_amd/csrc/fsim_gjk.hpp: gjk_pair), case by case: the library's own template,
compiled into the test tool tests/pair_distance_probe.hip, one lane per case, against the independent float64 reference
tests/collide_reference.py on the seeded case sets of tests/narrowphase_cases.py and three small sets drawn here for the type pairs that
catalogue lacks (capsule-capsule, sphere-hull, capsule-hull).

(a) Apart: the non-touching half of each set; B is moved along the reference's own separating direction d by t in T_MOVE, which makes the
    reference gap0 + t exactly.  dist, the separation along the device's normal, the witness points (on their shapes, and to - from =
    dist * normal).
(b) Overlapping: the touching half (gaps -0.0105 .. -1.7e-4).  Cores apart (the reference says so: gap + r1 + r2 > 0; and every plane pair):
    the bound of (a).  Cores intersecting: the portal answer -- negative, never shallower than the true depth, consistent with its own
    normal, and deeper than the true depth by no more than tests/test_narrowphase.py measured for the fp64 portal routine.

Every case of every set is asserted; nothing is left out."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests import collide_reference as cr
from tests import narrowphase_cases as nc
from tests import test_narrowphase as T
from tests.collide_reference import CAPSULE, MESH, PLANE, SPHERE, Shapes
from tests.test_narrowphase_gpu import pack

pytestmark = pytest.mark.gpu
PD_OUTW = 12
BR_PLANE, BR_APART, BR_PORTAL, BR_CAP, BR_NONE = range(5)
T_MOVE = (0.0, 0.05, 0.5)
N_EXTRA = 64
EXTRA = {"cap_cap": (CAPSULE, CAPSULE), "sphere_hull": (SPHERE, MESH), "cap_hull": (CAPSULE, MESH)}

# ---- measured on an MI355X over the cases of this file: every set of every test printed (profiles/pair_a_gpu_tests.txt) ----
# (a) largest |dist - (gap0 + t)|: 5.06e-6 (cap_cyl/generic at t = 0.5, allowed 6.0e-5 there; pairs without a cylinder stay below 1.5e-6).
#     Largest GJK iteration count: 40, the cap, reached by 28 of the 14 208 cases -- all with a cylinder (cyl_box flat 10, parallel 5,
#     rim_on_face 3, generic 1; cyl_cyl coaxial 4, generic 1; cap_cyl 2; cyl_hull 2): a curved rim seen from a face or a rim nearly parallel
#     to it -- and every one of them within the bound; without a cylinder at most 16 (box_hull).
# position tolerance of the witness points: 4 x the largest of |point_depth(A, from)|, |point_depth(B, to)|, |to - from - dist * normal| over
# the cases of (a), never below ULP16
MEASURED_POS = 4.03e-6   # (cyl_box/parallel at t = 0: 4.029e-6; without a cylinder 3.1e-7)
POS_TOL = max(4 * MEASURED_POS, T.ULP16)
# (b) portal pairs: 4 x the largest of (dist - gap)+ and |separation_along(normal) - dist| over the cases of (b), never below ULP16
MEASURED_PORTAL = 7.50e-6  # (cyl_box/flat: |separation - dist| 7.492e-6; shallower than the true depth by at most 1.746e-6, cyl_cyl/parallel; the order of FP32_DIST_PORTAL)
PORTAL_TOL = max(4 * MEASURED_PORTAL, T.ULP16)
# how much deeper than the true depth the portal answer is on the sets PORTAL_OVER_FP64 lacks (recorded, not asserted): box_box generic
# 2.9e-4, parallel 4.1e-4, yaw 4.8e-8, edge_edge 2.3e-3, corner_face 1.6e-4, inside 7.0e-2, flat 3.5e-4; sphere_box centre_inside 9.2e-2;
# sphere_cyl centre_inside 8.2e-2.  (sphere_box flat, sphere_cyl generic: their cores stay apart, no portal case.)


def dist_bound(ref):
    """the project's distance bound for rays and probes"""
    return 1e-4 * np.abs(ref) + 1e-5


def _tool():
    """tests/libpair_distance_probe.so: built by __graft_entry__.build(); compiled on the spot (hipcc, the library's own flags) in a tree that
    does not have it or has an older one than its source or the headers it includes"""
    from tests import pair_distance_tool
    if pair_distance_tool.stale():
        subprocess.check_call(pair_distance_tool.probe_command())
    L = ctypes.CDLL(pair_distance_tool.LIBRARY)
    L.pd_probe_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def tool():
    return _tool()


def device_pairs(tool, sets):
    """one launch over the concatenated case sets -> per set a dict of float64 arrays: d (N,), n, frm, to (N, 3), iters, branch (N,) int"""
    rec, typ = pack(sets)
    n = len(rec)
    verts = np.ascontiguousarray(nc.hull_vertices(), dtype=np.float32) if any(MESH in (cs["t1"], cs["t2"]) for cs in sets) else np.zeros((0, 3), dtype=np.float32)
    out = np.zeros((n, PD_OUTW), dtype=np.float32)
    rc = tool.pd_probe_pairs(rec.ctypes.data, typ.ctypes.data, n, verts.ctypes.data if len(verts) else None, len(verts), out.ctypes.data)
    assert rc == 0, "pd_probe_pairs: HIP error %d" % rc
    res, i0 = [], 0
    for cs in sets:
        o = out[i0:i0 + len(cs["A"])].astype(np.float64)
        res.append(dict(d=o[:, 0], n=o[:, 1:4], frm=o[:, 4:7], to=o[:, 7:10], iters=o[:, 10].astype(int), branch=o[:, 11].astype(int)))
        i0 += len(cs["A"])
    return res


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def extra_set(name):
    """N_EXTRA seeded cases of a type pair the catalogue lacks, in the catalogue's layout: even cases placed at a gap of -10 mm .. -BAND, odd
    ones at +BAND .. +3 mm; the gap is signed_gap(ndir=2000) of the placed shapes"""
    t1, t2 = EXTRA[name]
    n = N_EXTRA + 12
    rng = np.random.RandomState(nc.SEED + 7000 + sorted(EXTRA).index(name))
    verts = nc.hull_vertices()

    def sizes(t):
        s = rng.uniform(0.02, 0.15, size=(n, 3))
        s[:, 1 if t == SPHERE else 2:] = 0
        return s * (0 if t == MESH else 1)
    s1, s2 = sizes(t1), sizes(t2)
    p1 = rng.uniform(-0.55, 0.55, size=(n, 3))
    A = Shapes(t1, p1, nc.random_rotations(rng, n), s1, None)
    B = Shapes(t2, p1 + rng.uniform(-0.01, 0.01, size=(n, 3)), nc.random_rotations(rng, n), s2, verts if t2 == MESH else None)
    u = _unit(rng.normal(size=(n, 3)))
    touch = np.arange(n) % 2 == 0
    target = np.where(touch, rng.uniform(-0.010, -nc.BAND - 2e-5, size=n), rng.uniform(nc.BAND + 2e-5, 0.003, size=n))
    B = B.moved(cr.place_at_gap(A, B, u, target)[:, None] * u)
    gap = cr.signed_gap(A, B, ndir=2000, chunk=n)
    ok = np.where(touch, (gap >= -0.0105) & (gap <= -nc.BAND), (gap >= nc.BAND) & (gap <= 0.0035))
    idx = np.nonzero(ok)[0][:N_EXTRA]
    assert len(idx) == N_EXTRA, "%s: only %d of %d drawn cases were placed inside their range" % (name, len(idx), n)
    return dict(name=name, mode="generic", pt=10, t1=t1, t2=t2, portal=True, A=A.take(idx), B=B.take(idx), margin=np.zeros(N_EXTRA), touch=touch[idx], gap=gap[idx])


def sets_of(name):
    return [extra_set(name)] if name in EXTRA else [nc.case_set(name, mode) for mode in nc.KINDS[name][4]]


def sub(cs, sel, B=None):
    """the cases `sel` of a set, optionally with other second shapes"""
    out = dict(cs)
    out["A"], out["B"], out["margin"] = cs["A"].take(sel), (cs["B"].take(sel) if B is None else B), cs["margin"][sel]
    return out


def radii(S):
    return S.size[:, 0] if S.type in (SPHERE, CAPSULE) else np.zeros(len(S))


def check_exact(where, A, B, ref, got):
    """the assertions of (a) -> (largest distance error, largest position deviation)"""
    bound = dist_bound(ref)
    err = np.abs(got["d"] - ref)
    k = int(np.argmax(err - bound))
    assert (err <= bound).all(), "%s: case %d: dist %.9g, reference %.9g (branch %d, %d iterations)" % (where, k, got["d"][k], ref[k], got["branch"][k], got["iters"][k])
    ln = np.linalg.norm(got["n"], axis=1)
    assert (np.abs(ln - 1.0) <= 1e-5).all(), "%s: a normal of length %.7f" % (where, ln[np.argmax(np.abs(ln - 1.0))])
    sep = cr.separation_along(A, B, _unit(got["n"]))
    k = int(np.argmax(np.abs(sep - got["d"]) - bound))
    assert (np.abs(sep - got["d"]) <= bound).all(), "%s: case %d: the shapes leave %.9g along the device's normal, dist is %.9g" % (where, k, sep[k], got["d"][k])
    da, db = np.abs(cr.point_depth(A, got["frm"][:, None, :])[:, 0]), np.abs(cr.point_depth(B, got["to"][:, None, :])[:, 0])
    dv = np.linalg.norm(got["to"] - got["frm"] - got["d"][:, None] * got["n"], axis=1)
    pos = max(da.max(), db.max(), dv.max())
    print("%s: from off A by at most %.3e, to off B by %.3e, |to - from - dist * normal| %.3e" % (where, da.max(), db.max(), dv.max()))
    assert pos <= POS_TOL, "%s: witness points: from is %.3e off A, to %.3e off B, to - from - dist * normal %.3e (allowed %.3e)" % (where, da.max(), db.max(), dv.max(), POS_TOL)
    return float(err.max()), float(pos)


ALL = list(nc.KINDS) + list(EXTRA)


@pytest.mark.parametrize("name", ALL)
def test_apart_pairs_match_the_reference(name, tool):
    worst_d = worst_p = 0.0
    iters = 0
    for cs in sets_of(name):
        far = np.nonzero(~cs["touch"])[0]
        if len(far) == 0:  # (the "inside" modes hold overlapping cases only)
            continue
        A, B0 = cs["A"].take(far), cs["B"].take(far)
        gap0, d = cr.signed_gap(A, B0, ndir=2000, chunk=len(far), with_dir=True)
        moved = [B0.moved(t * d) for t in T_MOVE]
        for t, B, got in zip(T_MOVE, moved, device_pairs(tool, [sub(cs, far, B) for B in moved])):
            where = "%s/%s t=%g" % (name, cs["mode"], t)
            assert np.isin(got["branch"], (BR_PLANE, BR_APART, BR_CAP)).all(), "%s: an apart pair went to the portal routine (branches %s)" % (where, np.unique(got["branch"]))
            e, p = check_exact(where, A, B, gap0 + t, got)
            worst_d, worst_p, iters = max(worst_d, e), max(worst_p, p), max(iters, int(got["iters"].max()))
            print("%s: dist error %.3e, witness points %.3e, at most %d iterations, %d cases at the iteration cap" % (where, e, p, got["iters"].max(), (got["branch"] == BR_CAP).sum()))
    print("%s apart: largest dist error %.3e, largest position deviation %.3e (allowed %.3e), at most %d iterations" % (name, worst_d, worst_p, POS_TOL, iters))


@pytest.mark.parametrize("name", ALL)
def test_overlapping_pairs_match_the_reference(name, tool):
    worst = 0.0
    sets = sets_of(name)
    for cs, got_all in zip(sets, device_pairs(tool, sets)):
        where = "%s/%s" % (name, cs["mode"])
        tch = np.nonzero(cs["touch"])[0]
        A, B, gap = cs["A"].take(tch), cs["B"].take(tch), cs["gap"][tch]
        got = {k: v[tch] for k, v in got_all.items()}
        core = gap + radii(A) + radii(B)  # the signed gap of the cores
        assert (np.abs(core) > 1e-5).all() or cs["t1"] == PLANE, "%s: a case whose cores just touch" % where
        exact = np.full(len(tch), True) if cs["t1"] == PLANE else core > 0
        if exact.any():
            i = np.nonzero(exact)[0]
            assert np.isin(got["branch"][i], (BR_PLANE, BR_APART, BR_CAP)).all(), "%s: cores apart, yet the portal routine answered" % where
            e, p = check_exact(where + " (cores apart)", A.take(i), B.take(i), gap[i], {k: v[i] for k, v in got.items()})
            print("%s: %d overlapping cases with their cores apart: dist error %.3e, witness points %.3e" % (where, len(i), e, p))
        if (~exact).any():
            i = np.nonzero(~exact)[0]
            d, g, n = got["d"][i], gap[i], _unit(got["n"][i])
            assert (got["branch"][i] == BR_PORTAL).all(), "%s: cores intersecting, yet branches %s" % (where, np.unique(got["branch"][i]))
            assert (d < 0).all(), "%s: a portal answer that is not negative" % where
            sep = cr.separation_along(A.take(i), B.take(i), n)
            shallow, incons, over = float((d - g).max()), float(np.abs(sep - d).max()), float((g - d).max())
            worst = max(worst, shallow, incons)
            known = (name, cs["mode"]) in T.PORTAL_OVER_FP64
            print("%s: %d portal cases: shallower than the true depth by at most %.3e, |separation along the normal - dist| %.3e (allowed %.3e); deeper than the true depth by at most %.3e (%s)"
                  % (where, len(i), shallow, incons, PORTAL_TOL, over, "fp64 portal: %.3e" % T.PORTAL_OVER_FP64[name, cs["mode"]] if known else "not in PORTAL_OVER_FP64: recorded only"))
            assert shallow <= PORTAL_TOL, "%s: dist is shallower than the true depth by %.3e" % (where, shallow)
            assert incons <= PORTAL_TOL, "%s: dist differs from the separation along its own normal by %.3e" % (where, incons)
            ln = np.linalg.norm(got["n"][i], axis=1)
            assert (np.abs(ln - 1.0) <= 1e-5).all()
            dv = np.linalg.norm(got["to"][i] - got["frm"][i] - d[:, None] * got["n"][i], axis=1)
            assert dv.max() <= POS_TOL, "%s: to - from - dist * normal %.3e" % (where, dv.max())
            if known:
                assert over <= T.PORTAL_OVER_FP64[name, cs["mode"]] + PORTAL_TOL, "%s: deeper than the true depth by %.3e" % (where, over)
    print("%s overlapping: largest portal deviation %.3e (allowed %.3e)" % (name, worst, PORTAL_TOL))

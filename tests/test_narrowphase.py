"""The collision narrow phase, pair by pair, against exact geometry -- the CPU side.

(a) the independent float64 reference (tests/collide_reference.py: support functions, sampled + refined signed gap) against closed forms;
(b) the fp64 checker's per-pair entry osim_narrowphase (oracle/fsim_oracle.c: the dispatch collide() itself runs) against that reference;
(c) the fp32 control build of the same source (oracle/libfsim_cpu32.so) against the fp64 build: what fp32 arithmetic alone does to a
    contact.  The device tolerances of tests/test_narrowphase_gpu.py are multiples of what is measured here.

The case sets are tests/narrowphase_cases.py's.  The constants below are MEASUREMENTS of something other than the device; each test asserts
that its measurement stays within the constant, the GPU tests import them.

BAND (narrowphase_cases.BAND = 1.7e-4) is a condition of the construction, not a measurement: no case lies closer to the contact threshold.
It is four times FP32_DIST_PORTAL, the largest fp32 distance deviation measured in (c) (4.2e-5: more than the 2.5e-5 a band of 1e-4 allows)."""
import numpy as np
import pytest

from oracle import oracle_sim
from tests import collide_reference as cr
from tests import narrowphase_cases as nc
from tests.collide_reference import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE, Shapes

FS_PAIR_MAXCON = [1, 4, 4, 1, 1, 1, 8, 1, 1, 2, 1, 4]  # furniture_amd/csrc/fsim_collide.hpp, by PT_*

# ---- measured constants (seed narrowphase_cases.SEED = 20260; "all sets" = every (pair type, mode) of narrowphase_cases.KINDS, 256 cases
# each, 96 for the hull pairs) -----------------------------------------------------------------------------------------------------------
# (a) the reference's own error: |signed_gap - closed form| over test_reference_matches_closed_forms' 3 x 128 cases (sphere-sphere, sphere-box
#     outside and inside, box-box along a shared axis), at the 2 000 directions the case sets are placed with and at 40 000.
#     Measured maximum 4.1e-14.
REF_GAP_ERR = 1e-12
# (a') |gap at 2 000 directions - gap at 40 000 directions| on the first 16 (hulls: 6) cases of all sets.  Measured maximum 8.7e-9
#     (sphere_cyl; every other type below 3e-13).
REF_SAMPLING_ERR = 2e-8
# (b) the fp64 checker against the reference.  Closed-form types: |deepest dist - gap|, all sets.  Measured maximum 1.2e-11 (sphere_cyl).
#     (box_box: beyond box_box_slack, the documented preference for the face manifold.)
CHECKER_GAP_ERR = 1e-10
#     Portal pairs: how much MORE penetration than the true depth the portal routine reports (gap - deepest dist), per set: the measured
#     maximum of each (pair type, mode), rounded up to two digits.  It reports the distance to the face of the Minkowski difference that the
#     centre line leaves through, not to the nearest one -- cyl_cyl/parallel: two parallel cylinders side by side, 9 mm into each other
#     sideways, whose centres differ mostly along the axis, are reported 28 mm deep, through the end cap.  (0: measured below 1e-12.)
PORTAL_OVER_FP64 = {
    ("cyl_box", "generic"): 3.1e-4, ("cyl_box", "parallel"): 3.9e-4, ("cyl_box", "rim_on_face"): 1.1e-5, ("cyl_box", "on_side"): 0.0, ("cyl_box", "flat"): 1.9e-3,
    ("cyl_cyl", "generic"): 4.2e-4, ("cyl_cyl", "parallel"): 1.9e-2, ("cyl_cyl", "coaxial"): 0.0,
    ("sphere_cap", "generic"): 1.6e-4, ("cap_cyl", "generic"): 4.1e-4, ("cap_cyl", "parallel"): 1.1e-4,
    ("cap_box", "generic"): 6.1e-4, ("cap_box", "parallel"): 7.8e-4, ("cap_box", "flat"): 8.1e-4,
    ("box_hull", "generic"): 1.2e-3, ("box_hull", "parallel"): 3.1e-3, ("cyl_hull", "generic"): 1.4e-3, ("cyl_hull", "parallel"): 7.5e-7,
}
#     It never reports LESS penetration than the true depth, and its dist never differs from the separation along its own normal, by more
#     than 1.0e-7 measured (9.997e-8, cap_cyl/generic; its stopping rule is 1e-7).
PORTAL_UNDER_FP64 = 1e-7
# (c) the fp32 control build against fp64, contacts matched by nearest position, cases where both builds list the same number of contacts
#     (all but 10 plane_mesh cases, where the tilted "down" directions pick another vertex of a flat hull face in fp32).
#     Closed-form types, all sets: measured maxima dist 1.28e-7 (box_box), normal 1.31e-6 (sphere_cyl), position 5.4e-7 (box_box; plane_mesh
#     is left out of the position figure: the vertices it picks are a discrete choice, its position is checked by containment).
FP32_DIST_CLOSED = 1.3e-7
FP32_NORMAL_CLOSED = 1.4e-6
FP32_POS_CLOSED = 5.5e-7
#     Portal pairs, all portal sets: measured maxima dist 4.12e-5 (cap_box), normal 6.63e-3 (cyl_box).  The position is not compared: it
#     moved by up to 9.4e-2 on parallel faces, where it is ill-conditioned.
FP32_DIST_PORTAL = 4.2e-5
FP32_NORMAL_PORTAL = 6.7e-3
ULP16 = 16 * 2.0 ** -23  # 16 ulp of the largest coordinate (1 m): the floor of every device tolerance


def checker(cs, dtype=np.float64, sel=slice(None)):
    """osim_narrowphase over a case set -> (count (N,), contacts (N, 16, 7))"""
    A, B = cs["A"].take(sel), cs["B"].take(sel)
    return oracle_sim.narrowphase(cs["t1"], A.pos, A.R, A.size, cs["t2"], B.pos, B.R, B.size, cs["margin"][sel],
                                  verts1=cs["verts"] if cs["t1"] == MESH else None, verts2=cs["verts"] if cs["t2"] == MESH else None, dtype=dtype)


def match_contacts(ca, cb):
    """cb's contacts reordered so that each of ca's meets its nearest by position (greedy; both (K, 7))"""
    left = list(range(len(cb)))
    order = []
    for c in ca:
        j = min(left, key=lambda k: float(np.sum((cb[k, 1:4] - c[1:4]) ** 2)))
        left.remove(j)
        order.append(j)
    return cb[order]


def compare_builds(cs, cnt_a, con_a, cnt_b, con_b):
    """max deviations (dist, normal, position) over the cases where both list the same number of contacts, and the indices where they do not"""
    dev = np.zeros(3)
    for i in np.nonzero((cnt_a == cnt_b) & (cnt_a > 0))[0]:
        a = con_a[i, :cnt_a[i]]
        b = match_contacts(a, con_b[i, :cnt_b[i]])
        dev = np.maximum(dev, [np.abs(a[:, 0] - b[:, 0]).max(), np.abs(a[:, 4:7] - b[:, 4:7]).max(), np.abs(a[:, 1:4] - b[:, 1:4]).max()])
    return dev, np.nonzero(cnt_a != cnt_b)[0]


def box_box_slack(gap):
    """np_box_box / box_box keep the face manifold unless the best edge axis beats the best face axis by 1e-6 + 5 % of its depth (a rule
    against jitter between the two, MuJoCo's): with the true gap on an edge axis, the face axis kept may be deeper than the gap by that."""
    return (0.05 * np.abs(gap) + 1e-6) / 0.95


def check_against_reference(cs, cnt, con, tol_gap_lo, tol_gap_hi, tol_geom, who):
    """the assertions of (b), shared with the device test: existence, deepest dist against the gap, dist against the separation along the
    contact's own normal, unit normal from geom 1 to geom 2, positions inside both shapes to |dist| / 2, manifold size.
    tol_gap_lo / tol_gap_hi: how much deeper / shallower than the true gap the deepest dist may be.  Returns (max gap - deepest, max deepest - gap)."""
    A, B, gap, name = cs["A"], cs["B"], cs["gap"], "%s/%s %s" % (cs["name"], cs["mode"], who)
    expect = gap < 0 if cs["portal"] else gap <= cs["margin"]
    assert np.array_equal(expect, cs["touch"]), name  # (the construction: no case between the two)
    bad = np.nonzero((cnt > 0) != expect)[0]
    assert len(bad) == 0, "%s: contact / no contact differs from the reference gap at cases %s (gap %s, margin %s)" % (name, bad[:8], gap[bad[:8]], cs["margin"][bad[:8]])
    assert cnt.max() <= FS_PAIR_MAXCON[cs["pt"]], name
    hit = np.nonzero(cnt > 0)[0]
    K = int(cnt.max())
    act = np.arange(K)[None, :] < cnt[hit, None]
    c = con[hit, :K]
    dist, pos, n = c[..., 0], c[..., 1:4], c[..., 4:7]
    assert np.abs(np.linalg.norm(n, axis=2) - 1)[act].max() < max(tol_geom, 1e-9) * 4, name
    deepest = np.where(act, dist, np.inf).min(axis=1)
    over, under = gap[hit] - deepest, deepest - gap[hit]
    tol_gap_lo, tol_gap_hi = np.broadcast_to(tol_gap_lo, gap.shape)[hit], np.broadcast_to(tol_gap_hi, gap.shape)[hit]
    assert (over - tol_gap_lo).max() <= 0, "%s: deepest dist %.3e below the true gap beyond the allowed %.3e" % (name, (over - tol_gap_lo).max(), tol_gap_lo.min())
    assert (under - tol_gap_hi).max() <= 0, "%s: deepest dist %.3e above the true gap beyond the allowed %.3e" % (name, (under - tol_gap_hi).max(), tol_gap_hi.min())
    Ah, Bh = A.take(hit), B.take(hit)
    for k in range(K):
        a = act[:, k]
        if not a.any():
            continue
        nk = np.where(a[:, None], n[:, k], [0.0, 0.0, 1.0])
        sep = cr.separation_along(Ah, Bh, nk)  # (a plane's normal IS its direction: nk equals it or the next assertion fails)
        if cs["t1"] == PLANE:
            assert np.abs(nk - Ah.R[:, :, 2])[a].max() <= max(tol_geom, 1e-9) * 4, name
        # no contact is deeper than the two shapes overlap along its own normal; the normal points from geom 1 to geom 2 (along -n the
        # shapes "overlap" by their whole extent, which this would show as centimetres)
        lo = (sep - dist[:, k] - tol_gap_hi)[a].max()
        assert lo <= tol_geom, "%s: contact %d lies %.3e deeper than the overlap along its normal" % (name, k, lo)
        if cs["name"] == "box_box" or cs["portal"]:  # one normal per pair, the pair's best axis: the separation along it is the gap
            # (box_box: from both sides.  Portal pairs: gap - dist <= lo and |dist - sep| <= hi, hence gap - sep <= lo + hi; sep <= gap holds
            #  for any direction and would test the reference, not the routine)
            e = max((gap[hit] - sep - tol_gap_lo)[a].max(), (sep - gap[hit] - tol_gap_hi)[a].max()) if cs["name"] == "box_box" else (gap[hit] - sep - tol_gap_lo - tol_gap_hi)[a].max()
            assert e <= 0, "%s: the separation along the contact normal misses the gap by %.3e more than allowed" % (name, e)
        if cs["portal"]:  # ... and the portal's dist IS the separation along its normal
            e = (np.abs(sep - dist[:, k]) - tol_gap_hi)[a].max()
            assert e <= 0, "%s: dist differs from the separation along the contact normal by %.3e more than allowed" % (name, e)
        for S in (Ah, Bh):
            d = cr.point_depth(S, pos[:, k][:, None, :])[:, 0]
            worst = (d - 0.5 * np.abs(dist[:, k]))[a].max()
            assert worst <= tol_geom, "%s: contact %d position %.3e outside geom type %d beyond |dist| / 2" % (name, k, worst, S.type)
    return (over - (box_box_slack(gap[hit]) if cs["name"] == "box_box" else 0.0)).max(), under.max()


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------------
def _closed_form_cases(rng, n=128):
    R1, R2 = nc.random_rotations(rng, n), nc.random_rotations(rng, n)
    p1 = rng.uniform(-0.5, 0.5, size=(n, 3))
    s = lambda: rng.uniform(0.02, 0.15, size=(n, 3))
    out = []
    d = nc._unit(rng.normal(size=(n, 3))) * rng.uniform(0.0, 0.3, size=(n, 1))
    A, B = Shapes(SPHERE, p1, R1, s()), Shapes(SPHERE, p1 + d, R2, s())
    out.append(("sphere-sphere", A, B, cr.gap_sphere_sphere(A, B)))
    loc = rng.uniform(-0.3, 0.3, size=(n, 3))
    loc[::2] = rng.uniform(-1, 1, size=(n // 2, 3)) * 0.15  # half of them near or inside the box
    B = Shapes(BOX, p1, R2, s())
    A = Shapes(SPHERE, p1 + np.einsum("nij,nj->ni", R2, loc), R1, s())
    out.append(("sphere-box", A, B, cr.gap_sphere_box(A, B)))
    k = 2
    A = Shapes(BOX, p1, R1, s())
    B = Shapes(BOX, p1, R1, s())
    lat = rng.uniform(-0.3, 0.3, size=(n, 3)) * np.minimum(A.size, B.size) * [1.0, 1.0, 0.0]
    dz = (A.size[:, k] + B.size[:, k]) + rng.uniform(-0.01, 0.02, size=n)
    B = B.moved(np.einsum("nij,nj->ni", R1, lat + np.stack([0 * dz, 0 * dz, dz], axis=1)))
    out.append(("box-box along a shared axis", A, B, cr.gap_box_box_shared_axis(A, B, k)))
    return out


def test_reference_matches_closed_forms():
    rng = np.random.RandomState(nc.SEED)
    worst = 0.0
    for name, A, B, exact in _closed_form_cases(rng):
        for ndir in (2000, 40000):
            err = np.abs(cr.signed_gap(A, B, ndir=ndir) - exact).max()
            print("reference vs closed form, %s, %d directions: %.3e" % (name, ndir, err))
            worst = max(worst, err)
            assert err <= REF_GAP_ERR, (name, ndir, err)
    # plane against anything: the lowest of the shape's own points, written out per type
    n = 128
    P = Shapes(PLANE, rng.uniform(-0.5, 0.5, size=(n, 3)), nc.random_rotations(rng, n), np.zeros((n, 3)))
    nrm = P.R[:, :, 2]
    B = Shapes(BOX, rng.uniform(-0.5, 0.5, size=(n, 3)), nc.random_rotations(rng, n), rng.uniform(0.02, 0.15, size=(n, 3)))
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    cw = B.pos[:, None, :] + np.einsum("nij,nkj->nki", B.R, corners[None] * B.size[:, None, :])
    exact = np.einsum("nkj,nj->nk", cw - P.pos[:, None, :], nrm).min(axis=1)
    assert np.abs(cr.signed_gap(P, B) - exact).max() < 1e-12 and np.abs(cr.gap_plane(P, B) - exact).max() < 1e-12
    S = Shapes(SPHERE, B.pos, B.R, B.size)
    assert np.abs(cr.signed_gap(P, S) - (np.einsum("nj,nj->n", S.pos - P.pos, nrm) - S.size[:, 0])).max() < 1e-12
    H = Shapes(MESH, B.pos, B.R, np.zeros((n, 3)), nc.hull_vertices())
    hw = H.pos[:, None, :] + np.einsum("nij,kj->nki", H.R, H.verts)
    assert np.abs(cr.signed_gap(P, H) - np.einsum("nkj,nj->nk", hw - P.pos[:, None, :], nrm).min(axis=1)).max() < 1e-12
    # point_depth of a hull: zero (to rounding) at its own vertices, negative at its centroid
    assert np.abs(cr.point_depth(H.take(slice(0, 1)), hw[:1])).max() < 1e-9
    assert cr.point_depth(H.take(slice(0, 1)), hw[:1].mean(axis=1, keepdims=True))[0, 0] < -1e-3
    print("MEASURED REF_GAP_ERR %.3e" % worst)


@pytest.mark.parametrize("name", [k for k in nc.KINDS if nc.KINDS[k][1] != PLANE])  # (a plane's gap is a closed form, not sampled)
def test_placed_gap_agrees_with_the_full_sampling(name):
    """the gap the case sets carry (2 000 directions) against 40 000 directions on a subset: a missed maximum would show as a jump"""
    worst = 0.0
    for mode in nc.KINDS[name][4]:
        cs = nc.case_set(name, mode)
        sel = slice(0, cs["nsampled"])
        worst = max(worst, np.abs(cr.signed_gap(cs["A"].take(sel), cs["B"].take(sel), ndir=40000) - cs["gap"][sel]).max())
    print("MEASURED REF_SAMPLING_ERR %s %.3e" % (name, worst))
    assert worst <= REF_SAMPLING_ERR


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nc.KINDS))
def test_checker_pairs_match_the_reference(name):
    """Portal pairs: np_mpr / mpr_convex take no margin -- such a pair is a contact iff the true gap is below 0, whatever margin its geoms carry
    (Baxter's pedestal pairs carry 0.001); pinned here for the checker and in the GPU test for the device."""
    portal = nc.KINDS[name][3]
    over = under = 0.0
    for mode in nc.KINDS[name][4]:
        cs = nc.case_set(name, mode)
        cnt, con = checker(cs)
        ref = REF_GAP_ERR + REF_SAMPLING_ERR
        lo = (PORTAL_OVER_FP64[name, mode] if portal else CHECKER_GAP_ERR) + ref + (box_box_slack(cs["gap"]) if name == "box_box" else 0.0)
        o, u = check_against_reference(cs, cnt, con, lo, (PORTAL_UNDER_FP64 if portal else CHECKER_GAP_ERR) + ref, 1e-9, "fp64 checker")
        over, under = max(over, o), max(under, u)
        print("MEASURED %s/%s: deepest dist below the gap by %.3e, above it by %.3e" % (name, mode, o, u))
    print("MEASURED %s %s: deepest dist below the gap by at most %.3e, above it by at most %.3e" % ("PORTAL" if portal else "CHECKER_GAP_ERR", name, over, under))


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nc.KINDS))
def test_fp32_control_build_against_fp64(name):
    portal = nc.KINDS[name][3]
    dev, nmis, ntot = np.zeros(3), 0, 0
    for mode in nc.KINDS[name][4]:
        cs = nc.case_set(name, mode)
        c64, k64 = checker(cs)
        c32, k32 = checker(cs, np.float32)
        d, mis = compare_builds(cs, c64, k64, c32, k32)
        dev, nmis, ntot = np.maximum(dev, d), nmis + len(mis), ntot + len(c64)
        # existence never differs: every case is BAND away from the threshold
        assert np.array_equal(c64 > 0, c32 > 0), (name, mode, np.nonzero((c64 > 0) != (c32 > 0))[0][:8])
    print("MEASURED FP32 %s: dist %.3e normal %.3e pos %.3e; contact count differs in %d of %d cases" % (name, dev[0], dev[1], dev[2], nmis, ntot))
    if portal:
        assert dev[0] <= FP32_DIST_PORTAL and dev[1] <= FP32_NORMAL_PORTAL, dev
    else:
        assert dev[0] <= FP32_DIST_CLOSED and dev[1] <= FP32_NORMAL_CLOSED and (dev[2] <= FP32_POS_CLOSED or name == "plane_mesh"), dev


def test_per_pair_entry_runs_clean_under_asan_and_ubsan(tmp_path):
    """osim_narrowphase and the routines below it, built with -fsanitize=address,undefined into a stand-alone program
    (tests/narrowphase_san_main.c + oracle/fsim_oracle.c) and run over 16 cases of every set: no report, and bit for bit the contacts the
    shared library gives."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "narrowphase_san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    (tmp_path / "trivial.c").write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc"] + san + ["-o", str(tmp_path / "trivial"), str(tmp_path / "trivial.c")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "trivial")]).returncode != 0:
        pytest.skip("this gcc cannot build or run a sanitized program: " + r.stderr[-200:])
    r = subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
                        os.path.join(root, "tests", "narrowphase_san_main.c"), os.path.join(root, "oracle", "fsim_oracle.c"), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    sel = slice(0, 16)
    for name, mode in nc.all_sets():
        cs = nc.case_set(name, mode)
        A, B = cs["A"].take(sel), cs["B"].take(sel)
        n = len(A)
        verts = cs["verts"] if cs["verts"] is not None else np.zeros((0, 3))
        rec = np.concatenate([A.pos, A.R.reshape(n, 9), A.size, B.pos, B.R.reshape(n, 9), B.size, cs["margin"][sel, None]], axis=1)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([n, cs["t1"], cs["t2"], len(verts)], dtype=np.int32).tobytes() + np.ascontiguousarray(verts, dtype=np.float64).tobytes() + np.ascontiguousarray(rec).tobytes())
        p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, (name, mode, p.stderr[-3000:])
        got = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), dtype=np.dtype([("cnt", np.int32), ("con", np.float64, (16, 7))]))
        cnt, con = checker(cs, sel=sel)
        assert np.array_equal(got["cnt"], cnt), (name, mode)
        for i in range(n):
            assert np.array_equal(got["con"][i, :cnt[i]], con[i, :cnt[i]]), (name, mode, i)


def test_swapped_pair_gives_the_mirrored_contact():
    """osim_narrowphase orders the pair by type itself: the geoms passed the other way round give the same contacts with the normal negated
    (it points from the geom passed first to the geom passed second)"""
    for name, mode in (("sphere_box", "generic"), ("cyl_box", "generic"), ("plane_mesh", "generic")):
        cs = nc.case_set(name, mode)
        sel = slice(0, 32)
        A, B = cs["A"].take(sel), cs["B"].take(sel)
        cnt, con = checker(cs, sel=sel)
        c2, k2 = oracle_sim.narrowphase(cs["t2"], B.pos, B.R, B.size, cs["t1"], A.pos, A.R, A.size, cs["margin"][sel],
                                        verts1=cs["verts"] if cs["t2"] == MESH else None, verts2=cs["verts"] if cs["t1"] == MESH else None)
        assert cnt.sum() > 0 and np.array_equal(cnt, c2)
        assert np.array_equal(con[..., :4], k2[..., :4]) and np.array_equal(con[..., 4:], -k2[..., 4:])


def test_maxcon_table_is_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "furniture_amd", "csrc", "fsim_collide.hpp")).read()
    m = re.search(r"FS_PAIR_MAXCON\[12\]\s*=\s*\{([^}]*)\}", src)
    assert m and [int(x) for x in m.group(1).split(",")] == FS_PAIR_MAXCON


def test_band_covers_the_fp32_deviation():
    assert nc.BAND >= 4 * max(FP32_DIST_PORTAL, FP32_DIST_CLOSED)

"""Generate tests/golden/cone_states.npz: the states on which tests/test_conerows_gpu.py judges ONE Newton solve of the device against float64 where
its contact rows stand on the impedance curve, in every zone of the friction cone, at impact and sliding speed (the table of
tests/conerows_reference.py).

CPU only: every state is constructed here and judged with the checker (OracleSim in float64, its float32 control build and
oracle/libfsim_cpu32.so), never with the device, so the file can be regenerated and held to this script anywhere
(tests/test_conerows.py::test_generator_reproduces_the_file).  A part is put at a chosen depth by bisecting the height of its free joint (a finger:
its slide, an arm: one joint) on the oracle's own contact distances.  Every state is stored as float32 and must then meet
solve_reference.conditions, the zone conditions of conerows_reference and what its recipe asks for; a state that fails is replaced here, with the
next seed; nothing is skipped when the tests run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from furniture_amd import transform_utils as T  # noqa: E402
from oracle.oracle_sim import OracleSim  # noqa: E402
from tests import conerows_reference as cr  # noqa: E402
from tests import contacts_reference as cref  # noqa: E402
from tests import rows_reference as rref  # noqa: E402
from tests import solve_reference as sref  # noqa: E402

CPU32 = os.path.join(ROOT, "oracle", "libfsim_cpu32.so")
SEEDS = 60          # seeds tried for one env before the generator gives up
WIDTH = 1e-3        # geom_solimp[2] of every colliding geom: x = depth / WIDTH
G = 9.81


def f32(st):
    return {k: (np.asarray(v, dtype=np.int32) if k in sref.INT_FIELDS else cref.f32(v)) for k, v in st.items() if k in sref.FIELDS + ("cursor",)}


def rows(sts):
    return dict({k: np.stack([s[k] for s in sts]) for k in sref.FIELDS}, cursor=np.stack([s["cursor"] for s in sts]) if "cursor" in sts[0] else None)


def qmul(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def axis_angle(ax, angle):
    ax = np.asarray(ax, dtype=np.float64)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * ax / np.linalg.norm(ax)])


def mat2quat(R):
    """wxyz of a rotation matrix (the branch with the largest pivot)"""
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[0] >= 0 else -q


def blank(m):
    """a one-env state: the robot at its initial pose with its finger slides mid-range (open fingers rest ON their limit), the parts at theirs,
    nothing applied, no weld, every geom as the model has it"""
    q = np.array(m.qpos0, dtype=np.float64)
    q[m.arm_qposadr], q[m.grip_qposadr] = m.arm_initqpos, m.grip_initqpos
    lm = rref.limits(m)
    q[lm["qposadr"][lm["slide"]]] = lm["range"][lm["slide"]].mean(axis=1)
    for i in range(m.nparts):
        q[m.part_qposadr[i]:m.part_qposadr[i] + 7] = m.part_initqpos[i]
    return dict(qpos=q, qvel=np.zeros(m.nv), ctrl=np.zeros(m.nu), qfrc_applied=np.zeros(m.nv), xfrc_applied=np.zeros(6 * m.nparts),
                eq_data=np.asarray(m.arrays["eq_data0"], dtype=np.float64).reshape(-1).copy(), eq_active=np.zeros(m.neq, np.int32),
                geom_contype=np.asarray(m.geom_contype, dtype=np.int32).copy(), geom_conaffinity=np.asarray(m.geom_conaffinity, dtype=np.int32).copy(),
                qacc_warmstart=np.zeros(m.nv))


def look(m, o, st, iterations=1):
    """forward() of a one-env state: (contact pairs, distances)"""
    sref.put(o, m, rows([st]), 0, warm=False, iterations=iterations)
    o.forward()
    return o.contacts(), np.array(o.contact_dists())


def finish(m, o, st):
    """qfrc_applied on the robot's dofs such that its qacc_smooth is zero (gravity, the actuators at ctrl = 0 and the joint damping compensated),
    the float32 rounding, and the warm start: the float64 solution itself, rounded"""
    look(m, o, st)
    rd = sref.robot_dofs(m)
    want = np.array(o.data.qacc_smooth)
    want[rd] = 0.0
    st["qfrc_applied"][rd] = (o.full_M() @ (want - np.array(o.data.qacc_smooth)))[rd]
    st = f32(st)
    st["qacc_warmstart"] = cref.f32(sref.reference(o, m, rows([st]), 0, step=False)["qacc"])
    return st


def layout(m):
    """(x, y, yaw) of every part: the Sawyer's table beside the arm with the legs in a row behind it, along y; Baxter's desk where its parts start"""
    if m.nparts == 5:
        return [(0.15, -0.38, 0.0), (-0.05, -0.38, 0.0), (-0.25, -0.38, 0.0), (-0.45, -0.38, 0.0), (-0.19, 0.0, np.pi / 2)]
    return [(0.682, -0.054, 0.0), (-0.524, -0.032, 0.0), (0.079, -0.045, np.pi / 2), (0.9, -0.8, np.pi / 2)]


LIGHT = 0.01                            # kg: the Sawyer table's legs weigh 1 g
AWAY = (-2.0, -1.5, 1.0)                # where a part that takes no part in an env falls freely
B_FLOOR = 2.0 / (0.95 * 0.0105)         # b of a part's contact with the floor (solref 0.001 mixed with 0.02, above the 2 h clamp)


# ---- placing a part ----------------------------------------------------------------------------------------------------------------------------------
def part_geoms(m, p):
    gb, bp = np.asarray(m.geom_bodyid, dtype=np.int64), np.asarray(m.arrays["body_partid"])
    return [g for g in range(m.ngeom) if bp[gb[g]] == p and (m.geom_contype[g] or m.geom_conaffinity[g])]


def box_of(m, p):
    """the part's colliding box: (geom, half sizes, rotation body -> geom, offset in the body frame)"""
    g = part_geoms(m, p)
    assert len(g) == 1 and int(m.arrays["geom_type"][g[0]]) == 6, (p, g)
    A = m.arrays
    return g[0], np.asarray(A["geom_size"], dtype=np.float64).reshape(-1, 3)[g[0]], T.quat2mat_wxyz(np.asarray(A["geom_quat"], dtype=np.float64).reshape(-1, 4)[g[0]]), \
        np.asarray(A["geom_pos"], dtype=np.float64).reshape(-1, 3)[g[0]]


def orientation(m, p, up, yaw, tilt=0.0, tilt_axis=0.0):
    """the part's quaternion with the box's local axis `up` (0 1 2 by increasing half size) vertical, turned by yaw about the vertical, then
    tilted by `tilt` about the horizontal axis at angle tilt_axis"""
    _, size, Rbg, _ = box_of(m, p)
    a = int(np.argsort(size, kind="stable")[up])
    Rg = np.zeros((3, 3))  # geom axis a -> world z, the longer of the other two -> y, the third -> +-x (whichever makes a rotation)
    b, c = sorted([(a + 1) % 3, (a + 2) % 3], key=lambda k: -size[k])
    Rg[2, a], Rg[1, b], Rg[0, c] = 1.0, 1.0, 1.0
    Rg[0, c] = np.linalg.det(Rg)
    q = mat2quat(Rg @ Rbg.T)
    q = qmul(axis_angle([0, 0, 1], yaw), q)
    return qmul(axis_angle([np.cos(tilt_axis), np.sin(tilt_axis), 0], tilt), q) if tilt else q


def lowest(m, p, quat):
    """how far the box's lowest corner lies below the body's origin at this orientation, and the box's top above it"""
    _, size, Rbg, off = box_of(m, p)
    R = T.quat2mat_wxyz(quat)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * size
    z = (R @ (off[:, None] + Rbg @ corners.T))[2]
    return -z.min(), z.max()


def depth_of(m, o, st, mine, theirs):
    pairs, d = look(m, o, st)
    sel = [i for i, (a, b) in enumerate(pairs) if (a in mine and b in theirs) or (b in mine and a in theirs)]
    return -d[sel].min() if sel else -1.0


def place(m, o, st, p, quat, xy, x, on=None):
    """part p at orientation quat above xy with its deepest contact against the floor (on: against part `on`, lying flat) x * WIDTH deep"""
    qa = int(m.part_qposadr[p])
    floor = [int(np.asarray(m.arrays["floor_geomid"]).reshape(-1)[0])]
    theirs, base = floor, 0.0
    if on is not None:
        theirs = part_geoms(m, on)
        base = st["qpos"][int(m.part_qposadr[on]) + 2] + lowest(m, on, st["qpos"][int(m.part_qposadr[on]) + 3:][:4])[1]
    st["qpos"][qa:qa + 2], st["qpos"][qa + 3:qa + 7] = xy, quat
    touch = base + lowest(m, p, quat)[0]
    lo, hi = touch - 2.5 * WIDTH, touch + 0.2 * WIDTH
    mine = part_geoms(m, p)
    for _ in range(48):
        st["qpos"][qa + 2] = 0.5 * (lo + hi)
        if depth_of(m, o, st, mine, theirs) > x * WIDTH:
            lo = st["qpos"][qa + 2]
        else:
            hi = st["qpos"][qa + 2]
    st["qpos"][qa + 2] = float(np.float32(0.5 * (lo + hi)))
    got = depth_of(m, o, st, mine, theirs)
    assert abs(got - x * WIDTH) < 2e-7, (p, got, x)
    return st


def normal_force(m, o, st, p):
    """the sum of the normal forces on part p's contacts at the state as it is"""
    sref.put(o, m, rows([st]), 0, warm=False)
    o.forward()
    mine, c = part_geoms(m, p), o.contact_rows()
    return sum(c["force"][i, 0] for i, (a, b) in enumerate(o.contacts()) if a in mine or b in mine)


# ---- judging a state ----------------------------------------------------------------------------------------------------------------------------------
def judge(m, case, o, o32, st):
    """(problems, reference, per-contact table: zone, x, live, par) of a one-env state"""
    one = rows([st])
    _, _, pairs32 = sref.abi_solve(CPU32, m, one, warm=False)
    ref = cr.reference(o, m, one, 0, step=False)
    bad = cr.conditions(m, case, one, 0, ref, pairs32[0])
    c = ref["con"]
    par = cr.restate(m, c, ref["qvel"])
    zone, f, margin = cr.forces(m, c, par, ref["qacc"])
    lv = cr.live(c["force"])
    if st["eq_active"].any():
        bad.append("a weld is active")
    if (rref.violations(m, one["qpos"][0]) > 0).any() or (rref.violations(m, one["qpos"][0], np.float32) > 0).any():
        bad.append("a joint limit is active")
    if (margin[lv] <= cr.ZONE_BAND).any():
        bad.append("a contact that carries force is within %.0e of a zone boundary" % cr.ZONE_BAND)
    f32_ = cr.zones32(o32, m, one, 0, ref)
    if f32_ is None:
        bad.append("the float32 build lists other contacts")
    else:
        tol = 1e-4
        z32 = np.array([cr.zone_of_force(f32_[i], par["mu"][i], tol) for i in range(len(zone))])
        if (z32[lv] != zone[lv]).any():
            bad.append("the float32 build puts a contact that carries force into another zone")
    return bad, ref, dict(zone=zone, x=par["x"], live=lv, par=par, f=c["force"], row=c["row"], geoms=c["geoms"], dist=c["dist"])


# ---- the recipes ------------------------------------------------------------------------------------------------------------------------------------
def env_state(m, o, rng, recipe):
    """recipe: one dict per part -- up (0 flat, 1 on its side, 2 on end), yaw, tilt (rad; corner: about a random horizontal axis), x (depth over
    WIDTH), on (the part it lies on), away (it takes no part), link (it is placed by the caller), and what acts on it beyond a wrench of the order
    of its weight: slide (horizontal force as a multiple of fri f_n), lift (torque as a multiple of f_n x half length), vel (world, m/s; a
    part that leaves the floor is pressed down), spin (rad/s, about a horizontal axis through the centre)"""
    st = blank(m)
    order = sorted(range(m.nparts), key=lambda p: recipe[p].get("on") is not None)
    for p in order:
        r, qa = recipe[p], int(m.part_qposadr[p])
        x0, y0, yaw0 = layout(m)[p]
        if r.get("away") or "link" in r:  # no contact: the part falls freely, far from everything
            st["qpos"][qa:qa + 3] = AWAY[0] + 0.5 * p, AWAY[1], AWAY[2]
            continue
        xy = np.array([x0, y0]) + rng.uniform(-0.01, 0.01, 2)
        if r.get("on") is not None:
            xy = st["qpos"][int(m.part_qposadr[r["on"]]):][:2] + rng.uniform(-0.01, 0.01, 2)
        quat = orientation(m, p, r.get("up", 0), yaw0 + rng.uniform(-0.3, 0.3) + r.get("yaw", 0.0), r.get("tilt", 0.0), rng.uniform(0, 2 * np.pi) if r.get("corner") else r.get("tilt_axis", 0.0))
        place(m, o, st, p, quat, xy, r["x"], r.get("on"))
    mass = np.asarray(m.arrays["body_mass"], dtype=np.float64)[np.asarray(m.arrays["part_bodyid"], dtype=np.int64)]
    for p in range(m.nparts):
        r, da = recipe[p], int(m.part_dofadr[p])
        st["qvel"][da:da + 3] = r.get("vel", (0, 0, 0))
        if r.get("spin"):
            a = rng.uniform(0, 2 * np.pi)
            st["qvel"][da + 3:da + 6] = T.quat2mat_wxyz(st["qpos"][int(m.part_qposadr[p]) + 3:][:4]).T @ (r["spin"] * np.array([np.cos(a), np.sin(a), 0.0]))
    sizes = [np.sort(box_of(m, p)[1]) for p in range(m.nparts)]
    for p in range(m.nparts):  # first what presses: a wrench of the order of the weight, and what holds a part down that leaves the floor
        r, w = recipe[p], np.zeros(6)
        w[:3] = rng.uniform(-1, 1, 3) * mass[p] * G
        w[3:] = rng.uniform(-1, 1, 3) * mass[p] * G * sizes[p][1]
        if r.get("vel", (0, 0, 0))[2] > 0:  # a part that leaves the floor is pressed down hard enough to keep force on its contacts
            w[2] -= r.get("press", 1.5) * mass[p] * B_FLOOR * r["vel"][2]
        if mass[p] < LIGHT and any(q.get("away") for q in recipe):
            # a heavy part in free fall leaves 1e-7 of its weight as float32 rounding of its own dofs: the legs (1 g, forces of 1e-2 N) are pressed
            # down until their contact forces stand well above that
            w[2] -= rng.uniform(0.1, 0.3)
        if r.get("away") or "link" in r:
            w[:] = 0.0
        st["xfrc_applied"][6 * p:6 * p + 6] = w
    fn = [normal_force(m, o, st, p) if any(k in recipe[p] for k in ("slide", "lift")) else 0.0 for p in range(m.nparts)]
    for p in range(m.nparts):  # then the push along the floor and the torque that lifts an edge, as multiples of the normal force so far
        r, w = recipe[p], st["xfrc_applied"][6 * p:6 * p + 6]
        fri = 2.0 if r.get("on") is None else 1.0
        a = rng.uniform(0, 2 * np.pi)
        if "slide" in r:
            w[:2] += r["slide"] * fri * fn[p] * np.array([np.cos(a), np.sin(a)])
        if "lift" in r:
            w[3:5] += r["lift"] * fn[p] * sizes[p][-1] * np.array([np.cos(a), np.sin(a)])
    return st


def build_env(m, case, o, o32, seed, recipe, want=lambda tab: None):
    """the first seed whose state meets the conditions and what `want` asks of its contact table (want returns a complaint or None)"""
    why = None
    for s in range(SEEDS):
        rng = np.random.RandomState(seed + 1000 * s)
        try:
            st = env_state(m, o, rng, recipe) if not callable(recipe) else recipe(rng)
        except AssertionError as err:
            why = "%s, line %d" % (err, err.__traceback__.tb_next.tb_lineno if err.__traceback__.tb_next else err.__traceback__.tb_lineno)
            continue
        if st is None:
            continue
        st = finish(m, o, st)
        bad, ref, tab = judge(m, case, o, o32, st)
        miss = want(tab)
        if not bad and miss is None:
            return st
        why = (bad, miss)
    raise AssertionError("%s seed %d: no usable state (%s)" % (case, seed, why))


def zones_in(tab):
    return {int(z) for z in tab["zone"][tab["row"]]}


def all_zones(tab):
    missing = {cr.TOP, cr.BOTTOM, cr.MIDDLE} - zones_in(tab)
    return "zones %s are missing" % sorted(missing) if missing else None


def expected(m, recipe, extra=()):
    """want(): every contact of a part is with the floor or with the part its recipe puts it on (extra: further pairs that may be listed)"""
    floor = int(np.asarray(m.arrays["floor_geomid"]).reshape(-1)[0])
    ok = {sref.pair_key(floor, g) for p in range(m.nparts) for g in part_geoms(m, p)} | set(extra)
    ok |= {sref.pair_key(a, b) for p in range(m.nparts) if recipe[p].get("on") is not None for a in part_geoms(m, p) for b in part_geoms(m, recipe[p]["on"])}

    def want(tab):
        odd = [tuple(g) for g in tab["geoms"] if sref.pair_key(*g) not in ok]
        return "unexpected pairs %s" % odd if odd else None
    return want


def both(*wants):
    def want(tab):
        for w in wants:
            miss = w(tab)
            if miss:
                return miss
        return None
    return want


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------
def depth(p, e):
    return cr.DEPTHS[(p + e) % len(cr.DEPTHS)]


def floor_recipes(m, case):
    """8 envs: flat, on end, on an edge, on a corner, one part on another, pushed, moving slowly, on the side"""
    n, big = m.nparts, m.nparts - 1 if m.nparts == 5 else 2  # the heavy part: the table top, the desk top
    X = lambda e: [dict(x=depth(p, e)) for p in range(n)]
    R = []
    R.append(X(0))
    R.append([dict(r, up=2, away=(p == big)) for p, r in enumerate(X(1))])
    R.append([dict(r, tilt=0.05 if p == big else 0.1 + 0.08 * p) for p, r in enumerate(X(2))])
    R.append([dict(r, tilt=0.1 + 0.08 * p, corner=True, away=(p == big)) for p, r in enumerate(X(3))])
    on = X(4)
    on[0]["on"], on[1]["on"], on[1]["yaw"] = big, (2 if n == 5 else 2), np.pi / 2
    if n != 5:
        on[1].pop("on"), on[1].pop("yaw")
    R.append(on)
    R.append([dict(r, slide=(0.5, 3.0)[p % 2], lift=(0.0, 0.8)[(p // 2) % 2], away=(p == big)) for p, r in enumerate(X(5))])
    R.append([dict(r, vel=((0, 0, -0.5), (0.5, 0, 0), (0, 0, 0.5), (0, -0.5, 0.0), (0.3, 0.3, 0))[p % 5], slide=3.0 if p == big else 0.0) for p, r in enumerate(X(6))])
    R.append([dict(r, up=1, slide=(2.0, 0.3)[p % 2], lift=0.9, away=(p == big and n == 5)) for p, r in enumerate(X(7))])
    return R


def slide_recipes(m, case):
    """every env: one part pushed below fri f_n, one above, one with an edge lifted, and a part on another part (friction 1 against 1; on the
    floor 1 against 2), pushed across it; the table top takes part in the even envs"""
    n, big, R = m.nparts, m.nparts - 1, []
    for e in range(8):
        r = [dict(x=depth(p, e), up=(0, 1)[(p + e) % 2 if p != big else 0]) for p in range(n)]
        k = e % 4
        r[k]["slide"], r[(k + 1) % 4]["slide"], r[(k + 2) % 4]["lift"] = 0.5, 2.0 + e % 3, 0.6 + 0.1 * (e % 4)
        r[(k + 2) % 4]["slide"] = 0.4
        if e % 2 == 0:
            r[(k + 3) % 4].update(on=big, slide=(0.5, 3.0)[(e // 2) % 2], up=0)
            r[big].update(slide=(3.0, 0.5)[(e // 2) % 2], lift=0.5)
        else:
            r[(k + 3) % 4].update(on=k, yaw=np.pi / 2, slide=(0.5, 3.0)[(e // 2) % 2], up=0)
            r[k]["up"] = 0
            r[big]["away"] = True
        R.append(r)
    return R


def impact_recipes(m, case):
    """parts moving into the floor and out of it at 0.2, 1 and 3 m/s, sliding at up to 3 m/s, spinning at up to 20 rad/s about a horizontal axis
    through their centre (off every contact point); the table top takes part in the even envs"""
    n, big, R = m.nparts, m.nparts - 1, []
    V = (0.2, 1.0, 3.0)
    for e in range(6):
        r = [dict(x=depth(p, e), up=(0, 2, 1)[(p + e) % 3] if p != big else 0, away=(p == big and e % 2 == 1)) for p in range(n)]
        for p in range(n):
            kind, v = (p + e) % 5, V[(p + 2 * e) % 3]
            if kind == 0:
                r[p]["vel"] = (0, 0, -v)
            elif kind == 1:
                r[p]["vel"] = (0, 0, v)
            elif kind == 2:
                r[p]["vel"] = (v * np.cos(e + p), v * np.sin(e + p), 0.0)
            elif kind == 3:
                r[p]["spin"], r[p]["up"] = (5.0, 10.0, 20.0)[(p + e) % 3], 0
            else:
                r[p]["vel"], r[p]["spin"] = (v * np.sin(e + p), v * np.cos(e + p), -V[(p + e) % 3]), 5.0
        R.append(r)
    return R


RECIPES = dict(floor_curve=floor_recipes, floor_desk=floor_recipes, slide=slide_recipes, impact=impact_recipes)
SEED0 = dict(floor_curve=26000, floor_desk=26100, slide=26200, impact=26300, grip_curve=26400, margin=26500, cursor=26600)


def case_states(m, case, o, o32):
    sts = []
    if case in RECIPES:
        for e, r in enumerate(RECIPES[case](m, case)):
            want = both(expected(m, r), all_zones) if case == "slide" else expected(m, r)
            sts.append(build_env(m, case, o, o32, SEED0[case] + e, r, want))
    sts += EXTRA.get(case, lambda *a: [])(m, case, o, o32)
    return rows(sts)


# ---- a part against a link of the arm, a leg between the finger pads, the pedestal pairs ------------------------------------------------------------
def bisect(m, o, st, adr, deep, clear, mine, theirs, target, tol, field="qpos"):
    """qpos[adr] between `deep` (the pair mine x theirs deeper than target) and `clear` (shallower, or not listed) such that the pair's least
    distance is -target (target < 0: a positive distance, inside the pair's margin)"""
    for _ in range(60):
        st[field][adr] = 0.5 * (deep + clear)
        if depth_of(m, o, st, mine, theirs) > target:
            deep = st[field][adr]
        else:
            clear = st[field][adr]
    st[field][adr] = float(np.float32(0.5 * (deep + clear)))
    got = depth_of(m, o, st, mine, theirs)
    assert abs(got - target) < tol, (adr, got, target)


def at_link(m, o, st, rng, p, link, x, tol, hover=0.0):
    """part p, floating, moved along a ray towards the centre of arm geom `link` until it lies x * WIDTH deep in it (hover > 0: until the pair
    is first listed, then back along the ray by `hover`)"""
    look(m, o, st)
    c = np.array(o.data.geom_xpos).reshape(-1, 3)[link].copy()
    ray = rng.normal(size=3)
    ray[2] = -abs(ray[2])  # from below and beside: the arm's other links are above
    ray /= np.linalg.norm(ray)
    qa = int(m.part_qposadr[p])
    q = rng.normal(size=4)
    st["qpos"][qa + 3:qa + 7] = q / np.linalg.norm(q)
    mine, far = part_geoms(m, p), 0.5
    near = None
    for t in np.arange(far, 0.0, -2e-3):
        st["qpos"][qa:qa + 3] = c + t * ray
        if depth_of(m, o, st, mine, [link]) > x * WIDTH:
            near = t
            break
    assert near is not None, "the ray misses the link"
    lo, hi = near, near + 2e-3
    for _ in range(50):
        t = 0.5 * (lo + hi)
        st["qpos"][qa:qa + 3] = c + t * ray
        if depth_of(m, o, st, mine, [link]) > x * WIDTH:
            lo = t
        else:
            hi = t
    st["qpos"][qa:qa + 3] = cref.f32(c + (0.5 * (lo + hi) + hover) * ray)
    got = depth_of(m, o, st, mine, [link])
    assert (got == -1.0) if hover else abs(got - x * WIDTH) < tol, (link, got, x)


def arm_env(m, case, o, o32, seed, link, x, joint, speed, others):
    """impact: part 0 against arm geom `link`, x deep; arm joint `joint` turns at `speed` rad/s, with the sign that drives the link into the part;
    the other parts follow the recipe `others`"""
    recipe = [dict(link=link)] + others
    portal = cr.pair_type(m, link, part_geoms(m, 0)[0]) not in cr.CLOSED_FORM

    def make(rng):
        st = env_state(m, o, rng, [dict(away=True)] + others)
        at_link(m, o, st, rng, 0, link, x, 3e-5 if portal else 2e-7)
        d = int(np.asarray(m.arrays["jnt_dofadr"])[list(np.asarray(m.arrays["jnt_qposadr"])).index(int(m.arm_qposadr[joint]))])
        for sign in (1.0, -1.0):
            st["qvel"][d] = sign * speed
            ref = cr.reference(o, m, rows([f32(st)]), 0, step=False)
            c = ref["con"]
            mine = [i for i in range(len(c["mu"])) if link in c["geoms"][i]]
            if mine and all(c["J"][i, 0] @ ref["qvel"] < -0.05 for i in mine):
                return st
        return None
    want = both(expected(m, recipe, extra={sref.pair_key(link, g) for g in part_geoms(m, 0)}),
                lambda tab: None if any(link in g and f[0] > 0 for g, f in zip(tab["geoms"], tab["f"])) else "the link's contact carries no force")
    return build_env(m, case, o, o32, seed, make, want)


def impact_extra(m, case, o, o32):
    """a sphere of the arm (closed form) and a cylinder (the portal routine) moving into a floating leg at 2 rad/s of the second joint: fs_ptvel with
    two moving sides on different trees"""
    R = impact_recipes(m, case)
    return [arm_env(m, case, o, o32, SEED0[case] + 6, 23, 0.45, 1, 2.0, R[1][1:]), arm_env(m, case, o, o32, SEED0[case] + 7, 21, 0.6, 1, 2.0, R[0][1:])]


PADS = ((7, 32), (8, 37))  # (index of the finger's slide among the limited joints, its pad geom) of the Sawyer
GRIP_X = ((0.2, 0.9), (0.3, 0.7), (0.45, 0.55), (0.55, 0.3), (0.7, 0.2), (0.9, 0.45), (0.25, 0.6), (0.8, 0.35))


def grip_extra(m, case, o, o32):
    """the poses of the stored `pinch` states (tests/golden/solve_states.npz: a leg between the pads, 5 to 7 mm deep) with the fingers opened until
    each pad lies x * WIDTH deep (the finger bodies then clear the leg), everything at rest or the leg moving across at 0.1 m/s, the leg pulled in
    the pads' plane by 0.4 or 2.5 times fri (f_n of both pads); the other parts lie on the floor, pushed"""
    base, lm, out = sref.load()["pinch"]["st"], rref.limits(m), []
    for e, (xa, xb) in enumerate(GRIP_X):
        floor = [dict(x=depth(p, e), slide=(0.5, 3.0)[(p + e) % 2], lift=(0.0, 0.7)[(p // 2 + e) % 2], up=(0, 1)[(p + e) % 2] if p < 4 else 0, away=(p == 4 and e % 2 == 1)) for p in range(1, m.nparts)]

        def make(rng, e=e, xa=xa, xb=xb, floor=floor):
            st = env_state(m, o, rng, [dict(away=True)] + floor)
            k = e % len(base["qpos"])
            rd = np.setdiff1d(np.arange(m.nq), np.concatenate([int(a) + np.arange(7) for a in m.part_qposadr]))
            st["qpos"][rd] = base["qpos"][k][rd]
            qa = int(m.part_qposadr[0])
            st["qpos"][qa:qa + 7] = base["qpos"][k][qa:qa + 7]
            leg = part_geoms(m, 0)
            for (j, pad), x in zip(PADS, (xa, xb)):
                adr, closed = int(lm["qposadr"][j]), base["qpos"][k][int(lm["qposadr"][j])]
                bisect(m, o, st, adr, closed, closed + np.sign(lm["range"][j].mean() - closed) * 8e-3, leg, [pad], x * WIDTH, 2e-7)
            look(m, o, st)
            c = o.contact_rows()
            i = [i for i, g in enumerate(o.contacts()) if PADS[0][1] in g][0]
            n, t1, t2 = c["frame"][i]
            if e % 4 == 3:
                st["qvel"][int(m.part_dofadr[0]):][:3] = 0.1 * n * (1 if e % 8 == 3 else -1)
            fn = normal_force(m, o, st, 0)
            a = (0.0, np.pi / 2, 0.7, 2.3)[e % 4]
            st["xfrc_applied"][:3] = (0.4, 2.5)[(e // 2) % 2] * 2.0 * fn * (np.cos(a) * t1 + np.sin(a) * t2)
            return st
        pads = {sref.pair_key(pad, g) for _, pad in PADS for g in part_geoms(m, 0)}
        want = both(expected(m, [dict(link=0)] + floor, extra=pads),
                    lambda tab: None if {tuple(sorted(g)) for g, f in zip(tab["geoms"].tolist(), tab["f"]) if f[0] > 0} >= ({tuple(sorted(k)) for k in pads} if e % 4 != 3 else set()) else "a pad carries no force")
        out.append(build_env(m, case, o, o32, SEED0[case] + e, make, want))
    return out


MARGIN_D = (2e-4, 3e-4, 4.5e-4, 5.5e-4, 7e-4, 9e-4, 8e-4, 6e-4)
HEAD = ((1, 2, (21, 23)), (8, 4, (49, 51)))  # (index of the arm joint that is bisected, the head's sphere, the elbow cylinders that reach it) per arm


def margin_extra(m, case, o, o32):
    """Baxter: each arm's second joint lowered until an elbow cylinder stands d above a sphere of the head (sphere-cylinder, both soft, margin
    0.001), a part floating d before one of them (sphere-box, margin 0.001); d rotates over the three from env to env; the arms move
    at up to 0.5 rad/s.  Part 0 floats HOVER before a wrist cylinder, on the ray through the cylinder's centre along which it was first listed:
    a pair of the portal routine inside its margin, which lists nothing.  The other parts lie on the floor"""
    out = []
    for e in range(8):
        floor = [dict(link=cr.HOVER_LINK[e % 2])] + [dict(x=depth(p, e), slide=(0.5, 3.0)[(p + e) % 2]) for p in range(1, m.nparts - 1)]

        def make(rng, e=e, floor=floor):
            st = env_state(m, o, rng, floor + [dict(away=True)])
            for a, (j, sphere, cyl) in enumerate(HEAD):
                adr = int(m.arm_qposadr[j])
                lo = rref.limits(m)["range"][list(rref.limits(m)["qposadr"]).index(adr)][0]
                bisect(m, o, st, adr, lo + 0.02, st["qpos"][adr], list(cyl), [sphere], -MARGIN_D[(e + 3 * a) % 8], 2e-7)
            p, qa = m.nparts - 1, int(m.part_qposadr[m.nparts - 1])
            look(m, o, st)
            side = (2, 4)[e % 2]
            c = np.array(o.data.geom_xpos).reshape(-1, 3)[side].copy()
            ray = np.array([(-1.0, 1.0)[e % 2] * rng.uniform(0.3, 1.0), -1.0, rng.uniform(-0.5, 0.0)])
            ray /= np.linalg.norm(ray)
            q = rng.normal(size=4)
            st["qpos"][qa + 3:qa + 7] = q / np.linalg.norm(q)
            mine, lo_t, hi_t = part_geoms(m, p), None, 1.0
            for t in np.arange(1.0, 0.2, -2e-3):
                st["qpos"][qa:qa + 3] = c + t * ray
                if depth_of(m, o, st, mine, [2, 3, 4]) > -MARGIN_D[(e + 5) % 8]:
                    lo_t, hi_t = t, t + 2e-3
                    break
            assert lo_t is not None
            for _ in range(50):
                t = 0.5 * (lo_t + hi_t)
                st["qpos"][qa:qa + 3] = c + t * ray
                if depth_of(m, o, st, mine, [2, 3, 4]) > -MARGIN_D[(e + 5) % 8]:
                    lo_t = t
                else:
                    hi_t = t
            st["qpos"][qa:qa + 3] = cref.f32(c + 0.5 * (lo_t + hi_t) * ray)
            assert abs(depth_of(m, o, st, mine, [2, 3, 4]) + MARGIN_D[(e + 5) % 8]) < 2e-7
            at_link(m, o, st, rng, 0, cr.HOVER_LINK[e % 2], 0.0, 0.0, hover=cr.HOVER)
            st["qvel"][sref.robot_dofs(m)] = rng.uniform(-0.5, 0.5, len(sref.robot_dofs(m))) * (np.abs(np.asarray(m.arrays["dof_invweight0"])[sref.robot_dofs(m)]) < 1e3)
            return st
        pairs = {sref.pair_key(s_, c_) for _, s_, cyl in HEAD for c_ in cyl} | {sref.pair_key(k, g) for k in (2, 3, 4) for g in part_geoms(m, m.nparts - 1)}
        want = both(expected(m, floor + [dict(link=0)], extra=pairs),
                    lambda tab: None if sum(1 for g, f, d in zip(tab["geoms"], tab["f"], tab["dist"]) if d > 0 and f[0] > 0) >= 3 else "fewer than three contacts carry force at a positive distance")
        out.append(build_env(m, case, o, o32, SEED0[case] + e, make, want))
    return out


def cursor_extra(m, case, o, o32):
    """Cursor + toy_table: the parts where the model starts them, each lowered until its deepest contact with the floor is x * WIDTH deep, pushed by
    a wrench of one to three times its weight, the odd envs moving at up to 0.3 m/s.  Cursor 0 lies 2 to 12 mm deep in a leg (cylinder-box: the
    portal routine), cursor 1 stands 5 to 40 mm above the table top (which lies upside down) in the even envs (box-box inside the margin of 0.05) and 2 to 10 mm deep
    in it in the odd ones.  With gap 10 none of their contacts may become a row"""
    floor = [int(np.asarray(m.arrays["floor_geomid"]).reshape(-1)[0])]
    mass = np.asarray(m.arrays["body_mass"], dtype=np.float64)[np.asarray(m.arrays["part_bodyid"], dtype=np.int64)]
    legs, top, out = [p for p in range(m.nparts) if p != 1], 1, []
    for e in range(8):
        def make(rng, e=e):
            st = blank(m)
            st["cursor"] = np.zeros(8)
            st["cursor"][:6] = (5.0, 5.0, 5.0, -5.0, 5.0, 5.0)  # away while the parts are placed
            for p in range(m.nparts):
                qa, da = int(m.part_qposadr[p]), int(m.part_dofadr[p])
                st["qpos"][qa:qa + 2] += rng.uniform(-0.005, 0.005, 2)
                z0 = st["qpos"][qa + 2]
                bisect(m, o, st, qa + 2, z0 - 2.5 * WIDTH, z0 + WIDTH, part_geoms(m, p), floor, depth(p, e) * WIDTH, 2e-7)
                st["xfrc_applied"][6 * p:6 * p + 3] = rng.uniform(-1, 1, 3) * rng.uniform(1, 3) * mass[p] * G
                st["xfrc_applied"][6 * p + 3:6 * p + 6] = rng.uniform(-1, 1, 3) * mass[p] * G * 0.02
                if e % 2:
                    st["qvel"][da:da + 3] = rng.uniform(-0.3, 0.3, 3)
            leg = legs[e % len(legs)]
            qa, qt = int(m.part_qposadr[leg]), int(m.part_qposadr[top])
            st["cursor"][0:3] = st["qpos"][qa:qa + 3] + np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.05, 0.05), 0.02 + 0.05 - rng.uniform(0.002, 0.012)])
            above = rng.uniform(0.005, 0.04) if e % 2 == 0 else -rng.uniform(0.002, 0.01)
            st["cursor"][3:5] = st["qpos"][qt:qt + 2] + rng.uniform(-0.1, 0.1, 2)
            if above > 0:
                bisect(m, o, st, 5, st["qpos"][qt + 2] + 0.05, 0.5, [cr.CURSOR_GEOMS[1]], part_geoms(m, top), -above, 2e-6, field="cursor")
            else:  # into the plate, which is the table top's lowest geom (0.036 below its origin, 3 mm thick)
                st["cursor"][5] = st["qpos"][qt + 2] - 0.036 + 0.003 + 0.05 + above
            return st
        ok = {sref.pair_key(floor[0], g) for p in range(m.nparts) for g in part_geoms(m, p)}

        def want(tab, e=e):
            odd = [tuple(g) for g in tab["geoms"] if sref.pair_key(*g) not in ok and not set(g) & set(cr.CURSOR_GEOMS)]
            if odd:
                return "unexpected pairs %s" % odd
            cur = [(set(g) & set(cr.CURSOR_GEOMS), d) for g, d in zip(tab["geoms"].tolist(), tab["dist"]) if set(g) & set(cr.CURSOR_GEOMS) and floor[0] not in g]
            if not any(1 in c for c, d in cur) or not any(2 in c and (d > 0) == (e % 2 == 0) for c, d in cur):
                return "a cursor touches no part as asked"
            return None
        out.append(build_env(m, case, o, o32, SEED0[case] + e, make, want))
    return out


EXTRA = dict(impact=impact_extra, grip_curve=grip_extra, margin=margin_extra, cursor=cursor_extra)


def survey(m, case, o, o32, st):
    """one line per env and the case's coverage, from the reference alone"""
    total = np.zeros(3, np.int64)
    for e in range(len(st["qpos"])):
        one = {k: st[k][e] for k in sref.FIELDS + (("cursor",) if st["cursor"] is not None else ())}
        bad, ref, tab = judge(m, case, o, o32, one)
        z = [int(((tab["zone"] == k) & tab["row"]).sum()) for k in range(3)]
        total += z
        print("  env %d: %2d contacts, %2d with force, %2d live, zones top/bottom/middle %s, x %s, iterations %d %s" % (
            e, len(tab["zone"]), int((np.abs(tab["f"]).max(axis=1) > 0).sum()), int(tab["live"].sum()), z,
            sorted({round(float(x), 2) for x in tab["x"][tab["row"]] if x < 5}), ref["iters"], bad or ""), flush=True)
    print("  %s: zones top/bottom/middle %s" % (case, total.tolist()), flush=True)


def generate(only=None, verbose=False):
    """{name: dict(st, island)} of every case (or of those named)"""
    from tests.solve_bits_common import island_dofs
    out = {}
    for name in cr.CASES:
        if only and name not in only:
            continue
        m = cr.model(name)
        o, o32 = OracleSim(m), OracleSim(m, np.float32)
        st = case_states(m, name, o, o32)
        refs = [sref.reference(o, m, st, e, step=False) for e in range(len(st["qpos"]))]
        out[name] = dict(st=st, island=[island_dofs(m, r["contacts"], st["eq_active"][e])[0] for e, r in enumerate(refs)])
        print("%-12s %d envs, largest island %s, contacts %s, float64 Newton iterations %s" % (
            name, len(refs), out[name]["island"], [len(r["contacts"]) for r in refs], [r["iters"] for r in refs]), flush=True)
        if verbose:
            survey(m, name, o, o32, st)
        o.close(), o32.close()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "-v"]
    cases = generate(args or None, verbose="-v" in sys.argv)
    if len(cases) == len(cr.CASES):
        np.savez_compressed(cr.GOLDEN, **cr.pack(cases))
        print("wrote", cr.GOLDEN, os.path.getsize(cr.GOLDEN) // 1024, "KB")

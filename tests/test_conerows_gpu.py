"""ONE Newton solve of the device where its CONTACT ROWS stand on the impedance curve, in every zone of the friction cone and at impact and sliding
speed, against float64: the stored states of tests/conerows_reference.py -- parts on the floor, on each other, between the finger pads and against
a link of the arm with their deepest contact at x = 0.15 .. 0.9 of the curve's width, pushed below and above fri f_n, an edge lifted, moving into
and out of the contact at up to 3 m/s, sliding, spinning; Baxter's pedestal pairs carrying force at a positive distance inside their margin -- on
every kernel set of the model, from a cold start and from the stored warm start.

Part A is the procedure of tests/test_rows_gpu.py (with one deviation, below): set_state -> fsim_physics_forward -> qacc, the contact list and the iteration count, and on a
twin handle set_state -> fsim_physics_step(1) -> qvel.  Per env, none skipped: finite outputs; the reference's multiset of pairs (so a pair of the
portal routine inside its margin is listed by neither side); the measures force, island, step and row (one group per part and per limited dof);
the iteration count within 3 of the oracle's at the device's own tolerance and never at the cap; all kernel sets agree.  The deviation:
tests/test_rows_gpu.py asserts the reference's pair list exactly, on states whose geoms are off.  Here every geom is on, and the device may list,
beyond the reference's multiset, a pair that sits EXACTLY on its margin and that the float32 CPU build lists too (the Sawyer's l0 sphere on its base
cylinder, distance 0) -- the rule of tests/test_solve_gpu.py and of solve_reference.conditions.  Such a pair must be of two robot geoms
(asserted) and its device row must carry no force (part B).  The `cursor` case runs on the Cursor agent's default kernel set, one set, so for it
the agreement of the kernel sets has nothing to compare.

Part B reads the device's own contact list (ContactSet(..., contacts=True), fsim_contact_forces at the same state, cold) on the handle with 48 / 64
slots: every reference contact is matched to a device row by geom pair and nearest con_pos (a match is right within |dist| / 2 + 1e-6 m); con_fn
and con_force per contact over the env's largest contact force (fn, cforce); con_dist on the closed-form pairs (dist, metres); and the zone of
every contact that carries more than 1e-2 of the env's largest contact force, read off the device's own force: zero, strictly inside, or
|F_t| = fri f_n to the `cone` tolerance of tests/test_contacts_gpu.py; a contact that the reference lists without making it a row (the
cursor boxes of the `cursor` case: gap 10) must be listed by the device with con_fn and con_force exactly zero.  An aggregate cannot see two contacts of one body with their forces
swapped, or a tangential force turned in its plane; these can.

The tolerance of a measure is 4 x the largest value measured on an MI355X for the case (the rule of DESIGN.md 15; the values: DESIGN.md 26).
One condition is not a measurement: a measured value above 10 x the case's fp32 floor (cr.FLOOR) is a defect to find, not a tolerance to widen
(test_the_condition_on_the_measured_values).  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from furniture_amd.sim import default_config
from oracle.oracle_sim import OracleSim
from tests import conerows_reference as cr
from tests import solve_reference as sref

pytestmark = pytest.mark.gpu
# case -> the largest value of each measure on an MI355X, over its envs, its kernel sets and both starts (fn, cforce, dist: the 48 / 64-slot set, cold)
MEASURED = {
    "floor_curve": dict(force=4.606e-05, island=2.906e-05, step=4.602e-05, row=3.878e-03, fn=1.799e-05, cforce=6.530e-05, dist=3.439e-08),
    "floor_desk": dict(force=1.311e-05, island=2.125e-05, step=1.312e-05, row=3.516e-04, fn=2.214e-05, cforce=5.440e-05, dist=4.884e-08),
    "slide": dict(force=5.448e-06, island=8.986e-05, step=5.448e-06, row=5.448e-04, fn=8.008e-06, cforce=3.644e-05, dist=3.494e-08),
    "impact": dict(force=6.344e-06, island=6.463e-04, step=2.714e-05, row=5.194e-04, fn=8.841e-06, cforce=8.395e-05, dist=8.348e-08),
    "grip_curve": dict(force=1.008e-05, island=1.120e-04, step=1.008e-05, row=1.008e-03, fn=3.647e-06, cforce=2.623e-05, dist=1.258e-07),
    "cursor": dict(force=2.824e-05, island=3.884e-05, step=2.826e-05, row=3.884e-05, fn=1.481e-05, cforce=9.215e-05, dist=1.863e-08),
    "margin": dict(force=6.011e-05, island=3.033e-04, step=6.044e-05, row=3.033e-04, fn=7.237e-05, cforce=1.012e-04, dist=1.669e-07),
}
TOL = {g: {k: 4.0 * v for k, v in d.items()} for g, d in MEASURED.items()}
# con_dist against the oracle's distance on closed-form pairs has no fp32 floor from the CPU builds (they have no contact sensors); its condition
# is solve_reference.CONTACT_BAND, eight times what float32 does to a distance between bodies a metre or two from the origin
DIST_BOUND = sref.CONTACT_BAND
CONE_TOL = 4.0 * 5.187e-7  # tests/test_contacts_gpu.py TOL["cone"]: (|F_t| - fri f_n) / f_n of a force on the cone's surface
ITER_SLACK = 3  # (the bound of tests/test_solve_gpu.py)
N = sref.MAX_ENVS
RUNS = [(name, ks) for name, c in cr.CASES.items() for ks, _ in c["ksets"]]
LISTS = {name: c["ksets"][0][0] for name, c in cr.CASES.items()}  # spec-mw0 (48 slots), desk-mw0 (64), toy
_handles, _runs, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    sref.close_handles(_handles)


@pytest.fixture(scope="module")
def stored():
    return cr.load()


def _reference(name, stored, warm):
    """the float64 references of a case (solver at 1e-14, with the per-contact table) and the oracle's iteration counts at the device's own
    tolerance and cap"""
    if (name, warm) not in _refs:
        m, st = cr.model(name), stored[name]["st"]
        cfg = default_config()
        o, o32 = OracleSim(m), OracleSim(m, np.float32)
        refs = [cr.reference(o, m, st, e, warm=warm) for e in range(len(st["qpos"]))]
        for e, r in enumerate(refs):
            r["iters_dev_tol"] = sref.reference(o, m, st, e, warm=warm, iterations=cfg.solver_iterations, tolerance=cfg.solver_tolerance, step=False)["iters"]
            # what sits EXACTLY on its margin (solve_reference.conditions: two robot geoms, no force) is listed by float32 arithmetic alone
            sref.put(o32, m, st, e, warm, 1, 1e-7)
            o32.forward()
            r["on_margin"] = sorted(set(sref.pair_key(*p) for p in o32.contacts()) - set(sref.pair_key(*p) for p in r["contacts"]))
            robot = sref.robot_geom(m)
            assert all(robot[a] and robot[b] for a, b in r["on_margin"]), (name, e, r["on_margin"])  # (the exception cannot grow silently)
        o.close(), o32.close()
        _refs[(name, warm)] = refs
    return _refs[(name, warm)]


def _same_pairs(pairs, ref):
    """the device lists the reference's multiset of pairs; beyond it only pairs that sit exactly on their margin -> which of its rows those are"""
    mine, theirs = sorted(sref.pair_key(*p) for p in pairs), sorted(sref.pair_key(*p) for p in ref["contacts"])
    extra = [i for i, p in enumerate(pairs) if sref.pair_key(*p) in ref["on_margin"]]
    assert sorted(k for k in mine if k not in ref["on_margin"]) == theirs, (pairs, ref["contacts"])
    return extra


def _fields(name, stored, warm):
    m, st = cr.model(name), stored[name]["st"]
    assert len(st["qpos"]) == N
    fields = {k: st[k] for k in sref.FIELDS if st[k].shape[1] > 0}
    if st["cursor"] is not None:
        fields["cursor"] = st["cursor"]
    if not warm:
        fields["qacc_warmstart"] = np.zeros((N, m.nv))
    return fields


def _run(name, ks, stored, warm):
    """one solve and one substep of every env of the case -> dict of arrays"""
    if (name, ks, warm) not in _runs:
        st = stored[name]["st"]
        assert cr.KSETS[ks]["model"] == cr.CASES[name]["model"]
        fields = _fields(name, stored, warm)
        sim, twin = cr.handle(_handles, ks, N)
        sim.set_state(**fields)
        sim.physics_forward()
        got = {k: v.cpu().numpy() for k, v in sim.get_state("qacc", "ncon", "contact_geoms", "solver_iters").items()}
        twin.set_state(**fields)
        twin.physics_step(1)
        qvel = twin.get_state("qvel")["qvel"].cpu().numpy().astype(np.float64)
        got["acc_step"] = (qvel - st["qvel"]) / float(cr.model(name).arrays["opt"][0])
        got["pairs"] = [[(int(a), int(b)) for a, b in got["contact_geoms"][i].reshape(-1, 2) if a >= 0] for i in range(N)]
        _runs[(name, ks, warm)] = got
    return _runs[(name, ks, warm)]


@pytest.mark.parametrize("name", list(cr.CASES))
def test_the_condition_on_the_measured_values(name):
    """no measured value is above 10 x what fp32 alone does"""
    for k, v in MEASURED[name].items():
        if k in cr.FLOOR[name]:
            assert 0 < v <= 10.0 * cr.FLOOR[name][k], (name, k, v, cr.FLOOR[name][k])
    assert 0 < MEASURED[name]["dist"] <= DIST_BOUND


# ---- part A: the solve ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_one_solve_against_float64(name, ks, stored):
    m, c, cfg = cr.model(name), stored[name], default_config()
    grp = cr.groups(m)
    worst, lines, checks = dict.fromkeys(cr.MEASURES, 0.0), [], []
    for warm in (False, True):
        refs, got = _reference(name, stored, warm), _run(name, ks, stored, warm)
        for e, ref in enumerate(refs):
            assert np.isfinite(got["qacc"][e]).all() and np.isfinite(got["acc_step"][e]).all(), (name, ks, warm, e)
            assert int(got["ncon"][e, 0]) == len(got["pairs"][e]) <= _handles[ks][0].max_contacts
            _same_pairs(got["pairs"][e], ref)
            v = cr.measure(got["qacc"][e], got["acc_step"][e], ref, grp)
            it = int(got["solver_iters"][e, 0])
            lines.append("%s %s %s env %d: island %d, contacts %d, %s, iterations %d (oracle %d)" % (
                name, ks, "warm" if warm else "cold", e, c["island"][e], len(got["pairs"][e]), " ".join("%s %.3e" % (k, v[k]) for k in cr.MEASURES), it, ref["iters_dev_tol"]))
            for k in cr.MEASURES:
                worst[k] = max(worst[k], v[k])
            checks.append((warm, e, it, ref["iters_dev_tol"]))
    print("\n".join(lines))
    print("%s %s measured: %s" % (name, ks, "  ".join("%s %.3e" % (k, worst[k]) for k in cr.MEASURES)))
    wrong = ["%s %.3e exceeds %.3e" % (k, worst[k], TOL[name][k]) for k in cr.MEASURES if not worst[k] <= TOL[name][k]]
    wrong += ["%s env %d: %d iterations, the oracle %d" % ("warm" if warm else "cold", e, it, it_ref) for warm, e, it, it_ref in checks
              if abs(it - it_ref) > ITER_SLACK or it >= cfg.solver_iterations]
    assert not wrong, wrong


@pytest.mark.parametrize("name", list(cr.CASES))
def test_the_kernel_sets_agree(name, stored):
    """qacc of every pair of kernel sets, as a force through M on the scale of `force`: within twice the tolerance of `force`"""
    worst = 0.0
    sets = [ks for n, ks in RUNS if n == name]
    for warm in (False, True):
        refs = _reference(name, stored, warm)
        runs = [_run(name, ks, stored, warm)["qacc"] for ks in sets]
        for e, ref in enumerate(refs):
            scale = np.abs(ref["qfrc_constraint"]).max()
            f = np.stack([ref["M"] @ r[e].astype(np.float64) for r in runs])
            worst = max(worst, np.abs(f[:, None] - f[None, :]).max() / (scale if scale > 0 else 1.0))
    print("%s measured: kernel sets %s differ by %.3e" % (name, sets, worst))
    assert len(sets) >= (1 if name == "cursor" else 2) and worst <= 2.0 * TOL[name]["force"]


# ---- part B: per contact ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.CASES))
def test_every_contact_against_float64(name, stored):
    import torch
    from furniture_amd.contacts import ContactSet, part_sensors
    m, ks = cr.model(name), LISTS[name]
    refs = _reference(name, stored, False)
    sim, _ = cr.handle(_handles, ks, N)
    assert sim.max_contacts in (48, 64) or name == "cursor"
    sim.set_contacts(ContactSet(part_sensors(m), contacts=True))
    sim.set_state(**_fields(name, stored, False))
    res = sim.contact_forces()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    sim.set_contacts(None)
    assert (got["contact_status"] == 0).all()
    worst, lines, zones, checked = dict(fn=0.0, cforce=0.0, dist=0.0, far=0.0), [], [], 0
    for e, ref in enumerate(refs):
        c = ref["con"]
        n = int((got["con_geoms"][e][:, 0] >= 0).sum())
        geoms = got["con_geoms"][e][:n]
        extra = _same_pairs([tuple(g) for g in geoms.tolist()], ref)
        assert (got["con_fn"][e][extra] == 0).all()
        idx, far = cr.match(ref, geoms, got["con_pos"][e][:n])
        flip = np.array([1.0 if tuple(geoms[j]) == tuple(c["geoms"][i]) else -1.0 for i, j in enumerate(idx)])
        fn, F = got["con_fn"][e][idx].astype(np.float64), got["con_force"][e][idx].astype(np.float64) * flip[:, None]
        nrm = got["con_normal"][e][idx].astype(np.float64) * flip[:, None]
        idle = ~c["row"]  # listed, never a row: the cursors
        assert (fn[idle] == 0).all() and (F[idle] == 0).all(), (name, e, c["geoms"][idle], fn[idle])
        assert idle.any() == (name == "cursor")
        v = cr.contact_measure(fn, F, ref)
        closed = np.array([cr.pair_type(m, *g) in cr.CLOSED_FORM for g in c["geoms"]])
        v["dist"] = np.abs(got["con_dist"][e][idx] - c["dist"])[closed].max() if closed.any() else 0.0
        v["far"] = far[c["row"]].max()
        for k in worst:
            worst[k] = max(worst[k], v[k])
        lines.append("%s %s env %d: %d contacts, %s" % (name, ks, e, n, " ".join("%s %.3e" % kv for kv in v.items())))
        par = cr.restate(m, c, ref["qvel"])
        zone, _, _ = cr.forces(m, c, par, ref["qacc"])
        for i in np.nonzero(cr.live(c["force"]))[0]:
            ft = F[i] - (F[i] @ nrm[i]) * nrm[i]
            dev = cr.zone_of_force(np.array([fn[i], np.linalg.norm(ft), 0.0]), par["mu"][i], CONE_TOL)
            checked += 1
            if dev != zone[i]:
                zones.append("env %d contact %d %s: zone %d, the reference %d" % (e, i, tuple(c["geoms"][i]), dev, zone[i]))
    print("\n".join(lines))
    print("%s %s measured: %s (%d zones checked)" % (name, ks, "  ".join("%s %.3e" % (k, worst[k]) for k in ("fn", "cforce", "dist")), checked))
    wrong = ["%s %.3e exceeds %.3e" % (k, worst[k], TOL[name][k]) for k in ("fn", "cforce", "dist") if not worst[k] <= TOL[name][k]]
    assert not wrong and not zones and checked > 0, (wrong, zones)

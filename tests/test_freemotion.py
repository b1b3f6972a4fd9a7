"""The reference of tests/test_freemotion_gpu.py on the CPU (tests/freemotion_reference.py): the oracle's forward() and step() against a
numpy restatement that shares no code with it, closed forms of a free rigid body that need no oracle, the conditions the states must
meet, that the states can tell each of nine deliberate defects from fp32 rounding, and what fp32 alone does to every measure (FLOOR)."""
import numpy as np
import pytest

from oracle.oracle_sim import OracleSim
from tests import freemotion_reference as fm

NAMES = list(fm.MODELS)
_cache = {}


@pytest.fixture(scope="module", params=NAMES)
def case(request):
    name = request.param
    if name not in _cache:
        m, st, refs = fm.references(name)
        _cache[name] = dict(name=name, m=m, st=st, refs=refs)
    return _cache[name]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def test_oracle_matches_the_restatement(case):
    """forward() and step() of the oracle against the numpy restatement, to 1e-10 relative on every state; the restatement's own mass
    matrix (a sum over the bodies of J^T I J) against full_M() as well"""
    m, st = case["m"], case["st"]
    worst = {}
    for e, ref in enumerate(case["refs"]):
        r = fm.restate(m, st, e, M=ref["M"])
        d = dict(M=_rel(r["M"], ref["M"]), bias=_rel(r["bias"], ref["bias"]), qacc=_rel(r["qacc"], ref["qacc"]), qvel1=_rel(r["qvel1"], ref["qvel1"]),
                 qpos1=_rel(r["qpos1"], ref["qpos1"]), qpos_fwd=_rel(r["qpos_fwd"], ref["qpos_fwd"]), xpos=_rel(r["xpos"], ref["xpos"]))
        if m.nu:
            d["actuator"] = _rel(r["actuator"], ref["actuator"])
        if fm.group(e) == "near":  # with its own M throughout (8 m out both mass matrices round at eps m |c|^2 against the parts' small inertias: 1.5e-10)
            own = fm.restate(m, st, e)
            d["qacc_own"], d["qvel1_own"] = _rel(own["qacc"], ref["qacc"]), _rel(own["qvel1"], ref["qvel1"])
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= fm.RESTATE_TOL, (case["name"], e, k, v)
    print("%s measured: oracle against the restatement %s" % (case["name"], "  ".join("%s %.1e" % kv for kv in worst.items())))


def _inertia(m, b):
    A = m.arrays
    Ri = fm._rot(np.asarray(A["body_iquat"], dtype=np.float64).reshape(-1, 4)[b])
    return Ri @ np.diag(np.asarray(A["body_inertia"], dtype=np.float64).reshape(-1, 3)[b]) @ Ri.T


def test_closed_forms_of_a_free_part(case):
    """Newton and Euler for every part of every state, from the model's tables and the state alone: with the wrench (f at the body origin, n)
    that the damping, qfrc_applied and xfrc_applied put on the part's six dofs, m a_c = m g + f and I w' + w x I w = n - r x R^T f about
    the centre of mass c = x + R r, body frame; the translation dofs accelerate at a_c - R (w' x r + w x (w x r)) and the rotation dofs at
    w'.  Without damping, forces and offset that is qacc = g and -I^-1 (w x I w), which the rest state and the parts with r = 0 show.
    The tolerance is 1e-10 of the part's largest acceleration, and where the reference's own rounding is more than that, that: the oracle
    holds a body's inertia about the world origin, I + m (|c|^2 - c c^T), which rounds at eps m |c|^2, and the angular acceleration divides by
    the smallest principal inertia -- 8 eps m |c|^2 / I_min is 1.4e-9 for toy_table's thinnest part 8 m out (measured 1.5e-10) and below
    1e-10 for every part within 2 m."""
    m, st, A = case["m"], case["st"], case["m"].arrays
    g, D = np.asarray(A["opt"][1:4], dtype=np.float64), np.asarray(A["dof_damping"], dtype=np.float64)
    pb, pd, pq = (np.asarray(x, dtype=np.int64) for x in (A["part_bodyid"], m.part_dofadr, m.part_qposadr))
    worst, plain = 0.0, 0
    for e, ref in enumerate(case["refs"]):
        for i in range(m.nparts):
            b, d, a = pb[i], pd[i], pq[i]
            mass, I, r = float(A["body_mass"][b]), _inertia(m, b), np.asarray(A["body_ipos"], dtype=np.float64).reshape(-1, 3)[b]
            R = fm._rot(st["qpos"][e][a + 3:a + 7])
            v, w = st["qvel"][e][d:d + 3], st["qvel"][e][d + 3:d + 6]
            F, T = st["xfrc_applied"][e][6 * i:6 * i + 3], st["xfrc_applied"][e][6 * i + 3:6 * i + 6]
            f = -D[d:d + 3] * v + st["qfrc_applied"][e][d:d + 3]
            n = -D[d + 3:d + 6] * w + st["qfrc_applied"][e][d + 3:d + 6]
            wdot = np.linalg.solve(I, n - np.cross(r, R.T @ f) + R.T @ T - np.cross(w, I @ w))
            ac = g + (f + F) / mass
            want = np.concatenate([ac - R @ (np.cross(wdot, r) + np.cross(w, np.cross(w, r))), wdot])
            err = np.abs(ref["qacc"][d:d + 6] - want).max() / np.abs(want).max()
            worst = max(worst, err)
            c = st["qpos"][e][a:a + 3] + R @ r
            tol = max(fm.CLOSED_TOL, 8.0 * np.finfo(np.float64).eps * mass * (c @ c) / np.linalg.eigvalsh(I).min())
            assert tol == fm.CLOSED_TOL or e in fm.FAMILY["far"]
            assert err <= tol, (case["name"], e, i, err, tol)
            if not f.any() and not n.any() and not F.any() and not T.any() and not r.any():  # the plain statement
                plain += 1
                assert np.abs(ref["qacc"][d:d + 3] - g).max() <= fm.CLOSED_TOL * 9.81
    print("%s measured: closed form of a free part %.1e" % (case["name"], worst))
    if not np.asarray(A["body_ipos"], dtype=np.float64).reshape(-1, 3)[pb].any():
        assert plain >= m.nparts  # (the rest state at least)


def test_bias_is_gravity_at_rest_and_qpos_is_normalised(case):
    m, st, A = case["m"], case["st"], case["m"].arrays
    g, mass = np.asarray(A["opt"][1:4], dtype=np.float64), np.asarray(A["body_mass"], dtype=np.float64)
    e = fm.FAMILY["rest"][0]
    o = OracleSim(m)
    fm.put(o, m, st, e)
    o.forward()
    want = np.zeros(m.nv)
    for b in range(1, m.nbody):
        if mass[b] > 0:
            want -= mass[b] * (o.body_jac(b, o.data.xipos[b])[0].T @ g)
    o.close()
    err = np.abs(case["refs"][e]["bias"] - want).max() / np.abs(want).max()
    print("%s measured: bias against the weights through the Jacobians at rest %.1e" % (case["name"], err))
    assert err <= fm.CLOSED_TOL
    quat = np.zeros(m.nq, dtype=bool)
    for a in np.asarray(m.part_qposadr, dtype=np.int64):
        quat[a + 3:a + 7] = True
    for e, ref in enumerate(case["refs"]):
        q = ref["qpos_fwd"]
        assert (q[~quat] == st["qpos"][e][~quat]).all()
        for a in np.asarray(m.part_qposadr, dtype=np.int64):
            q0 = st["qpos"][e][a + 3:a + 7]
            assert abs(np.linalg.norm(q[a + 3:a + 7]) - 1.0) <= 4e-16 and np.abs(q[a + 3:a + 7] - q0 / np.linalg.norm(q0)).max() <= 4e-16, (e, a)


def test_conditions_on_the_states(case):
    m, st, refs, A = case["m"], case["st"], case["refs"], case["m"].arrays
    pd, pq = np.asarray(m.part_dofadr, dtype=np.int64), np.asarray(m.part_qposadr, dtype=np.int64)
    for k in ("qpos", "qvel", "ctrl", "qfrc_applied", "xfrc_applied"):
        assert (st[k] == st[k].astype(np.float32).astype(np.float64)).all() and st[k].shape[0] == fm.N, k
    assert not st["geom_contype"].any() and not st["geom_conaffinity"].any() and not st["eq_active"].any()
    for e, ref in enumerate(refs):
        assert ref["ncon"] == 0 and ref["nefc"] == 0, (case["name"], e, ref["ncon"], ref["nefc"])
    # every limited joint well inside its range
    lim = np.asarray(A["jnt_limited"]).astype(bool)
    qa, rg = np.asarray(A["jnt_qposadr"], dtype=np.int64)[lim], np.asarray(A["jnt_range"], dtype=np.float64).reshape(-1, 2)[lim]
    assert (st["qpos"][:, qa] >= rg[:, 0] + 0.99 * fm.JOINT_INSET).all() and (st["qpos"][:, qa] <= rg[:, 1] - 0.99 * fm.JOINT_INSET).all()
    # the families
    assert not st["qvel"][fm.FAMILY["rest"][0]].any()
    for e in fm.FAMILY["fast"]:
        w = np.array([np.linalg.norm(st["qvel"][e][d + 3:d + 6]) for d in pd])
        v = np.array([np.linalg.norm(st["qvel"][e][d:d + 3]) for d in pd])
        assert (w >= 10).all() and (w <= 30.001).all() and (v >= 1).all() and (v <= 5.001).all()
    for e in fm.FAMILY["far"]:
        assert all(abs(np.linalg.norm(st["qpos"][e][a:a + 3]) - fm.FAR) < 1e-5 for a in pq)
    for e in range(fm.N):
        nrm = np.array([np.linalg.norm(st["qpos"][e][a + 3:a + 7]) for a in pq])
        if e in fm.FAMILY["unnormalised"]:
            assert (nrm >= 0.5).all() and (nrm <= 2.0).all() and (np.abs(nrm - 1.0) > 1e-3).any()
        else:
            assert np.abs(nrm - 1.0).max() < 1e-6
    e = fm.FAMILY["still-spin"][0]
    assert not st["qvel"][e][pd[0] + 3:pd[0] + 6].any() and st["qvel"][e][pd[0]:pd[0] + 3].any()
    assert np.linalg.norm(st["qvel"][e][pd[1] + 3:pd[1] + 6]) == float(np.float32(1e-18))
    if m.nu:
        cr, fr = np.asarray(A["actuator_ctrlrange"], dtype=np.float64).reshape(-1, 2), np.asarray(A["actuator_forcerange"], dtype=np.float64).reshape(-1, 2)
        cl, fl = np.asarray(A["actuator_ctrllimited"]).astype(bool), np.asarray(A["actuator_forcelimited"]).astype(bool)
        jd = np.asarray(A["jnt_dofadr"], dtype=np.int64)[np.asarray(A["actuator_jntid"], dtype=np.int64)]
        seen_c, seen_f = set(), set()
        for e in fm.FAMILY["ctrl"]:
            c = st["ctrl"][e]
            seen_c |= {("low", "inside", "high")[int(c[u] > cr[u, 0]) + int(c[u] > cr[u, 1])] for u in range(m.nu) if cl[u]}
            frc = refs[e]["actuator"][jd]  # (gear 1, one actuator per dof: the reference's clamped force)
            assert (np.asarray(A["actuator_gear"]) == 1).all() and len(set(jd.tolist())) == m.nu
            seen_f |= {"low" if frc[u] == fr[u, 0] else "high" if frc[u] == fr[u, 1] else "inside" for u in range(m.nu) if fl[u]}
            assert all(fr[u, 0] <= frc[u] <= fr[u, 1] for u in range(m.nu) if fl[u])
        assert seen_c == {"low", "inside", "high"} and seen_f == {"low", "inside", "high"}, (seen_c, seen_f)
    else:
        assert case["name"] == "toy"
    for e in fm.FAMILY["applied"]:
        x = st["xfrc_applied"][e].reshape(-1, 6)
        zero = ~x.any(axis=1)
        assert zero.any() and (~zero).any() and abs(int(zero.sum()) - int((~zero).sum())) <= 1
        assert any((r[:5] == 0).all() and r[5] != 0 for r in x)  # the lone z torque
        assert np.abs(st["qfrc_applied"][e]).min() > 0 and np.abs(st["qfrc_applied"][e]).max() <= 5
        assert np.linalg.norm(x[:, :3], axis=1).max() <= 2.0001 and np.linalg.norm(x[:, 3:], axis=1).max() <= 0.20001
    for e in fm.FAMILY["wrench"]:
        assert not st["qfrc_applied"][e].any() and st["xfrc_applied"][e].reshape(-1, 6)[:, :3].any(axis=1).all()


def _applies(m, defect):
    A = m.arrays
    if defect == "armature":
        return bool(np.asarray(A["dof_armature"]).any())
    if defect in ("ctrl_clamp", "force_clamp"):
        return m.nu > 0
    if defect == "xfrc_arm":  # the arm is the part's centre-of-mass offset
        return bool(np.asarray(A["body_ipos"], dtype=np.float64).reshape(-1, 3)[np.asarray(A["part_bodyid"], dtype=np.int64)].any())
    return True


@pytest.mark.parametrize("defect", fm.DEFECTS)
def test_the_states_can_tell(case, defect):
    """each deliberate defect of the restatement exceeds 100 x the fp32 floor of some measure on some env, on every model that has what the
    defect is about (armature: Baxter; the clamps: a model with actuators; the arm of xfrc: parts whose centre of mass is off their origin)"""
    m, st, name = case["m"], case["st"], case["name"]
    if not _applies(m, defect):
        ref = case["refs"][0]
        assert _rel(fm.restate(m, st, 0, M=ref["M"], defect=defect)["qacc"], ref["qacc"]) <= fm.RESTATE_TOL  # (the defect changes nothing here)
        return
    best = (0.0, None, None)
    for e, ref in enumerate(case["refs"]):
        r = fm.restate(m, st, e, M=ref["M"], defect=defect)
        for k, v in fm.measures(m, ref, {k: r[k] for k in ("xpos", "bias", "qacc", "qvel1", "qpos1")}).items():
            ratio = v / fm.FLOOR[name][fm.group(e)][k]
            if ratio > best[0]:
                best = (ratio, k, e)
    print("%s measured: defect %s shows as %.1f x the floor of %s in env %d" % (name, defect, best[0], best[1], best[2]))
    assert best[0] > fm.CAN_TELL, (name, defect, best)


def _check_floor(name, refs):
    fresh = fm.what_fp32_alone_does(name, refs)
    for g in fm.GROUPS:
        print("%s %s measured: fp32 floor %s" % (name, g, "  ".join("%s %.3e" % kv for kv in fresh[g].items())))
    for g in fm.GROUPS:
        assert set(fresh[g]) == set(fm.FLOOR[name][g])
        for k, v in fresh[g].items():
            assert 0.99 * fm.FLOOR[name][g][k] <= v <= fm.FLOOR[name][g][k], (name, g, k, v, fm.FLOOR[name][g][k])


def test_what_fp32_alone_does(case):
    """FLOOR is what a fresh run of the checker's float32 build gives"""
    _check_floor(case["name"], case["refs"])

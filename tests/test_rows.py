"""The states of tests/test_rows_gpu.py on the CPU (tests/rows_reference.py): every stored state meets the conditions of
tests/solve_reference.py on its inputs, both CPU builds agree on which rows are active, the generator reproduces the file, the float64 reference
is consistent with itself, a solve that does nothing would fail, what fp32 alone does to the four measures (rref.FLOOR, from the checker's float32
build) -- and the coverage the cases exist for, as conditions: every limited joint on both sides and every violation size on a row with force,
many rows at once, rows that are active with exactly zero force; every weld active, and far from the identity.  The device:
tests/test_rows_gpu.py."""
import os

import numpy as np
import pytest

from oracle.oracle_sim import OracleSim
from tests import rows_reference as rref
from tests import solve_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU32 = os.path.join(ROOT, "oracle", "libfsim_cpu32.so")
LIMITS = [n for n, c in rref.CASES.items() if c["kind"] == "limit"]
WELDS = [n for n, c in rref.CASES.items() if c["kind"] == "weld"]


@pytest.fixture(scope="module")
def stored():
    return rref.load()


@pytest.fixture(scope="module")
def solved(stored):
    """name -> per start (cold, warm): the float64 references of every env and the float32 build's qacc, step acceleration and contact pairs"""
    out = {}
    for name, c in stored.items():
        m = rref.model(name)
        o = OracleSim(m)
        out[name] = {}
        for warm in (False, True):
            refs = [sref.reference(o, m, c["st"], e, warm=warm) for e in range(len(c["island"]))]
            out[name][warm] = (refs,) + sref.abi_solve(CPU32, m, c["st"], warm)
        o.close()
    return out


def test_the_file_holds_every_case(stored):
    assert list(stored) == list(rref.CASES)
    for name, c in stored.items():
        m, n = rref.model(name), len(c["island"])
        assert 1 <= n <= sref.MAX_ENVS, name
        shapes = dict(qpos=m.nq, qvel=m.nv, ctrl=m.nu, qfrc_applied=m.nv, xfrc_applied=6 * m.nparts, eq_data=7 * m.neq, eq_active=m.neq, geom_contype=m.ngeom,
                      geom_conaffinity=m.ngeom, qacc_warmstart=m.nv)
        assert {k: c["st"][k].shape for k in sref.FIELDS} == {k: (n, d) for k, d in shapes.items()}, name
        assert all(np.isfinite(c["st"][k]).all() for k in sref.FIELDS)
        assert np.abs(c["st"]["qacc_warmstart"]).max() > 0, name
        assert sorted({int(k) for k in c["island"]}) == sorted(rref.CASES[name]["island"]), name
        assert all(max(k for _, k in rref.CASES[name]["ksets"]) >= k for k in c["island"])
    assert rref.model("welds_billy").nv > 64  # behind the second row pass


@pytest.mark.parametrize("name", list(rref.CASES))
def test_states_meet_the_conditions(name, stored, solved):
    """solve_reference.conditions; every geom is off except in the one contact env, and there is no contact anywhere else, in either build; both builds
    hold the same rows active: the contact pairs (conditions), the welds (an input), and every side of every limited joint, decided in float32 as in float64"""
    m, c = rref.model(name), stored[name]
    refs, _, _, pairs32 = solved[name][False]
    on = [e for e in range(len(refs)) if c["st"]["geom_contype"][e].any() or c["st"]["geom_conaffinity"][e].any()]
    assert on == ([len(refs) - 1] if name == "limits_sawyer" else [])
    for e, ref in enumerate(refs):
        assert rref.conditions(m, name, c["st"], e, ref, pairs32[e]) == [], (name, e)
        assert sref.island_dofs(m, ref["contacts"], c["st"]["eq_active"][e])[0] == c["island"][e]
        assert (len(ref["contacts"]) == 0 and len(pairs32[e]) == 0) or e in on, (name, e)
        v64, v32 = rref.violations(m, c["st"]["qpos"][e]), rref.violations(m, c["st"]["qpos"][e], np.float32)
        assert ((v64 > 0) == (v32 > 0)).all(), (name, e)
        if e in on:  # contact rows and limit rows in one island of 15 dofs
            dof = rref.limits(m)["dof"]
            assert len(ref["contacts"]) >= 1 and len(ref["islands"][0]) == 15 and any(v64[j].max() > 0 and d in ref["islands"][0] for j, d in enumerate(dof))
    print("%s: largest island %s, contacts %s, float64 Newton iterations cold %s warm %s" % (
        name, c["island"].tolist(), [len(r["contacts"]) for r in refs], [r["iters"] for r in refs], [r["iters"] for r in solved[name][True][0]]))


@pytest.mark.parametrize("name", LIMITS)
def test_limit_states_cover_every_row(name, stored, solved):
    """every (limited joint, side) carries force in some env, every violation size occurs on a row with force, one env has many rows with force at
    once, and the last-but-one env (Sawyer; Baxter: the last) holds at least two violated rows whose force is exactly 0 -- the joint leaves its limit"""
    m, c = rref.model(name), stored[name]
    lm, refs = rref.limits(m), solved[name][False][0]
    loaded, sizes, most, zero = set(), set(), 0, []
    for e, ref in enumerate(refs):
        if len(ref["contacts"]):
            continue  # (with a contact on the arm, qfrc_constraint on a limited dof is not the row's force alone)
        v, f = rref.violations(m, c["st"]["qpos"][e]), ref["qfrc_constraint"][lm["dof"]]
        assert (f[v.max(axis=1) <= 0] == 0).all() and (f[v[:, 0] > 0] >= 0).all() and (f[v[:, 1] > 0] <= 0).all(), (name, e)
        rows = [(j, side) for j in range(len(f)) for side in (0, 1) if v[j, side] > 0]
        assert all(rref.size_index(v[j, side], lm["slide"][j]) >= 0 for j, side in rows), (name, e)
        loaded |= {r for r in rows if f[r[0]] != 0}
        sizes |= {(bool(lm["slide"][j]), rref.size_index(v[j, side], lm["slide"][j])) for j, side in rows if f[j] != 0}
        most = max(most, sum(f[j] != 0 for j, _ in rows))
        zero.append(sum(f[j] == 0 for j, _ in rows))
    print("%s: %d (joint, side) with force, sizes %s, at most %d rows with force at once, violated rows without force per env %s" % (name, len(loaded), sorted(sizes), most, zero))
    assert loaded == {(j, side) for j in range(len(lm["dof"])) for side in (0, 1)}
    assert {k for slide, k in sizes if not slide} == set(range(7)) and {k for slide, k in sizes if slide} == set(range(7))
    assert most >= rref.CASES[name]["many"]
    assert zero[6 if name == "limits_sawyer" else 7] >= 2 and sum(zero) == zero[6 if name == "limits_sawyer" else 7]


@pytest.mark.parametrize("name", WELDS)
def test_weld_states_cover_every_weld(name, stored, solved):
    """every weld of the model is active in some env and every active weld carries force on both its parts; the pose errors are the sizes of
    rref.WELD_ERRORS, the largest quaternion error at least QUAT_ERROR in the vector part"""
    m, c = rref.model(name), stored[name]
    active = c["st"]["eq_active"].astype(bool)
    assert active.any(axis=0).all(), name
    worst = np.zeros(6)
    for e, ref in enumerate(solved[name][False][0]):
        err = np.abs(rref.weld_errors(m, c["st"]["qpos"][e], c["st"]["eq_data"][e]))[active[e]]
        worst = np.maximum(worst, err.max(axis=0))
        for k in np.nonzero(active[e])[0]:
            for p in (int(m.eq_part1[k]), int(m.eq_part2[k])):
                assert np.abs(ref["qfrc_constraint"][int(m.part_dofadr[p]):][:6]).min() > 0, (name, e, k)
        for p in range(m.nparts):  # a part outside the sub-assembly is free
            if not any(active[e][k] and p in (int(m.eq_part1[k]), int(m.eq_part2[k])) for k in range(m.neq)):
                assert (ref["qfrc_constraint"][int(m.part_dofadr[p]):][:6] == 0).all()
    print("%s: largest pose error of an active weld %s m, %s in the quaternion's vector part" % (name, worst[:3].max(), worst[3:].max()))
    assert worst[3:].max() >= rref.QUAT_ERROR and worst[:3].max() >= rref.WELD_ERRORS[-1][0]


def test_generator_reproduces_the_file():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_row_states", os.path.join(ROOT, "scripts", "make_golden_row_states.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = sref.pack(gen.generate())
    with np.load(rref.GOLDEN) as z:
        assert sorted(z.files) == sorted(new)
        for k in z.files:
            assert z[k].dtype == new[k].dtype and z[k].tobytes() == new[k].tobytes(), k


@pytest.mark.parametrize("name", list(rref.CASES))
def test_the_reference_is_consistent_with_itself(name, solved):
    """M (qacc - qacc_smooth) = qfrc_constraint, and the cold start against the warm start"""
    ident = cw = 0.0
    for cold, warm in zip(solved[name][False][0], solved[name][True][0]):
        for r in (cold, warm):
            ident = max(ident, sref.force(r["qacc"], r))
        cw = max(cw, np.abs(cold["qacc"] - warm["qacc"]).max() / max(np.abs(cold["qacc"]).max(), 1.0))
        assert sorted(cold["contacts"]) == sorted(warm["contacts"])
    print("%s measured: identity %.3e, cold against warm %.3e" % (name, ident, cw))
    assert ident <= sref.IDENTITY_TOL and cw <= sref.COLD_WARM_TOL


@pytest.mark.parametrize("name", list(rref.CASES))
def test_a_solve_that_does_nothing_would_fail(name, stored, solved):
    """the cold start's candidates, qacc = 0 and qacc = qacc_smooth, miss the solution in every env by the `island` measure"""
    refs = solved[name][False][0]
    zero = [sref.island(np.zeros_like(r["qacc"]), r) for r in refs]
    smooth = [sref.island(r["qacc_smooth"], r) for r in refs]
    print("%s measured: qacc = 0 %s, qacc_smooth %s" % tuple([name] + [" ".join("%.1e" % v for v in x) for x in (zero, smooth)]))
    assert min(zero + smooth) >= sref.START_FLOORS * rref.FLOOR[name]["island"]


@pytest.mark.parametrize("name", list(rref.CASES))
def test_what_fp32_alone_does(name, solved):
    """the four measures of the checker's float32 build against float64, cold and warm: rref.FLOOR holds, and no case is vacuous"""
    grp = rref.groups(rref.model(name))
    worst = dict.fromkeys(rref.MEASURES, 0.0)
    for warm in (False, True):
        refs, qacc, acc, _ = solved[name][warm]
        vals = [rref.measure(qacc[e], acc[e], ref, grp) for e, ref in enumerate(refs)]
        for k in rref.MEASURES:
            worst[k] = max(worst[k], max(v[k] for v in vals))
        print("%-14s %s: fp32 floor %s" % (name, "warm" if warm else "cold", "  ".join("%s %.3e (%s)" % (k, max(v[k] for v in vals), " ".join("%.1e" % v[k] for v in vals)) for k in rref.MEASURES)))
    print("%s measured: fp32 floor %s" % (name, "  ".join("%s %.3e" % (k, worst[k]) for k in rref.MEASURES)))
    assert all(worst[k] <= rref.FLOOR[name][k] for k in rref.MEASURES)
    assert all(worst[k] <= sref.VACUITY for k in rref.MEASURES)

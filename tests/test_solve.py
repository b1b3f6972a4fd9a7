"""The states of tests/test_solve_gpu.py on the CPU (tests/solve_reference.py): every stored state meets the conditions on its inputs --
away from the contact and limit thresholds, its largest island on the path the case exists for, its contacts within the slots --, the
generator reproduces the file, the float64 reference is consistent with itself, and what fp32 alone does to the three measures
(sref.FLOOR, from the checker's float32 build).  The device: tests/test_solve_gpu.py."""
import os

import numpy as np
import pytest

from oracle.oracle_sim import OracleSim
from tests import solve_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU32 = os.path.join(ROOT, "oracle", "libfsim_cpu32.so")


@pytest.fixture(scope="module")
def stored():
    return sref.load()


@pytest.fixture(scope="module")
def solved(stored):
    """name -> per start (cold, warm): the float64 references of every env and the float32 build's qacc, step acceleration and contact pairs"""
    out = {}
    for name, c in stored.items():
        m = sref.model(name)
        o = OracleSim(m)
        out[name] = {}
        for warm in (False, True):
            refs = [sref.reference(o, m, c["st"], e, warm=warm) for e in range(len(c["island"]))]
            out[name][warm] = (refs,) + sref.abi_solve(CPU32, m, c["st"], warm)
        o.close()
    return out


def test_the_file_holds_every_case(stored):
    assert list(stored) == list(sref.CASES)
    for name, c in stored.items():
        m, n = sref.model(name), len(c["island"])
        assert 1 <= n <= sref.MAX_ENVS, name
        shapes = dict(qpos=m.nq, qvel=m.nv, ctrl=m.nu, qfrc_applied=m.nv, xfrc_applied=6 * m.nparts, eq_data=7 * m.neq, eq_active=m.neq, geom_contype=m.ngeom,
                      geom_conaffinity=m.ngeom, qacc_warmstart=m.nv)
        assert {k: c["st"][k].shape for k in sref.FIELDS} == {k: (n, d) for k, d in shapes.items()}, name
        assert all(np.isfinite(c["st"][k]).all() for k in sref.FIELDS)
        assert np.abs(c["st"]["qacc_warmstart"]).max() > 0, name  # the warm start is one
    # the sizes between them: the rows (<= 16), the tile (17..31), fs_chol_lds (32..64), fs_chol_all_lds (> 64); the piles behind the second row pass
    lack = sorted({int(k) for n, c in stored.items() if sref.CASES[n]["model"] == sref.LACK for k in c["island"]})
    piles = sorted({int(k) for n, c in stored.items() if sref.CASES[n]["model"] == sref.BILLY for k in c["island"]})
    assert lack == [9, 15, 21, 30, 39] and piles == [12, 18, 30, 36, 60, 66] and sref.model("pile2").nv > 64


@pytest.mark.parametrize("name", list(sref.CASES))
def test_states_meet_the_conditions(name, stored, solved):
    m, c = sref.model(name), stored[name]
    refs, _, _, pairs32 = solved[name][False]
    for e, ref in enumerate(refs):
        assert sref.conditions(m, name, c["st"], e, ref, pairs32[e]) == [], (name, e)
        assert sref.island_dofs(m, ref["contacts"], c["st"]["eq_active"][e])[0] == c["island"][e]
    print("%s: largest island %s, contacts %s, float64 Newton iterations cold %s warm %s" % (
        name, c["island"].tolist(), [len(r["contacts"]) for r in refs], [r["iters"] for r in refs], [r["iters"] for r in solved[name][True][0]]))
    if name == "limit":  # the limit row is there and carries force: the wrist joint is beyond its range and pushed back
        from tests.solve_bits_common import LIMIT_JOINT
        assert all(c["st"]["qpos"][e][LIMIT_JOINT] > m.jnt_range[LIMIT_JOINT][1] and r["qfrc_constraint"][LIMIT_JOINT] < 0 for e, r in enumerate(refs))
    if name in ("weld", "table30", "welded39"):
        assert c["st"]["eq_active"].any(axis=1).all()
    if name in ("table30", "welded39"):
        assert c["st"]["eq_active"].all()


def test_generator_reproduces_the_file():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_solve_states", os.path.join(ROOT, "scripts", "make_golden_solve_states.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = sref.pack(gen.generate())
    with np.load(sref.GOLDEN) as z:
        assert sorted(z.files) == sorted(new)
        for k in z.files:
            assert z[k].dtype == new[k].dtype and z[k].tobytes() == new[k].tobytes(), k


@pytest.mark.parametrize("name", list(sref.CASES))
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


@pytest.mark.parametrize("name", list(sref.CASES))
def test_a_solve_that_does_nothing_would_fail(name, stored, solved):
    """the start points against the solution, by the `island` measure: qacc = 0 and qacc = qacc_smooth, the cold start's candidates, miss it in every
    env; the stored warm start is printed (a previous step's solution is close, which is its purpose)"""
    refs = solved[name][False][0]
    zero = [sref.island(np.zeros_like(r["qacc"]), r) for r in refs]
    smooth = [sref.island(r["qacc_smooth"], r) for r in refs]
    warm = [sref.island(stored[name]["st"]["qacc_warmstart"][e], r) for e, r in enumerate(refs)]
    print("%s measured: qacc = 0 %s, qacc_smooth %s, warm start %s" % tuple([name] + [" ".join("%.1e" % v for v in x) for x in (zero, smooth, warm)]))
    assert min(zero + smooth) >= sref.START_FLOORS * sref.FLOOR[name]["island"]


@pytest.mark.parametrize("name", list(sref.CASES))
def test_what_fp32_alone_does(name, solved):
    """the three measures of the checker's float32 build against float64, cold and warm: sref.FLOOR holds, and no case is vacuous"""
    worst = dict.fromkeys(sref.MEASURES, 0.0)
    for warm in (False, True):
        refs, qacc, acc, _ = solved[name][warm]
        vals = [sref.measure(qacc[e], acc[e], ref) for e, ref in enumerate(refs)]
        for k in sref.MEASURES:
            worst[k] = max(worst[k], max(v[k] for v in vals))
        print("%-10s %s: fp32 floor %s" % (name, "warm" if warm else "cold", "  ".join("%s %.3e (%s)" % (k, max(v[k] for v in vals), " ".join("%.1e" % v[k] for v in vals)) for k in sref.MEASURES)))
    print("%s measured: fp32 floor %s" % (name, "  ".join("%s %.3e" % (k, worst[k]) for k in sref.MEASURES)))
    assert all(worst[k] <= sref.FLOOR[name][k] for k in sref.MEASURES)
    assert worst["force"] <= sref.VACUITY and worst["island"] <= sref.VACUITY

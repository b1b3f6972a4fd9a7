"""ONE Newton solve of the device per kind of constraint row of csrc/fsim_solver.hpp fs_make_constraints, against float64: the stored states of
tests/rows_reference.py -- every limited joint of the Sawyer and of Baxter beyond its range on either side, by 0.2 to 0.9 of the impedance
curve's width and far beyond it, one to nineteen limit rows at once, rows that are active and carry no force, limit rows in one island with a contact;
the welds of three models with pose errors up to 2e-2 m and 0.3 rad, 1 to 37 welds at once, islands of 12 to 66 dofs -- on every kernel set that
can hold them, from a cold start and from the stored warm start.  The procedure is that of tests/test_solve_gpu.py: set_state ->
fsim_physics_forward -> qacc, the contact list and the iteration count, and on a twin handle set_state -> fsim_physics_step(1) -> qvel.

Per env, none skipped: qacc is finite; the device lists no contact where the reference lists none (every geom of these states is off) and the
reference's pairs in the one contact env; the four measures of rows_reference (force, island, step of solve_reference, and row: each limited
joint's dof and each part's six dofs judged near its own force) against float64; the iteration count within 3 of the oracle's at the device's own
tolerance and never at the cap; and all kernel sets agree with each other.

The tolerance of a measure is 4 x the largest value measured on an MI355X for the case (the rule of DESIGN.md 15; the values: DESIGN.md 24).
One condition is not a measurement: a measured value above 10 x the case's fp32 floor (rref.FLOOR) is a defect to find, not a tolerance to
widen -- these states found one in the weld cases (test_the_condition_on_the_measured_values).  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from furniture_amd.sim import default_config
from oracle.oracle_sim import OracleSim
from tests import rows_reference as rref
from tests import solve_reference as sref

pytestmark = pytest.mark.gpu
# case -> the largest value of each measure on an MI355X, over its envs, its kernel sets and both starts
MEASURED = {
    "limits_sawyer": dict(force=7.990e-05, island=2.136e-05, step=8.383e-05, row=2.514e-03),
    "limits_baxter": dict(force=3.239e-05, island=3.330e-05, step=3.730e-05, row=3.239e-03),
    "welds_lack": dict(force=3.723e-05, island=1.836e-05, step=3.767e-05, row=8.890e-04),
    "welds_billy": dict(force=7.232e-04, island=7.232e-04, step=7.232e-04, row=1.153e-03),
    "welds_desk": dict(force=1.314e-04, island=1.314e-04, step=1.314e-04, row=2.818e-04),
}
TOL = {g: {k: 4.0 * v for k, v in d.items()} for g, d in MEASURED.items()}
ITER_SLACK = 3  # (the bound of tests/test_solve_gpu.py)
N = sref.MAX_ENVS
RUNS = [(name, ks) for name, c in rref.CASES.items() for ks, _ in c["ksets"]]
_handles, _runs, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    sref.close_handles(_handles)


@pytest.fixture(scope="module")
def stored():
    return rref.load()


def _envs(name, ks, stored):
    """the envs of the case that the kernel set is given: those whose largest island it holds"""
    return [e for e, k in enumerate(stored[name]["island"]) if k <= dict(rref.CASES[name]["ksets"])[ks]]


def _reference(name, stored, warm):
    """the float64 references of a case (solver at 1e-14) and the oracle's iteration counts at the device's own tolerance and cap"""
    if (name, warm) not in _refs:
        m, st = rref.model(name), stored[name]["st"]
        cfg = default_config()
        o = OracleSim(m)
        refs = [sref.reference(o, m, st, e, warm=warm) for e in range(len(st["qpos"]))]
        for e, r in enumerate(refs):
            r["iters_dev_tol"] = sref.reference(o, m, st, e, warm=warm, iterations=cfg.solver_iterations, tolerance=cfg.solver_tolerance, step=False)["iters"]
        o.close()
        _refs[(name, warm)] = refs
    return _refs[(name, warm)]


def _run(name, ks, stored, warm):
    """one solve and one substep of every env of the case that the kernel set is given -> dict of arrays indexed as those envs are"""
    if (name, ks, warm) not in _runs:
        m, st, envs = rref.model(name), stored[name]["st"], _envs(name, ks, stored)
        assert sref.KSETS[ks]["model"] == rref.CASES[name]["model"] and envs
        n = len(envs)
        rows = np.asarray(envs)[np.arange(N) % n]  # (fewer than N envs: its envs again)
        fields = {k: st[k][rows] for k in sref.FIELDS if st[k].shape[1] > 0}
        if not warm:
            fields["qacc_warmstart"] = np.zeros((N, m.nv))
        sim, twin = sref.handle(_handles, ks, N)
        sim.set_state(**fields)
        sim.physics_forward()
        got = {k: v.cpu().numpy()[:n] for k, v in sim.get_state("qacc", "ncon", "contact_geoms", "solver_iters").items()}
        twin.set_state(**fields)
        twin.physics_step(1)
        qvel = twin.get_state("qvel")["qvel"].cpu().numpy()[:n].astype(np.float64)
        got["acc_step"] = (qvel - st["qvel"][envs]) / float(m.arrays["opt"][0])
        got["pairs"] = [[(int(a), int(b)) for a, b in got["contact_geoms"][i].reshape(-1, 2) if a >= 0] for i in range(n)]
        _runs[(name, ks, warm)] = got
    return _runs[(name, ks, warm)]


@pytest.mark.parametrize("name", list(rref.CASES))
def test_the_condition_on_the_measured_values(name):
    """no measured value is above 10 x what fp32 alone does.  The weld cases were, from a cold start, before fs_solve's last exit learnt about weld rows:
    force 2.921e-3 against a floor of 3.419e-5 (welds_lack), 5.875e-3 against 5.473e-4 (welds_billy), 3.170e-3 against 1.262e-4 (welds_desk); DESIGN.md 24"""
    for k, v in MEASURED[name].items():
        assert 0 < v <= 10.0 * rref.FLOOR[name][k], (name, k, v, rref.FLOOR[name][k])


@pytest.mark.parametrize("name,ks", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_one_solve_against_float64(name, ks, stored):
    m, c, cfg = rref.model(name), stored[name], default_config()
    grp = rref.groups(m)
    worst, lines, checks = dict.fromkeys(rref.MEASURES, 0.0), [], []
    for warm in (False, True):
        refs, got = _reference(name, stored, warm), _run(name, ks, stored, warm)
        for i, e in enumerate(_envs(name, ks, stored)):
            ref = refs[e]
            assert np.isfinite(got["qacc"][i]).all() and np.isfinite(got["acc_step"][i]).all(), (name, ks, warm, e)
            assert int(got["ncon"][i, 0]) == len(got["pairs"][i]) <= sref.KSETS[ks]["slots"]
            # every geom is off: no contact on either side; the contact env: the reference's pairs (conditions keep them CONTACT_BAND from their margin)
            assert {sref.pair_key(*p) for p in got["pairs"][i]} == {sref.pair_key(*p) for p in ref["contacts"]}, (name, ks, warm, e, got["pairs"][i], ref["contacts"])
            assert len(got["pairs"][i]) == len(ref["contacts"]) and (len(ref["contacts"]) == 0 or c["st"]["geom_contype"][e].any())
            v = rref.measure(got["qacc"][i], got["acc_step"][i], ref, grp)
            it = int(got["solver_iters"][i, 0])
            lines.append("%s %s %s env %d: island %d, contacts %d, %s, iterations %d (oracle %d)" % (
                name, ks, "warm" if warm else "cold", e, c["island"][e], len(got["pairs"][i]), " ".join("%s %.3e" % (k, v[k]) for k in rref.MEASURES), it, ref["iters_dev_tol"]))
            for k in rref.MEASURES:
                worst[k] = max(worst[k], v[k])
            checks.append((warm, e, it, ref["iters_dev_tol"]))
    print("\n".join(lines))
    print("%s %s measured: %s" % (name, ks, "  ".join("%s %.3e" % (k, worst[k]) for k in rref.MEASURES)))
    wrong = ["%s %.3e exceeds %.3e" % (k, worst[k], TOL[name][k]) for k in rref.MEASURES if not worst[k] <= TOL[name][k]]
    wrong += ["%s env %d: %d iterations, the oracle %d" % ("warm" if warm else "cold", e, it, it_ref) for warm, e, it, it_ref in checks
              if abs(it - it_ref) > ITER_SLACK or it >= cfg.solver_iterations]
    assert not wrong, wrong


@pytest.mark.parametrize("name", list(rref.CASES))
def test_the_kernel_sets_agree(name, stored):
    """qacc of every pair of kernel sets on the envs both are given, as a force through M on the scale of `force`: within twice the tolerance of `force`"""
    worst = 0.0
    sets = [ks for n, ks in RUNS if n == name]
    for warm in (False, True):
        refs = _reference(name, stored, warm)
        runs = [dict(zip(_envs(name, ks, stored), _run(name, ks, stored, warm)["qacc"])) for ks in sets]
        for e, ref in enumerate(refs):
            scale = np.abs(ref["qfrc_constraint"]).max()
            f = np.stack([ref["M"] @ r[e].astype(np.float64) for r in runs if e in r])
            assert len(f) == sum(k >= stored[name]["island"][e] for _, k in rref.CASES[name]["ksets"])
            worst = max(worst, np.abs(f[:, None] - f[None, :]).max() / (scale if scale > 0 else 1.0))
    print("%s measured: kernel sets %s differ by %.3e" % (name, sets, worst))
    assert len(sets) >= 2 and worst <= 2.0 * TOL[name]["force"]


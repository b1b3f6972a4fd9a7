"""The connect action of the step kernels on the device against float64: env_try_connect, env_is_aligned_core, env_lookat, env_slerp, env_ttq,
env_move_group, env_connect with its lift and weld of csrc/fsim_env.hpp, in the cases of tests/connect_reference.py -- every allowed angle with
and without a twist in each branch of env_lookat, connectors without an angle list down to a twist of exactly 0, two-angle and single-angle
connectors, lateral offset, gap and tilt, welded groups of 2 to 4 parts on either side, the exits of the slerp, 1.3 m from the origin, the floor
lift kept and undone, and one refusal per threshold.  One handle per model and kernel set, one env per case: Cursor + table_lack_0825 on its
default kernel and with four waves per env (FSIM_MW=all), toy_table, chair_agne_0007 and desk_mikael_1064 on their default kernels.

Per env, none skipped: everything is finite; every integer is the reference's after every call -- num_connected, connected_this_step (so the call
at which it connects), eq_active, the group roots, both mask arrays, the cursors' selection words (cursor 1's dropped by the connect); a refused env
never connects, its held parts stay where they are, and its twin connects on the 11th call after the counter was at 3 and restarted; every
measure of connect_reference.measures is within its tolerance.

The tolerance of a measure is 4 x the largest value measured on an MI355X against float64 over the kernel sets of the model (the rule of
DESIGN.md 15; the values: DESIGN.md 27), kept apart for the cases 1.3 m out and for the lift (cr.GROUPS).  One condition is not a measurement: a
measured value above 10 x the model's fp32 floor (cr.FLOOR: what the checker's float32 build does to the same measure) would be a defect to
find, not a tolerance to widen.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from furniture_amd import sim as fsim
from tests import connect_reference as cr
from tests.test_solve_gpu import _environment

pytestmark = pytest.mark.gpu
# model -> group -> the largest value of each measure on an MI355X, over the cases of the group and the kernel sets of the model
MEASURED = {
    "lack": dict(
        near=dict(approach_pos=1.677e-07, approach_ang=3.658e-07, snap_pos=2.047e-07, snap_ang=3.305e-07, site_gap=1.957e-07, site_ang=3.305e-07, rigid=2.435e-07, weld_pos=1.424e-07, weld_ang=3.375e-07, qnorm=1.327e-07, still=0.000e+00),
        far=dict(approach_pos=8.723e-08, approach_ang=1.480e-07, snap_pos=2.118e-07, snap_ang=3.491e-07, site_gap=1.998e-07, site_ang=3.491e-07, weld_pos=1.926e-07, weld_ang=2.541e-07, qnorm=1.257e-07),
        lift=dict(approach_pos=1.200e-07, approach_ang=2.731e-07, snap_pos=1.661e-07, snap_ang=5.048e-07, site_gap=1.059e-07, site_ang=5.048e-07, weld_pos=8.027e-08, weld_ang=3.068e-07, qnorm=1.188e-07),
    ),
    "toy": dict(
        near=dict(approach_pos=3.277e-07, approach_ang=1.368e-06, snap_pos=9.147e-07, snap_ang=3.107e-06, site_gap=2.276e-07, site_ang=3.107e-06, weld_pos=9.002e-07, weld_ang=3.096e-06, qnorm=1.263e-07, still=0.000e+00),
        parallel=dict(approach_pos=9.785e-05, approach_ang=3.883e-04, snap_pos=1.653e-04, snap_ang=5.905e-04, site_gap=3.073e-07, site_ang=5.905e-04, weld_pos=1.653e-04, weld_ang=5.905e-04, qnorm=1.209e-07),
    ),
    "agne": dict(
        near=dict(approach_pos=1.925e-07, approach_ang=2.177e-07, snap_pos=1.547e-07, snap_ang=1.717e-07, site_gap=1.532e-07, site_ang=1.584e-07, weld_pos=1.211e-07, weld_ang=1.542e-07, qnorm=1.327e-07, still=0.000e+00),
    ),
    "desk": dict(
        near=dict(approach_pos=1.196e-07, approach_ang=2.919e-07, snap_pos=2.245e-07, snap_ang=2.917e-07, site_gap=2.002e-07, site_ang=2.792e-07, weld_pos=1.633e-07, weld_ang=1.822e-07, qnorm=1.376e-07, still=0.000e+00),
    ),
}
TOL = {n: {g: {k: 4.0 * v for k, v in d.items()} for g, d in gs.items()} for n, gs in MEASURED.items()}
# kernel set -> model (of cr.MODELS) and the environment fsim_create reads
KSETS = {
    "lack": dict(name="lack", env={}),
    "lack-mwall": dict(name="lack", env=dict(FSIM_MW="all")),
    "toy": dict(name="toy", env={}),
    "agne": dict(name="agne", env={}),
    "desk": dict(name="desk", env={}),
}
_runs = {}


def _run(ks):
    """list over the cases of {calls: [...]} from a handle of the kernel set (cr.abi_run)"""
    if ks not in _runs:
        from tests.abi_session import Abi, Session
        k = KSETS[ks]
        m, cs = cr.model(k["name"]), cr.cases(k["name"])
        with _environment(k["env"]):
            ses = Session(Abi(fsim.library_path(), device="cuda"), m.to_blob(), len(cs), auto_reset=0)
        try:
            _runs[ks] = cr.abi_run(ses, m, cs)
        finally:
            ses.close()
    return _runs[ks]


def test_the_condition_on_the_measured_values():
    assert set(MEASURED) == set(cr.MODELS)
    for name, gs in MEASURED.items():
        assert set(gs) == set(cr.FLOOR[name]), name
        for g, d in gs.items():
            assert set(d) == set(cr.FLOOR[name][g]), (name, g)
            for k, v in d.items():
                # (a refused part that does not move at all does so on every side: 0 <= 0)
                assert 0 <= v <= 10.0 * cr.FLOOR[name][g][k] and (v > 0 or k == "still"), (name, g, k, v, cr.FLOOR[name][g][k])


def test_every_model_has_a_kernel_set():
    assert {k["name"] for k in KSETS.values()} == set(cr.MODELS)
    assert {ks for ks, k in KSETS.items() if k["name"] == "lack"} == {"lack", "lack-mwall"}


@pytest.mark.parametrize("ks", list(KSETS))
def test_connect_against_float64(ks):
    name = KSETS[ks]["name"]
    m, cs, refs = cr.model(name), cr.cases(name), cr.reference(name)
    got = _run(ks)
    worst, wrong = {}, []
    for e, (c, r, g) in enumerate(zip(cs, refs, got)):
        tag = "case %d (%s%s%s)" % (e, c["family"], " " + c["note"] if c["note"] else "", " refused: " + c["refused"] if c["refused"] else "")
        if not cr.finite(g):
            t = [t for t, rec in enumerate(g["calls"]) if not (np.isfinite(rec["qpos"]).all() and np.isfinite(rec["eq_data"]).all())][0]
            wrong.append("%s: not finite after call %d" % (tag, t))
            print("%s %s: NOT FINITE after call %d" % (ks, tag, t))
            continue
        at, at_ref = cr.connected_at(g["calls"][:len(r["calls"])]), cr.connected_at(r["calls"])
        if at != at_ref:
            wrong.append("%s: connects at calls %s, the reference at %s" % (tag, at, at_ref))
        names = ("num_connected", "connected_this_step", "eq_active", "group roots", "geom_contype", "geom_conaffinity", "cursor selection")
        for t in range(len(r["calls"])):
            a, b = cr.integers(r["calls"][t]), cr.integers(g["calls"][t])
            if a != b:
                wrong.append("%s: after call %d %s differ from the reference's" % (tag, t, ", ".join(n for n, x, y in zip(names, a, b) if x != y)))
                break
        # (the reference: at call 11 and never again; refused: never in the refused calls, the twin on its 11th call after the restart -- tests/test_connect.py)
        assert at_ref == ([cr.SECOND_CONNECT] if c["refused"] else [cr.CALLS]), (tag, at_ref)
        if at != at_ref:  # (what follows compares poses call by call)
            continue
        v = cr.measures(m, c, r, g)
        print("%s %s [%s]: %s" % (ks, tag, c["group"], "  ".join("%s %.3e" % kv for kv in v.items())))
        w = worst.setdefault(c["group"], {})
        for k, x in v.items():
            w[k] = max(w.get(k, 0.0), float(x))
    for grp, w in worst.items():
        print("%s %s measured: dict(%s)" % (ks, grp, ", ".join("%s=%.3e" % kv for kv in w.items())))
    assert name in TOL, "no measured values for %s" % name
    for grp, w in worst.items():
        assert set(w) == set(TOL[name][grp]), (ks, grp, sorted(w))
        for k, x in w.items():
            # a refused env's parts are held to the tolerance of a re-posed part
            tol = TOL[name][grp]["snap_pos"] if k == "still" else TOL[name][grp][k]
            if not x <= tol:
                wrong.append("%s %s %.3e exceeds %.3e" % (grp, k, x, tol))
    assert not wrong, wrong

"""The step kernels leave the same BITS as the library that tests/golden/solve_bits.npz was recorded with (scripts/make_golden_solve_bits.py).

Work on the Newton solve that removes instructions without touching the arithmetic -- operand forms, selects, register traffic -- has to leave every
floating-point operation and its order as it was; this test holds it to that, word by word: qpos, qvel, qacc_warmstart, observation, reward, done, the
info row, the Newton iteration count and the four-wave step count after each of six steps, from stored start snapshots and stored actions.  The
scenarios are the smallest that reach each factorisation path (tests/solve_bits_common.py), each under FSIM_MW = 0, 1 and all, which pins the
one-wave, the bundle / team and the four-wave instantiations of the solver.  So that a case cannot pass by missing its path, the islands the device
itself reports (its contact list and active welds after every step) must show the size the case exists for."""
import numpy as np
import pytest

from tests.solve_bits_common import CASES, GOLDEN, LIMIT_JOINT, MODES, record

pytestmark = pytest.mark.gpu

BITS = ("qpos", "qvel", "qacc_warmstart", "obs", "reward", "done", "info", "niter", "mw_steps", "eq_active", "ncon", "island")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_step_bits_match_the_recorded_library(sawyer_lack, golden, name, mode):
    m, c = sawyer_lack, CASES[name]
    pre = "%s/snap/" % name
    snap = {k[len(pre):]: golden[k] for k in golden.files if k.startswith(pre)}
    acts = golden["%s/actions" % name]
    assert acts.shape == (c["steps"], c["n"], 9)
    rec = record(m, mode, snap, acts)
    # the path the case exists for was taken
    lo, hi = c["island"]
    isl = rec["island"]
    assert ((isl >= lo) & (isl <= hi)).any(), ("no env reached an island of %d..%d dofs" % (lo, hi), isl.tolist())
    assert (rec["niter"] >= 50).all(), "fewer Newton iterations than substeps"
    if mode == "0":
        assert (rec["mw_steps"] == 0).all()
    elif mode == "all":
        assert (rec["mw_steps"][-1] == c["steps"]).all()
    elif name in ("grip_table", "weld"):  # the rule did send the hard envs to the four-wave teams (never on the first step: no history yet)
        assert (rec["mw_steps"][-1] > 0).all() and (rec["mw_steps"][-1] < c["steps"]).all(), rec["mw_steps"][-1].tolist()
    if name == "weld":
        assert rec["eq_active"][-1].any(axis=1).all(), "no weld became active"
    if name == "limit":  # the wrist started 0.01 rad beyond its range: an active limit row pushed it back
        q0, q1 = snap["qpos"].view(np.float32)[:, LIMIT_JOINT], rec["qpos"][0].view(np.float32)[:, LIMIT_JOINT]
        assert (q0 > m.jnt_range[LIMIT_JOINT][1]).all() and (q1 < q0 - 1e-4).all(), (q0.tolist(), q1.tolist())
    # every word
    for k in BITS:
        want = golden["%s/%s/%s" % (name, mode, k)]
        assert rec[k].shape == want.shape and rec[k].dtype == want.dtype, k
        bad = np.argwhere(rec[k] != want)
        assert len(bad) == 0, "%s: %d of %d words differ, first at (step, env, ...) = %s" % (k, len(bad), want.size, bad[0].tolist())

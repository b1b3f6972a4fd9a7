"""The free-motion dynamics and the integrator of the step kernels on the device against float64: fs_kinematics, fs_com_inertia,
fs_crb_factor, fs_velocity_bias and fs_smooth of csrc/fsim_physics.hpp, the unconstrained exit of fs_solve and fs_integrate_body of
csrc/fsim_solver.hpp, in the states of tests/freemotion_reference.py -- every geom switched off, so that no state has a contact and none is
skipped: at rest, fast, 8 m from the origin, with unnormalised quaternions, with a spin of exactly 0 and of 1e-18, with ctrl and gripper
force at and beyond their clamps, with qfrc_applied and xfrc_applied -- on the ten kernel sets of tests/test_solve_gpu.py, on Baxter +
table_liden_0921 (nv = 91, a reduced body on bit 31 of the masks) with two and with eight contact-slot sets per lane (its 12 parts put it
on the kernels with 128 slots, which have one wave per env: fsim_create refuses FSIM_MW=all for it, which is checked), on Cursor + toy_table
and on the torque variant of Sawyer + table_lack_0825.  A run is one handle of 8 envs: set_state -> fsim_physics_forward -> qacc, xpos, xquat,
qfrc_bias, qpos, ncon; set_state again -> fsim_physics_step(1) -> qvel, qpos; set_state again -> fsim_physics_step(100) -> qpos.

Per env, none skipped: everything is finite; ncon == 0; qpos after the forward pass holds the normalised quaternions and nothing else has
changed; every measure of freemotion_reference.measures is within its tolerance; the parts of the still-spin state get the reference's new
quaternion.

The tolerance of a measure is 4 x the largest value measured on an MI355X against float64 over the kernel sets of the model (the rule of
DESIGN.md 15; the values: DESIGN.md 23), kept apart for the env 8 m out (fm.GROUPS).  One condition is not a measurement: a measured value
above 10 x the model's fp32 floor (fm.FLOOR: what the checker's float32 build does to the same measure) would be a defect to find, not a
tolerance to widen.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from furniture_amd.sim import FSim
from tests import freemotion_reference as fm
from tests import solve_reference as sref
from tests.test_solve_gpu import KSETS as SOLVE_KSETS
from tests.test_solve_gpu import _environment

pytestmark = pytest.mark.gpu
# model -> group -> the largest value of each measure on an MI355X, over the envs of the group and the kernel sets of the model
MEASURED = {
    "lack": dict(
        near=dict(pose=2.967e-07, bias=3.940e-07, force=1.069e-05, acc=1.039e-05, actuator=5.538e-06, step=5.902e-06, move=5.729e-05, tumble_pos=3.166e-07, tumble_ang=1.341e-05, tumble_norm=9.104e-08),
        far=dict(pose=1.522e-07, bias=1.502e-07, force=4.000e-07, acc=4.065e-06, actuator=3.760e-06, step=4.117e-06, move=5.878e-05, tumble_pos=2.758e-06, tumble_ang=1.379e-06, tumble_norm=5.034e-08),
    ),
    "lack_torque": dict(
        near=dict(pose=2.967e-07, bias=3.940e-07, force=1.069e-05, acc=1.039e-05, actuator=6.437e-06, step=5.902e-06, move=5.638e-05, tumble_pos=3.166e-07, tumble_ang=1.341e-05, tumble_norm=9.104e-08),
        far=dict(pose=1.522e-07, bias=1.235e-07, force=4.000e-07, acc=4.065e-06, actuator=2.580e-06, step=4.117e-06, move=5.878e-05, tumble_pos=2.758e-06, tumble_ang=1.379e-06, tumble_norm=5.034e-08),
    ),
    "billy": dict(
        near=dict(pose=2.325e-07, bias=8.246e-07, force=4.195e-05, acc=9.129e-06, actuator=1.248e-05, step=8.431e-06, move=6.411e-05, tumble_pos=1.780e-06, tumble_ang=6.509e-06, tumble_norm=9.668e-08),
        far=dict(pose=1.406e-07, bias=4.504e-07, force=1.389e-05, acc=1.728e-05, actuator=1.733e-06, step=1.715e-05, move=1.073e-04, tumble_pos=2.340e-06, tumble_ang=7.023e-06, tumble_norm=8.126e-08),
    ),
    "desk": dict(
        near=dict(pose=1.963e-07, bias=5.577e-07, force=3.489e-06, acc=8.199e-06, actuator=3.379e-06, step=1.181e-05, move=6.359e-05, tumble_pos=8.648e-07, tumble_ang=1.845e-05, tumble_norm=7.114e-08),
        far=dict(pose=1.358e-07, bias=1.914e-07, force=1.537e-06, acc=6.459e-06, actuator=1.694e-06, step=5.128e-06, move=8.239e-05, tumble_pos=1.341e-05, tumble_ang=9.554e-06, tumble_norm=5.779e-08),
    ),
    "toy": dict(
        near=dict(pose=1.358e-07, bias=7.968e-07, force=1.346e-04, acc=1.290e-05, step=1.255e-05, move=1.083e-04, tumble_pos=2.331e-07, tumble_ang=5.685e-06, tumble_norm=5.370e-08),
        far=dict(pose=1.625e-08, bias=3.140e-06, force=1.916e-05, acc=5.115e-05, step=4.876e-05, move=9.275e-05, tumble_pos=9.957e-07, tumble_ang=7.939e-06, tumble_norm=6.706e-08),
    ),
    "liden": dict(
        near=dict(pose=2.345e-07, bias=2.239e-07, force=6.798e-05, acc=2.485e-05, actuator=3.964e-06, step=2.377e-05, move=9.968e-05, tumble_pos=1.438e-07, tumble_ang=4.181e-06, tumble_norm=1.039e-07),
        far=dict(pose=1.313e-07, bias=1.360e-07, force=3.910e-05, acc=7.230e-06, actuator=1.190e-06, step=5.668e-06, move=1.068e-04, tumble_pos=2.605e-06, tumble_ang=1.243e-06, tumble_norm=7.568e-08),
    ),
}
TOL = {n: {g: {k: 4.0 * v for k, v in d.items()} for g, d in gs.items()} for n, gs in MEASURED.items()}
# A quaternion normalised in float32: each component is within 4 spacings of 1.0 of the exact quotient (a square root and a division that
# are not correctly rounded, 2.5 ulp each at most, and the rounding of the sum of squares)
QNORM_TOL = 4.0 * 2.0 ** -23
_NAME_OF = {sref.LACK: "lack", sref.BILLY: "billy", sref.DESK: "desk"}
# kernel set -> model (of fm.MODELS), the environment fsim_create reads, and for the sets of tests/test_solve_gpu.py the variant and slots
KSETS = {ks: dict(name=_NAME_OF[k["model"]], env=k["env"], variant=k["variant"], slots=k["slots"]) for ks, k in SOLVE_KSETS.items()}
KSETS.update({
    "liden-mw0": dict(name="liden", env=dict(FSIM_MW="0"), variant="generic2", slots=128),
    "liden-generic8": dict(name="liden", env=dict(FSIM_MW="0", FSIM_NCON_MAX="512"), variant="generic8", slots=512),
    "toy": dict(name="toy", env={}),
    "lack-torque": dict(name="lack_torque", env={}),
})
_handles, _runs, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for sim in _handles.values():
        sim.close()
    _handles.clear()


def _handle(ks):
    if ks not in _handles:
        k = KSETS[ks]
        with _environment(k["env"]):
            _handles[ks] = FSim(fm.model(k["name"]), fm.N)
        sim = _handles[ks]
        if "variant" in k:
            assert sim.kernel_variant == k["variant"] and sim.max_contacts == k["slots"], (ks, sim.kernel_variant, sim.max_contacts)
    return _handles[ks]


def _reference(name):
    if name not in _refs:
        _refs[name] = fm.references(name)
    return _refs[name]


def _run(ks):
    """list over the envs of the `got` dict of fm.measures, from the kernel set's handle"""
    if ks not in _runs:
        m, st, _ = _reference(KSETS[ks]["name"])
        sim, fields = _handle(ks), fm.fields(st)
        read = lambda *names: {k: v.cpu().numpy() for k, v in sim.get_state(*names).items()}
        sim.set_state(**fields)
        sim.physics_forward()
        fwd = read("qacc", "xpos", "xquat", "qfrc_bias", "qpos", "ncon")
        sim.set_state(**fields)
        sim.physics_step(1)
        one = read("qvel", "qpos")
        sim.set_state(**fields)
        sim.physics_step(fm.TUMBLE_STEPS)
        far = read("qpos")
        _runs[ks] = [dict(xpos=fwd["xpos"][e], xquat=fwd["xquat"][e], bias=fwd["qfrc_bias"][e], qacc=fwd["qacc"][e], qpos_fwd=fwd["qpos"][e], ncon=int(fwd["ncon"][e, 0]),
                          qvel1=one["qvel"][e], qpos1=one["qpos"][e], qpos_tumble=far["qpos"][e]) for e in range(fm.N)]
    return _runs[ks]


def test_the_condition_on_the_measured_values():
    assert set(MEASURED) == set(fm.MODELS)
    for name, gs in MEASURED.items():
        for g in fm.GROUPS:
            assert set(gs[g]) == set(fm.FLOOR[name][g]), (name, g)
            for k, v in gs[g].items():
                assert 0 < v <= 10.0 * fm.FLOOR[name][g][k], (name, g, k, v, fm.FLOOR[name][g][k])


def test_every_model_has_a_kernel_set():
    assert {k["name"] for k in KSETS.values()} == set(fm.MODELS) and len(KSETS) == 14
    assert {ks for ks, k in KSETS.items() if k["name"] == "liden"} == {"liden-mw0", "liden-generic8"}


def test_four_waves_per_env_are_refused_for_the_model_with_91_dofs():
    """the kernels with four waves per env hold at most 64 contact slots and one row pass over the dofs: asked for them, fsim_create says so"""
    from furniture_amd.sim import FsimError
    with _environment(dict(FSIM_MW="all")):
        with pytest.raises(FsimError, match="no multi-wave kernel"):
            FSim(fm.model("liden"), fm.N)


@pytest.mark.parametrize("ks", list(KSETS))
def test_free_motion_against_float64(ks):
    name = KSETS[ks]["name"]
    m, st, refs = _reference(name)
    got = _run(ks)
    pq = np.asarray(m.part_qposadr, dtype=np.int64)
    quat = np.zeros(m.nq, dtype=bool)
    for a in pq:
        quat[a + 3:a + 7] = True
    worst, wrong = {g: {} for g in fm.GROUPS}, []
    for e, ref in enumerate(refs):
        g = got[e]
        # (the 100 substeps are judged from the fast states alone: a torque of 5 N m spins a leg of 1.8e-7 kg m^2 up until the explicit
        #  gyroscopic term diverges, and the float64 oracle stops as unstable after 3 to 6 substeps from the states with qfrc_applied)
        wrong += ["env %d: %s is not finite" % (e, k) for k, v in g.items() if not np.isfinite(v).all() and (k != "qpos_tumble" or e in fm.TUMBLE_ENVS)]
        if g["ncon"] != 0:
            wrong.append("env %d: %d contacts" % (e, g["ncon"]))
        # the forward pass normalises the part quaternions in place and leaves the rest of qpos as it was written
        if not (g["qpos_fwd"][~quat] == st["qpos"][e][~quat].astype(np.float32)).all():
            wrong.append("env %d: the forward pass changed qpos outside the part quaternions" % e)
        qerr = fm.normalised_qpos_error(m, ref, g["qpos_fwd"])
        v = fm.measures(m, ref, g)
        print("%s env %d (%s): %s  normalised qpos %.3e" % (ks, e, fm.group(e), "  ".join("%s %.3e" % kv for kv in v.items()), qerr))
        if qerr > QNORM_TOL:
            wrong.append("env %d: qpos after the forward pass is %.3e off the normalised quaternions" % (e, qerr))
        for k, x in v.items():
            worst[fm.group(e)][k] = max(worst[fm.group(e)].get(k, 0.0), float(x))
    for grp in fm.GROUPS:
        print("%s %s measured: %s" % (ks, grp, "  ".join("%s %.3e" % kv for kv in worst[grp].items())))
    # the still-spin state: w exactly 0 leaves the quaternion alone, |w| = 1e-18 turns it by nothing that float32 holds
    e = fm.FAMILY["still-spin"][0]
    still = _part_moves(m, refs[e], got[e]["qpos1"])[:2]
    print("%s measured: still-spin parts %s" % (ks, "  ".join("%.3e" % x for x in still)))
    assert name in TOL, "no measured values for %s" % name
    wrong += ["still-spin part %d: move %.3e exceeds %.3e" % (i, x, TOL[name]["near"]["move"]) for i, x in enumerate(still) if not x <= TOL[name]["near"]["move"]]
    for grp in fm.GROUPS:
        assert set(worst[grp]) == set(TOL[name][grp]), (ks, grp, sorted(worst[grp]))
        wrong += ["%s %s %.3e exceeds %.3e" % (grp, k, x, TOL[name][grp][k]) for k, x in worst[grp].items() if not x <= TOL[name][grp][k]]
    assert not wrong, wrong


def _part_moves(m, ref, qpos1):
    """the `move` error of every part's free joint, in the order of the parts"""
    A = m.arrays
    jq = np.asarray(A["jnt_qposadr"], dtype=np.int64)
    per = fm.move_errors(m, ref, np.asarray(qpos1, dtype=np.float64))
    return [float(per[int(np.nonzero(jq == a)[0][0])]) for a in np.asarray(m.part_qposadr, dtype=np.int64)]

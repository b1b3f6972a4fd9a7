"""Centre-of-mass, momentum and energy sensors on the device (include/fsim_momentum.h) through the library, against the float64 reference
tests/momentum_reference.py evaluated at the device's own qpos / qvel: four models -- Baxter + table_liden_0921 among them, whose nv = 91
takes a second round over the dofs and whose last part is bit 31 of the masks -- in random states near the origin and with every part 8 m
out, and on Sawyer + table_lack_0825 after a reset and 30 random steps; the cross-checks against the dynamics tensors; what the header
states (outputs one at a time, a sensor alone, an env alone, the exact zeros of the Jacobian, read-only evaluation); the C-ABI's set,
refused set, clear and call without a set; the env surface.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each
call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from furniture_amd.dynamics import Dynamics
from furniture_amd.envs import FurnitureBatchEnv
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.momentum import MomentumSensor, MomentumSet, all_parts_sensor, masses, part_sensors, robot_sensor
from furniture_amd.sim import FSim, FsimError, FsimMomentumOut, lib
from oracle.oracle_sim import OracleSim
from tests import momentum_reference as mref
from tests.test_camera_gpu import _make, _poison, _steps
from tests.test_dynamics_gpu import TOL as DYN_TOL
from tests.test_frames_gpu import _handle, _state_of
from tests.test_momentum import _moved_columns

pytestmark = pytest.mark.gpu
MODELS = mref.MODELS
KEYS = ("mom_com", "mom_linvel", "mom_angmom", "mom_jac", "mom_energy")
# The tolerance of each measure is 4 x the largest value measured on an MI355X against the float64 reference over all cases of this file (the
# rule of DESIGN.md 15; the values: DESIGN.md 25), the states near the origin and those 8 m out apart.  The measure of a quantity is the
# largest absolute error over the env's sensors divided by the largest reference magnitude of that quantity in the env.  One condition, not
# a measurement: no measured value exceeds 10 x what fp32 alone does to the reference's own formulas, mref.FLOOR (tests/test_momentum.py);
# a value above that would be a defect to find, not a tolerance to widen.  Every test prints its own figures before it asserts.
# Measured, near: com 2.162e-7, linvel 6.939e-7, angmom 8.432e-7, energy 1.682e-7 (all table_lack_0825 after 30 steps), jac 1.244e-7
# (table_liden_0921); far: com 5.821e-8, angmom 9.058e-7, energy 1.510e-7 (toy_table), linvel 1.624e-7 (table_lack_0825), jac 1.244e-7
# (table_liden_0921).  The largest against its floor: linvel near, 6.6 x.
MEASURED = dict(near=dict(com=2.162e-7, linvel=6.939e-7, angmom=8.432e-7, jac=1.244e-7, energy=1.682e-7),
                far=dict(com=5.821e-8, linvel=1.624e-7, angmom=9.058e-7, jac=1.244e-7, energy=1.510e-7))
TOL = {g: {k: 4.0 * v for k, v in MEASURED[g].items()} for g in MEASURED}
FULL = dict(jacobian=True, energy=True)


def test_the_condition_on_the_measured_values():
    for g in mref.GROUPS:
        for k in mref.KEYS:
            assert MEASURED[g][k] <= 10.0 * mref.FLOOR[g][k], (g, k)


def _mom(sim, **kw):
    _poison()
    res = sim.momenta(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _reference(m, sensors, qpos, qvel, cursor):
    """the reference of every env at the device's own state"""
    osim = OracleSim(m)
    rows = [mref.evaluate(osim, m, sensors, qpos[e], qvel[e], None if cursor is None else cursor[e]) for e in range(len(qpos))]
    osim.close()
    return rows


def _measure(got, refs):
    """{measure: [n]} of every output in `got`: no element of any output is left out"""
    rows = [mref.measures(refs[e], {k[len("mom_"):]: got[k][e] for k in got}) for e in range(len(refs))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def _assert_close(tag, group, got, refs):
    ms = _measure(got, refs)
    print("%s %s measured: %s" % (tag, group, "  ".join("%s %.3e" % (k, v.max()) for k, v in ms.items())))
    for k, v in ms.items():
        assert v.max() <= TOL[group][k], "%s %s: %s error %.3e in env %d, tolerance %.3e" % (tag, group, k, v.max(), v.argmax(), TOL[group][k])
    return ms


def _everything(m):
    """one sensor over everything that moves"""
    robot = robot_sensor(m)
    return MomentumSensor((robot.bodies if robot is not None else []) + list(m.meta["part_names"]), subtree=False)


# ---- 1. the four models, near and far: one evaluation per model, shared by the tests below ------------------------------------------------
@pytest.fixture(scope="module", params=MODELS, ids=[f for _, f in MODELS])
def case(request):
    agent, furniture = request.param
    n = mref.n_envs(furniture)
    m, sim = _handle(agent, furniture, n)
    sensors = mref.sensor_sets(m)
    sim.set_momenta(MomentumSet(sensors, **FULL))
    got, refs = {}, {}
    for g in mref.GROUPS[::-1]:  # (near last: the state the cross-checks and the other sets below are evaluated at)
        qpos, qvel = mref.states(m, furniture, g)
        sim.set_state(qpos=qpos, qvel=qvel)
        got[g] = _mom(sim)
        qpos, qvel, cursor = _state_of(m, sim)
        refs[g] = _reference(m, sensors, qpos, qvel, cursor)
    qvel = qvel.copy()
    # the same sensors inside a set of 64, in another order, and each alone
    step = next(k for k in (5, 7, 3) if math.gcd(k, len(sensors)) == 1)
    order = [(step * i + 3) % len(sensors) for i in range(64)]
    sim.set_momenta(MomentumSet([sensors[i] for i in order], **FULL))
    many = _mom(sim)
    alone = []
    for s in sensors:
        sim.set_momenta(MomentumSet([s], **FULL))
        alone.append(_mom(sim))
    # the cross-checks: one sensor over everything that moves, beside the dynamics tensors of all dofs
    sim.set_momenta(MomentumSet([_everything(m)], **FULL))
    whole = _mom(sim)
    sim.set_dynamics(Dynamics(mass=True, bias=False, gravity=True))
    _poison()
    dyn = {k: v.cpu().numpy() for k, v in sim.dynamics().items()}
    torch.cuda.synchronize()
    sim.close()
    return dict(m=m, tag=furniture, n=n, sensors=sensors, got=got, refs=refs, order=order, many=many, alone=alone, whole=whole, dyn=dyn, qvel=qvel)


@pytest.mark.parametrize("group", mref.GROUPS)
def test_outputs_match_reference(case, group):
    m, got, n, S = case["m"], case["got"][group], case["n"], len(case["sensors"])
    assert list(got) == list(KEYS) and all(v.dtype == np.float32 for v in got.values())
    assert got["mom_com"].shape == got["mom_linvel"].shape == got["mom_angmom"].shape == (n, S, 3) and got["mom_jac"].shape == (n, S, 3, m.nv) and got["mom_energy"].shape == (n, 2)
    if case["tag"] == "table_liden_0921":
        assert m.nv == 91 and int(np.asarray(m.arrays["rdims"])[0]) == 32 and int(m.arrays["body_red"][m.meta["body_names"].index(m.meta["part_names"][-1])]) == 31
    _assert_close(case["tag"], group, got, case["refs"][group])
    assert got["mom_com"][0].tobytes() != got["mom_com"][1].tobytes() and got["mom_angmom"][0].tobytes() != got["mom_angmom"][1].tobytes()  # the envs differ
    if group == "far":  # the parts are 8 m out, and what does not depend on where they are is the same bits as near the origin
        assert np.linalg.norm(got["mom_com"][:, 0] - case["got"]["near"]["mom_com"][:, 0], axis=-1) == pytest.approx(8.0, abs=1e-5)
        assert got["mom_linvel"][:, :m.nparts].tobytes() == case["got"]["near"]["mom_linvel"][:, :m.nparts].tobytes()


def test_jacobian_zeros_are_exact(case):
    m, sensors = case["m"], case["sensors"]
    moved = np.stack(_moved_columns(m, sensors))  # [S, nv]
    for g in mref.GROUPS:
        J = case["got"][g]["mom_jac"]
        assert (~moved).sum() > 0 and all((J[:, i][:, :, ~moved[i]] == 0).all() and np.abs(J[:, i][:, :, moved[i]]).max() > 0 for i in range(len(sensors)))
        # a part's translation columns are the identity: m_b e_k over the mass the lane summed, exact zeros off the diagonal
        for i in range(m.nparts):
            da = int(np.asarray(m.part_dofadr)[i])
            blk = J[:, i, :, da:da + 3]
            assert (blk[:, ~np.eye(3, dtype=bool)] == 0).all() and np.abs(blk[:, np.eye(3, dtype=bool)] - 1.0).max() <= 2.0 ** -22
    J, v = case["got"]["near"]["mom_jac"].astype(np.float64), case["got"]["near"]["mom_linvel"]
    err = np.abs(np.einsum("eskd,ed->esk", J, case["qvel"]) - v).max() / np.abs(v).max()
    print("%s measured: mom_jac @ qvel against mom_linvel: %.3e" % (case["tag"], err))
    assert err <= TOL["near"]["jac"] * np.abs(case["qvel"]).sum(axis=1).max() + TOL["near"]["linvel"]  # |J| <= 1: each entry within TOL, summed over |qvel|


def test_a_sensor_alone_is_the_sensor_inside_a_set_of_64(case):
    """a sensor's bits do not depend on the other sensors of the set, nor on its place in it"""
    near, many, order = case["got"]["near"], case["many"], case["order"]
    assert many["mom_com"].shape[1] == 64 and set(order) == set(range(len(case["sensors"])))
    for k in KEYS[:4]:
        assert many[k].tobytes() == np.ascontiguousarray(near[k][:, order]).tobytes(), k
        for i, one in enumerate(case["alone"]):
            assert one[k].shape[1] == 1 and one[k][:, 0].tobytes() == near[k][:, i].tobytes(), (k, i)
    assert many["mom_energy"].tobytes() == near["mom_energy"].tobytes() and all(one["mom_energy"].tobytes() == near["mom_energy"].tobytes() for one in case["alone"])


def test_cross_checks_against_the_dynamics_tensors(case):
    """With one sensor over everything that moves: 1/2 qvel^T dyn_mass qvel == energy[1] and dyn_gravity == -m_total mom_jac^T g, the
    products in float64 on the device's float32 outputs.  The bounds follow from the two families' own tolerances, entry by entry: dyn_mass is
    within DYN_TOL[mass] max|M| of M, so the form is within 1/2 (sum |qvel|)^2 of that, and energy within TOL[energy] max|energy|; mom_jac
    is within TOL[jac] max|jac| of the Jacobian, so m_total jac^T g is within m_total |g|_1 of that, and dyn_gravity within
    DYN_TOL[gravity] max|gravity|."""
    m, whole, dyn, qvel = case["m"], case["whole"], case["dyn"], case["qvel"]
    mtot = float(masses(m, MomentumSet([_everything(m)]))[0])
    g = mref.gravity(m)
    worst = [0.0, 0.0]
    for e in range(case["n"]):
        M, E, J = dyn["dyn_mass"][e].astype(np.float64), whole["mom_energy"][e].astype(np.float64), whole["mom_jac"][e, 0].astype(np.float64)
        bound = 0.5 * np.abs(qvel[e]).sum() ** 2 * DYN_TOL["mass"] * np.abs(M).max() + TOL["near"]["energy"] * np.abs(E).max()
        worst[0] = max(worst[0], abs(0.5 * qvel[e] @ M @ qvel[e] - E[1]) / bound)
        G = dyn["dyn_gravity"][e].astype(np.float64)
        bound = mtot * np.abs(g).sum() * TOL["near"]["jac"] * np.abs(J).max() + DYN_TOL["gravity"] * np.abs(G).max()
        worst[1] = max(worst[1], np.abs(G + mtot * (J.T @ g)).max() / bound)
    print("%s measured: 1/2 v^T dyn_mass v against energy[1]: %.3e of its bound; dyn_gravity against -m jac^T g: %.3e of its bound" % (case["tag"], worst[0], worst[1]))
    assert max(worst) <= 1.0
    assert whole["mom_energy"].tobytes() == case["got"]["near"]["mom_energy"].tobytes()  # the energy is the env's, whatever the set


# ---- 2. outputs one at a time, independence of the batch ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lack():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 4)
    qpos, qvel = mref.states(m, "table_lack_0825", "far")
    sim.set_state(qpos=qpos, qvel=qvel)
    spec = MomentumSet(mref.sensor_sets(m), **FULL)
    sim.set_momenta(spec)
    full = _mom(sim)
    yield m, sim, spec, full
    sim.close()


def test_each_output_alone_and_out_buffers(lack):
    m, sim, spec, full = lack
    shapes = sim.momentum_shapes()
    S = spec.n_sensors
    assert list(shapes) == list(KEYS) and shapes["mom_com"][0] == (S, 3) and shapes["mom_jac"][0] == (S, 3, m.nv) and shapes["mom_energy"][0] == (2,)
    L, h = lib(), sim._h
    for i, k in enumerate(KEYS):  # each pointer alone, through the C-ABI
        buf = torch.full((4,) + shapes[k][0], 77.0, device=sim.device)
        ptrs = [None] * 5
        ptrs[i] = buf.data_ptr()
        _poison()
        assert L.fsim_momenta(h, ctypes.byref(FsimMomentumOut(*ptrs))) == 0
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    for k, (sh, dt) in shapes.items():  # out= with a single key
        buf = torch.full((4,) + sh, 77, dtype=dt, device=sim.device)
        res = _mom(sim, out={k: buf})
        assert list(res) == [k] and res[k].tobytes() == full[k].tobytes() and buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    with pytest.raises(ValueError, match="out holds"):
        sim.momenta(out={})
    with pytest.raises(ValueError, match="out holds"):
        sim.momenta(out={"mom_inertia": torch.zeros(4, device=sim.device)})
    with pytest.raises(ValueError, match="not a contiguous"):
        sim.momenta(out={"mom_energy": torch.zeros((4, 3), device=sim.device)})
    sim.set_momenta(MomentumSet(spec.sensors))  # the defaults: neither the Jacobian nor the energy
    assert list(sim.momentum_shapes()) == list(KEYS[:3])
    res = _mom(sim)
    assert sorted(res) == sorted(KEYS[:3]) and all(res[k].tobytes() == full[k].tobytes() for k in res)
    sim.set_momenta(spec)


def test_env_alone_is_bit_identical(lack):
    m, sim, spec, full = lack
    st = sim.get_state("qpos", "qvel")
    alone = FSim(m, 1)
    alone.set_momenta(spec)
    for e in range(4):
        alone.set_state(qpos=st["qpos"][e:e + 1], qvel=st["qvel"][e:e + 1])
        one = _mom(alone)
        for k in full:
            assert one[k][0].tobytes() == full[k][e].tobytes(), (e, k)
    assert len({full["mom_angmom"][e].tobytes() for e in range(4)}) == 4
    alone.close()


# ---- 3. after a reset and 30 steps: the reference at the device's own state, and read-only evaluation ------------------------------------
def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_after_reset_and_steps_and_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 8)
    _, twin = _make("Sawyer", "table_lack_0825", 8)
    _steps(sim, 30)
    _steps(twin, 30)
    sensors = mref.sensor_sets(m)
    sim.set_momenta(MomentumSet(sensors, **FULL))
    before = _all_state(sim)  # every field, env_block included
    assert "env_block" in before and "qvel" in before
    got = _mom(sim)
    _mom(sim, out={"mom_jac": torch.empty((8, len(sensors), 3, m.nv), device=sim.device)})
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    qpos, qvel, cursor = _state_of(m, sim)
    _assert_close("table_lack_0825 30 steps", "near", got, _reference(m, sensors, qpos, qvel, cursor))
    again = _mom(sim)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    _steps(sim, 2, seed=8)  # a step after a call == the same step without one, bit for bit
    _steps(twin, 2, seed=8)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 4. the C-ABI: set, refused set, clear, a call without a set -----------------------------------------------------------------------
def test_c_abi_behaviour():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 2)
    L, h = lib(), sim._h
    names, red = m.meta["body_names"], np.asarray(m.arrays["body_red"])
    part = [names.index(p) for p in m.meta["part_names"]]
    fixed = [b for b in range(1, m.nbody) if red[b] == 0]
    buf = torch.full((2, 3, 3), 7.0, device=sim.device)  # room for three sensors
    msg = lambda: L.fsim_last_error().decode()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)

    def refused(rc, text):
        assert rc == -1 and text in msg(), (rc, text, msg())

    def set_mom(n, adr, bodies, subtree=None):
        a, b, s = i32(adr), i32(bodies), i32(subtree if subtree is not None else [0] * len(bodies))
        return L.fsim_set_momenta(h, n, a.ctypes.data, b.ctypes.data, s.ctypes.data)

    def com():
        assert L.fsim_momenta(h, ctypes.byref(FsimMomentumOut(buf.data_ptr(), None, None, None, None))) == 0
        torch.cuda.synchronize()
        return buf.cpu().numpy().reshape(2, -1).copy()  # [2 envs][room for 3 sensors x 3]
    out = FsimMomentumOut(buf.data_ptr(), None, None, None, None)
    for call_ in (sim.momenta, sim.momentum_shapes):
        with pytest.raises(FsimError, match="no sensor set"):
            call_()
    refused(L.fsim_momenta(h, ctypes.byref(out)), "no sensor set")
    z = i32([0, 1])
    refused(L.fsim_set_momenta(None, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data), "null handle")
    refused(L.fsim_momenta(None, ctypes.byref(out)), "null handle")
    assert set_mom(2, [0, 1, 2], [part[1], part[0]]) == 0  # the set the refusals below must leave in place
    first = com()
    first = first.reshape(-1)
    assert (first[:12] != 7.0).all() and (first[12:] == 7.0).all()  # [2 envs][2][3], nothing past them
    refused(L.fsim_set_momenta(h, 1, None, z.ctypes.data, z.ctypes.data), "null argument")
    refused(L.fsim_set_momenta(h, 1, z.ctypes.data, None, z.ctypes.data), "null argument")
    refused(L.fsim_set_momenta(h, 1, z.ctypes.data, z.ctypes.data, None), "null argument")
    refused(set_mom(-1, [0, 1], [part[0]]), "-1 sensors")
    refused(set_mom(65, list(range(66)), [part[0]] * 65), "65 sensors")
    refused(set_mom(1, [1, 2], [part[0], part[0]]), "adr[0] is 1")
    refused(set_mom(2, [0, 1, 1], [part[0]]), "sensor 1: adr gives it 0 bodies")
    refused(set_mom(1, [0, 2], [part[0], m.nbody]), "sensor 0: unknown body %d" % m.nbody)
    refused(set_mom(2, [0, 1, 2], [part[0], -1]), "sensor 1: unknown body -1")
    refused(set_mom(1, [0, 1], [0]), "body 0 does not move")
    refused(set_mom(1, [0, 2], [part[0], fixed[0]], [0, 1]), "body %d does not move" % fixed[0])
    # (a model with more than 32 reduced bodies or nv above 128 is refused by fsim_create already, and no shipped body that moves is
    #  without mass: those refusals cannot be reached through a handle; the host check states them too, tests/test_momentum.py)
    again = com()
    assert again.reshape(-1).tobytes() == first.tobytes()  # a refused call leaves the set before it: the two parts, in that order
    refused(L.fsim_momenta(h, None), "null argument")
    refused(L.fsim_momenta(h, ctypes.byref(FsimMomentumOut(None, None, None, None, None))), "no output")
    # a body listed twice, or covered twice through a subtree, counts once
    link = names.index(mref.arm_link(m))
    below = [b for b in range(link + 1, m.nbody) if int(m.arrays["body_parentid"][b]) == link and red[b] != red[link]][0]
    assert set_mom(3, [0, 1, 4, 6], [link, link, below, link, part[0], part[0]], [1, 1, 1, 0, 0, 1]) == 0
    three = com().reshape(2, 3, 3)
    assert three[:, 0].tobytes() == three[:, 1].tobytes() and three[:, 2].tobytes() == first[:12].reshape(2, 2, 3)[:, 1].tobytes()
    # n_sensors == 0 is the documented clear, with or without tables: afterwards there is no set
    assert set_mom(0, [0, 1], [part[0]]) == 0
    refused(L.fsim_momenta(h, ctypes.byref(out)), "no sensor set")
    assert L.fsim_set_momenta(h, 0, None, None, None) == 0 and L.fsim_set_momenta(h, 0, None, None, None) == 0  # clearing twice is fine
    sim.set_momenta(MomentumSet(part_sensors(m)))
    sim.set_momenta(None)
    with pytest.raises(FsimError, match="no sensor set"):
        sim.momenta()
    with pytest.raises(TypeError, match="MomentumSet"):
        sim.set_momenta(part_sensors(m))
    with pytest.raises(ValueError, match="does not move"):
        sim.set_momenta(MomentumSet([MomentumSensor("world")]))
    assert sim.momenta_set is None
    sim.close()


# ---- 5. the env surface -----------------------------------------------------------------------------------------------------------------
def test_env_surface():
    from furniture_amd.envs import make_config
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    m = load_compiled("Sawyer", "table_lack_0825")
    spec = MomentumSet(part_sensors(m) + [all_parts_sensor(m), robot_sensor(m)], **FULL)
    S = spec.n_sensors
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), momenta=spec)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-5:] == list(KEYS) and S == m.nparts + 2
    for k, tail in zip(KEYS, ((S, 3), (S, 3), (S, 3), (S, 3, m.nv), (2,))):
        assert tuple(ob[k].shape) == (4,) + tail and ob[k].dtype == torch.float32 and sp[k].shape == tail and sp[k].dtype == np.float32, k
    fresh = env.sim.momenta()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], ob[k]), k
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert list(ob.keys()) == list(sp.keys()) and all(sp[k].contains(ob[k][0].cpu().numpy()) for k in KEYS)
    # the furniture's centre of mass is the mass-weighted mean of the parts', and its momentum the sum of theirs
    mass = torch.as_tensor(masses(m, spec)[:m.nparts], dtype=torch.float64, device=ob["mom_com"].device)
    for k in ("mom_com", "mom_linvel"):
        mean = (ob[k][:, :m.nparts].double() * mass[None, :, None]).sum(dim=1) / mass.sum()
        assert (mean - ob[k][:, m.nparts].double()).abs().max().item() <= 4 * TOL["near"][k[len("mom_"):]] * max(1.0, ob[k].abs().max().item())
    assert (ob["mom_energy"][:, 1] >= 0).all()
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), momenta=MomentumSet(part_sensors(m)))  # the defaults: neither the Jacobian nor the energy
    ob2 = env.reset()
    assert list(ob2.keys()) == list(env.observation_space.spaces.keys()) and list(ob2.keys())[-3:] == list(KEYS[:3]) and ob2["mom_com"].shape == (2, m.nparts, 3)
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg())  # without momenta: the keys of before
    keys = list(env.reset())
    assert keys == list(env.observation_space.spaces) == [k for k in ob2 if not k.startswith("mom_")] and env.sim.momenta_set is None and env.momenta is None
    env.close()

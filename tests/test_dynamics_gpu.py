"""Mass-matrix, inverse-inertia and bias-force tensors on the device (include/fsim_dynamics.h) through the library, against the float64
reference tests/dynamics_reference.py evaluated at the device's own qpos / qvel: four models -- Baxter + table_liden_0921 among them, whose
nv = 91 takes a second round over the dofs and whose last part uses bit 31 of the masks -- in random states written with set_state and, on
the first three, after a reset and 30 random steps; what must be exact (symmetry, zeros, bias == gravity at rest, selections, outputs one at
a time, independence of the batch), read-only evaluation, the env surface with an operational-space inertia built from frame_jac and
dyn_minv, and the C-ABI's error paths.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each call."""
import ctypes

import numpy as np
import pytest
import torch

from furniture_amd.dynamics import Dynamics, arm_dofs, tree_dofs
from furniture_amd.envs import FurnitureBatchEnv
from furniture_amd.frames import Frame, FrameSensor, FrameSet
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import FSim, FsimError, lib
from oracle.oracle_sim import OracleSim
from tests import dynamics_reference as dref
from tests import frames_reference as fref
from tests.test_camera_gpu import _make, _poison, _steps
from tests.test_frames_gpu import JAC_TOL, _handle, _random_states, _state_of

pytestmark = pytest.mark.gpu
MODELS = dref.MODELS
# The tolerance of each measure is 4 x the largest value measured on an MI355X against the float64 reference over all cases of this file (the
# rule of DESIGN.md 15; the values: DESIGN.md 20).  mass, bias, gravity: the largest absolute error over the env's largest reference
# magnitude of that quantity; minv: the error over the largest |Minv| entry of the same tree.  Two conditions, not measurements: for mass,
# bias and gravity a measured value above 1e-4 would be a defect to find, not a tolerance to widen; for minv the same holds above 10 x what
# fp32 alone does to this M, dref.MINV_FLOOR = 2.810e-7 (numpy's inverse of M rounded to float32, tests/test_dynamics.py).
# Measured: mass 5.628e-7 (desk_mikael_1064 after 30 steps), minv 1.640e-6 (table_lack_0825, 5.8 x the floor), bias 3.845e-7 (desk_mikael_1064),
# gravity 3.587e-7 (table_lack_0825 after 30 steps); every test prints its own figures before it asserts.
MEASURED = dict(mass=5.628e-7, minv=1.640e-6, bias=3.845e-7, gravity=3.587e-7)
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
KEYS = ("dyn_mass", "dyn_minv", "dyn_bias", "dyn_gravity")
ALL = dict(mass=True, inverse=True, bias=True, gravity=True)


def test_the_two_conditions_on_the_measured_values():
    assert all(MEASURED[k] <= 1e-4 for k in ("mass", "bias", "gravity"))
    assert MEASURED["minv"] <= 10.0 * dref.MINV_FLOOR


def _dyn(sim, **kw):
    _poison()
    res = sim.dynamics(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _reference(m, qpos, qvel, cursor):
    """the reference of every env at the device's own state"""
    osim = OracleSim(m)
    rows = [dref.evaluate(osim, m, qpos[e], qvel[e], None if cursor is None else cursor[e]) for e in range(len(qpos))]
    osim.close()
    return rows


def _measure(m, got, refs, dofs):
    """{measure: [n]} of the outputs `got` over the selection `dofs`"""
    rows = [dref.measures(m, refs[e], dofs, mass=got["dyn_mass"][e], minv=got["dyn_minv"][e], bias=got["dyn_bias"][e], gravity=got["dyn_gravity"][e]) for e in range(len(refs))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def _assert_close(tag, m, got, refs, dofs):
    ms = _measure(m, got, refs, dofs)
    print("%s measured: %s" % (tag, "  ".join("%s %.3e" % (k, v.max()) for k, v in ms.items())))
    for k, v in ms.items():
        assert v.max() <= TOL[k], "%s: %s error %.3e in env %d, tolerance %.3e" % (tag, k, v.max(), v.argmax(), TOL[k])
    return ms


# ---- 1. the four models in random states: one evaluation per model, shared by the tests below ------------------------------------------
@pytest.fixture(scope="module", params=MODELS, ids=[f for _, f in MODELS])
def case(request):
    agent, furniture = request.param
    n = dref.n_envs(furniture)
    m, sim = _handle(agent, furniture, n)
    qpos, qvel = _random_states(m, n, seed=dref.SEED)
    sim.set_state(qpos=qpos, qvel=qvel)
    sim.set_dynamics(Dynamics(**ALL))
    got = _dyn(sim)
    qpos, qvel, cursor = _state_of(m, sim)
    refs = _reference(m, qpos, qvel, cursor)
    # a selection in another order: the arm tree backwards, then every third dof of the rest
    t0 = tree_dofs(m, 0)
    sel = [int(d) for d in t0[::-1]] + [d for d in range(m.nv - 1, -1, -3) if d not in set(t0.tolist())]
    sim.set_dynamics(Dynamics(dofs=sel, **ALL))
    part = _dyn(sim)
    sim.set_dynamics(Dynamics(**ALL))
    sim.set_state(qvel=np.zeros((n, m.nv)))
    rest = _dyn(sim)
    sim.close()
    return dict(m=m, tag=furniture, n=n, got=got, refs=refs, sel=sel, part=part, rest=rest)


def test_tensors_match_reference_in_random_states(case):
    m, got, n = case["m"], case["got"], case["n"]
    assert got["dyn_mass"].shape == (n, m.nv, m.nv) and got["dyn_minv"].shape == (n, m.nv, m.nv) and got["dyn_bias"].shape == (n, m.nv) and got["dyn_gravity"].shape == (n, m.nv)
    assert all(v.dtype == np.float32 for v in got.values())
    if case["tag"] == "table_liden_0921":
        assert m.nv == 91 and int(np.asarray(m.arrays["rdims"])[0]) == 32 and int(m.arrays["body_red"][m.meta["body_names"].index(m.meta["part_names"][-1])]) == 31
    _assert_close(case["tag"], m, got, case["refs"], np.arange(m.nv))
    assert got["dyn_mass"][0].tobytes() != got["dyn_mass"][1].tobytes() and got["dyn_bias"][0].tobytes() != got["dyn_bias"][1].tobytes()  # the envs differ


def test_inverse_times_mass_is_the_identity(case):
    """M64 @ minv over every whole tree.  An entry of minv is within MINV_TOL * max|Minv_tree| of M^-1, so an entry of M @ minv is within
    ||M_tree||_inf * MINV_TOL * max|Minv_tree| of the identity: the measure is the residual over ||M_tree||_inf * max|Minv_tree|."""
    m, got = case["m"], case["got"]
    worst = 0.0
    for e, ref in enumerate(case["refs"]):
        for d in dref.tree_blocks(m):
            ix = np.ix_(d, d)
            res = ref["M"][ix] @ got["dyn_minv"][e][ix].astype(np.float64) - np.eye(len(d))
            worst = max(worst, np.abs(res).max() / (np.abs(ref["M"][ix]).sum(axis=1).max() * np.abs(ref["Minv"][ix]).max()))
    print("%s measured: M64 @ minv - I over the trees: %.3e" % (case["tag"], worst))
    assert worst <= TOL["minv"]


def test_what_must_be_exact(case):
    m, got, rest, part, sel = case["m"], case["got"], case["rest"], case["part"], case["sel"]
    M, Mi = got["dyn_mass"], got["dyn_minv"]
    # symmetry, bit for bit
    assert M.tobytes() == np.ascontiguousarray(M.transpose(0, 2, 1)).tobytes() and Mi.tobytes() == np.ascontiguousarray(Mi.transpose(0, 2, 1)).tobytes()
    # zeros across trees and across branches of a tree; nothing else is zero in the reference, and the device agrees
    smask, tmask = dref.structural_mask(m), dref.tree_mask(m)
    assert (~smask).sum() > 0 and (M[:, ~smask] == 0).all() and (Mi[:, ~tmask] == 0).all()
    assert (np.diagonal(M, axis1=1, axis2=2) > 0).all() and (np.diagonal(Mi, axis1=1, axis2=2) > 0).all()
    if case["tag"] == "desk_mikael_1064":  # two finger joints of one hand: one tree, neither an ancestor of the other
        branch = smask != tmask
        assert branch.sum() >= 2 and (M[:, branch] == 0).all() and (np.abs(Mi[:, branch]) > 0).any()
    # qvel = 0: bias == gravity bit for bit, and everything but bias as before
    assert rest["dyn_bias"].tobytes() == rest["dyn_gravity"].tobytes()
    for k in ("dyn_mass", "dyn_minv", "dyn_gravity"):
        assert rest[k].tobytes() == got[k].tobytes(), k
    assert got["dyn_bias"].tobytes() != got["dyn_gravity"].tobytes()
    # a selection, in another order, is the gathered rows and columns of the all-dofs output
    K = len(sel)
    assert part["dyn_mass"].shape == (case["n"], K, K) and part["dyn_bias"].shape == (case["n"], K) and K >= 9 and sel != sorted(sel)
    for k in ("dyn_mass", "dyn_minv"):
        assert part[k].tobytes() == np.ascontiguousarray(got[k][:, sel][:, :, sel]).tobytes(), k
    for k in ("dyn_bias", "dyn_gravity"):
        assert part[k].tobytes() == np.ascontiguousarray(got[k][:, sel]).tobytes(), k


# ---- 2. after a reset and 30 random steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", MODELS[:3])
def test_tensors_match_reference_after_reset_and_steps(agent, furniture):
    m, sim = _make(agent, furniture, 4)
    _steps(sim, 30)
    sim.set_dynamics(Dynamics(**ALL))
    got = _dyn(sim)
    qpos, qvel, cursor = _state_of(m, sim)
    _assert_close(furniture + " 30 steps", m, got, _reference(m, qpos, qvel, cursor), np.arange(m.nv))
    sim.close()


# ---- 3. outputs one at a time, independence of the batch ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lack():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 4)
    qpos, qvel = _random_states(m, 4, seed=5)
    sim.set_state(qpos=qpos, qvel=qvel)
    sim.set_dynamics(Dynamics(**ALL))
    full = _dyn(sim)
    yield m, sim, full
    sim.close()


def test_each_output_alone_and_out_buffers(lack):
    m, sim, full = lack
    sim.set_dynamics(Dynamics(**ALL))
    shapes = sim.dynamics_shapes()
    assert list(shapes) == list(KEYS) and shapes["dyn_mass"][0] == (m.nv, m.nv) and shapes["dyn_gravity"][0] == (m.nv,)
    L, h = lib(), sim._h
    for i, k in enumerate(KEYS):  # each pointer alone, through the C-ABI
        buf = torch.full((4,) + shapes[k][0], 77.0, device=sim.device)
        ptrs = [None] * 4
        ptrs[i] = buf.data_ptr()
        _poison()
        assert L.fsim_dynamics(h, *ptrs) == 0
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    for k, (sh, dt) in shapes.items():  # out= with a single key
        buf = torch.full((4,) + sh, 77, dtype=dt, device=sim.device)
        res = _dyn(sim, out={k: buf})
        assert list(res) == [k] and res[k].tobytes() == full[k].tobytes() and buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    with pytest.raises(ValueError, match="out holds"):
        sim.dynamics(out={})
    with pytest.raises(ValueError, match="out holds"):
        sim.dynamics(out={"dyn_coriolis": torch.zeros(4, device=sim.device)})
    with pytest.raises(ValueError, match="not a contiguous"):
        sim.dynamics(out={"dyn_bias": torch.zeros((4, 1), device=sim.device)})
    sim.set_dynamics(Dynamics())  # the defaults: mass and bias
    assert list(sim.dynamics_shapes()) == ["dyn_mass", "dyn_bias"]
    res = _dyn(sim)
    assert sorted(res) == ["dyn_bias", "dyn_mass"] and all(res[k].tobytes() == full[k].tobytes() for k in res)
    arm = arm_dofs(m)[0]
    sim.set_dynamics(Dynamics(dofs=arm, mass=False, inverse=True, bias=False, gravity=True))  # the arm's seven dofs: minv is the whole inverse's block
    res = _dyn(sim)
    assert sorted(res) == ["dyn_gravity", "dyn_minv"] and res["dyn_minv"].shape == (4, 7, 7)
    assert res["dyn_minv"].tobytes() == np.ascontiguousarray(full["dyn_minv"][:, :7, :7]).tobytes() and res["dyn_gravity"].tobytes() == np.ascontiguousarray(full["dyn_gravity"][:, :7]).tobytes()
    blk = np.linalg.inv(full["dyn_mass"][0, :7, :7].astype(np.float64))  # ... not the inverse of the selected block
    assert np.abs(blk - res["dyn_minv"][0]).max() > 100 * TOL["minv"] * np.abs(blk).max()
    sim.set_dynamics(Dynamics(dofs=[38]))  # K = 1
    res = _dyn(sim)
    assert res["dyn_mass"].shape == (4, 1, 1) and res["dyn_mass"].tobytes() == np.ascontiguousarray(full["dyn_mass"][:, 38:, 38:]).tobytes()


def test_env_alone_is_bit_identical(lack):
    m, sim, full = lack
    st = sim.get_state("qpos", "qvel")
    alone = FSim(m, 1)
    alone.set_dynamics(Dynamics(**ALL))
    for e in range(4):
        alone.set_state(qpos=st["qpos"][e:e + 1], qvel=st["qvel"][e:e + 1])
        one = _dyn(alone)
        for k in full:
            assert one[k][0].tobytes() == full[k][e].tobytes(), (e, k)
    assert len({full["dyn_mass"][e].tobytes() for e in range(4)}) == 4
    alone.close()


def test_second_round_over_dofs_alone():
    """Baxter + table_liden_0921 (nv = 91): an env of the batch is the same state alone, and the dofs of the second round alone are their rows"""
    m = load_compiled("Baxter", "table_liden_0921")
    sim = FSim(m, 2)
    qpos, qvel = _random_states(m, 2, seed=9)
    sim.set_state(qpos=qpos, qvel=qvel)
    sim.set_dynamics(Dynamics(**ALL))
    full = _dyn(sim)
    late = list(range(90, 63, -1))
    sim.set_dynamics(Dynamics(dofs=late, **ALL))
    part = _dyn(sim)
    for k in ("dyn_mass", "dyn_minv"):
        assert part[k].tobytes() == np.ascontiguousarray(full[k][:, late][:, :, late]).tobytes(), k
    for k in ("dyn_bias", "dyn_gravity"):
        assert part[k].tobytes() == np.ascontiguousarray(full[k][:, late]).tobytes(), k
    st = sim.get_state("qpos", "qvel")
    alone = FSim(m, 1)
    alone.set_dynamics(Dynamics(**ALL))
    alone.set_state(qpos=st["qpos"][1:2], qvel=st["qvel"][1:2])
    one = _dyn(alone)
    for k in full:
        assert one[k][0].tobytes() == full[k][1].tobytes(), k
    alone.close()
    sim.close()


# ---- 4. read-only evaluation ----------------------------------------------------------------------------------------------------------
def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_evaluation_is_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _, twin = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 3)
    _steps(twin, 3)
    sim.set_dynamics(Dynamics(**ALL))
    before = _all_state(sim)  # every field, env_block included
    assert "env_block" in before and "qvel" in before
    first = _dyn(sim)
    _dyn(sim, out={"dyn_minv": torch.empty((2, m.nv, m.nv), device=sim.device)})
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    again = _dyn(sim)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    _steps(sim, 2, seed=8)  # a step after a call == the same step without one, bit for bit
    _steps(twin, 2, seed=8)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


def test_a_selection_never_queried_changes_nothing():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _, twin = _make("Sawyer", "table_lack_0825", 2)
    sim.set_dynamics(Dynamics(dofs=tree_dofs(m, 0), **ALL))
    _steps(sim, 10)
    _steps(twin, 10)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 5. the env surface -----------------------------------------------------------------------------------------------------------------
def test_env_surface_and_operational_space_inertia():
    from furniture_amd.envs import FurnitureSawyerEnv, furniture_names, make_config
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    m = load_compiled("Sawyer", "table_lack_0825")
    tree = tree_dofs(m, arm_dofs(m)[0][0])
    K = len(tree)
    spec = Dynamics(dofs=tree, **ALL)
    grip = FrameSet([FrameSensor(Frame(site="grip_site"))], jacobian=True)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), frames=grip, dynamics=spec)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-4:] == list(KEYS) and K == 9
    for k, tail in zip(KEYS, ((K, K), (K, K), (K,), (K,))):
        assert tuple(ob[k].shape) == (4,) + tail and ob[k].dtype == torch.float32 and sp[k].shape == tail and sp[k].dtype == np.float32, k
    fresh = env.sim.dynamics()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], ob[k]), k
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert list(ob.keys()) == list(sp.keys()) and all(sp[k].contains(ob[k][0].cpu().numpy()) for k in KEYS)
    # the inverse operational-space inertia of the grip site, Lambda^-1 = J Minv J^T, on the device, against the float64 reference's
    # J M^-1 J^T.  J is supported on the arm tree, so the whole inverse's block over the tree makes the product exact.  With dJ <= JAC_TOL
    # and dMinv <= MINV_TOL * max|Minv_tree| entry by entry, an entry of the product (K^2 terms J_ri Minv_ij J_sj) is within
    # K^2 Jmax max|Minv| (2 JAC_TOL + Jmax MINV_TOL), plus 2^-23 of K^2 Jmax^2 max|Minv| for the two fp32 products' own rounding.
    J = ob["frame_jac"][:, 0][:, :, torch.as_tensor(tree, dtype=torch.long, device=ob["frame_jac"].device)]  # [4, 6, K]
    assert (ob["frame_jac"][:, 0][:, :, K:] == 0).all()
    lam_inv = torch.bmm(torch.bmm(J, ob["dyn_minv"]), J.transpose(1, 2)).cpu().numpy().astype(np.float64)
    qpos, qvel, cursor = _state_of(m, env.sim)
    osim = OracleSim(m)
    worst = 0.0
    for e in range(4):
        ref = dref.evaluate(osim, m, qpos[e], qvel[e])
        Jr = fref.evaluate_set(osim, m, grip.sensors)["jac"][0]
        want = Jr @ ref["Minv"] @ Jr.T
        jmax, imax = np.abs(Jr).max(), np.abs(ref["Minv"][np.ix_(tree, tree)]).max()
        bound = K * K * jmax * imax * (2 * JAC_TOL + jmax * TOL["minv"] + 2.0 ** -23 * jmax)
        err = np.abs(lam_inv[e] - want).max()
        worst = max(worst, err / bound)
        assert np.linalg.eigvalsh(0.5 * (lam_inv[e] + lam_inv[e].T)).min() > 0
    osim.close()
    print("table_lack_0825 measured: J Minv J^T against the reference: %.3e of its bound" % worst)
    assert worst <= 1.0
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), dynamics=Dynamics(dofs=arm_dofs(m)[0]))  # the defaults: mass and bias
    ob2 = env.reset()
    assert list(ob2.keys()) == list(env.observation_space.spaces.keys()) and list(ob2.keys())[-2:] == ["dyn_mass", "dyn_bias"] and ob2["dyn_mass"].shape == (2, 7, 7)
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg())  # without dynamics: the keys of before
    keys = list(env.reset())
    assert keys == list(env.observation_space.spaces) == [k for k in ob2 if not k.startswith("dyn_")] and env.sim.dyn is None and env.dynamics is None
    env.close()
    with pytest.raises(NotImplementedError, match="dynamics= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, dynamics=spec)
    with pytest.raises(NotImplementedError, match="dynamics= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(dynamics=spec))
    e1 = FurnitureSawyerEnv(config=cfg(), dynamics=Dynamics(dofs=arm_dofs(m)[0], gravity=True))
    first = e1.reset()  # the single env keeps its selection through reset(furniture_id)
    assert first["dyn_mass"].shape == (7, 7) and first["dyn_gravity"].shape == (7,)
    other = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert e1._b.furniture_name == "chair_agne_0010" and e1._b.dynamics is not None and e1._b.sim.dyn is e1._b.dynamics and list(other.keys()) == list(first.keys())
    assert other["dyn_mass"].shape == (7, 7) and np.isfinite(np.asarray(other["dyn_mass"])).all()
    e1.close()


# ---- 6. the C-ABI's error paths -----------------------------------------------------------------------------------------------------------
def test_c_abi_error_paths():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 2)
    L, h = lib(), sim._h
    buf = torch.full((2, 3, 3), 7.0, device=sim.device)  # room for three dofs
    msg = lambda: L.fsim_last_error().decode()

    def refused(rc, text):
        assert rc == -1 and text in msg(), (rc, text, msg())

    def set_dyn(n, dofs):
        t = np.ascontiguousarray(dofs, dtype=np.int32)
        return L.fsim_set_dynamics(h, n, t.ctypes.data)
    for call_ in (sim.dynamics, sim.dynamics_shapes):
        with pytest.raises(FsimError, match="no dof selection"):
            call_()
    refused(L.fsim_dynamics(h, buf.data_ptr(), None, None, None), "no dof selection")
    refused(L.fsim_set_dynamics(None, 1, np.zeros(1, np.int32).ctypes.data), "null handle")
    refused(L.fsim_dynamics(None, buf.data_ptr(), None, None, None), "null handle")
    assert set_dyn(2, [3, 1]) == 0  # the selection the refusals below must leave in place
    refused(L.fsim_set_dynamics(h, 1, None), "null argument")
    refused(set_dyn(-1, [0]), "-1 dofs")
    refused(set_dyn(m.nv + 1, list(range(m.nv)) + [0]), "%d dofs" % (m.nv + 1))
    refused(set_dyn(2, [0, m.nv]), "is %d" % m.nv)
    refused(set_dyn(2, [-1, 0]), "is -1")
    refused(set_dyn(3, [4, 5, 4]), "dof 4 is listed twice")
    # (a model with more than 32 reduced bodies or nv above 128 is refused by fsim_create already: the two refusals of fsim_set_dynamics
    #  cannot be reached through a handle; the host check states them too, tests/test_dynamics.py)
    assert L.fsim_dynamics(h, buf.data_ptr(), None, None, None) == 0  # a refused call leaves the selection before it: two dofs
    torch.cuda.synchronize()
    res = buf.cpu().numpy().reshape(-1)
    assert (res[:8] != 7.0).all() and (res[8:] == 7.0).all()  # [2 envs][2][2], nothing past them
    assert res[1] == res[2] and res[0] > 0 and res[3] > 0
    refused(L.fsim_dynamics(h, None, None, None, None), "no output")
    # n_dofs == 0 is the documented clear, with or without a list: afterwards there is no selection
    assert set_dyn(0, [5]) == 0
    refused(L.fsim_dynamics(h, buf.data_ptr(), None, None, None), "no dof selection")
    assert L.fsim_set_dynamics(h, 0, None) == 0 and L.fsim_set_dynamics(h, 0, None) == 0  # clearing twice is fine
    assert set_dyn(m.nv, list(range(m.nv))[::-1]) == 0  # K = nv
    sim.set_dynamics(Dynamics(dofs=[0]))
    sim.set_dynamics(None)
    with pytest.raises(FsimError, match="no dof selection"):
        sim.dynamics()
    with pytest.raises(TypeError, match="Dynamics"):
        sim.set_dynamics([0, 1])
    with pytest.raises(ValueError, match="out of range"):
        sim.set_dynamics(Dynamics(dofs=[m.nv]))
    sim.close()

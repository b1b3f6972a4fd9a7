"""Body and site frame sensors on the device (include/fsim_frames.h) through the library, against the float64 reference
tests/frames_reference.py evaluated at the device's own qpos / qvel: the grip site, part bodies, connector-site pairs, offsets, world-fixed
frames and frames relative to themselves on four models -- Baxter + table_liden_0921 among them, whose nv = 91 takes a second round over
the dofs and whose last part uses bit 31 of the ancestor masks -- in random states written with set_state and, on the first three, after a
reset and 30 random steps; what must be exact (zeros, the cursor offset), outputs one at a time, independence of the other sensors and of the
batch, read-only evaluation, the env surface and the C-ABI's error paths.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern
before each call."""
import ctypes

import numpy as np
import pytest
import torch

from furniture_amd.envs import FurnitureBatchEnv
from furniture_amd.frames import Frame, FrameSensor, FrameSet, connector_pairs
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import FSim, FsimError, FsimFrameSensor, lib
from oracle.oracle_sim import OracleSim
from tests import frames_reference as fref
from tests.test_camera_gpu import _make, _poison, _steps
from tests.test_rays_gpu import _device_state

pytestmark = pytest.mark.gpu
MODELS = [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table"), ("Baxter", "table_liden_0921")]
# The tolerance of each measure is 4 x the largest value measured on an MI355X against the float64 reference over all cases of this file (the
# rule of DESIGN.md 15; the values: DESIGN.md 19).  A measured value above 1e-4 would be a defect to find, not a tolerance to widen.
# Measured: pos 4.837e-7 m (table_liden_0921), quat 1.769e-7 (table_lack_0825 after 30 steps), vel_lin 2.404e-6 of S (the same), vel_ang
# 7.137e-7 of S (table_lack_0825), jac 1.071e-6 (desk_mikael_1064); every test prints its own figures before it asserts.
MEASURED = dict(pos=4.837e-7, quat=1.769e-7, vel_lin=2.404e-6, vel_ang=7.137e-7, jac=1.071e-6)
POS_TOL, QUAT_TOL, VEL_LIN_TOL, VEL_ANG_TOL, JAC_TOL = (4.0 * MEASURED[k] for k in ("pos", "quat", "vel_lin", "vel_ang", "jac"))
TOL = dict(pos=POS_TOL, quat=QUAT_TOL, vel_lin=VEL_LIN_TOL, vel_ang=VEL_ANG_TOL, jac=JAC_TOL)
S_FLOOR = 1e-3
KEYS = ("frame_pos", "frame_quat", "frame_vel", "frame_jac")


def _frames(sim, **kw):
    _poison()
    res = sim.frame_state(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _handle(agent, furniture, n):
    """a handle whose state is written with set_state: no reset (Baxter + table_liden_0921's reset climbs the re-step ladder); the Cursor
    agent's handle is reset once, which places its cursors"""
    if agent == "Cursor":
        return _make(agent, furniture, n)
    m = load_compiled(agent, furniture)
    return m, FSim(m, n)


def _random_states(m, n, seed):
    """[n, nq], [n, nv]: qpos0 with every part turned by a random unit quaternion and shifted, every hinge and slide joint uniform within
    its limits, qvel uniform(-1, 1) on every dof"""
    rng = np.random.RandomState(seed)
    A = m.arrays
    qpos = np.tile(np.asarray(A["qpos0"], dtype=np.float64), (n, 1))
    for e in range(n):
        for a in np.asarray(m.part_qposadr, dtype=np.int64):
            qpos[e, a:a + 3] += rng.uniform(-0.2, 0.2, 3)
            u = rng.normal(size=4)
            qpos[e, a + 3:a + 7] = u / np.linalg.norm(u)
        for jt, qa, lim, rg in zip(np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"]), np.asarray(A["jnt_limited"]), np.asarray(A["jnt_range"]).reshape(-1, 2)):
            if jt != 0:
                qpos[e, int(qa)] = rng.uniform(rg[0], rg[1]) if lim else rng.uniform(-1.0, 1.0)
    return qpos, rng.uniform(-1.0, 1.0, (n, m.nv))


def _grips(m):
    """the frames of the model's grip sites (the Cursor agent: its two cursor bodies)"""
    if m.meta["agent"] == "Cursor":
        return [Frame(body="cursor0"), Frame(body="cursor1")]
    return [Frame(site=m.meta["site_names"][int(k)]) for k in np.asarray(m.arrays["eef_siteid"])]


def _welded(m):
    """a body other than the world that is welded to it (reduced body 0) and is no cursor, or the world body itself"""
    red = np.asarray(m.arrays["body_red"])
    cur = set(int(b) for b in np.asarray(m.arrays["cursor_bodyid"])) if "cursor_bodyid" in m.arrays else set()
    ids = [b for b in range(1, m.nbody) if red[b] == 0 and b not in cur]
    return m.meta["body_names"][ids[-1] if ids else 0]


def _sensors(m):
    """about a dozen: the grip site in the world, part bodies in the world, connector pairs, grip site relative to a part and back, a body
    with an offset pose, a world-fixed frame relative to a moving body, frames relative to themselves, frames that cannot move; listed with
    what is expected of them: "" (nothing special), "self" or "still" """
    parts = m.meta["part_names"]
    G = _grips(m)
    pick = lambda lst: lst if len(lst) <= 5 else [lst[0], lst[len(lst) // 2], lst[-1]]  # (the last part of table_liden_0921 is reduced body 31)
    conn = pick(connector_pairs(m))
    off = Frame(body=parts[1], pos=(0.05, -0.02, 0.1), quat=(0.8, 0.2, -0.4, 0.3))
    out = [(FrameSensor(G[0]), "")]
    out += [(FrameSensor(Frame(body=p)), "") for p in pick(parts)]
    out += [(FrameSensor(Frame(site=a), ref=Frame(site=b)), "") for a, b in conn]
    out += [(FrameSensor(G[0], ref=Frame(body=parts[0])), ""), (FrameSensor(Frame(body=parts[-1]), ref=G[-1]), ""), (FrameSensor(G[-1], ref=G[0]), "" if len(G) > 1 else "self")]
    out += [(FrameSensor(off), ""), (FrameSensor(Frame(site=conn[0][0]), ref=off), "")]
    out += [(FrameSensor(Frame(pos=(0.3, 0.1, 0.5), quat=(0.9, 0.1, 0.2, 0.3)), ref=Frame(body=parts[0])), "")]
    out += [(FrameSensor(G[0], ref=G[0]), "self"), (FrameSensor(Frame(site=conn[0][1]), ref=Frame(site=conn[0][1])), "self"), (FrameSensor(off, ref=off), "self")]
    out += [(FrameSensor(Frame(body=m.meta["body_names"][0])), "still"), (FrameSensor(Frame(body=_welded(m), pos=(0.1, 0.2, 0.3))), "still"),
            (FrameSensor(Frame(pos=(1.0, 2.0, 3.0), quat=(0.5, 0.5, 0.5, 0.5))), "still")]
    return [s for s, _ in out], [k for _, k in out]


def _state_of(m, sim):
    qpos, cursor = _device_state(m, sim)
    return qpos, sim.get_state("qvel")["qvel"].cpu().numpy().astype(np.float64), cursor


def _reference(m, sensors, qpos, qvel, cursor):
    """the reference of every env at the device's own state"""
    osim = OracleSim(m)
    rows = []
    for e in range(len(qpos)):
        fref.set_state(osim, m, qpos[e], qvel[e], None if cursor is None else cursor[e])
        rows.append(fref.evaluate_set(osim, m, sensors))
    osim.close()
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def _measures(got, ref):
    """the error measures, [n, S] each: |dpos| in metres, the quaternion error up to sign, |dvel| / max(S, 1e-3) per half, |djac| absolute"""
    q, r = got["frame_quat"].astype(np.float64), ref["quat"]
    v = got["frame_vel"].astype(np.float64) - ref["vel"]
    return dict(pos=np.linalg.norm(got["frame_pos"] - ref["pos"], axis=-1), quat=np.minimum(np.linalg.norm(q - r, axis=-1), np.linalg.norm(q + r, axis=-1)),
                vel_lin=np.linalg.norm(v[..., :3], axis=-1) / np.maximum(ref["scale_lin"], S_FLOOR), vel_ang=np.linalg.norm(v[..., 3:], axis=-1) / np.maximum(ref["scale_ang"], S_FLOOR),
                jac=np.abs(got["frame_jac"] - ref["jac"]).max(axis=(-1, -2)))


def _assert_close(tag, got, ref):
    ms = _measures(got, ref)
    print("%s measured: %s" % (tag, "  ".join("%s %.3e" % (k, v.max()) for k, v in ms.items())))
    for k, v in ms.items():
        assert v.max() <= TOL[k], "%s: %s error %.3e at (env, sensor) %s, tolerance %.3e" % (tag, k, v.max(), np.unravel_index(v.argmax(), v.shape), TOL[k])
    return ms


def _dof_masks(m, sensors):
    """[S, nv] bool: the dofs whose reduced body is an ancestor-or-self of the sensor's frame's or reference's reduced body"""
    A = m.arrays
    red, anc, dofb = np.asarray(A["body_red"]), np.asarray(A["r_ancmask"]).astype(np.int64) & 0xffffffff, np.asarray(A["dof_rbody"]).astype(np.int64)
    cur = set(int(b) for b in np.asarray(A["cursor_bodyid"])) if "cursor_bodyid" in A else set()
    out = np.zeros((len(sensors), m.nv), dtype=bool)
    for i, s in enumerate(sensors):
        for f in (s.frame, s.ref):
            b = f.resolve(m)[0]
            if b >= 0 and b not in cur:
                out[i] |= ((anc[red[b]] >> dofb) & 1).astype(bool)
    return out


# ---- 1. the four models in random states: one evaluation per model, shared by the tests below ------------------------------------------
@pytest.fixture(scope="module", params=MODELS, ids=[f for _, f in MODELS])
def case(request):
    agent, furniture = request.param
    n = 2
    m, sim = _handle(agent, furniture, n)
    qpos, qvel = _random_states(m, n, seed=21)
    sim.set_state(qpos=qpos, qvel=qvel)
    sensors, kinds = _sensors(m)
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    got = _frames(sim)
    qpos, qvel, cursor = _state_of(m, sim)
    ref = _reference(m, sensors, qpos, qvel, cursor)
    sim.set_state(qvel=np.zeros((n, m.nv)))
    rest = _frames(sim)
    sim.close()
    return dict(m=m, tag=furniture, sensors=sensors, kinds=kinds, got=got, ref=ref, rest=rest, qvel=qvel, cursor=cursor)


def test_sensors_match_reference_in_random_states(case):
    m, got, ref = case["m"], case["got"], case["ref"]
    S = len(case["sensors"])
    assert got["frame_pos"].shape == (2, S, 3) and got["frame_quat"].shape == (2, S, 4) and got["frame_vel"].shape == (2, S, 6) and got["frame_jac"].shape == (2, S, 6, m.nv)
    assert 12 <= S <= 24
    if case["tag"] == "table_liden_0921":
        assert m.nv == 91 and int(np.asarray(m.arrays["rdims"])[0]) == 32 and int(m.arrays["body_red"][m.meta["body_names"].index(m.meta["part_names"][-1])]) == 31
    _assert_close(case["tag"], got, ref)
    assert np.abs(np.linalg.norm(got["frame_quat"], axis=-1) - 1.0).max() <= 1e-6
    assert got["frame_pos"][0].tobytes() != got["frame_pos"][1].tobytes()  # the envs differ


def test_what_must_be_exact(case):
    m, got, ref, kinds, sensors = case["m"], case["got"], case["ref"], case["kinds"], case["sensors"]
    # qvel = 0: vel == 0 everywhere, pose and Jacobian as before
    assert (case["rest"]["frame_vel"] == 0).all()
    for k in ("frame_pos", "frame_quat", "frame_jac"):
        assert case["rest"][k].tobytes() == got[k].tobytes(), k
    # a frame on the world or on a body of reduced body 0, referenced to the world: vel == 0 and jac == 0
    still = [i for i, k in enumerate(kinds) if k == "still"]
    assert len(still) == 3 and (got["frame_vel"][:, still] == 0).all() and (got["frame_jac"][:, still] == 0).all()
    # columns of dofs that move neither frame are exactly 0; the others are the reference's non-zero columns
    mask = _dof_masks(m, sensors)
    for i in range(len(sensors)):
        assert (got["frame_jac"][:, i][:, :, ~mask[i]] == 0).all(), i
        assert (np.abs(ref["jac"][:, i]).max(axis=1)[:, ~mask[i]] == 0).all(), i
    if m.meta["agent"] != "Cursor":
        cols = (np.abs(ref["jac"][0, 0]).max(axis=0) > 0)
        assert cols.sum() >= 7 and (cols <= mask[0]).all() and (np.abs(got["frame_jac"][0, 0]).max(axis=0) > 0)[cols].all()  # an arm's grip site
    else:  # a cursor-body frame has no velocity and no columns
        assert (got["frame_vel"][:, 0] == 0).all() and (got["frame_jac"][:, 0] == 0).all() and not mask[0].any()
    # a frame relative to itself: jac exactly 0 (every dof moves both frames or neither); pos 0, quat (+-1, 0, 0, 0), vel 0 within tolerance
    own = [i for i, k in enumerate(kinds) if k == "self"]
    assert len(own) >= 3 and (got["frame_jac"][:, own] == 0).all()
    assert np.abs(got["frame_pos"][:, own]).max() <= POS_TOL and np.abs(got["frame_vel"][:, own]).max() <= min(VEL_LIN_TOL, VEL_ANG_TOL) * S_FLOOR
    q = got["frame_quat"][:, own]
    assert np.abs(np.abs(q[..., 0]) - 1.0).max() <= QUAT_TOL and np.abs(q[..., 1:]).max() <= QUAT_TOL


def test_velocity_is_jacobian_times_qvel_on_the_device(case):
    got, ref = case["got"], case["ref"]
    jv = np.einsum("esrd,ed->esr", got["frame_jac"].astype(np.float64), case["qvel"])
    d = got["frame_vel"].astype(np.float64) - jv
    lin = np.linalg.norm(d[..., :3], axis=-1) / np.maximum(ref["scale_lin"], S_FLOOR)
    ang = np.linalg.norm(d[..., 3:], axis=-1) / np.maximum(ref["scale_ang"], S_FLOOR)
    print("%s measured: vel against jac @ qvel: linear %.3e angular %.3e" % (case["tag"], lin.max(), ang.max()))
    assert lin.max() <= 2 * VEL_LIN_TOL and ang.max() <= 2 * VEL_ANG_TOL  # (each side within its tolerance of the reference)


# ---- 2. after a reset and 30 random steps; world-referenced body frames against the step's own xpos / xquat ---------------------------
@pytest.mark.parametrize("agent,furniture", MODELS[:3])
def test_sensors_match_reference_after_reset_and_steps(agent, furniture):
    m, sim = _make(agent, furniture, 2)
    _steps(sim, 30)
    sensors, _ = _sensors(m)
    names = m.meta["body_names"]
    bodies = [b for b in range(m.nbody) if "cursor" not in names[b]][-(64 - len(sensors)):]
    sensors = sensors + [FrameSensor(Frame(body=names[b])) for b in bodies]  # up to S = 64
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    got = _frames(sim)
    qpos, qvel, cursor = _state_of(m, sim)
    _assert_close(furniture + " 30 steps", got, _reference(m, sensors, qpos, qvel, cursor))
    # the device's own forward kinematics
    sim.physics_forward()
    st = sim.get_state("xpos", "xquat")
    xpos, xquat = st["xpos"].cpu().numpy().reshape(2, m.nbody, 3), st["xquat"].cpu().numpy().reshape(2, m.nbody, 4)
    k0 = len(sensors) - len(bodies)
    dp = np.linalg.norm(got["frame_pos"][:, k0:] - xpos[:, bodies], axis=-1)
    qa, qb = got["frame_quat"][:, k0:].astype(np.float64), xquat[:, bodies].astype(np.float64)
    dq = np.minimum(np.linalg.norm(qa - qb, axis=-1), np.linalg.norm(qa + qb, axis=-1))
    print("%s measured: against xpos / xquat: pos %.3e quat %.3e (%d bodies)" % (furniture, dp.max(), dq.max(), len(bodies)))
    assert len(bodies) >= 6 and dp.max() <= POS_TOL and dq.max() <= QUAT_TOL
    sim.close()


# ---- 3. the cursor ------------------------------------------------------------------------------------------------------------------------
def test_cursor_frame_moves_by_exactly_the_cursor_offset():
    m, sim = _make("Cursor", "toy_table", 2)
    A = m.arrays
    sim.set_frames(FrameSet([FrameSensor(Frame(body="cursor0")), FrameSensor(Frame(body="cursor1")), FrameSensor(Frame(body="0_part0"), ref=Frame(body="cursor0"))], velocity=True))
    cb = [int(b) for b in A["cursor_bodyid"]]
    fold = np.asarray(A["body_relpos"], dtype=np.float64).reshape(-1, 3)[cb].astype(np.float32)  # what the library folds the cursor bodies to
    pos0 = np.asarray(A["body_pos"], dtype=np.float64).reshape(-1, 3)[cb].astype(np.float32)  # the model's cursor_pos0 table
    cur = sim.get_state("cursor")["cursor"]
    seen = []
    for shift in (None, (0.125, -0.0625, 0.03125), (-0.3, 0.2, 0.1)):
        if shift is not None:
            c = cur.clone()
            c[:, 0:3] += torch.as_tensor(shift, dtype=c.dtype, device=c.device)
            c[1, 3:6] -= torch.as_tensor(shift, dtype=c.dtype, device=c.device)
            sim.set_state(cursor=c)
        got = _frames(sim)
        now = sim.get_state("cursor")["cursor"].cpu().numpy()
        for k in range(2):
            want = (fold[k][None] + now[:, 3 * k:3 * k + 3]) - pos0[k][None]  # float32, the device's order of operations
            assert got["frame_pos"][:, k].tobytes() == want.astype(np.float32).tobytes(), (shift, k)
        assert (got["frame_vel"][:, :2] == 0).all() and np.abs(got["frame_quat"][:, :2] - np.float32([1, 0, 0, 0])).max() <= QUAT_TOL
        seen.append(got)
    assert seen[0]["frame_pos"].tobytes() != seen[1]["frame_pos"].tobytes() != seen[2]["frame_pos"].tobytes()
    # the part seen from the cursor moves the other way, by the same offset
    d = seen[1]["frame_pos"][:, 2].astype(np.float64) - seen[0]["frame_pos"][:, 2]
    print("toy_table measured: the part seen from the shifted cursor: %.3e off the offset" % np.abs(d + np.array([0.125, -0.0625, 0.03125])).max())
    assert np.abs(d + np.array([0.125, -0.0625, 0.03125])).max() <= 2 * POS_TOL  # (two positions, each within its tolerance)
    sim.close()


# ---- 4. outputs one at a time, S = 1 and S = 64, independence of the other sensors and of the batch ------------------------------------
@pytest.fixture(scope="module")
def lack():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 3)
    qpos, qvel = _random_states(m, 3, seed=5)
    sim.set_state(qpos=qpos, qvel=qvel)
    sensors, _ = _sensors(m)
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    full = _frames(sim)
    yield m, sim, sensors, full
    sim.close()


def test_each_output_alone_and_out_buffers(lack):
    m, sim, sensors, full = lack
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    shapes = sim.frame_shapes()
    assert list(shapes) == list(KEYS) and shapes["frame_jac"][0] == (len(sensors), 6, m.nv)
    L, h = lib(), sim._h
    for i, k in enumerate(KEYS):  # each pointer alone, through the C-ABI
        buf = torch.full((3,) + shapes[k][0], 77.0, device=sim.device)
        ptrs = [None] * 4
        ptrs[i] = buf.data_ptr()
        _poison()
        assert L.fsim_frame_state(h, *ptrs) == 0
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    for k, (sh, dt) in shapes.items():  # out= with a single key
        buf = torch.full((3,) + sh, 77, dtype=dt, device=sim.device)
        res = _frames(sim, out={k: buf})
        assert list(res) == [k] and res[k].tobytes() == full[k].tobytes() and buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    with pytest.raises(ValueError, match="out holds"):
        sim.frame_state(out={})
    with pytest.raises(ValueError, match="out holds"):
        sim.frame_state(out={"frame_acc": torch.zeros(3, device=sim.device)})
    with pytest.raises(ValueError, match="not a contiguous"):
        sim.frame_state(out={"frame_pos": torch.zeros((3, 1), device=sim.device)})
    sim.set_frames(FrameSet(sensors))
    assert list(sim.frame_shapes()) == ["frame_pos", "frame_quat"]
    res = _frames(sim)
    assert sorted(res) == ["frame_pos", "frame_quat"] and all(res[k].tobytes() == full[k].tobytes() for k in res)
    sim.set_frames(FrameSet(sensors, jacobian=True))
    res = _frames(sim)
    assert sorted(res) == ["frame_jac", "frame_pos", "frame_quat"] and all(res[k].tobytes() == full[k].tobytes() for k in res)


def test_sensor_alone_one_and_sixty_four(lack):
    m, sim, sensors, full = lack
    for i in (0, len(sensors) // 2, len(sensors) - 4):  # S = 1: a sensor of the set is the same sensor alone
        sim.set_frames(FrameSet(sensors[i], velocity=True, jacobian=True))
        one = _frames(sim)
        for k in full:
            assert one[k].shape[1] == 1 and one[k][:, 0].tobytes() == np.ascontiguousarray(full[k][:, i]).tobytes(), (i, k)
    order = [(7 * j) % len(sensors) for j in range(64)]  # S = 64: the sensors again, in another order
    sim.set_frames(FrameSet([sensors[i] for i in order], velocity=True, jacobian=True))
    big = _frames(sim)
    for k in full:
        assert big[k].shape[1] == 64 and big[k].tobytes() == np.ascontiguousarray(full[k][:, order]).tobytes(), k


def test_env_alone_is_bit_identical(lack):
    m, sim, sensors, full = lack
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    st = sim.get_state("qpos", "qvel")
    alone = FSim(m, 1)
    alone.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    for e in range(3):
        alone.set_state(qpos=st["qpos"][e:e + 1], qvel=st["qvel"][e:e + 1])
        one = _frames(alone)
        for k in full:
            assert one[k][0].tobytes() == full[k][e].tobytes(), (e, k)
    assert len({full["frame_pos"][e].tobytes() for e in range(3)}) == 3
    alone.close()


def test_second_round_over_dofs_alone_and_sixty_four():
    """Baxter + table_liden_0921 (nv = 91): S = 64 and S = 1 give the rows of each other, and an env of the batch is the same state alone"""
    m = load_compiled("Baxter", "table_liden_0921")
    sim = FSim(m, 3)
    qpos, qvel = _random_states(m, 3, seed=9)
    sim.set_state(qpos=qpos, qvel=qvel)
    sensors, _ = _sensors(m)
    order = [(5 * j) % len(sensors) for j in range(64)]
    sim.set_frames(FrameSet([sensors[i] for i in order], velocity=True, jacobian=True))
    big = _frames(sim)
    assert big["frame_jac"].shape == (3, 64, 6, 91)
    for j in (0, 17, 63):
        sim.set_frames(FrameSet(sensors[order[j]], velocity=True, jacobian=True))
        one = _frames(sim)
        for k in big:
            assert one[k][:, 0].tobytes() == np.ascontiguousarray(big[k][:, j]).tobytes(), (j, k)
    st = sim.get_state("qpos", "qvel")
    alone = FSim(m, 1)
    alone.set_frames(FrameSet([sensors[i] for i in order], velocity=True, jacobian=True))
    alone.set_state(qpos=st["qpos"][2:3], qvel=st["qvel"][2:3])
    one = _frames(alone)
    for k in big:
        assert one[k][0].tobytes() == big[k][2].tobytes(), k
    alone.close()
    sim.close()


# ---- 5. read-only evaluation ----------------------------------------------------------------------------------------------------------
def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_evaluation_is_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _, twin = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 3)
    _steps(twin, 3)
    sensors, _ = _sensors(m)
    sim.set_frames(FrameSet(sensors, velocity=True, jacobian=True))
    before = _all_state(sim)  # every field, env_block included
    assert "env_block" in before and "qvel" in before
    first = _frames(sim)
    _frames(sim, out={"frame_vel": torch.empty((2, len(sensors), 6), device=sim.device)})
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    again = _frames(sim)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    _steps(sim, 2, seed=8)  # a step after a call == the same step without one, bit for bit
    _steps(twin, 2, seed=8)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 6. the env surface -----------------------------------------------------------------------------------------------------------------
def test_env_surface():
    from furniture_amd.envs import FurnitureSawyerEnv, furniture_names, make_config
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    m = load_compiled("Sawyer", "table_lack_0825")
    spec = FrameSet([FrameSensor(Frame(site=a), ref=Frame(site=b)) for a, b in connector_pairs(m)] + [FrameSensor(Frame(site="grip_site"))], velocity=True, jacobian=True)
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), frames=spec)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-4:] == list(KEYS) and "pair_distance" not in ob
    for k, tail in zip(KEYS, ((3,), (4,), (6,), (6, m.nv))):
        assert tuple(ob[k].shape) == (2, 5) + tail and ob[k].dtype == torch.float32 and sp[k].shape == (5,) + tail and sp[k].dtype == np.float32, k
    fresh = env.sim.frame_state()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], ob[k]), k
    rng = np.random.RandomState(0)
    for _ in range(3):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (2, env.dof)).astype(np.float32))
    assert bool(done.all()) and list(ob.keys()) == list(sp.keys())
    kept = {k: ob[k].clone() for k in fresh}
    fresh = env.sim.frame_state()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], kept[k]) and sp[k].contains(ob[k][0].cpu().numpy()), k
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), frames=FrameSet(spec.sensors))  # without the rates
    ob = env.reset()
    assert list(ob.keys()) == list(env.observation_space.spaces.keys()) and list(ob.keys())[-2:] == ["frame_pos", "frame_quat"] and "frame_vel" not in ob
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg())  # without frames: the keys of before
    keys = list(env.reset())
    assert keys == list(env.observation_space.spaces) == [k for k in ob if not k.startswith("frame_")] and env.sim.frames is None and env.frames is None
    env.close()
    e1 = FurnitureSawyerEnv(config=cfg(), frames=FrameSet([FrameSensor(Frame(site="grip_site")), FrameSensor(Frame(body="0_part0"), ref=Frame(site="grip_site"))], velocity=True))
    first = e1.reset()  # the single env keeps its frame set through reset(furniture_id)
    assert first["frame_pos"].shape == (2, 3) and first["frame_vel"].shape == (2, 6)
    other = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert e1._b.furniture_name == "chair_agne_0010" and e1._b.frames is not None and e1._b.sim.frames is e1._b.frames and list(other.keys()) == list(first.keys())
    assert other["frame_pos"].shape == (2, 3) and np.isfinite(np.asarray(other["frame_pos"])).all() and abs(np.linalg.norm(np.asarray(other["frame_quat"])[1]) - 1.0) < 1e-5
    e1.close()


# ---- 7. the C-ABI's error paths -----------------------------------------------------------------------------------------------------------
def test_c_abi_error_paths():
    m = load_compiled("Sawyer", "table_lack_0825")
    sim = FSim(m, 2)
    L, h = lib(), sim._h
    buf = torch.zeros((2, 70), device=sim.device)
    msg = lambda: L.fsim_last_error().decode()

    def table(n=1, body=5, ref_body=-1, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), ref_quat=(1.0, 0.0, 0.0, 0.0)):
        t = (FsimFrameSensor * n)()
        for k in t:
            k.frame.body, k.ref.body = body, ref_body
            k.frame.pos[:], k.frame.quat[:] = list(pos), list(quat)
            k.ref.pos[:], k.ref.quat[:] = [0.0, 0.0, 0.0], list(ref_quat)
        return t

    def refused(rc, text):
        assert rc == -1 and text in msg(), (rc, text, msg())

    def set_frames(n, t):  # (t stays alive over the call)
        return L.fsim_set_frames(h, n, ctypes.addressof(t) if t is not None else None)
    for call_ in (sim.frame_state, sim.frame_shapes):
        with pytest.raises(FsimError, match="no frame set"):
            call_()
    refused(L.fsim_frame_state(h, buf.data_ptr(), None, None, None), "no frame set")
    t0 = table()
    refused(L.fsim_set_frames(None, 1, ctypes.addressof(t0)), "null handle")
    refused(L.fsim_frame_state(None, buf.data_ptr(), None, None, None), "null handle")
    refused(L.fsim_set_frames(h, 1, None), "null argument")
    refused(set_frames(-1, table()), "-1 sensors")
    refused(set_frames(65, table(65)), "65 sensors")
    refused(set_frames(1, table(body=m.nbody)), "frame: unknown body %d" % m.nbody)
    refused(set_frames(1, table(body=-2)), "frame: unknown body -2")
    refused(set_frames(1, table(ref_body=m.nbody + 7)), "reference: unknown body %d" % (m.nbody + 7))
    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0)):
        refused(set_frames(1, table(pos=bad)), "frame: bad pose")
    refused(set_frames(1, table(quat=(0.0, 0.0, 0.0, 0.0))), "frame: bad pose")
    refused(set_frames(1, table(quat=(float("nan"), 0.0, 0.0, 0.0))), "frame: bad pose")
    refused(set_frames(1, table(ref_quat=(0.0, 0.0, 0.0, 0.0))), "reference: bad pose")
    # (a model with more than 32 reduced bodies or nv above 128 is refused by fsim_create already: the two refusals of fsim_set_frames cannot
    #  be reached through a handle; the host check states them too, tests/test_frames.py)
    assert set_frames(64, table(64)) == 0
    assert set_frames(2, table(2, body=-1, quat=(0.0, 2.0, 0.0, 0.0))) == 0  # normalised by the library
    refused(set_frames(1, table(body=-2)), "unknown body")
    big = torch.full((2, 3, 4), 7.0, device=sim.device)  # room for three sensors
    assert L.fsim_frame_state(h, None, big.data_ptr(), None, None) == 0  # a refused set leaves the one before it: two sensors
    torch.cuda.synchronize()
    res = big.cpu().numpy().reshape(-1)
    assert np.abs(res[:16].reshape(4, 4) - np.float32([0, 1, 0, 0])).max() <= 1e-6 and (res[16:] == 7.0).all()  # [2 envs][2 sensors][4], nothing past them
    refused(L.fsim_frame_state(h, None, None, None, None), "no output")
    assert L.fsim_set_frames(h, 0, None) == 0  # clear
    refused(L.fsim_frame_state(h, buf.data_ptr(), None, None, None), "no frame set")
    assert L.fsim_set_frames(h, 0, None) == 0 and L.fsim_set_frames(h, 0, None) == 0  # clearing twice is fine
    sim.set_frames(FrameSet(FrameSensor(Frame(body="right_hand"))))
    sim.set_frames(None)
    with pytest.raises(FsimError, match="no frame set"):
        sim.frame_state()
    with pytest.raises(TypeError, match="FrameSet"):
        sim.set_frames([FrameSensor(Frame(body="right_hand"))])
    sim.close()

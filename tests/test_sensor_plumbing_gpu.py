"""The host plumbing the seven state-sensor families share (FSim._set_sensors / _sensor_outputs / _sensor_call, sensor_install and
sensor_clear of the library, SENSOR_FAMILIES of the env layer), family by family on Sawyer + table_lack_0825 with 2 envs after a reset and
one step: every key alone through out= against the full call bit for bit, the refusals of a wrong out=, set / refused set / clear through
the C ABI, and the observation dict and space of one env with all seven and a camera.  What the outputs hold is the business of
tests/test_{rays,probes,pairs,frames,dynamics,contacts,wrench}_gpu.py; each set here is the smallest that has every key.
FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each call."""
import ctypes

import numpy as np
import pytest
import torch

from furniture_amd.camera import Camera
from furniture_amd.contacts import ContactSet
from furniture_amd.contacts import part_sensors as contact_part_sensors
from furniture_amd.dynamics import Dynamics, arm_dofs
from furniture_amd.envs import FurnitureBatchEnv, make_config
from furniture_amd.frames import Frame, FrameSensor, FrameSet
from furniture_amd.pairs import PairSensor, PairSet, gripper_bodies
from furniture_amd.probes import ProbeSensor, ProbeSet
from furniture_amd.rays import RaySensor, RaySet, lidar
from furniture_amd.sim import FsimContactOut, FsimWrenchOut, lib
from furniture_amd.wrench import WrenchSet, wrist_sensor
from tests.test_camera_gpu import _make, _poison, _steps

pytestmark = pytest.mark.gpu
EINVAL = -1  # FSIM_EINVAL
FAMILIES = ["rays", "probes", "pairs", "frames", "dynamics", "contacts", "wrenches"]


def specs(m):
    """{family: its smallest set with every key}"""
    pts = [(0.0, 0.0, 0.05), (0.02, 0.0, 0.1), (0.0, 0.03, 0.2), (-0.05, 0.0, 0.4)]
    return dict(rays=RaySet([RaySensor((0.0, 0.0, 0.0), lidar(4), body="right_hand", tmax=3.0)], normal=True),
                probes=ProbeSet([ProbeSensor((0.0, 0.0, 0.0), pts, body="right_hand", dmax=1.0)], gradient=True),
                pairs=PairSet([PairSensor(gripper_bodies(m), "0_part0", dmax=3.0)], fromto=True, normal=True),
                frames=FrameSet([FrameSensor(Frame(body="right_hand")), FrameSensor(Frame(body="0_part0"), ref=Frame(body="right_hand"))], velocity=True, jacobian=True),
                dynamics=Dynamics(dofs=arm_dofs(m)[0], mass=True, inverse=True, bias=True, gravity=True),
                contacts=ContactSet(contact_part_sensors(m)[:1], contacts=True),
                wrenches=WrenchSet(wrist_sensor(m), external=True, joint=True))


# family -> (FSim setter, shapes, call; a set the library refuses with FSIM_EINVAL, the clear and a one-pointer call, all three straight through the C ABI)
def _bad_sensors(name, n_extra):
    def bad(L, h):
        tab = (ctypes.c_char * 4096)()  # (a non-NULL table: the count is what is refused)
        return getattr(L, name)(h, -1, ctypes.addressof(tab), *([4, ctypes.addressof(tab), 0, None, None, None] if n_extra else []))
    return bad


def _clear(name, n_extra):
    return lambda L, h: getattr(L, name)(h, 0, None, *([0, None, 0, None, None, None] if n_extra else []))


def _call_ptrs(name, n):
    return lambda L, h, ptr: getattr(L, name)(h, ptr, *[None] * (n - 1))


def _call_struct(name, cls):
    return lambda L, h, ptr: getattr(L, name)(h, ctypes.byref(cls(force=ptr)))


PLUMBING = dict(
    rays=("set_rays", "ray_shapes", "cast_rays", _bad_sensors("fsim_set_rays", True), _clear("fsim_set_rays", True), _call_ptrs("fsim_cast_rays", 3)),
    probes=("set_probes", "probe_shapes", "probe_distance", _bad_sensors("fsim_set_probes", True), _clear("fsim_set_probes", True), _call_ptrs("fsim_probe_distance", 3)),
    pairs=("set_pairs", "pair_shapes", "pair_distance", _bad_sensors("fsim_set_pairs", False), _clear("fsim_set_pairs", False), _call_ptrs("fsim_pair_distance", 4)),
    frames=("set_frames", "frame_shapes", "frame_state", _bad_sensors("fsim_set_frames", False), _clear("fsim_set_frames", False), _call_ptrs("fsim_frame_state", 4)),
    dynamics=("set_dynamics", "dynamics_shapes", "dynamics", _bad_sensors("fsim_set_dynamics", False), _clear("fsim_set_dynamics", False), _call_ptrs("fsim_dynamics", 4)),
    contacts=("set_contacts", "contact_shapes", "contact_forces", _bad_sensors("fsim_set_contacts", False), _clear("fsim_set_contacts", False), _call_struct("fsim_contact_forces", FsimContactOut)),
    wrenches=("set_wrenches", "wrench_shapes", "wrenches", _bad_sensors("fsim_set_wrenches", False), _clear("fsim_set_wrenches", False), _call_struct("fsim_wrenches", FsimWrenchOut)),
)


@pytest.fixture(scope="module")
def handle():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 1)
    yield m, sim
    sim.close()


def _bytes(sim, call, **kw):
    _poison()
    res = getattr(sim, call)(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in res.items()}


@pytest.mark.parametrize("family", FAMILIES)
def test_family(handle, family):
    m, sim = handle
    setter, shapes, call, bad_set, clear, raw_call = PLUMBING[family]
    L, h = lib(), sim._h
    getattr(sim, setter)(specs(m)[family])
    want = getattr(sim, shapes)()
    full = _bytes(sim, call)
    assert list(full) == list(want)
    filled = lambda k: torch.full((2,) + want[k][0], 7, dtype=want[k][1], device=sim.device)
    seven = {k: filled(k).cpu().numpy().tobytes() for k in want}
    # each key alone through out=: the full call's array bit for bit, and nothing else written
    for k in want:
        bufs = {j: filled(j) for j in want}
        got = _bytes(sim, call, out={k: bufs[k]})
        assert list(got) == [k] and got[k] == full[k], (family, k)
        for j in want:
            assert bufs[j].cpu().numpy().tobytes() == (full[j] if j == k else seven[j]), (family, k, j)
    # a wrong out=
    k0 = next(iter(want))
    shape, dt = (2,) + want[k0][0], want[k0][1]
    assert len(shape) >= 2
    for out in ({}, {"no_such_key": filled(k0)}, {k0: filled(k0), "no_such_key": filled(k0)}):
        with pytest.raises(ValueError, match="out holds"):
            getattr(sim, call)(out=out)
    wrong = dict(one_dimension_too_few=filled(k0)[0], wrong_dtype=filled(k0).to(torch.float64), not_contiguous=torch.zeros((), dtype=dt, device=sim.device).expand(shape),
                 on_the_cpu=torch.zeros(shape, dtype=dt))
    assert not wrong["not_contiguous"].is_contiguous()
    for what, t in wrong.items():
        with pytest.raises(ValueError, match="not a contiguous"):
            getattr(sim, call)(out={k0: t})
    # through the C ABI: a refused set leaves the one before it, clearing twice is fine, and then there is nothing to call
    assert bad_set(L, h) == EINVAL
    assert _bytes(sim, call) == full
    assert clear(L, h) == 0 and clear(L, h) == 0
    assert raw_call(L, h, filled(k0).data_ptr()) == EINVAL
    torch.cuda.synchronize()
    getattr(sim, setter)(None)  # (the Python attribute follows)


# the observation of one env with all seven families and a camera: the keys in order, then (shape, dtype, low, high) of observation_space
# (Sawyer + table_lack_0825 under the default ik control: 15 robot values, nv 39, 51 geoms, 48 contact slots; 4 rays, 4 probes, 1 pair
# sensor, 2 frame sensors, 7 arm dofs, 1 contact sensor, 1 wrench sensor; camera 8 x 6, zfar 6)
INF = np.inf
EXPECTED_SPACE = [
    ("object_ob", (35,), np.float32, -INF, INF), ("robot_ob", (15,), np.float32, -INF, INF),
    ("camera_depth", (1, 6, 8), np.float32, 0.0, 6.0), ("camera_segmentation", (1, 6, 8), np.int32, -1, 50),
    ("ray_distance", (4,), np.float32, -1.0, INF), ("ray_geom", (4,), np.int32, -1, 50), ("ray_normal", (4, 3), np.float32, -1.0, 1.0),
    ("probe_distance", (4,), np.float32, -INF, 1.0), ("probe_geom", (4,), np.int32, -1, 50), ("probe_gradient", (4, 3), np.float32, -1.0, 1.0),
    ("pair_distance", (1,), np.float32, -INF, 3.0), ("pair_geoms", (1, 2), np.int32, -1, 50), ("pair_fromto", (1, 6), np.float32, -INF, INF),
    ("pair_normal", (1, 3), np.float32, -1.0, 1.0),
    ("frame_pos", (2, 3), np.float32, -INF, INF), ("frame_quat", (2, 4), np.float32, -INF, INF), ("frame_vel", (2, 6), np.float32, -INF, INF),
    ("frame_jac", (2, 6, 39), np.float32, -INF, INF),
    ("dyn_mass", (7, 7), np.float32, -INF, INF), ("dyn_minv", (7, 7), np.float32, -INF, INF), ("dyn_bias", (7,), np.float32, -INF, INF),
    ("dyn_gravity", (7,), np.float32, -INF, INF),
    ("contact_force", (1, 3), np.float32, -INF, INF), ("contact_touch", (1,), np.float32, 0.0, INF), ("contact_count", (1,), np.int32, 0, 48),
    ("contact_status", (), np.int32, 0, 3), ("con_geoms", (48, 2), np.int32, -1, 50), ("con_pos", (48, 3), np.float32, -INF, INF),
    ("con_normal", (48, 3), np.float32, -INF, INF), ("con_dist", (48,), np.float32, -INF, INF), ("con_force", (48, 3), np.float32, -INF, INF),
    ("con_fn", (48,), np.float32, 0.0, INF),
    ("wrench_force", (1, 3), np.float32, -INF, INF), ("wrench_torque", (1, 3), np.float32, -INF, INF), ("wrench_accel", (1, 3), np.float32, -INF, INF),
    ("wrench_angacc", (1, 3), np.float32, -INF, INF), ("wrench_external", (1, 6), np.float32, -INF, INF), ("wrench_qacc", (39,), np.float32, -INF, INF),
    ("wrench_qfrc_constraint", (39,), np.float32, -INF, INF), ("wrench_status", (), np.int32, 0, 3),
]


def test_env_with_all_seven_families_and_a_camera():
    from furniture_amd.mjcf.model import load_compiled
    m = load_compiled("Sawyer", "table_lack_0825")
    cam = Camera((1.2, -0.9, 1.3), lookat=(0.0, 0.0, 0.8), fovy=50, width=8, height=6, znear=0.02, zfar=6.0)
    cfg = make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=50, seed=3)
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg, cameras=[cam], **specs(m))
    try:
        space = env.observation_space.spaces
        keys = [row[0] for row in EXPECTED_SPACE]
        assert list(space) == keys
        for k, shape, dt, lo, hi in EXPECTED_SPACE:
            b = space[k]
            assert (b.shape, b.dtype) == (shape, np.dtype(dt)) and np.all(b.low == np.asarray(lo, dtype=dt)) and np.all(b.high == np.asarray(hi, dtype=dt)), k
        ob = env.reset()
        assert list(ob) == keys
        _poison()
        ob = env.step(torch.zeros((2, env.dof), device=env.sim.device))[0]
        torch.cuda.synchronize()
        assert list(ob) == keys
        for k in keys:
            assert tuple(ob[k].shape) == (2,) + space[k].shape and ob[k].cpu().numpy().dtype == space[k].dtype, k
    finally:
        env.close()

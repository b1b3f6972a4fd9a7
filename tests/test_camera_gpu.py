"""Depth / segmentation cameras on the device (include/fsim_camera.h) against the float64 reference caster (tests/camera_reference.py)
driven by the oracle's geom poses at the device's own qpos; render is read-only; an env's image is independent of its batch; the env
surface.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each render (stale LDS cannot hide)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from furniture_amd.camera import CAMERA_DTYPE, Camera, hull_plane_table
from furniture_amd.envs import ResetTableSampler, make_config
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import INFO_DIM, FSim, FsimError, default_config, lib
from oracle.oracle_sim import OracleSim
from tests import camera_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
_POISON = os.environ.get("FSIM_TEST_POISON")


def _poison():
    """FSIM_TEST_POISON=<hex>: fill every CU's LDS with the pattern (called before a render)"""
    if _POISON:
        tool = ctypes.CDLL(os.path.join(ROOT, "tests", "liblds_poison.so"))
        for _ in range(2):
            assert tool.lds_poison(ctypes.c_uint(int(_POISON, 16))) == 0


def _render(sim, **kw):
    _poison()
    d, s = sim.render(**kw)
    torch.cuda.synchronize()
    return d, s


def _make(agent, furniture, n, seed=11, max_steps=150):
    m = load_compiled(agent, furniture)
    ecfg = make_config(unity=False, record_vid=False, furniture_name=furniture, max_episode_steps=max_steps, seed=seed)
    tabs = ResetTableSampler(m, ecfg, seed, 0, n)
    cfg = default_config()
    cfg.max_episode_steps, cfg.auto_reset = max_steps, 0
    sim = FSim(m, n, config=cfg)
    p, nz = tabs.draw()
    sim.set_reset_tables(p, nz if agent != "Cursor" else None)
    obs = torch.zeros((n, sim.obs_dim), device=sim.device)
    sim.reset(None, obs)
    sim.sync()
    return m, sim


def _steps(sim, k, seed=5):
    n, dev = sim.n_envs, sim.device
    obs, rew = torch.zeros((n, sim.obs_dim), device=dev), torch.zeros(n, device=dev)
    done, info = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, INFO_DIM), dtype=torch.int32, device=dev)
    rng = np.random.RandomState(seed)
    for _ in range(k):
        act = torch.as_tensor(rng.uniform(-1, 1, (n, sim.dof_action)).astype(np.float32), device=dev)
        torch.cuda.synchronize()
        sim.step(act, obs, rew, done, info)
        sim.sync()


def _cameras(m, qpos, attach, w=W, h=H):
    parts = np.stack([qpos[int(a):int(a) + 3] for a in m.part_qposadr])
    c = parts.mean(0)
    world = Camera(c + np.array([1.1, -0.9, 0.9]), lookat=c, fovy=50, width=w, height=h, znear=0.02, zfar=6.0)
    if attach == "cursor0":  # the cursor box from 0.3 m above, looking straight down
        cam = Camera((0.0, 0.0, 0.3), fovy=70, width=w, height=h, znear=0.02, zfar=6.0, body=attach)
    else:  # wrist camera behind the hand, looking along the gripper
        cam = Camera((0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, width=w, height=h, znear=0.02, zfar=6.0, body=attach)
    return [world, cam]


def _check_against_reference(m, sim, cams, envs, cursor=None):
    sim.set_cameras(cams)
    depth, seg = _render(sim)
    depth, seg = depth.cpu().numpy(), seg.cpu().numpy()
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    osim = OracleSim(m)
    seen = set()
    for e in envs:
        osim.data.qpos[:] = qpos[e]
        if cursor is not None:
            for k, b in enumerate(m.arrays["cursor_bodyid"]):
                osim.model.body_pos[int(b)] = cursor[e, 3 * k:3 * k + 3]
        osim.forward()
        geoms = ref.model_geoms(m, osim.data.geom_xpos, osim.data.geom_xmat)
        for c, cam in enumerate(cams):
            b = cam.body_id(m)
            p, R = cam.world_pose(osim.data.xpos[b] if b >= 0 else None, osim.data.xquat[b] if b >= 0 else None)
            rd, rs = ref.render(p, R, cam.fovy, W, H, cam.znear, cam.zfar, geoms)
            sil = ref.silhouette(p, R, cam.fovy, W, H, cam.znear, cam.zfar, geoms)
            ds, dd = seg[e, c], depth[e, c]
            bad = ds != rs
            assert not (bad & ~sil).any(), "env %d cam %d: %d label mismatches off the silhouette" % (e, c, int((bad & ~sil).sum()))
            assert bad.mean() <= 0.005, "env %d cam %d: %.3f %% silhouette mismatches" % (e, c, 100 * bad.mean())
            ok = ~bad
            err = np.abs(dd[ok] - rd[ok])
            assert (err <= 1e-4 * rd[ok] + 1e-5).all(), "env %d cam %d: depth error %.3g m" % (e, c, err.max())
            seen |= set(np.unique(rs).tolist())
    osim.close()
    return seen


def test_sawyer_lack_reset_then_steps_match_reference():
    m, sim = _make("Sawyer", "table_lack_0825", 8)
    q0 = sim.get_state("qpos")["qpos"][0].cpu().numpy()
    cams = _cameras(m, q0, "right_hand")
    seen = _check_against_reference(m, sim, cams, range(8))
    assert len(seen - {-1}) >= 5  # floor, robot links and parts are in view
    _steps(sim, 30)
    _check_against_reference(m, sim, cams, range(8))
    sim.close()


def test_pinch_attach_state_matches_reference():
    from tests.scenarios import pinch_attach_state
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    sim.physics_forward()
    st = sim.get_state("qpos", "xpos", "xquat")
    q = st["qpos"][0].cpu().numpy().astype(np.float64)
    xp = st["xpos"][0].cpu().numpy().reshape(-1, 3).astype(np.float64)
    xq = st["xquat"][0].cpu().numpy().reshape(-1, 4).astype(np.float64)
    qn, _, _ = pinch_attach_state(m, q, xp, xq)
    sim.set_state(qpos=np.stack([qn, qn]).astype(np.float32))
    cams = _cameras(m, qn, "right_hand")
    seen = _check_against_reference(m, sim, cams, range(2))
    assert len(seen - {-1}) >= 4
    sim.close()


@pytest.mark.parametrize("agent,furniture,attach", [("Sawyer", "chair_agne_0010", "right_hand"), ("Baxter", "desk_mikael_1064", "left_hand"),
                                                    ("Cursor", "toy_table", "cursor0")])
def test_other_models_match_reference(agent, furniture, attach):
    m, sim = _make(agent, furniture, 2)
    cursor = sim.get_state("cursor")["cursor"].cpu().numpy().astype(np.float64) if agent == "Cursor" else None
    q0 = sim.get_state("qpos")["qpos"][0].cpu().numpy()
    seen = _check_against_reference(m, sim, _cameras(m, q0, attach), range(2), cursor)
    if furniture == "chair_agne_0010":  # the hull collider is in view
        g = int(m.arrays["cg_orig"][int(np.nonzero(np.asarray(m.arrays["cg_meshnum"]) > 0)[0][0])])
        assert g in seen
    sim.close()


def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_render_is_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 4)
    sim.physics_forward()
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    before = _all_state(sim)
    _render(sim)
    _render(sim, segmentation=False)
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    sim.close()
    # twenty steps with a render after each == twenty steps without, bit for bit
    runs = []
    for with_render in (False, True):
        m, sim = _make("Sawyer", "table_lack_0825", 4)
        if with_render:
            sim.set_cameras(cams)
        n, dev = sim.n_envs, sim.device
        obs, rew = torch.zeros((n, sim.obs_dim), device=dev), torch.zeros(n, device=dev)
        done, info = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, INFO_DIM), dtype=torch.int32, device=dev)
        rng = np.random.RandomState(9)
        rec = []
        for _ in range(20):
            act = torch.as_tensor(rng.uniform(-1, 1, (n, sim.dof_action)).astype(np.float32), device=dev)
            torch.cuda.synchronize()
            sim.step(act, obs, rew, done, info)
            sim.sync()
            if with_render:
                _render(sim)
            rec.append(b"".join(t.cpu().numpy().tobytes() for t in (obs, rew, done, info)))
        rec.append(b"".join(v.tobytes() for v in _all_state(sim).values()))
        runs.append(rec)
        sim.close()
    assert runs[0] == runs[1]


def test_batch_independence():
    m, big = _make("Sawyer", "table_lack_0825", 4096)
    _steps(big, 2)
    cams = _cameras(m, big.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    big.set_cameras(cams)
    d, s = _render(big)
    state = big.get_state("qpos")["qpos"]
    one = FSim(m, 1, config=big.cfg)
    one.set_cameras(cams)
    for i in (0, 1, 2047, 4095):
        one.set_state(qpos=state[i:i + 1])
        d1, s1 = _render(one)
        assert d1[0].cpu().numpy().tobytes() == d[i].cpu().numpy().tobytes(), i
        assert s1[0].cpu().numpy().tobytes() == s[i].cpu().numpy().tobytes(), i
    one.close()
    big.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv
    cams = [Camera((1.5, -1.0, 1.2), lookat=(0.5, 0.0, 0.3), width=W, height=H), Camera((0, 0, 0.05), body="right_hand", width=W, height=H)]
    cfg = make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg, cameras=cams)
    sp = env.observation_space.spaces
    ob = env.reset()
    for k in ("camera_depth", "camera_segmentation"):
        assert tuple(ob[k].shape) == (4,) + tuple(sp[k].shape)
    assert ob["camera_depth"].dtype == torch.float32 and ob["camera_segmentation"].dtype == torch.int32
    assert list(ob.keys()) == list(sp.keys())
    lab = env.geom_labels()
    assert lab.shape == (env.model.ngeom,)
    parts = torch.where(ob["camera_segmentation"] >= 0, lab[ob["camera_segmentation"].clamp(min=0).long()], torch.full_like(ob["camera_segmentation"], -1))
    assert set(torch.unique(parts).tolist()) <= set(range(-3, env.n_obj)) and len(torch.unique(parts)) >= 2
    rng = np.random.RandomState(0)
    for t in range(3):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert bool(done.all())  # every env auto-reset in the last step: the images show the reset state the observation describes
    d, s = _render(env.sim)
    assert torch.equal(d, ob["camera_depth"]) and torch.equal(s, ob["camera_segmentation"])
    env.close()
    # without cameras: the observation dict of before
    env = FurnitureBatchEnv("Sawyer", 2, config=make_config(unity=False, record_vid=False, furniture_name="table_lack_0825"))
    assert "camera_depth" not in env.reset() and "camera_depth" not in env.observation_space.spaces and env.sim.cameras is None
    env.close()
    # the single env
    e1 = FurnitureSawyerEnv(config=make_config(unity=False, record_vid=False, furniture_name="table_lack_0825"), cameras=cams[:1])
    e1.reset()
    img = e1.render("depth_array")
    assert img.shape == (H, W) and img.dtype == np.float32 and (img > 0).all() and (img <= 10.0).all()
    with pytest.raises(NotImplementedError, match="visual meshes"):
        e1.render("rgb_array")
    e1.close()
    e2 = FurnitureSawyerEnv(config=make_config(unity=False, record_vid=False, furniture_name="table_lack_0825"))
    with pytest.raises(ValueError, match="needs cameras"):
        e2.render("depth_array")
    e2.close()


def test_c_abi_error_paths():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    with pytest.raises(FsimError, match="no cameras set"):
        sim.render()
    rc = lib().fsim_render(sim._h, None, None)
    assert rc == -1
    planes, adr, num = hull_plane_table(m)

    def call(**over):
        tab = np.zeros(2, dtype=CAMERA_DTYPE)
        tab[:] = (-1, (0, 0, 1), (1, 0, 0, 0), 45.0, 0.01, 10.0, 64, 48)
        for k, v in over.items():
            tab[0][k] = v
        return lib().fsim_set_cameras(sim._h, 2, tab.ctypes.data, 0, None, adr.ctypes.data, num.ctypes.data)
    for over, msg in ((dict(body=10000), "unknown body"), (dict(fovy=180.0), "fovy"), (dict(fovy=0.0), "fovy"), (dict(znear=0.0), "znear"),
                      (dict(zfar=0.005), "znear"), (dict(width=0), "size"), (dict(width=513, height=48), "size"), (dict(width=32), "differs")):
        assert call(**over) == -1, over
        assert msg in lib().fsim_last_error().decode(), (over, lib().fsim_last_error())
    tab = np.zeros(9, dtype=CAMERA_DTYPE)
    tab[:] = (-1, (0, 0, 1), (1, 0, 0, 0), 45.0, 0.01, 10.0, 64, 48)
    assert lib().fsim_set_cameras(sim._h, 9, tab.ctypes.data, 0, None, None, None) == -1
    assert call() == 0
    with pytest.raises(FsimError, match="no output"):
        sim._chk(lib().fsim_render(sim._h, None, None))
    sim.close()
    # a mesh collider needs its planes
    mc, simc = _make("Sawyer", "chair_agne_0010", 1)
    tab = np.zeros(1, dtype=CAMERA_DTYPE)
    tab[:] = (-1, (0, 0, 1), (1, 0, 0, 0), 45.0, 0.01, 10.0, 64, 48)
    assert lib().fsim_set_cameras(simc._h, 1, tab.ctypes.data, 0, None, None, None) == -1
    assert "hull planes" in lib().fsim_last_error().decode()
    simc.close()


def test_refusals():
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    cams = [Camera((1, 0, 1), lookat=(0, 0, 0))]
    with pytest.raises(NotImplementedError, match="mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, cameras=cams)
    with pytest.raises(NotImplementedError, match="VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(cameras=cams))
    with pytest.raises(ValueError, match="visual_ob"):
        from furniture_amd.envs import FurnitureBatchEnv
        FurnitureBatchEnv("Sawyer", 1, config=make_config(unity=False, record_vid=False, visual_ob=True))

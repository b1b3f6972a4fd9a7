"""Point clouds on the device (include/fsim_points.h) against the float64 back-projection and the float32 reference FPS
(tests/points_reference.py): the dense map, the labels, the images of the same call, the sampled rows bit for bit, padding, read-only,
batch independence, the env surface and the C-ABI's limits.  States: four models, each after a few random steps."""
import numpy as np
import pytest
import torch

from furniture_amd.camera import Camera
from furniture_amd.envs import make_config
from furniture_amd.points import PointCloud, geom_keep
from furniture_amd.sim import INFO_DIM, FSim, FsimError, lib
from oracle.oracle_sim import OracleSim
from tests import points_reference as ref
from tests.test_camera_gpu import _cameras, _make, _steps

pytestmark = pytest.mark.gpu
ALL = ("parts", "robot", "floor")
# (agent, furniture, body of the second camera): world + wrist / cursor camera, 64 x 48 each
STATES = [("Sawyer", "table_lack_0825", "right_hand"), ("Baxter", "desk_mikael_1064", "left_hand"), ("Cursor", "toy_table", "cursor0"),
          ("Sawyer", "chair_agne_0010", "right_hand")]


def _state(agent, furniture, attach, n=2, steps=3):
    m, sim = _make(agent, furniture, n)
    _steps(sim, steps)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), attach)
    sim.set_cameras(cams)
    return m, sim, cams


def _points(sim, spec, images=False):
    sim.set_points(spec)
    res = sim.render_points(images=images)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _dense(sim):
    """(xyz [n, C, H, W, 3], seg [n, C, H, W], depth) of the dense map with every geom kept and no crop"""
    r = _points(sim, PointCloud(0, include=ALL), images=True)
    return r["point_cloud"], r["camera_segmentation"], r["camera_depth"], r


def _expected_rows(xyz, seg, keep, box, n):
    """(pix [n], K) of the sampled mode by the reference: kept pixels of the dense map in (camera, row, column) order, then FPS"""
    ok = ref.kept(xyz, seg, keep, box).reshape(-1)
    cand = np.nonzero(ok)[0]
    rows = ref.fps(xyz.reshape(-1, 3)[cand], n)
    return np.where(rows >= 0, cand[np.maximum(rows, 0)] if len(cand) else -1, -1), len(cand)


@pytest.mark.parametrize("agent,furniture,attach", STATES)
def test_dense_map_and_labels(agent, furniture, attach):
    """dense xyz == the float64 back-projection of the device's own depth through the oracle's camera pose, to 1e-5 x depth + 1e-5 m: the
    device pose is fp32 kinematics of the same qpos (the camera tests hold its depth to 1e-4 relative against float64; the pose alone is
    good to a few 1e-7 relative), and the point adds three fp32 roundings.  pseg == the segmentation on kept pixels, -1 elsewhere.  The
    images of the call == fsim_render's, bit for bit."""
    m, sim, cams = _state(agent, furniture, attach)
    xyz, seg, depth, r = _dense(sim)
    d0, s0 = sim.render()
    torch.cuda.synchronize()
    assert depth.tobytes() == d0.cpu().numpy().tobytes() and seg.tobytes() == s0.cpu().numpy().tobytes()
    assert np.isfinite(xyz).all()
    np.testing.assert_array_equal(r["point_cloud_segmentation"], np.where(seg >= 0, seg, -1))
    np.testing.assert_array_equal(r["point_cloud_count"], (seg >= 0).reshape(sim.n_envs, -1).sum(1))
    # labels with a narrower keep set
    r2 = _points(sim, PointCloud(0, include=("parts",)))
    keep = geom_keep(m, ("parts",)).astype(bool)
    want = np.where((seg >= 0) & keep[np.maximum(seg, 0)], seg, -1)
    np.testing.assert_array_equal(r2["point_cloud_segmentation"], want)
    assert r2["point_cloud"].tobytes() == xyz.tobytes()
    assert (want >= 0).any() and (want < 0).any()
    # against the float64 back-projection
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    cursor = sim.get_state("cursor")["cursor"].cpu().numpy().astype(np.float64) if agent == "Cursor" else None
    osim = OracleSim(m)
    for e in range(sim.n_envs):
        osim.data.qpos[:] = qpos[e]
        if cursor is not None:
            for k, b in enumerate(m.arrays["cursor_bodyid"]):
                osim.model.body_pos[int(b)] = cursor[e, 3 * k:3 * k + 3]
        osim.forward()
        for c, cam in enumerate(cams):
            b = cam.body_id(m)
            p, R = cam.world_pose(osim.data.xpos[b] if b >= 0 else None, osim.data.xquat[b] if b >= 0 else None)
            want = ref.back_project(depth[e, c], p, R, cam.fovy)
            err = np.abs(xyz[e, c].astype(np.float64) - want).max(-1)
            tol = 1e-5 * depth[e, c] + 1e-5
            assert (err <= tol).all(), "env %d cam %d: %.3g m off (at depth %.3g)" % (e, c, err.max(), depth[e, c].flat[np.argmax(err - tol)])
    osim.close()
    sim.close()


@pytest.mark.parametrize("agent,furniture,attach", STATES)
def test_sampled_matches_reference_fps(agent, furniture, attach):
    """pix exactly the reference FPS's on the dense map's kept pixels; xyz bit-identical to the dense map at pix; pseg == seg at pix"""
    m, sim, cams = _state(agent, furniture, attach)
    xyz, seg, _, _ = _dense(sim)
    lo = np.percentile(xyz[..., 0][seg >= 0], 20), np.percentile(xyz[..., 1][seg >= 0], 20), -0.5
    hi = np.percentile(xyz[..., 0][seg >= 0], 90), np.percentile(xyz[..., 1][seg >= 0], 90), 3.0
    cases = [(("parts", "robot"), None, 256), (("parts",), None, 128), (ALL, None, 300), (("parts", "robot", "floor"), (lo, hi), 200)]
    n, sampled = sim.n_envs, 0
    for include, box, N in cases:
        r = _points(sim, PointCloud(N, include=include, box=box), images=True)
        assert r["camera_segmentation"].tobytes() == seg.tobytes()
        keep = geom_keep(m, include)
        for e in range(n):
            pix, K = _expected_rows(xyz[e], seg[e], keep, None if box is None else np.asarray(box, np.float32), N)
            assert r["point_cloud_count"][e] == K, (include, box, e)
            sampled += K > N
            np.testing.assert_array_equal(r["point_cloud_pixel"][e], pix, err_msg="%s %s env %d" % (include, box, e))
            assert r["point_cloud"][e].tobytes() == xyz[e].reshape(-1, 3)[pix].tobytes()
            np.testing.assert_array_equal(r["point_cloud_segmentation"][e], seg[e].reshape(-1)[pix])
    assert sampled >= len(cases)  # most (env, case) pairs have more candidates than rows: FPS chose among them
    sim.close()


def test_padding_and_empty():
    m, sim, cams = _state("Sawyer", "table_lack_0825", "right_hand")
    xyz, seg, _, _ = _dense(sim)
    keep = geom_keep(m, ALL)
    # a 2 cm box about a seen point: fewer than N kept pixels, rows K .. N-1 repeat row 0
    c = xyz[0].reshape(-1, 3)[np.nonzero(seg[0].reshape(-1) >= 0)[0][100]]
    box = (c - 0.01, c + 0.01)
    N = 64
    r = _points(sim, PointCloud(N, include=ALL, box=box))
    for e in range(sim.n_envs):
        pix, K = _expected_rows(xyz[e], seg[e], keep, np.asarray(box, np.float32), N)
        assert r["point_cloud_count"][e] == K and K < N
        np.testing.assert_array_equal(r["point_cloud_pixel"][e], pix)
        if K:
            assert (r["point_cloud_pixel"][e][K:] == r["point_cloud_pixel"][e][0]).all()
            assert r["point_cloud"][e].tobytes() == xyz[e].reshape(-1, 3)[pix].tobytes()
    assert r["point_cloud_count"][0] >= 1
    # a box that keeps nothing
    r = _points(sim, PointCloud(N, include=ALL, box=((50, 50, 50), (51, 51, 51))))
    assert (r["point_cloud_count"] == 0).all()
    assert (r["point_cloud"] == 0).all() and (r["point_cloud_segmentation"] == -1).all() and (r["point_cloud_pixel"] == -1).all()
    # dense mode with that box: every point is still written, none kept
    r = _points(sim, PointCloud(0, include=ALL, box=((50, 50, 50), (51, 51, 51))))
    assert r["point_cloud"].tobytes() == xyz.tobytes() and (r["point_cloud_segmentation"] == -1).all() and (r["point_cloud_count"] == 0).all()
    sim.close()


def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_render_points_is_read_only():
    m, sim, cams = _state("Sawyer", "table_lack_0825", "right_hand", n=4)
    before = _all_state(sim)
    _points(sim, PointCloud(128), images=True)
    _points(sim, PointCloud(0))
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    sim.close()
    runs = []
    for with_points in (False, True):
        m, sim = _make("Sawyer", "table_lack_0825", 4)
        if with_points:
            sim.set_cameras(cams)
            sim.set_points(PointCloud(128))
        n, dev = sim.n_envs, sim.device
        obs, rew = torch.zeros((n, sim.obs_dim), device=dev), torch.zeros(n, device=dev)
        done, info = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, INFO_DIM), dtype=torch.int32, device=dev)
        rng = np.random.RandomState(9)
        rec = []
        for _ in range(10):
            act = torch.as_tensor(rng.uniform(-1, 1, (n, sim.dof_action)).astype(np.float32), device=dev)
            torch.cuda.synchronize()
            sim.step(act, obs, rew, done, info)
            sim.sync()
            if with_points:
                sim.render_points()
                torch.cuda.synchronize()
            rec.append(b"".join(t.cpu().numpy().tobytes() for t in (obs, rew, done, info)))
        rec.append(b"".join(v.tobytes() for v in _all_state(sim).values()))
        runs.append(rec)
        sim.close()
    assert runs[0] == runs[1]


def test_batch_independence():
    """env i of a batch of 64 == the same state in a batch of 1; one 128 x 128 camera (16384 pixels: the largest candidate layout)"""
    m, big = _make("Sawyer", "table_lack_0825", 64)
    _steps(big, 2)
    q0 = big.get_state("qpos")["qpos"][0].cpu().numpy()
    c = np.stack([q0[int(a):int(a) + 3] for a in m.part_qposadr]).mean(0)
    cams = [Camera(c + np.array([0.9, -0.7, 0.8]), lookat=c, fovy=55, width=128, height=128, znear=0.02, zfar=6.0)]
    spec = PointCloud(512, include=ALL)
    big.set_cameras(cams)
    rb = _points(big, spec)
    state = big.get_state("qpos")["qpos"]
    one = FSim(m, 1, config=big.cfg)
    one.set_cameras(cams)
    for i in (0, 1, 33, 63):
        one.set_state(qpos=state[i:i + 1])
        r1 = _points(one, spec)
        for k in r1:
            assert r1[k][0].tobytes() == rb[k][i].tobytes(), (i, k)
    assert (rb["point_cloud_count"] > 512).all()
    one.close()
    big.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv, furniture_names
    cams = [Camera((1.5, -1.0, 1.2), lookat=(0.5, 0.0, 0.3), width=64, height=48), Camera((0, 0, 0.05), body="right_hand", width=64, height=48)]
    cfg = lambda: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4)
    keys = ("point_cloud", "point_cloud_segmentation", "point_cloud_count")
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), cameras=cams, point_cloud=PointCloud(256))
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and all(k in ob for k in keys + ("camera_depth", "camera_segmentation"))
    assert tuple(ob["point_cloud"].shape) == (4, 256, 3) and ob["point_cloud"].dtype == torch.float32
    assert tuple(ob["point_cloud_segmentation"].shape) == (4, 256) and ob["point_cloud_segmentation"].dtype == torch.int32
    assert tuple(ob["point_cloud_count"].shape) == (4,) and ob["point_cloud_count"].dtype == torch.int32
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    for k in keys + ("camera_depth", "camera_segmentation"):
        for e in range(4):
            assert sp[k].contains(ob[k][e].cpu().numpy()), (k, e)
    # the images and the points come from the one call: the same as a separate render of the same state
    d, s = env.sim.render()
    torch.cuda.synchronize()
    assert torch.equal(d, ob["camera_depth"]) and torch.equal(s, ob["camera_segmentation"])
    pc = ob["point_cloud_segmentation"]
    assert bool((pc >= 0).all())  # 256 of thousands of kept pixels: no padding
    env.close()
    # dense mode
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(0))
    ob = env.reset()
    assert tuple(ob["point_cloud"].shape) == (2, 2, 48, 64, 3) and tuple(ob["point_cloud_segmentation"].shape) == (2, 2, 48, 64)
    assert env.observation_space.spaces["point_cloud"].shape == (2, 48, 64, 3)
    env.close()
    # without point_cloud: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams)
    ob = env.reset()
    assert not any(k in ob or k in env.observation_space.spaces for k in keys) and env.sim.points is None
    assert list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, config=cfg(), point_cloud=PointCloud())
    # the single env carries the point cloud over a furniture change
    e1 = FurnitureSawyerEnv(config=cfg(), cameras=cams[:1], point_cloud=PointCloud(64))
    assert e1.reset()["point_cloud"].shape == (64, 3)
    ob = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert ob["point_cloud"].shape == (64, 3) and e1._b.furniture_name == "chair_agne_0010"
    e1.close()


def test_c_abi_limits():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    xyz, pseg, pix, cnt = (torch.zeros(4096 * 3, device=sim.device), torch.zeros(4096, dtype=torch.int32, device=sim.device),
                           torch.zeros(4096, dtype=torch.int32, device=sim.device), torch.zeros(1, dtype=torch.int32, device=sim.device))
    call = lambda: lib().fsim_render_points(sim._h, None, None, xyz.data_ptr(), pseg.data_ptr(), pix.data_ptr(), cnt.data_ptr())
    assert call() == -1 and "no points settings" in lib().fsim_last_error().decode()
    assert lib().fsim_set_points(sim._h, 16, None, None) == 0
    assert call() == -1 and "no cameras set" in lib().fsim_last_error().decode()
    assert lib().fsim_set_points(sim._h, 4097, None, None) == -1 and "n_points" in lib().fsim_last_error().decode()
    assert lib().fsim_set_points(sim._h, -1, None, None) == -1
    box = np.array([0, 0, 1, 1, 1, 0], np.float32)
    assert lib().fsim_set_points(sim._h, 16, None, box.ctypes.data) == -1 and "box" in lib().fsim_last_error().decode()
    box = np.array([0, 0, 0, 1, np.inf, 1], np.float32)
    assert lib().fsim_set_points(sim._h, 16, None, box.ctypes.data) == -1 and "finite" in lib().fsim_last_error().decode()
    # the pixel cap is checked at render time: cameras that grow past it after set_points
    sim.set_cameras([Camera((1, 0, 1), lookat=(0, 0, 0), width=128, height=128)])
    assert lib().fsim_set_points(sim._h, 16, None, None) == 0
    assert call() == 0
    torch.cuda.synchronize()
    sim.set_cameras([Camera((1, 0, 1), lookat=(0, 0, 0), width=128, height=128)] * 2)
    assert call() == -1 and "pixels per env" in lib().fsim_last_error().decode()
    with pytest.raises(FsimError, match="pixels per env"):
        sim.points = PointCloud(16)
        sim.render_points()
    assert lib().fsim_render_points(sim._h, None, None, None, pseg.data_ptr(), pix.data_ptr(), cnt.data_ptr()) == -1
    sim.close()

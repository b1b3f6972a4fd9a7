"""Voxel grids on the device (include/fsim_voxels.h) against the float32 reference binning (tests/voxels_reference.py) applied to the
device's own dense map of fsim_render_points, taken with the same keep set and box: count and label equal on every cell, for grids of
one LDS chunk, of a non-cubic non-power-of-two shape, of an odd cell count and of several chunks.  Also the images of the same call,
saturation, read-only rendering, batch independence, the env surface and the C-ABI's limits.  States: four models, each after a few
random steps, with a world camera and a wrist or cursor camera."""
import numpy as np
import pytest
import torch

from furniture_amd.camera import Camera
from furniture_amd.envs import make_config
from furniture_amd.points import PointCloud, geom_keep
from furniture_amd.sim import INFO_DIM, FSim, FsimError, lib
from furniture_amd.voxels import VoxelGrid
from tests import voxels_reference as ref
from tests.test_camera_gpu import _make, _steps
from tests.test_points_gpu import ALL, STATES, _all_state, _points, _state

pytestmark = pytest.mark.gpu
# (dims, what it covers): one LDS chunk; non-cubic, non-power-of-two; an odd cell count (int16 stores one by one); four chunks
GRIDS = [(32, 32, 32), (30, 20, 17), (17, 9, 5), (64, 64, 16)]


def _voxels(sim, grid, images=False):
    sim.set_voxels(grid)
    res = sim.render_voxels(images=images)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _boxes(xyz, seg):
    """a box about everything the cameras see, and a tighter one that crops part of it"""
    p = xyz[seg >= 0]
    lo, hi = p.min(0), p.max(0)
    tight_lo = np.percentile(p, 15, axis=0)
    tight_hi = np.percentile(p, 85, axis=0)
    return (lo - 0.01, hi + 0.01), (tight_lo, tight_hi)


def _expect(sim, grid):
    """(count, label) [n, dx, dy, dz] by the reference on the device's dense map, taken with the grid's keep set and box"""
    r = _points(sim, PointCloud(0, include=grid.include, box=grid.box))
    return np.stack([np.stack(ref.voxelize(r["point_cloud"][e], r["point_cloud_segmentation"][e], grid.dims, grid.box)) for e in range(sim.n_envs)], 1)


@pytest.mark.parametrize("agent,furniture,attach", STATES)
def test_grid_matches_reference(agent, furniture, attach):
    m, sim, cams = _state(agent, furniture, attach)
    r = _points(sim, PointCloud(0, include=ALL), images=True)
    xyz, seg = r["point_cloud"], r["camera_segmentation"]
    d0, s0 = r["camera_depth"], seg
    wide, tight = _boxes(xyz, seg)
    filled = multi = dropped = 0
    for dims in GRIDS:
        for include, box in ((ALL, wide), (("parts", "robot"), tight)):
            grid = VoxelGrid(dims, box, include=include)
            want_c, want_l = _expect(sim, grid)
            got = _voxels(sim, grid, images=True)
            assert got["camera_depth"].tobytes() == d0.tobytes() and got["camera_segmentation"].tobytes() == s0.tobytes()
            assert got["voxel_count"].dtype == np.int16 and got["voxel_count"].shape == (sim.n_envs,) + dims
            for e in range(sim.n_envs):
                np.testing.assert_array_equal(got["voxel_count"][e], want_c[e], err_msg="%s %s env %d count" % (dims, include, e))
                np.testing.assert_array_equal(got["voxel_segmentation"][e], want_l[e], err_msg="%s %s env %d label" % (dims, include, e))
            filled += int((want_c > 0).sum())
            multi += int((want_c > 1).sum())
            dropped += int(want_c.sum() < (seg >= 0).sum())
    assert filled > 0 and multi > 0 and dropped > 0  # occupied cells, cells of many pixels, pixels the keep set or box drop
    sim.close()


def test_contention():
    """a 128 x 128 camera looking down from 2 m with the floor kept, over a 4 x 4 x 4 grid: most pixels share a few cells"""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 2)
    sim.set_cameras([Camera((0.3, 0.0, 2.0), lookat=(0.3, 0.01, 0.0), fovy=60, width=128, height=128, znear=0.02, zfar=6.0)])
    r = _points(sim, PointCloud(0, include=ALL), images=True)
    xyz, seg = r["point_cloud"], r["camera_segmentation"]
    box = (xyz[seg >= 0].min(0), xyz[seg >= 0].max(0))
    grid = VoxelGrid((4, 4, 4), box, include=ALL)
    want_c, want_l = _expect(sim, grid)
    got = _voxels(sim, grid)
    np.testing.assert_array_equal(got["voxel_count"], want_c)
    np.testing.assert_array_equal(got["voxel_segmentation"], want_l)
    assert want_c.reshape(2, -1).max(1).min() > 500 and want_c.reshape(2, -1).sum(1).min() > 0.9 * 128 * 128
    sim.close()


def test_saturation():
    """one 192 x 192 camera looking down from 2 m, so that nearly every pixel sees the floor or something on it, over a 1 x 1 x 1 grid
    whose box holds everything within zfar: more than 32767 kept pixels in the one cell"""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 2)
    sim.set_cameras([Camera((0.3, 0.0, 2.0), lookat=(0.3, 0.01, 0.0), fovy=60, width=192, height=192, znear=0.02, zfar=6.0)])
    got = _voxels(sim, VoxelGrid((1, 1, 1), ((-10, -10, -10), (10, 10, 10)), include=ALL), images=True)
    seg = got["camera_segmentation"].reshape(2, -1)
    assert ((seg >= 0).sum(1) > 32767).all()
    assert got["voxel_count"].reshape(2).tolist() == [32767, 32767]
    first = [int(seg[e][np.nonzero(seg[e] >= 0)[0][0]]) for e in range(2)]  # the label: the first kept pixel's geom
    assert got["voxel_segmentation"].reshape(2).tolist() == first
    # the same with the floor dropped: the count of the other pixels, below the cap
    keep = np.asarray(geom_keep(m, ("parts", "robot")), bool)
    got = _voxels(sim, VoxelGrid((1, 1, 1), ((-10, -10, -10), (10, 10, 10)), include=("parts", "robot")))
    kept = (seg >= 0) & keep[np.maximum(seg, 0)]
    assert got["voxel_count"].reshape(2).tolist() == np.minimum(kept.sum(1), 32767).tolist()
    sim.close()


def test_render_voxels_is_read_only():
    m, sim, cams = _state("Sawyer", "table_lack_0825", "right_hand", n=4)
    before = _all_state(sim)
    box = ((-0.5, -0.6, 0.0), (1.0, 0.6, 1.5))
    _voxels(sim, VoxelGrid((32, 32, 32), box), images=True)
    _voxels(sim, VoxelGrid((64, 64, 16), box, include=ALL))
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    sim.close()
    runs = []
    for with_voxels in (False, True):
        m, sim = _make("Sawyer", "table_lack_0825", 4)
        if with_voxels:
            sim.set_cameras(cams)
            sim.set_voxels(VoxelGrid((32, 32, 32), box))
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
            if with_voxels:
                sim.render_voxels()
                torch.cuda.synchronize()
            rec.append(b"".join(t.cpu().numpy().tobytes() for t in (obs, rew, done, info)))
        rec.append(b"".join(v.tobytes() for v in _all_state(sim).values()))
        runs.append(rec)
        sim.close()
    assert runs[0] == runs[1]


def test_batch_independence():
    """env i of a batch of 64 == the same state in a batch of 1; a grid of four LDS chunks"""
    m, big = _make("Sawyer", "table_lack_0825", 64)
    _steps(big, 2)
    q0 = big.get_state("qpos")["qpos"][0].cpu().numpy()
    c = np.stack([q0[int(a):int(a) + 3] for a in m.part_qposadr]).mean(0)
    cams = [Camera(c + np.array([0.9, -0.7, 0.8]), lookat=c, fovy=55, width=96, height=96, znear=0.02, zfar=6.0)]
    grid = VoxelGrid((64, 64, 16), (c - 0.6, c + 0.6), include=ALL)
    big.set_cameras(cams)
    rb = _voxels(big, grid)
    state = big.get_state("qpos")["qpos"]
    one = FSim(m, 1, config=big.cfg)
    one.set_cameras(cams)
    for i in (0, 1, 33, 63):
        one.set_state(qpos=state[i:i + 1])
        r1 = _voxels(one, grid)
        for k in r1:
            assert r1[k][0].tobytes() == rb[k][i].tobytes(), (i, k)
    assert (rb["voxel_count"].reshape(64, -1).sum(1) > 100).all()
    one.close()
    big.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv, furniture_names
    cams = [Camera((1.5, -1.0, 1.2), lookat=(0.5, 0.0, 0.3), width=64, height=48), Camera((0, 0, 0.05), body="right_hand", width=64, height=48)]
    cfg = lambda: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4)
    keys = ("voxel_count", "voxel_segmentation")
    grid = VoxelGrid((30, 20, 17), ((-0.6, -0.6, -0.1), (1.0, 0.6, 1.4)), include=ALL)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), cameras=cams, voxels=grid)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and all(k in ob for k in keys + ("camera_depth", "camera_segmentation"))
    for k in keys:
        assert tuple(ob[k].shape) == (4, 30, 20, 17) and ob[k].dtype == torch.int16 and sp[k].shape == (30, 20, 17) and sp[k].dtype == np.int16
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert list(ob.keys()) == list(sp.keys())
    for k in keys + ("camera_depth", "camera_segmentation"):
        for e in range(4):
            assert sp[k].contains(ob[k][e].cpu().numpy()), (k, e)
    # the images and the grid come from the one call: the same as a separate render of the same state
    d, s = env.sim.render()
    torch.cuda.synchronize()
    assert torch.equal(d, ob["camera_depth"]) and torch.equal(s, ob["camera_segmentation"])
    assert bool((ob["voxel_count"].reshape(4, -1).sum(1) > 0).all())
    env.close()
    # with a point cloud as well: both sets of keys, in the order of the observation space
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(64), voxels=grid)
    ob = env.reset()
    assert list(ob.keys()) == list(env.observation_space.spaces.keys()) and "point_cloud" in ob and "voxel_count" in ob
    env.close()
    # without voxels: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams)
    ob = env.reset()
    assert not any(k in ob or k in env.observation_space.spaces for k in keys) and env.sim.voxels is None
    assert list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, config=cfg(), voxels=grid)
    # the single env carries the grid over a furniture change
    e1 = FurnitureSawyerEnv(config=cfg(), cameras=cams[:1], voxels=grid)
    assert e1.reset()["voxel_count"].shape == (30, 20, 17)
    ob = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert ob["voxel_count"].shape == (30, 20, 17) and e1._b.furniture_name == "chair_agne_0010"
    e1.close()


def test_refusals_with_a_device():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    grid = VoxelGrid((8, 8, 8), ((-1, -1, 0), (1, 1, 2)))
    with pytest.raises(NotImplementedError, match="mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, voxels=grid)
    with pytest.raises(NotImplementedError, match="VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(voxels=grid))
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    sim.set_voxels(grid)  # voxel settings alone: no cameras, no points
    with pytest.raises(NotImplementedError, match="voxel grids"):
        step_wait_and_gather(sim, None, None, None)
    sim.close()


def test_c_abi_limits():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    dev = sim.device
    cnt, lab = torch.zeros(4096, dtype=torch.int16, device=dev), torch.zeros(4096, dtype=torch.int16, device=dev)
    err = lambda: lib().fsim_last_error().decode()
    call = lambda: lib().fsim_render_voxels(sim._h, None, None, cnt.data_ptr(), lab.data_ptr())
    i32 = lambda *d: np.array(d, np.int32)
    f32 = lambda *b: np.array(b, np.float32)
    box = f32(-1, -1, 0, 1, 1, 2)
    setv = lambda d, b, keep=None: lib().fsim_set_voxels(sim._h, d.ctypes.data if d is not None else None, b.ctypes.data if b is not None else None, keep)
    assert call() == -1 and "no voxel settings" in err()
    assert setv(i32(16, 16, 16), box) == 0
    assert call() == -1 and "no cameras set" in err()
    # dims
    for d in ((0, 4, 4), (4, -1, 4), (4, 4, 257)):
        assert setv(i32(*d), box) == -1 and "dims" in err(), d
    assert setv(i32(64, 64, 65), box) == -1 and "cells" in err()
    assert setv(i32(256, 1, 1), box) == 0 and setv(i32(64, 64, 64), box) == 0
    # the box
    assert setv(i32(4, 4, 4), None) == -1 and "box" in err()
    assert setv(None, box) == -1
    for b in ((-1, -1, 0, 1, np.inf, 2), (-1, np.nan, 0, 1, 1, 2)):
        assert setv(i32(4, 4, 4), f32(*b)) == -1 and "finite" in err(), b
    for b in ((-1, -1, 0, 1, 1, 0), (-1, -1, 2, 1, 1, 0), (1, -1, 0, -1, 1, 2)):
        assert setv(i32(4, 4, 4), f32(*b)) == -1 and "lo" in err(), b
    assert setv(i32(4, 4, 4), f32(-3e38, -1, 0, 3e38, 1, 2)) == -1 and "scale" in err()
    # NULL outputs
    sim.set_cameras([Camera((1, 0, 1), lookat=(0, 0, 0), width=16, height=16)])
    assert setv(i32(16, 16, 16), box) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert lib().fsim_render_voxels(sim._h, None, None, None, lab.data_ptr()) == -1 and "NULL output" in err()
    assert lib().fsim_render_voxels(sim._h, None, None, cnt.data_ptr(), None) == -1 and "NULL output" in err()
    with pytest.raises(FsimError, match="no voxel settings"):
        sim.render_voxels()  # (the settings above went through the C-ABI, not FSim.set_voxels)
    assert sim.cm.ngeom <= 32767  # (the ngeom limit: no catalogue model comes near it)
    sim.close()

"""Flow / velocity images on the device (include/fsim_flow.h) against the float64 reference (tests/flow_reference.py) evaluated at the
device's own depth and segmentation images and the device's own qpos / qvel; the exact properties (nothing seen, nothing moving, the
world seen from a world camera); ego-motion cancelling on the wrist camera's own body; read-only rendering; batch independence; image
sizes that leave partial rounds; the scratch following the camera set; the env surface; the C-ABI's error paths.
FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each render.

Every hit pixel is compared: no silhouette or margin exclusion.  The measures are flow_reference.measures: the velocity error and the
depth-rate error relative to max(S, 1e-3), S the magnitude of what the pixel's velocity was added up from, and the image-plane flow
error in its metric form (times d s / (1 + |cx| + |cy|)), so that near pixels do not dominate."""
import numpy as np
import pytest
import torch

from furniture_amd.camera import Camera
from furniture_amd.envs import make_config
from furniture_amd.flow import Flow
from furniture_amd.points import PointCloud
from furniture_amd.sim import FSim, FsimError, lib
from oracle.oracle_sim import OracleSim
from tests import flow_reference as fref
from tests.test_camera_gpu import _cameras, _make, _poison, _steps

pytestmark = pytest.mark.gpu
W, H = 64, 48  # 3072 pixels: two chunks of the flow pass, the second one half full
# fp32 kinematics (2e-6 m against the oracle) and rounding: of order 1e-5.  The tolerance is 4 x the largest ratio measured on
# an MI355X over the cases of this file, and never above 1e-3
FLOW_TOL = 3.2e-5  # measured: 7.84e-6 (the velocity of Sawyer + table_lack_0825 after the reset with random qvel, 12176 hit pixels)
BOTH = Flow(flow=True, velocity=True)


def _render(sim, **kw):
    _poison()
    res = sim.render_flow(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _random_qvel(sim, seed=7):
    sim.set_state(qvel=np.random.RandomState(seed).uniform(-1, 1, (sim.n_envs, sim.nv)).astype(np.float32))


def _reference(m, sim, cams, res, envs, cursor=None):
    """the reference of the listed envs at the device's own images and state -> list of flow_reference.render dicts"""
    st = sim.get_state("qpos", "qvel")
    qpos, qvel = st["qpos"].cpu().numpy().astype(np.float64), st["qvel"].cpu().numpy().astype(np.float64)
    osim = OracleSim(m)
    out = [fref.render(osim, m, qpos[e], qvel[e], cams, res["camera_depth"][e], res["camera_segmentation"][e], None if cursor is None else cursor[e])
           for e in envs]
    osim.close()
    return out


def _check_against_reference(m, sim, cams, envs, cursor=None, tag=""):
    """every hit pixel of every image of the listed envs against the reference; the images against FSim.render's; seg < 0 gives zeros.
    -> (the device's outputs, the references, the largest ratio)"""
    sim.set_cameras(cams)
    sim.set_flow(BOTH)
    res = _render(sim, images=True)
    d0, s0 = sim.render()
    torch.cuda.synchronize()
    assert res["camera_depth"].tobytes() == d0.cpu().numpy().tobytes() and res["camera_segmentation"].tobytes() == s0.cpu().numpy().tobytes()
    seg, flow, vel = res["camera_segmentation"], res["camera_flow"], res["camera_velocity"]
    w, h = cams[0].width, cams[0].height
    for a in (flow, vel):
        assert a.shape == (sim.n_envs, len(cams), h, w, 3) and a.dtype == np.float32 and np.isfinite(a).all()
    assert (flow[seg < 0] == 0).all() and (vel[seg < 0] == 0).all()
    refs = _reference(m, sim, cams, res, envs, cursor)
    worst = dict(velocity=0.0, flow_xy=0.0, flow_z=0.0)
    pixels = 0
    for e, ref in zip(envs, refs):
        hit = seg[e] >= 0
        for k, v in fref.measures(ref, flow[e], vel[e]).items():
            worst[k] = max(worst[k], float(v[hit].max(initial=0.0)))
        pixels += int(hit.sum())
    print("%s: %d hit pixels, velocity within %.3g, flow within %.3g (image plane) and %.3g (depth rate)" %
          (tag, pixels, worst["velocity"], worst["flow_xy"], worst["flow_z"]))
    for k, v in worst.items():
        assert v <= FLOW_TOL, "%s: %s off by %.3g" % (tag, k, v)
    return res, refs, max(worst.values())


@pytest.mark.parametrize("agent,furniture,attach", [("Sawyer", "table_lack_0825", "right_hand"), ("Baxter", "desk_mikael_1064", "left_hand"),
                                                    ("Cursor", "toy_table", "cursor0"), ("Sawyer", "chair_agne_0010", "right_hand")])
def test_models_match_reference(agent, furniture, attach):
    """after a reset with every dof given a random velocity (free bodies spinning included), then as 30 random steps leave the state"""
    m, sim = _make(agent, furniture, 2)
    cursor = (lambda: sim.get_state("cursor")["cursor"].cpu().numpy().astype(np.float64)) if agent == "Cursor" else (lambda: None)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), attach)
    _random_qvel(sim)
    res, refs, _ = _check_against_reference(m, sim, cams, range(2), cursor(), tag="%s reset + qvel" % furniture)
    hit = res["camera_segmentation"] >= 0
    assert hit.sum() > 4000 and np.abs(res["camera_velocity"][hit]).max() > 0.1 and np.abs(res["camera_flow"][hit]).max() > 1.0
    if attach != "cursor0":  # the wrist camera moves: what stands still in the world flows in its image
        assert max(r["scale"][1].max() for r in refs) > 0.1
    if furniture == "chair_agne_0010":
        assert 7 in np.asarray(m.arrays["geom_type"])[np.unique(res["camera_segmentation"][hit])]  # the hull collider is in view
    _steps(sim, 30)
    _check_against_reference(m, sim, cams, range(2), cursor(), tag="%s 30 steps" % furniture)
    sim.close()


def test_exact_zeros():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_flow(BOTH)
    # nothing moves: both outputs are zero everywhere, the wrist camera's included
    sim.set_state(qvel=np.zeros((2, sim.nv), np.float32))
    res = _render(sim, images=True)
    assert (res["camera_segmentation"] >= 0).sum() > 4000
    assert (res["camera_flow"] == 0).all() and (res["camera_velocity"] == 0).all()
    # everything moves: what the world camera sees of reduced body 0 (floor, arena) stands still, exactly
    _random_qvel(sim)
    res = _render(sim, images=True)
    seg = res["camera_segmentation"][:, 0]
    rbody = np.asarray(m.arrays["body_red"])[np.asarray(m.arrays["geom_bodyid"])]
    still = (seg >= 0) & (rbody[np.maximum(seg, 0)] == 0)
    moving = (seg >= 0) & ~still
    assert still.sum() > 500 and moving.sum() > 200
    assert (res["camera_flow"][:, 0][still] == 0).all() and (res["camera_velocity"][:, 0][still] == 0).all()
    assert (np.abs(res["camera_velocity"][:, 0][moving]).max(-1) > 0).mean() > 0.99
    assert (res["camera_flow"][res["camera_segmentation"] < 0] == 0).all() and (res["camera_velocity"][res["camera_segmentation"] < 0] == 0).all()
    sim.close()


def test_ego_motion_cancels_on_the_cameras_own_body():
    """the wrist camera rides on the hand: the hand's own geoms move in the world and stand still in its image"""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_flow(BOTH)
    _random_qvel(sim)
    res = _render(sim, images=True)
    refs = _reference(m, sim, cams, res, range(2))
    body_red = np.asarray(m.arrays["body_red"])
    rbody = body_red[np.asarray(m.arrays["geom_bodyid"])]
    examined = 0
    for e, ref in enumerate(refs):
        seg = res["camera_segmentation"][e, 1]
        own = (seg >= 0) & (rbody[np.maximum(seg, 0)] == body_red[cams[1].body_id(m)]) & (ref["scale"][1] >= 0.1)
        examined += int(own.sum())
        zero = dict(ref, flow=np.zeros_like(ref["flow"]))
        ms = fref.measures(zero, flow=res["camera_flow"][e])
        worst = max(float(ms["flow_xy"][1][own].max(initial=0.0)), float(ms["flow_z"][1][own].max(initial=0.0)))
        print("env %d: %d pixels on the camera's own body, flow within %.3g of zero" % (e, own.sum(), worst))
        assert worst <= FLOW_TOL
        assert (np.abs(res["camera_velocity"][e, 1][own]).max(-1) > 0).all()
    assert examined >= 200
    sim.close()


def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_render_flow_is_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 3)
    _steps(sim, 2)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_flow(BOTH)
    before = _all_state(sim)
    _render(sim)
    _render(sim, images=True)
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    sim.close()


def test_batch_independence():
    m, big = _make("Sawyer", "table_lack_0825", 3)
    _steps(big, 2)
    cams = _cameras(m, big.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    big.set_cameras(cams)
    big.set_flow(BOTH)
    rb = _render(big, images=True)
    st = big.get_state("qpos", "qvel")
    assert float(st["qvel"].abs().max()) > 0
    one = FSim(m, 1, config=big.cfg)
    one.set_cameras(cams)
    one.set_flow(BOTH)
    for i in range(3):
        one.set_state(qpos=st["qpos"][i:i + 1], qvel=st["qvel"][i:i + 1])
        r1 = _render(one, images=True)
        for k in r1:
            assert r1[k][0].tobytes() == rb[k][i].tobytes(), (i, k)
    one.close()
    big.close()


def test_five_by_three_image():
    """15 pixels: one partial round of one chunk, every other lane idle.  Against the reference, and the same as three cameras"""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _random_qvel(sim)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand", 5, 3)
    both, _, _ = _check_against_reference(m, sim, cams, range(2), tag="5x3 x2")
    assert (both["camera_segmentation"] >= 0).sum() > 20
    for k, cam in enumerate(cams):
        one, _, _ = _check_against_reference(m, sim, [cam], range(2), tag="5x3 cam %d" % k)
        for key in one:
            assert one[key][:, 0].tobytes() == both[key][:, k].tobytes(), (key, k)
    sim.close()


def test_one_output_at_a_time_and_out_buffers():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _random_qvel(sim)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_flow(BOTH)
    both = _render(sim)
    assert sorted(both) == ["camera_flow", "camera_velocity"] and np.abs(both["camera_flow"]).max() > 0
    sim.set_flow(Flow(flow=True, velocity=False))
    only = _render(sim)
    assert list(only) == ["camera_flow"] and only["camera_flow"].tobytes() == both["camera_flow"].tobytes()
    sim.set_flow(Flow(flow=False, velocity=True))
    only = _render(sim, images=True)
    assert sorted(only) == ["camera_depth", "camera_segmentation", "camera_velocity"] and only["camera_velocity"].tobytes() == both["camera_velocity"].tobytes()
    # out=: the caller's tensors are the ones written and returned; a key left out gets a new tensor
    sim.set_flow(BOTH)
    dev = sim.device
    out = dict(camera_flow=torch.full((2, 2, H, W, 3), 7.0, device=dev), camera_depth=torch.full((2, 2, H, W), 7.0, device=dev))
    _poison()
    res = sim.render_flow(images=True, out=out)
    torch.cuda.synchronize()
    assert res["camera_flow"] is out["camera_flow"] and res["camera_depth"] is out["camera_depth"]
    assert res["camera_flow"].cpu().numpy().tobytes() == both["camera_flow"].tobytes()
    assert res["camera_velocity"].cpu().numpy().tobytes() == both["camera_velocity"].tobytes()
    assert res["camera_depth"].cpu().numpy().tobytes() == sim.render()[0].cpu().numpy().tobytes()
    with pytest.raises(AssertionError, match="wrong shape"):
        sim.render_flow(out=dict(camera_flow=torch.zeros((2, 2, H, W, 2), device=dev)))
    sim.close()


def test_scratch_follows_the_camera_set():
    """a small camera set first, then more and larger images: the twist scratch and the image scratch are sized by the set of the call"""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _random_qvel(sim)
    st = sim.get_state("qpos", "qvel")
    q0 = st["qpos"][0].cpu().numpy()
    sim.set_flow(BOTH)
    sim.set_cameras(_cameras(m, q0, "right_hand", 33, 17)[:1])
    small = _render(sim)
    assert small["camera_flow"].shape == (2, 1, 17, 33, 3)
    cams = _cameras(m, q0, "right_hand")
    sim.set_cameras(cams)
    got = _render(sim)
    fresh = FSim(m, 2, config=sim.cfg)
    fresh.set_state(qpos=st["qpos"], qvel=st["qvel"])
    fresh.set_cameras(cams)
    fresh.set_flow(BOTH)
    want = _render(fresh, images=True)
    for k in got:
        assert got[k].shape == (2, 2, H, W, 3) and got[k].tobytes() == want[k].tobytes(), k
    sim.set_cameras(_cameras(m, q0, "right_hand", 33, 17)[:1])  # and back
    again = _render(sim)
    for k in small:
        assert again[k].tobytes() == small[k].tobytes(), k
    fresh.close()
    sim.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv
    cams = [Camera((1.5, -1.0, 1.2), lookat=(0.5, 0.0, 0.3), width=W, height=H), Camera((0, 0, 0.05), body="right_hand", width=W, height=H)]
    cfg = lambda: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4)
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, flow=BOTH)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-4:] == ["camera_depth", "camera_segmentation", "camera_flow", "camera_velocity"]
    for k in ("camera_flow", "camera_velocity"):
        assert tuple(ob[k].shape) == (2, 2, H, W, 3) and ob[k].dtype == torch.float32
        assert sp[k].shape == (2, H, W, 3) and sp[k].dtype == np.float32
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (2, env.dof)).astype(np.float32))
    assert list(ob.keys()) == list(sp.keys()) and float(ob["camera_velocity"].abs().max()) > 0
    kept = {k: ob[k].clone() for k in ("camera_depth", "camera_segmentation", "camera_flow", "camera_velocity")}
    fresh = env.sim.render_flow(images=True)
    torch.cuda.synchronize()
    for k in kept:
        assert torch.equal(fresh[k], kept[k]), k
    env.close()
    # with a point cloud as well: point_cloud_velocity is camera_velocity at the cloud's pixels
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(64), flow=BOTH)
    env.reset()
    ob, _, _, _ = env.step(rng.uniform(-1, 1, (2, env.dof)).astype(np.float32))
    assert list(ob.keys()) == list(env.observation_space.spaces.keys())
    assert list(ob.keys())[-3:] == ["camera_flow", "camera_velocity", "point_cloud_velocity"] and tuple(ob["point_cloud_velocity"].shape) == (2, 64, 3)
    pix = env._pts_out["point_cloud_pixel"].cpu().numpy()
    assert (pix >= 0).all()
    img = ob["camera_velocity"].cpu().numpy().reshape(2, -1, 3)
    want = np.stack([img[e][pix[e]] for e in range(2)])
    assert ob["point_cloud_velocity"].cpu().numpy().tobytes() == want.tobytes() and np.abs(want).max() > 0
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(0, include=("robot",)), flow=Flow(flow=False, velocity=True))
    env.reset()
    ob, _, _, _ = env.step(rng.uniform(-1, 1, (2, env.dof)).astype(np.float32))
    assert "camera_flow" not in ob and list(ob.keys()) == list(env.observation_space.spaces.keys())
    assert tuple(ob["point_cloud_velocity"].shape) == (2, 2, H, W, 3) and env.observation_space.spaces["point_cloud_velocity"].shape == (2, H, W, 3)
    lab, v_img, v_pts = ob["point_cloud_segmentation"].cpu().numpy(), ob["camera_velocity"].cpu().numpy(), ob["point_cloud_velocity"].cpu().numpy()
    assert (lab >= 0).any() and ((lab < 0) & (ob["camera_segmentation"].cpu().numpy() >= 0)).any()  # pixels the keep set drops
    assert (v_pts[lab < 0] == 0).all() and v_pts[lab >= 0].tobytes() == v_img[lab >= 0].tobytes()
    env.close()
    # flow only with a point cloud: no point_cloud_velocity
    env = FurnitureBatchEnv("Sawyer", 1, config=cfg(), cameras=cams, point_cloud=PointCloud(16), flow=Flow())
    ob = env.reset()
    assert "camera_flow" in ob and "camera_velocity" not in ob and "point_cloud_velocity" not in ob and list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    # without flow: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams)
    ob = env.reset()
    new = ("camera_flow", "camera_velocity", "point_cloud_velocity")
    assert not any(k in ob or k in env.observation_space.spaces for k in new) and env.sim.flow is None
    assert list(ob.keys())[-2:] == ["camera_depth", "camera_segmentation"] and list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    # the single env, without flow=: a temporary default Flow
    e1 = FurnitureSawyerEnv(config=cfg(), cameras=cams[1:])
    first = e1.reset()
    e1.step(rng.uniform(-1, 1, e1._b.dof).astype(np.float32))
    img = e1.render("flow_array")
    assert img.shape == (H, W, 3) and img.dtype == np.float32 and np.abs(img).max() > 0
    vel = e1.render("velocity_array")
    assert vel.shape == (H, W, 3) and vel.dtype == np.float32 and np.abs(vel).max() > 0
    assert e1._b.sim.flow is None
    assert list(e1.reset().keys()) == list(first.keys())  # rendering a picture leaves the observations as they were
    e1.close()
    e2 = FurnitureSawyerEnv(config=cfg(), cameras=cams[1:], flow=Flow())
    e2.reset()
    ob, _, _, _ = e2.step(rng.uniform(-1, 1, e2._b.dof).astype(np.float32))
    assert ob["camera_flow"].shape == (1, H, W, 3) and "camera_velocity" not in ob
    assert (e2.render("flow_array") == ob["camera_flow"][0].astype(np.float32)).all()
    assert e2.render("velocity_array").shape == (H, W, 3) and e2._b.sim.flow is e2._b.flow
    e2.close()
    e3 = FurnitureSawyerEnv(config=cfg())
    with pytest.raises(ValueError, match="needs cameras"):
        e3.render("flow_array")
    e3.close()


def test_c_abi_error_paths():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    dev = sim.device
    buf = torch.full((16 * 16 * 3 + 3,), 5.0, dtype=torch.float32, device=dev)
    err = lambda: lib().fsim_last_error().decode()
    call = lambda f, v: lib().fsim_render_flow(sim._h, None, None, f, v)
    assert lib().fsim_render_flow(None, None, None, buf.data_ptr(), None) == -1 and "null handle" in err()
    assert call(buf.data_ptr(), None) == -1 and "no cameras set" in err()
    sim.set_cameras([Camera((1, 0, 1), lookat=(0, 0, 0), width=16, height=16)])
    assert call(None, None) == -1 and "no output" in err()
    assert call(buf.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[16 * 16 * 3:] == 5.0).all() and np.isfinite(got).all() and (got[:16 * 16 * 3] != 5.0).any()  # nothing past the image
    assert call(None, buf.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy()[16 * 16 * 3:] == 5.0).all()
    with pytest.raises(FsimError, match="no flow settings"):
        sim.render_flow()  # (FSim.set_flow was never called)
    sim.close()

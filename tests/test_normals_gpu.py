"""Normal / shaded images on the device (include/fsim_normals.h) against the float64 reference (tests/normals_reference.py) driven by the
oracle's geom poses at the device's own qpos; the structure of the normal image; the shaded image against the header's formula applied
to the device's own normals; image sizes that leave partial rounds and chunks; read-only rendering; batch independence; the env
surface; the C-ABI's error paths.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each render.

Which pixels are compared with the reference: those whose label the device and the reference agree on, off the reference's silhouette,
with an ambiguity margin (normals_reference) of at least 5e-4 m -- the hit point carries the depth error, so nearer to an edge than that
the other face may legitimately win -- and on a flat face or a curved one of radius at least 5 mm.  At most 15 % of an image's hit
pixels may be left out.  Flat pixels: every component within 1e-5 (the normal is a column of the geom's rotation; the device's
kinematics agree with the oracle's to 2e-6).  Curved pixels: the angle to the reference is at most CURVED_TOL."""
import numpy as np
import pytest
import torch

from furniture_amd.camera import Camera
from furniture_amd.envs import make_config
from furniture_amd.normals import Normals, default_palette
from furniture_amd.points import PointCloud
from furniture_amd.sim import INFO_DIM, FSim, FsimError, lib
from furniture_amd.voxels import VoxelGrid
from oracle.oracle_sim import OracleSim
from tests import camera_reference as cref
from tests import normals_reference as nref
from tests.test_camera_gpu import _cameras, _make, _poison, _steps

pytestmark = pytest.mark.gpu
W, H = 64, 48  # 3072 pixels: two chunks of the normal pass, the second one half full
MARGIN, MIN_RADIUS, LEFT_OUT, FLAT_TOL = 5e-4, 5e-3, 0.15, 1e-5
# curved surfaces (sphere, capsule, cylinder side): the normal turns by (error of the hit point) / radius.  The tolerance is 4 x the
# largest angle measured on an MI355X over the cases of this file, and never above 1e-2 rad
CURVED_TOL = 6.1e-5  # measured: 1.51e-5 rad (a cylinder of chair_agne_0010's robot, 874 curved pixels)
BOTH = Normals(normal=True, shaded=True, ambient=0.25, background=(30, 30, 40, 255))


def _render(sim, **kw):
    _poison()
    res = sim.render_normals(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _shade(normal, seg, depth, cam_pos, cam_R, cam, spec, palette):
    """the header's shading formula in numpy float32, from the device's normal, label and depth and the oracle's camera pose"""
    f = np.float32
    h, w = seg.shape
    rays = cref.pixel_rays(cam_R, cam.fovy, w, h).astype(f)
    q = cam_pos.astype(f) + rays * depth[..., None]
    v = cam_pos.astype(f) - q
    ln = np.sqrt((v * v).sum(-1, dtype=f))
    v = np.where(ln[..., None] < 1e-20, f(0), v / np.maximum(ln, f(1e-30))[..., None])
    lam = np.abs((normal * v).sum(-1, dtype=f))
    inten = f(spec.ambient) + (f(1) - f(spec.ambient)) * lam
    pal = palette[np.maximum(seg, 0)]
    out = np.empty((h, w, 4), dtype=np.uint8)
    out[..., :3] = np.minimum(np.floor(pal[..., :3].astype(f) * inten[..., None] + f(0.5)), 255).astype(np.uint8)
    out[..., 3] = pal[..., 3]
    out[seg < 0] = spec.background
    return out


def _check_against_reference(m, sim, cams, envs, cursor=None, spec=BOTH, cap=LEFT_OUT, tag=""):
    """every image of the listed envs: normals against the reference, the structure of the normal image, the shaded image against the
    formula.  -> (the device's outputs, {flat, curved: pixels compared}, the largest curved angle)"""
    sim.set_cameras(cams)
    sim.set_normals(spec)
    res = _render(sim, images=True)
    d0, s0 = sim.render()
    torch.cuda.synchronize()
    assert res["camera_depth"].tobytes() == d0.cpu().numpy().tobytes() and res["camera_segmentation"].tobytes() == s0.cpu().numpy().tobytes()
    seg, depth, normal, shaded = res["camera_segmentation"], res["camera_depth"], res["camera_normal"], res["camera_shaded"]
    w, h = cams[0].width, cams[0].height
    assert normal.shape == (sim.n_envs, len(cams), h, w, 3) and normal.dtype == np.float32
    assert shaded.shape == (sim.n_envs, len(cams), h, w, 4) and shaded.dtype == np.uint8
    # structure
    ln = np.linalg.norm(normal.astype(np.float64), axis=-1)
    assert (np.abs(ln[seg >= 0] - 1.0) <= 1e-5).all(), "|n| off 1 by %.3g" % np.abs(ln[seg >= 0] - 1.0).max()
    assert (normal[seg < 0] == 0).all()
    palette = spec.palette_for(m)
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    osim = OracleSim(m)
    count = dict(flat=0, curved=0)
    worst_angle, worst_flat, differ, channels = 0.0, 0.0, 0, 0
    for e in envs:
        osim.data.qpos[:] = qpos[e]
        if cursor is not None:
            for k, b in enumerate(m.arrays["cursor_bodyid"]):
                osim.model.body_pos[int(b)] = cursor[e, 3 * k:3 * k + 3]
        osim.forward()
        geoms = cref.model_geoms(m, osim.data.geom_xpos, osim.data.geom_xmat)
        for c, cam in enumerate(cams):
            b = cam.body_id(m)
            p, R = cam.world_pose(osim.data.xpos[b] if b >= 0 else None, osim.data.xquat[b] if b >= 0 else None)
            r = nref.render(p, R, cam.fovy, w, h, cam.znear, cam.zfar, geoms)
            sil = cref.silhouette(p, R, cam.fovy, w, h, cam.znear, cam.zfar, geoms)
            hit = r["seg"] >= 0
            compared = hit & (seg[e, c] == r["seg"]) & ~sil & (r["margin"] >= MARGIN) & (np.isinf(r["radius"]) | (r["radius"] >= MIN_RADIUS))
            left = int((hit & ~compared).sum())
            print("%s env %d cam %d: %d hit pixels, %d left out (%.1f %%)" % (tag, e, c, hit.sum(), left, 100.0 * left / max(int(hit.sum()), 1)))
            if cap is not None and hit.any():
                assert left <= cap * hit.sum(), "env %d cam %d: %d of %d hit pixels left out" % (e, c, left, hit.sum())
            flat, curved = compared & np.isinf(r["radius"]), compared & ~np.isinf(r["radius"])
            dn = normal[e, c].astype(np.float64) - r["normal"]
            if flat.any():
                worst_flat = max(worst_flat, float(np.abs(dn[flat]).max()))
            if curved.any():  # the angle between two unit vectors from their chord
                worst_angle = max(worst_angle, float((2.0 * np.arcsin(np.minimum(0.5 * np.linalg.norm(dn[curved], axis=-1), 1.0))).max()))
            count["flat"] += int(flat.sum())
            count["curved"] += int(curved.sum())
            # shaded, against the formula on the device's own normals
            want = _shade(normal[e, c], seg[e, c], depth[e, c], p, R, cam, spec, palette)
            got = shaded[e, c]
            bg = seg[e, c] < 0
            assert (got[bg] == np.asarray(spec.background, np.uint8)).all()
            assert (got[~bg][:, 3] == palette[seg[e, c][~bg]][:, 3]).all()
            diff = np.abs(got[..., :3].astype(np.int32) - want[..., :3].astype(np.int32))
            assert diff.max(initial=0) <= 1, "env %d cam %d: a shaded channel off by %d levels" % (e, c, diff.max())
            differ += int((diff > 0).sum())
            channels += diff.size
    osim.close()
    print("%s: %d flat pixels within %.3g, %d curved pixels within %.3g rad, %d of %d shaded channels differ" %
          (tag, count["flat"], worst_flat, count["curved"], worst_angle, differ, channels))
    assert worst_flat <= FLAT_TOL, "a flat normal off by %.3g" % worst_flat
    assert worst_angle <= CURVED_TOL, "a curved normal off by %.3g rad" % worst_angle
    assert differ <= 0.01 * channels, "%d of %d shaded channels differ" % (differ, channels)
    return res, count, worst_angle


def test_sawyer_lack_reset_then_steps_match_reference():
    m, sim = _make("Sawyer", "table_lack_0825", 4)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    _, count, _ = _check_against_reference(m, sim, cams, range(4), tag="lack reset")
    assert count["flat"] > 1000 and count["curved"] > 100  # boxes and the floor; the arm's cylinders / capsules
    _steps(sim, 30)
    _check_against_reference(m, sim, cams, range(4), tag="lack 30 steps")
    sim.close()


@pytest.mark.parametrize("agent,furniture,attach", [("Sawyer", "chair_agne_0010", "right_hand"), ("Baxter", "desk_mikael_1064", "left_hand"),
                                                    ("Cursor", "toy_table", "cursor0")])
def test_other_models_match_reference(agent, furniture, attach):
    m, sim = _make(agent, furniture, 2)
    cursor = sim.get_state("cursor")["cursor"].cpu().numpy().astype(np.float64) if agent == "Cursor" else None
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), attach)
    res, count, _ = _check_against_reference(m, sim, cams, range(2), cursor, tag=furniture)
    assert count["flat"] > 1000
    types = np.asarray(m.arrays["geom_type"])[np.unique(res["camera_segmentation"][res["camera_segmentation"] >= 0])]
    if furniture == "chair_agne_0010":
        assert nref.MESH in types  # the hull collider is in view
    if agent == "Baxter":
        assert count["curved"] > 100  # the arms' cylinders, spheres and the capsule
    sim.close()


@pytest.mark.parametrize("w,h", [(33, 17), (1, 1)])
def test_odd_sizes_alone_and_as_three_cameras(w, h):
    """561 pixels: two full rounds and one of 49 lanes; one pixel: one lane.  Against the reference, and an image does not depend on how
    many cameras the handle has."""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    q0 = sim.get_state("qpos")["qpos"][0].cpu().numpy()
    c = np.stack([q0[int(a):int(a) + 3] for a in m.part_qposadr]).mean(0)
    three = [Camera(c + np.array(o), lookat=c, fovy=50, width=w, height=h, znear=0.02, zfar=6.0) for o in ((1.1, -0.9, 0.9), (0.0, 0.3, 1.5), (-0.9, -1.0, 0.4))]
    three[1] = _cameras(m, q0, "right_hand", w, h)[1]
    # the pixels left out are nearly all silhouette, a count that grows with an image's side while the hit pixels grow with its area: at
    # 33 pixels across instead of 64 their share is 64 / 33 times larger, so the 15 % cap of the 64 x 48 images becomes 29 % here.  The
    # one pixel of a 1 x 1 image spans 50 degrees and may well be all silhouette: no cap
    cap = LEFT_OUT * W / w if w > 1 else None
    both, count, _ = _check_against_reference(m, sim, three, range(2), cap=cap, tag="%dx%d x3" % (w, h))
    compared = count["flat"] + count["curved"]
    for k, cam in enumerate(three):
        one, cnt, _ = _check_against_reference(m, sim, [cam], range(2), cap=cap, tag="%dx%d cam %d" % (w, h, k))
        for key in one:
            assert one[key][:, 0].tobytes() == both[key][:, k].tobytes(), (key, k)
        compared += cnt["flat"] + cnt["curved"]
    if w > 1:
        assert compared > 300
    sim.close()


def test_one_output_at_a_time():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 2)
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_normals(BOTH)
    both = _render(sim)
    assert sorted(both) == ["camera_normal", "camera_shaded"]
    sim.set_normals(Normals(normal=True, shaded=False))
    only = _render(sim)
    assert list(only) == ["camera_normal"] and only["camera_normal"].tobytes() == both["camera_normal"].tobytes()
    sim.set_normals(Normals(normal=False, shaded=True, ambient=BOTH.ambient, background=BOTH.background))
    only = _render(sim, images=True)
    assert sorted(only) == ["camera_depth", "camera_segmentation", "camera_shaded"] and only["camera_shaded"].tobytes() == both["camera_shaded"].tobytes()
    # the settings are the call's: another ambient and background change the picture, not the normals
    sim.set_normals(Normals(normal=True, shaded=True, ambient=1.0, background=(1, 2, 3, 4)))
    flat = _render(sim, images=True)
    assert flat["camera_normal"].tobytes() == both["camera_normal"].tobytes()
    pal, seg = default_palette(m), flat["camera_segmentation"]
    assert (flat["camera_shaded"][seg >= 0] == pal[seg[seg >= 0]]).all()  # ambient 1: the palette's colour itself
    assert (flat["camera_shaded"][seg < 0] == (1, 2, 3, 4)).all()
    sim.close()


def test_one_image_scratch_serves_points_voxels_and_normals():
    """With images=False the three calls render into the one image scratch the handle owns, and a larger camera set needs a larger one:
    each result is, byte for byte, that of the same call with images=True (the caller's images, no scratch) made right after it."""
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 2)
    q0 = sim.get_state("qpos")["qpos"][0].cpu().numpy()
    c = np.stack([q0[int(a):int(a) + 3] for a in m.part_qposadr]).mean(0)
    sim.set_points(PointCloud(0))
    sim.set_voxels(VoxelGrid((17, 9, 5), (c - 0.8, c + 0.8)))
    sim.set_normals(BOTH)
    calls = {"points": sim.render_points, "voxels": sim.render_voxels, "normals": sim.render_normals}
    compared = 0
    for (w, h), order in (((33, 17), ("points", "voxels", "normals")), ((64, 48), ("normals", "points", "voxels"))):
        sim.set_cameras(_cameras(m, q0, "right_hand", w, h))
        for name in order:
            _poison()
            got = {k: v.cpu().numpy() for k, v in calls[name](images=False).items()}
            want = {k: v.cpu().numpy() for k, v in calls[name](images=True).items()}
            assert sorted(want) == sorted(list(got) + ["camera_depth", "camera_segmentation"]), (w, h, name)
            for k in got:
                assert got[k].tobytes() == want[k].tobytes(), (w, h, name, k)
                compared += 1
    assert compared == 2 * (3 + 2 + 2)  # point_cloud, _segmentation, _count; voxel_count, _segmentation; camera_normal, _shaded
    sim.close()


def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_render_normals_is_read_only():
    m, sim = _make("Sawyer", "table_lack_0825", 4)
    sim.physics_forward()
    cams = _cameras(m, sim.get_state("qpos")["qpos"][0].cpu().numpy(), "right_hand")
    sim.set_cameras(cams)
    sim.set_normals(BOTH)
    before = _all_state(sim)
    _render(sim)
    _render(sim, images=True)
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    sim.close()
    # twenty steps with a render_normals after each == twenty steps without, bit for bit
    runs = []
    for with_render in (False, True):
        m, sim = _make("Sawyer", "table_lack_0825", 4)
        if with_render:
            sim.set_cameras(cams)
            sim.set_normals(BOTH)
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
    big.set_normals(BOTH)
    rb = _render(big, images=True)
    state = big.get_state("qpos")["qpos"]
    one = FSim(m, 1, config=big.cfg)
    one.set_cameras(cams)
    one.set_normals(BOTH)
    for i in (0, 1, 2047, 4095):
        one.set_state(qpos=state[i:i + 1])
        r1 = _render(one, images=True)
        for k in r1:
            assert r1[k][0].tobytes() == rb[k][i].tobytes(), (i, k)
    one.close()
    big.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv
    cams = [Camera((1.5, -1.0, 1.2), lookat=(0.5, 0.0, 0.3), width=W, height=H), Camera((0, 0, 0.05), body="right_hand", width=W, height=H)]
    cfg = lambda: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), cameras=cams, normals=BOTH)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-4:] == ["camera_depth", "camera_segmentation", "camera_normal", "camera_shaded"]
    assert tuple(ob["camera_normal"].shape) == (4, 2, H, W, 3) and ob["camera_normal"].dtype == torch.float32
    assert tuple(ob["camera_shaded"].shape) == (4, 2, H, W, 4) and ob["camera_shaded"].dtype == torch.uint8
    assert sp["camera_normal"].shape == (2, H, W, 3) and sp["camera_normal"].dtype == np.float32
    assert float(sp["camera_normal"].low.min()) == -1.0 and float(sp["camera_normal"].high.max()) == 1.0
    assert sp["camera_shaded"].shape == (2, H, W, 4) and sp["camera_shaded"].dtype == np.uint8
    rng = np.random.RandomState(0)
    for _ in range(3):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert bool(done.all())  # every env auto-reset in the last step: the images show the reset state the observation describes
    assert list(ob.keys()) == list(sp.keys())
    for e in range(4):
        assert sp["camera_shaded"].contains(ob["camera_shaded"][e].cpu().numpy()), e
    assert float(ob["camera_normal"].abs().max()) <= 1.0 + 1e-6  # (a unit vector in fp32: a component may pass 1 by a rounding error)
    kept = {k: ob[k].clone() for k in ("camera_depth", "camera_segmentation", "camera_normal", "camera_shaded")}
    fresh = env.sim.render_normals(images=True)
    torch.cuda.synchronize()
    for k in kept:
        assert torch.equal(fresh[k], kept[k]), k
    env.close()
    # with a point cloud as well: point_cloud_normal is camera_normal at the cloud's pixels
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(64), normals=Normals())
    ob = env.reset()
    assert list(ob.keys()) == list(env.observation_space.spaces.keys()) and "camera_shaded" not in ob
    assert list(ob.keys())[-2:] == ["camera_normal", "point_cloud_normal"] and tuple(ob["point_cloud_normal"].shape) == (2, 64, 3)
    pix = env._pts_out["point_cloud_pixel"].cpu().numpy()
    assert (pix >= 0).all()
    img = ob["camera_normal"].cpu().numpy().reshape(2, -1, 3)
    want = np.stack([img[e][pix[e]] for e in range(2)])
    assert ob["point_cloud_normal"].cpu().numpy().tobytes() == want.tobytes()
    assert (np.abs(np.linalg.norm(want, axis=-1) - 1.0) < 1e-5).all()  # every sampled point lies on a surface
    env.close()
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, point_cloud=PointCloud(0, include=("parts",)), normals=Normals())
    ob = env.reset()
    assert tuple(ob["point_cloud_normal"].shape) == (2, 2, H, W, 3) and env.observation_space.spaces["point_cloud_normal"].shape == (2, H, W, 3)
    lab, n_img, n_pts = ob["point_cloud_segmentation"].cpu().numpy(), ob["camera_normal"].cpu().numpy(), ob["point_cloud_normal"].cpu().numpy()
    assert (lab >= 0).any() and ((lab < 0) & (ob["camera_segmentation"].cpu().numpy() >= 0)).any()  # pixels the keep set drops
    assert (n_pts[lab < 0] == 0).all() and n_pts[lab >= 0].tobytes() == n_img[lab >= 0].tobytes()
    env.close()
    # shaded only with a point cloud: no point_cloud_normal
    env = FurnitureBatchEnv("Sawyer", 1, config=cfg(), cameras=cams, point_cloud=PointCloud(16), normals=Normals(normal=False, shaded=True))
    ob = env.reset()
    assert "camera_shaded" in ob and "camera_normal" not in ob and "point_cloud_normal" not in ob and list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    # without normals: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams)
    ob = env.reset()
    new = ("camera_normal", "camera_shaded", "point_cloud_normal")
    assert not any(k in ob or k in env.observation_space.spaces for k in new) and env.sim.normals is None
    assert list(ob.keys())[-2:] == ["camera_depth", "camera_segmentation"] and list(ob.keys()) == list(env.observation_space.spaces.keys())
    env.close()
    # the single env
    e1 = FurnitureSawyerEnv(config=cfg(), cameras=cams[:1])
    first = e1.reset()
    img = e1.render("normal_array")
    assert img.shape == (H, W, 3) and img.dtype == np.float32 and (np.abs(np.linalg.norm(img, axis=-1) - 1.0) < 1e-5).any()
    pic = e1.render("shaded_array")
    assert pic.shape == (H, W, 3) and pic.dtype == np.uint8 and len(np.unique(pic.reshape(-1, 3), axis=0)) > 3
    assert e1.render("depth_array").shape == (H, W)
    assert list(e1.reset().keys()) == list(first.keys())  # rendering a picture leaves the observations as they were
    with pytest.raises(NotImplementedError, match="visual meshes"):
        e1.render("rgb_array")
    with pytest.raises(NotImplementedError, match="visual meshes"):
        e1.render("human")
    e1.close()
    e2 = FurnitureSawyerEnv(config=cfg(), cameras=cams[:1], normals=BOTH)
    ob = e2.reset()
    assert ob["camera_normal"].shape == (1, H, W, 3) and ob["camera_shaded"].shape == (1, H, W, 4)
    assert (e2.render("shaded_array") == ob["camera_shaded"][0][:, :, :3].astype(np.uint8)).all()
    e2.close()
    e3 = FurnitureSawyerEnv(config=cfg())
    with pytest.raises(ValueError, match="needs cameras"):
        e3.render("normal_array")
    e3.close()


def test_c_abi_error_paths():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    dev = sim.device
    nrm = torch.zeros(16 * 16 * 3, dtype=torch.float32, device=dev)
    shd = torch.zeros(16 * 16 * 4 + 4, dtype=torch.uint8, device=dev)
    err = lambda: lib().fsim_last_error().decode()
    call = lambda n, s: lib().fsim_render_normals(sim._h, None, None, n, s)
    pal = np.ascontiguousarray(default_palette(m))
    bg = np.array([1, 2, 3, 4], np.uint8)
    setn = lambda p, b, a: lib().fsim_set_normals(sim._h, p.ctypes.data if p is not None else None, b.ctypes.data if b is not None else None, a)
    assert call(nrm.data_ptr(), None) == -1 and "no cameras set" in err()
    sim.set_cameras([Camera((1, 0, 1), lookat=(0, 0, 0), width=16, height=16)])
    assert call(nrm.data_ptr(), None) == -1 and "no normals settings" in err()
    for a in (-0.01, 1.01, float("nan"), float("inf")):
        assert setn(pal, bg, a) == -1 and "ambient" in err(), a
    assert call(nrm.data_ptr(), None) == -1 and "no normals settings" in err()  # a refused setting sets nothing
    assert setn(None, None, 0.0) == 0
    assert call(None, None) == -1 and "no output" in err()
    assert call(nrm.data_ptr(), shd.data_ptr()) == -1 and "without a palette" in err()
    assert call(nrm.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert setn(pal, None, 1.0) == 0
    assert call(None, shd.data_ptr() + 1) == -1 and "aligned" in err()
    assert call(None, shd.data_ptr()) == 0
    torch.cuda.synchronize()
    seg = sim.render()[1].cpu().numpy().reshape(-1)
    got = shd.cpu().numpy()[:16 * 16 * 4].reshape(-1, 4)
    assert (got[seg < 0] == 0).all() and (got[seg >= 0] == pal[seg[seg >= 0]]).all()  # NULL background: zeros; ambient 1: the palette
    assert (shd.cpu().numpy()[16 * 16 * 4:] == 0).all()  # nothing past the image
    with pytest.raises(FsimError, match="no normals settings"):
        sim.render_normals()  # (the settings above went through the C-ABI, not FSim.set_normals)
    sim.close()

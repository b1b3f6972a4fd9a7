"""Ray sensors on the device (include/fsim_rays.h): the camera pattern against the float64 camera and normal references and against
the device's own renders; free patterns (world lidar, hand lidar, a clipped range) against tests/rays_reference.py; ray counts that end
mid-wave; outputs one at a time; read-only casting; batch independence; the env surface; the C-ABI's error paths.  The references are
driven by the oracle's geom poses at the device's own qpos.  FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before
each cast.

Normals are compared where tests/test_normals_gpu.py compares them: on rays whose label the device and the reference agree on, off the
silhouette (camera pattern) or off the ambiguous and near-clip rays (free patterns), with an ambiguity margin of at least 5e-4 m, on a
flat face or a curved one of radius at least 5 mm.  Flat: every component within 1e-5.  Curved: the angle is at most CURVED_TOL."""
import ctypes

import numpy as np
import pytest
import torch

from furniture_amd.camera import hull_plane_table
from furniture_amd.envs import make_config
from furniture_amd.normals import Normals
from furniture_amd.rays import RaySensor, RaySet, camera_rays, lidar
from furniture_amd.sim import FSim, FsimError, FsimRaySensor, lib
from oracle.oracle_sim import OracleSim
from tests import camera_reference as cref
from tests import normals_reference as nref
from tests import rays_reference as rref
from tests.test_camera_gpu import _cameras, _make, _poison, _steps

pytestmark = pytest.mark.gpu
W, H = 64, 48
MARGIN, MIN_RADIUS, LEFT_OUT, FLAT_TOL = 5e-4, 5e-3, 0.15, 1e-5  # tests/test_normals_gpu.py's
# curved surfaces: 4 x the largest angle to the float64 reference measured on an MI355X over the cases of this file,
# and never above 1e-2 rad
CURVED_TOL = 1.1e-4  # measured: 2.79e-5 rad (a capsule of the Sawyer arm seen by the hand lidar at 0.1 - 0.6 m, table_lack_0825 and chair_agne_0010)
MODELS = [("Sawyer", "chair_agne_0010", "right_hand"), ("Baxter", "desk_mikael_1064", "left_hand"), ("Cursor", "toy_table", "cursor0")]


def _cast(sim, **kw):
    _poison()
    res = sim.cast_rays(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _device_state(m, sim):
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    cursor = sim.get_state("cursor")["cursor"].cpu().numpy().astype(np.float64) if m.meta.get("agent") == "Cursor" else None
    return qpos, cursor


def _pose_oracle(osim, m, qpos, cursor, e):
    """the oracle at env e's state -> the colliding geoms at their world poses"""
    osim.data.qpos[:] = qpos[e]
    if cursor is not None:
        for k, b in enumerate(m.arrays["cursor_bodyid"]):
            osim.model.body_pos[int(b)] = cursor[e, 3 * k:3 * k + 3]
    osim.forward()
    return cref.model_geoms(m, osim.data.geom_xpos, osim.data.geom_xmat)


def _frame(osim, m, mounted):
    """world pose of a Camera or RaySensor from the oracle's body poses"""
    b = mounted.body_id(m)
    return mounted.world_pose(osim.data.xpos[b] if b >= 0 else None, osim.data.xquat[b] if b >= 0 else None)


def _skip_ids(m, body):
    """the default exclusion, written out a second time: the model geom ids a sensor on `body` does not see"""
    if body is None:
        return []
    A = m.arrays
    b = m.meta["body_names"].index(body)
    red = np.asarray(A["body_red"])
    gbody = np.asarray(A["geom_bodyid"])
    return [int(g) for g in np.asarray(A["cg_orig"]) if (gbody[g] == b if red[b] == 0 else red[gbody[g]] == red[b])]


def _angles(got, want):
    """the angle between unit vectors from their chord"""
    return 2.0 * np.arcsin(np.minimum(0.5 * np.linalg.norm(got.astype(np.float64) - want, axis=-1), 1.0))


def _check_normals(normal, lab, ref, trusted, stats, cap=None, tag=""):
    """normals on the trusted rays the two agree on; stats: the running worst flat error and curved angle"""
    hit = ref["geom" if "geom" in ref else "seg"] >= 0
    seg = ref["geom" if "geom" in ref else "seg"]
    compared = hit & (lab == seg) & trusted & (ref["margin"] >= MARGIN) & (np.isinf(ref["radius"]) | (ref["radius"] >= MIN_RADIUS))
    if cap is not None and hit.any():
        assert (hit & ~compared).sum() <= cap * hit.sum(), "%s: %d of %d hit rays left out of the normal check" % (tag, (hit & ~compared).sum(), hit.sum())
    flat, curved = compared & np.isinf(ref["radius"]), compared & ~np.isinf(ref["radius"])
    if flat.any():
        stats["flat"] = max(stats["flat"], float(np.abs(normal[flat].astype(np.float64) - ref["normal"][flat]).max()))
    if curved.any():
        stats["curved"] = max(stats["curved"], float(_angles(normal[curved], ref["normal"][curved]).max()))
    stats["n_flat"] += int(flat.sum())
    stats["n_curved"] += int(curved.sum())
    ln = np.linalg.norm(normal.astype(np.float64), axis=-1)
    assert (np.abs(ln[lab >= 0] - 1.0) <= 1e-5).all() and (normal[lab < 0] == 0).all(), tag


def _finish(stats, tag):
    print("%s: %d flat rays within %.3g, %d curved rays within %.3g rad" % (tag, stats["n_flat"], stats["flat"], stats["n_curved"], stats["curved"]))
    assert stats["flat"] <= FLAT_TOL, "%s: a flat normal off by %.3g" % (tag, stats["flat"])
    assert stats["curved"] <= CURVED_TOL, "%s: a curved normal off by %.3g rad" % (tag, stats["curved"])


def _new_stats():
    return dict(flat=0.0, curved=0.0, n_flat=0, n_curved=0)


# ---- 1. the camera pattern ---------------------------------------------------------------------------------------------------------
def _check_camera_pattern(m, sim, attach, envs, tag):
    qpos, cursor = _device_state(m, sim)
    cams = _cameras(m, qpos[0].astype(np.float32), attach)
    sim.set_cameras(cams)
    sim.set_normals(Normals())
    dev = {k: v.cpu().numpy() for k, v in sim.render_normals(images=True).items()}
    got, dz = [], []
    for cam in cams:  # two 64 x 48 cameras are 6144 rays: one sensor per ray set
        sensor = camera_rays(cam, tmin=0.0, tmax=1e3, exclude=None)
        sim.set_rays(RaySet([sensor], normal=True))
        got.append(_cast(sim))
        dz.append(-sensor.directions[:, 2].reshape(H, W))
    osim = OracleSim(m)
    stats, seen, n_plain = _new_stats(), set(), [0] * len(cams)
    for e in envs:
        geoms = _pose_oracle(osim, m, qpos, cursor, e)
        for c, cam in enumerate(cams):
            p, R = _frame(osim, m, cam)
            # the references with the near plane at 0: a pixel ray is scaled to unit depth per unit t, so depth >= 0 is the sensor's tmin = 0
            r = nref.render(p, R, cam.fovy, W, H, 0.0, cam.zfar, geoms)
            sil = cref.silhouette(p, R, cam.fovy, W, H, 0.0, cam.zfar, geoms)
            dist, lab = got[c]["ray_distance"][e].reshape(H, W), got[c]["ray_geom"][e].reshape(H, W)
            nrm = got[c]["ray_normal"][e].reshape(H, W, 3)
            assert ((dist == -1.0) == (lab == -1)).all() and (dist[lab >= 0] >= 0).all()
            depth = np.where(lab >= 0, dist.astype(np.float64) * dz[c], np.inf)
            bound = lambda d: 1e-4 * d + 1e-5
            # against the float64 references
            clipped = r["seg"] < 0
            assert (depth[clipped & ~sil] >= cam.zfar - bound(cam.zfar)).all(), "%s env %d cam %d: a ray hits inside the range where the reference sees nothing" % (tag, e, c)
            bad = lab != r["seg"]
            bad &= ~(clipped & (depth >= cam.zfar - bound(cam.zfar)))  # (the ray's range has no far plane: beyond zfar it may hit)
            assert not (bad & ~sil).any(), "%s env %d cam %d: %d label mismatches off the silhouette" % (tag, e, c, int((bad & ~sil).sum()))
            assert bad.mean() <= 0.005, "%s env %d cam %d: %.3f %% silhouette mismatches" % (tag, e, c, 100 * bad.mean())
            ok = (lab == r["seg"]) & ~clipped
            err = np.abs(depth[ok] - r["depth"][ok])
            assert (err <= bound(r["depth"][ok])).all(), "%s env %d cam %d: depth error %.3g m" % (tag, e, c, err.max())
            _check_normals(nrm, lab, r, ~sil, stats, cap=LEFT_OUT, tag="%s env %d cam %d" % (tag, e, c))
            seen |= set(np.unique(lab).tolist())
            # against the device's own render of the same camera
            # (where the camera's own near plane plays no part: the wrist cameras sit within znear of the hand's geoms, which a ray with
            #  tmin = 0 sees and the camera looks through.  Measured, pixels that survive per wrist camera image of 3072: Sawyer 1610
            #  (both furniture), the cursor camera 2652, Baxter's left_hand camera 0 -- it sits inside a geom of the hand, so every one of
            #  its rays ends on that geom's exit face, which the reference with the near plane at 0 checks; the world cameras 2700 - 2840)
            rd, rs = cref.render(p, R, cam.fovy, W, H, cam.znear, cam.zfar, geoms)
            plain = (rs == r["seg"]) & (np.abs(rd - r["depth"]) <= 1e-9) & ~sil & ~cref.silhouette(p, R, cam.fovy, W, H, cam.znear, cam.zfar, geoms)
            dseg, ddepth = dev["camera_segmentation"][e, c], dev["camera_depth"][e, c]
            both = plain & (dseg >= 0)
            n_plain[c] += int(plain.sum())
            assert (lab[both] == dseg[both]).all(), "%s env %d cam %d: labels differ from fsim_render's" % (tag, e, c)
            assert (np.abs(depth[both] - ddepth[both]) <= bound(ddepth[both].astype(np.float64))).all()
            far = plain & (dseg < 0)
            assert (depth[far] >= cam.zfar - bound(cam.zfar)).all()
            same = both & (r["margin"] >= MARGIN) & np.isinf(r["radius"])  # a flat face: a column of the same rotation
            assert np.abs(nrm[same] - dev["camera_normal"][e, c][same]).max(initial=0.0) <= 1e-6
    osim.close()
    _finish(stats, tag)
    print("%s: pixels compared with fsim_render, per camera: %s of %d" % (tag, n_plain, len(envs) * W * H))
    assert n_plain[0] > 0.8 * len(envs) * W * H  # the world camera: all but its silhouettes
    return seen, stats


def test_camera_pattern_sawyer_lack_reset_then_steps():
    m, sim = _make("Sawyer", "table_lack_0825", 8)
    seen, stats = _check_camera_pattern(m, sim, "right_hand", range(8), "lack reset")
    assert len(seen - {-1}) >= 5 and stats["n_flat"] > 1000 and stats["n_curved"] > 100
    _steps(sim, 30)
    _check_camera_pattern(m, sim, "right_hand", range(8), "lack 30 steps")
    sim.close()


@pytest.mark.parametrize("agent,furniture,attach", MODELS)
def test_camera_pattern_other_models(agent, furniture, attach):
    m, sim = _make(agent, furniture, 2)
    seen, stats = _check_camera_pattern(m, sim, attach, range(2), furniture)
    assert stats["n_flat"] > 1000
    if furniture == "chair_agne_0010":  # the hull collider is in view
        assert int(m.arrays["cg_orig"][int(np.nonzero(np.asarray(m.arrays["cg_meshnum"]) > 0)[0][0])]) in seen
    sim.close()


# ---- 2. free patterns ------------------------------------------------------------------------------------------------------------
def _free_sensors(m, qpos0, attach):
    parts = np.stack([qpos0[int(a):int(a) + 3] for a in m.part_qposadr])
    ring = lidar(64, 16, elevation=(-75.0, 75.0))
    return [RaySensor(parts.mean(0) + np.array([0.0, 0.0, 0.8]), lidar(64, 16, elevation=(-60.0, 20.0)), tmax=6.0),
            RaySensor((0.0, 0.0, 0.0), ring, body=attach),
            RaySensor((0.0, 0.0, 0.0), ring, body=attach, tmin=0.1, tmax=0.6)]


def _bent(m, seed=3):
    """qpos0 with every arm joint moved by a seeded uniform(-0.25, 0.25) rad: a second state whose reference can be evaluated without a GPU"""
    q = np.asarray(m.arrays["qpos0"], dtype=np.float64).copy()
    adr = np.asarray(m.arm_qposadr, dtype=np.int64).reshape(-1)
    q[adr] += np.random.RandomState(seed).uniform(-0.25, 0.25, len(adr))
    return q


def _check_against_rays_reference(m, sim, sensors, skips, envs, tag, cap=0.005, cap_rays=None):
    """every sensor in the listed envs, cast as one ray set, against rays_reference -> (the device's outputs, per-sensor hit share).
    In every env the label mismatches plus the rays left out as ambiguous or near a range bound are at most the share `cap` of the
    env's rays, or at most `cap_rays` rays where that is given (sets too small for a share)."""
    sim.set_rays(RaySet(sensors, normal=True))
    got = _cast(sim)
    slices = sim.sensor_slices()
    qpos, cursor = _device_state(m, sim)
    osim = OracleSim(m)
    stats = _new_stats()
    hits = np.zeros(len(sensors))
    for e in envs:
        geoms = _pose_oracle(osim, m, qpos, cursor, e)
        left = wrong = 0  # mismatches + rays left out, and mismatches alone, over the env's whole ray set
        for i, s in enumerate(sensors):
            o, R = _frame(osim, m, s)
            d = s.directions @ R.T
            r = rref.cast(o, d, geoms, s.tmin, s.tmax, skips[i])
            amb = rref.ambiguous(o, d, geoms, s.tmin, s.tmax, skips[i])
            loose = amb | r["near_clip"]
            dist, lab, nrm = got["ray_distance"][e, slices[i]], got["ray_geom"][e, slices[i]], got["ray_normal"][e, slices[i]]
            miss = lab < 0
            assert (dist[miss] == -1.0).all() and (nrm[miss] == 0).all() and (dist[~miss] >= s.tmin).all() and (dist[~miss] <= s.tmax).all()
            assert not set(lab[~miss].tolist()) & set(skips[i]), "%s env %d sensor %d sees a geom it excludes" % (tag, e, i)
            bad = lab != r["geom"]
            assert not (bad & ~loose).any(), "%s env %d sensor %d: %d label mismatches on unambiguous rays" % (tag, e, i, int((bad & ~loose).sum()))
            print("%s env %d sensor %d: %d rays, %d hit, %d mismatches, %d left out (%d ambiguous, %d near a range bound)" %
                  (tag, e, i, len(lab), (~miss).sum(), bad.sum(), (loose & ~bad).sum(), amb.sum(), r["near_clip"].sum()))
            if amb.any():
                print("   ambiguous rays: geoms %s, distances %s" % (r["geom"][amb].tolist(), np.round(r["dist"][amb], 3).tolist()))
            left += int((bad | loose).sum())
            wrong += int(bad.sum())
            ok = ~bad & ~miss
            err = np.abs(dist[ok] - r["dist"][ok])
            assert (err <= 1e-4 * r["dist"][ok] + 1e-5).all(), "%s env %d sensor %d: distance error %.3g m" % (tag, e, i, err.max())
            _check_normals(nrm, lab, r, ~loose, stats, tag="%s env %d sensor %d" % (tag, e, i))
            hits[i] += (~miss).mean() / len(envs)
        print("%s env %d: %d mismatches, %d mismatches + rays left out, of %d rays (%.2f %%)" % (tag, e, wrong, left, got["ray_geom"].shape[1], 100.0 * left / got["ray_geom"].shape[1]))
        allowed = cap_rays if cap_rays is not None else cap * got["ray_geom"].shape[1]
        assert left <= allowed, "%s env %d: %d mismatches + rays left out of %d (at most %g)" % (tag, e, left, got["ray_geom"].shape[1], allowed)
    osim.close()
    _finish(stats, tag)
    return got, hits


@pytest.mark.parametrize("agent,furniture,attach", [("Sawyer", "table_lack_0825", "right_hand")] + MODELS)
def test_free_patterns_match_reference(agent, furniture, attach):
    """The two envs are put into states whose reference can be evaluated without a GPU, so that the share of rays the reference itself
    sets aside is known beforehand: env 0 at qpos0 and env 1 at qpos0 with every arm joint moved by up to 0.25 rad (_bent; the Cursor
    agent has no arm: its env 1 differs by the cursor position the reset drew).  From the float64 reference alone, ambiguous plus
    near-clip rays are 0.16 - 0.33 % of the 3072 rays in each of these states on the four models, so the issue's 0.5 % on mismatches
    plus rays left out is asserted in every env.  (In the reset states of _make, with the parts scattered, the reference alone set
    aside 0.75 % on chair_agne_0010 and 0.72 % on desk_mikael_1064, with no label mismatch: states the rule was not made for.)"""
    m, sim = _make(agent, furniture, 2)
    q = sim.get_state("qpos")["qpos"]
    q[0] = torch.as_tensor(np.asarray(m.arrays["qpos0"], dtype=np.float32), device=q.device)
    q[1] = torch.as_tensor(_bent(m).astype(np.float32), device=q.device)
    sim.set_state(qpos=q)
    qpos, _ = _device_state(m, sim)
    sensors = _free_sensors(m, qpos[0], attach)
    skips = [[], _skip_ids(m, attach), _skip_ids(m, attach)]
    got, hits = _check_against_rays_reference(m, sim, sensors, skips, range(2), furniture)
    print("%s: hit share per sensor %s" % (furniture, np.round(hits, 3).tolist()))
    assert hits[0] > 0.5 and hits[1] > 0.3  # the world lidar sees the floor; the mounted one is not blind behind its own body
    assert len(np.unique(got["ray_geom"][0, sim.sensor_slices()[1]])) >= 2
    sim.close()


def test_without_exclusion_the_hand_sensor_sees_the_gripper_base():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    ring = lidar(64, 16, elevation=(-75.0, 75.0))
    sensors = [RaySensor((0.0, 0.0, 0.0), ring, body="right_hand", exclude=None)]
    got, _ = _check_against_rays_reference(m, sim, sensors, [[]], range(2), "no exclusion")
    own = set(_skip_ids(m, "right_hand"))
    base = m.meta["body_names"].index("right_gripper_base")
    base_geoms = {g for g in own if int(m.arrays["geom_bodyid"][g]) == base}
    labels = got["ray_geom"][0]
    assert base_geoms and np.isin(labels, sorted(base_geoms)).mean() > 0.5  # the origin lies inside the gripper-base box: most rays end on it
    assert np.isin(labels, sorted(own)).mean() > 0.9
    sim.set_rays(RaySet([RaySensor((0.0, 0.0, 0.0), ring, body="right_hand")]))
    assert not set(_cast(sim)["ray_geom"][0].tolist()) & own
    sim.close()


# ---- 3. ray counts that end mid-wave ----------------------------------------------------------------------------------------------
def test_shapes_that_break_indexing():
    m, sim = _make("Sawyer", "table_lack_0825", 3)
    _steps(sim, 2)
    qpos, _ = _device_state(m, sim)
    c = np.stack([qpos[0][int(a):int(a) + 3] for a in m.part_qposadr]).mean(0)
    rng = np.random.RandomState(1)
    down = lambda k: rng.normal(size=(k, 3)) * (1.0, 1.0, 0.3) - (0.0, 0.0, 1.0)
    sets = {"3+70+1": [RaySensor(c + (0.0, 0.0, 0.7), down(3), tmax=5.0), RaySensor((0.0, 0.0, 0.0), down(70), body="right_hand", tmax=3.0),
                       RaySensor(c + (0.3, 0.2, 0.5), down(1), tmax=5.0)],
            "1": [RaySensor(c + (0.0, 0.0, 0.7), [(0.05, 0.0, -1.0)], tmax=5.0)],
            "65": [RaySensor(c + (0.1, -0.2, 0.9), down(65), tmax=5.0)]}
    for name, sensors in sets.items():
        skips = [_skip_ids(m, s.body) for s in sensors]
        got, _ = _check_against_rays_reference(m, sim, sensors, skips, range(3), name, cap_rays=2)  # (one ray of 74 is 1.4 %: a count, not a share)
        sl = sim.sensor_slices()
        for i, s in enumerate(sensors):  # the same rays as the one sensor of a handle
            sim.set_rays(RaySet([s], normal=True))
            alone = _cast(sim)
            for k in alone:
                assert alone[k].tobytes() == np.ascontiguousarray(got[k][:, sl[i]]).tobytes(), (name, i, k)
    sim.close()


# ---- 4. outputs one at a time and out= buffers ---------------------------------------------------------------------------------------
def test_one_output_at_a_time():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    _steps(sim, 2)
    qpos, _ = _device_state(m, sim)
    sensors = _free_sensors(m, qpos[0], "right_hand")[:2] + [RaySensor((0.0, 0.0, 0.0), lidar(5), body="right_hand", tmax=2.0)]
    sim.set_rays(RaySet(sensors, normal=True))
    shapes = sim.ray_shapes()
    assert list(shapes) == ["ray_distance", "ray_geom", "ray_normal"] and shapes["ray_normal"][0] == (2053, 3)
    everything = _cast(sim)
    assert sorted(everything) == sorted(shapes) and (everything["ray_geom"] >= 0).any() and (everything["ray_geom"] < 0).any()
    for k, (sh, dt) in shapes.items():
        buf = {k: torch.full((2,) + sh, 77, dtype=dt, device=sim.device)}
        only = _cast(sim, out=buf)
        assert list(only) == [k] and only[k].tobytes() == everything[k].tobytes(), k
        assert buf[k].cpu().numpy().tobytes() == everything[k].tobytes()  # written in place
    with pytest.raises(ValueError, match="out holds"):
        sim.cast_rays(out={"ray_depth": None})
    sim.set_rays(RaySet(sensors))  # without the normal
    two = _cast(sim)
    assert sorted(two) == ["ray_distance", "ray_geom"] and all(two[k].tobytes() == everything[k].tobytes() for k in two)
    sim.close()


# ---- 5. read-only -----------------------------------------------------------------------------------------------------------------
def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_cast_is_read_only_and_independent_of_cameras():
    m, sim = _make("Sawyer", "table_lack_0825", 4)
    m2, twin = _make("Sawyer", "table_lack_0825", 4)
    _steps(sim, 3)
    _steps(twin, 3)
    qpos, _ = _device_state(m, sim)
    rays = RaySet(_free_sensors(m, qpos[0], "right_hand"), normal=True)
    cams = _cameras(m, qpos[0].astype(np.float32), "right_hand")
    twin.set_cameras(cams)
    plain = [t.cpu().numpy() for t in twin.render()]  # fsim_render without rays set
    sim.set_rays(rays)  # no cameras set
    before = _all_state(sim)
    first = _cast(sim)
    _cast(sim, out={"ray_geom": torch.empty((4, rays.n_rays), dtype=torch.int32, device=sim.device)})
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert (first["ray_geom"] >= 0).mean() > 0.3
    sim.set_cameras(cams)  # cameras set afterwards: the rays are what they were, the images what they are without rays
    with_rays = [t.cpu().numpy() for t in sim.render()]
    again = _cast(sim)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    for a, b in zip(plain, with_rays):
        assert a.tobytes() == b.tobytes()
    # a step after a cast == the same step without one, bit for bit
    _steps(sim, 2, seed=8)
    _steps(twin, 2, seed=8)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 6. batch independence -----------------------------------------------------------------------------------------------------------
def test_batch_independence():
    m, big = _make("Sawyer", "table_lack_0825", 8)
    _steps(big, 3)
    qpos, _ = _device_state(m, big)
    rays = RaySet(_free_sensors(m, qpos[0], "right_hand") + [RaySensor((0.0, 0.0, 0.0), lidar(4), body="right_hand", tmax=0.3)], normal=True)
    big.set_rays(rays)
    rb = _cast(big)
    state = big.get_state("qpos")["qpos"]
    one = FSim(m, 1, config=big.cfg)
    one.set_rays(rays)
    for i in range(8):
        one.set_state(qpos=state[i:i + 1])
        r1 = _cast(one)
        for k in r1:
            assert r1[k][0].tobytes() == rb[k][i].tobytes(), (i, k)
    assert len({rb["ray_distance"][i].tobytes() for i in range(8)}) == 8  # the envs differ
    one.close()
    big.close()


# ---- 7. the env surface ------------------------------------------------------------------------------------------------------------
def test_env_surface():
    from furniture_amd.envs import FurnitureBatchEnv, FurnitureSawyerEnv
    from furniture_amd.envs import furniture_names
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    rays = RaySet([RaySensor((0.5, 0.0, 1.2), lidar(16, 2, elevation=(-60.0, -20.0)), tmax=4.0), RaySensor((0.0, 0.0, 0.0), lidar(5), body="right_hand", tmax=1.0)], normal=True)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), rays=rays)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-3:] == ["ray_distance", "ray_geom", "ray_normal"] and "camera_depth" not in ob
    assert tuple(ob["ray_distance"].shape) == (4, 37) and ob["ray_distance"].dtype == torch.float32 and sp["ray_distance"].shape == (37,)
    assert tuple(ob["ray_geom"].shape) == (4, 37) and ob["ray_geom"].dtype == torch.int32 and sp["ray_geom"].dtype == np.int32
    assert tuple(ob["ray_normal"].shape) == (4, 37, 3) and ob["ray_normal"].dtype == torch.float32 and sp["ray_normal"].shape == (37, 3)
    assert float(sp["ray_distance"].low.min()) == -1.0 and np.isinf(sp["ray_distance"].high).all() and sp["ray_distance"].dtype == np.float32
    assert int(sp["ray_geom"].low.min()) == -1 and int(sp["ray_geom"].high.max()) == env.model.ngeom - 1
    fresh = env.sim.cast_rays()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], ob[k]), k
    assert (ob["ray_geom"] >= 0).any()
    rng = np.random.RandomState(0)
    for _ in range(3):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert bool(done.all()) and list(ob.keys()) == list(sp.keys())
    kept = {k: ob[k].clone() for k in fresh}
    fresh = env.sim.cast_rays()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], kept[k]), k
    for e in range(4):
        assert sp["ray_distance"].contains(ob["ray_distance"][e].cpu().numpy()) and sp["ray_geom"].contains(ob["ray_geom"][e].cpu().numpy())
    env.close()
    # without the normal, and beside cameras
    cams = _cameras(env.model, np.asarray(env.model.arrays["qpos0"], dtype=np.float32), "right_hand", 16, 12)
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), cameras=cams, rays=RaySet(rays.sensors))
    ob = env.reset()
    assert list(ob.keys()) == list(env.observation_space.spaces.keys()) and list(ob.keys())[-4:] == ["camera_depth", "camera_segmentation", "ray_distance", "ray_geom"]
    env.close()
    # without rays: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg())
    assert not any(k.startswith("ray_") for k in list(env.reset()) + list(env.observation_space.spaces)) and env.sim.rays is None
    env.close()
    # the single env keeps its rays through reset(furniture_id)
    e1 = FurnitureSawyerEnv(config=cfg(), rays=rays)
    first = e1.reset()
    assert first["ray_distance"].shape == (37,) and first["ray_normal"].shape == (37, 3)
    other = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert e1._b.furniture_name == "chair_agne_0010" and e1._b.rays is rays and list(other.keys()) == list(first.keys())
    assert other["ray_distance"].shape == (37,) and (other["ray_geom"] >= 0).any()
    e1.close()


# ---- 8. the C-ABI's error paths ------------------------------------------------------------------------------------------------------
def test_c_abi_error_paths():
    m, sim = _make("Sawyer", "table_lack_0825", 1)
    ncg = len(m.arrays["cg_orig"])
    err = lambda: lib().fsim_last_error().decode()
    out = torch.zeros(8, dtype=torch.float32, device=sim.device)
    for call_ in (sim.cast_rays, sim.ray_shapes, sim.sensor_slices):
        with pytest.raises(FsimError, match="no rays set"):
            call_()
    assert lib().fsim_cast_rays(sim._h, out.data_ptr(), None, None) == -1 and "no rays set" in err()

    def call(n_rays=4, dirs=None, counts=(3, 1), n_sensors=None, n_planes=0, **over):
        tab = (FsimRaySensor * max(len(counts), 1))()
        at = 0
        for i, k in enumerate(counts):
            tab[i].body, tab[i].tmin, tab[i].tmax, tab[i].first_ray, tab[i].n_rays = -1, 0.0, 5.0, at, k
            tab[i].pos[:], tab[i].quat[:] = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0)
            at += k
        for k, v in over.items():
            if k in ("pos", "quat", "exclude"):
                getattr(tab[0], k)[:] = v
            else:
                setattr(tab[0], k, v)
        d = np.ascontiguousarray(np.tile([0.0, 0.0, -1.0], (max(n_rays, 1), 1)) if dirs is None else dirs, dtype=np.float32)
        return lib().fsim_set_rays(sim._h, len(counts) if n_sensors is None else n_sensors, ctypes.addressof(tab), n_rays, d.ctypes.data, n_planes, None, None, None)
    bad_dir = np.tile([0.0, 0.0, -1.0], (4, 1))
    words = lambda bits: tuple((bits >> (32 * j)) & 0xffffffff for j in range(3))
    beyond, every = words(1 << ncg), words((1 << ncg) - 1)
    cases = [(dict(n_sensors=17, counts=(1,) * 17, n_rays=17), "17 sensors"), (dict(n_sensors=-1), "-1 sensors"),
             (dict(n_rays=0), "0 rays"), (dict(n_rays=4097, counts=(4097,)), "4097 rays"), (dict(counts=(4, 0)), "0 rays (at least 1)"),
             (dict(counts=(3, 2)), "not contiguous"), (dict(counts=(2, 1)), "cover 3 of the 4"), (dict(first_ray=1), "not contiguous"),
             (dict(body=10000), "unknown body"), (dict(body=-2), "unknown body"), (dict(tmin=-0.5), "tmin"), (dict(tmin=5.0), "tmin"),
             (dict(tmax=float("inf")), "tmin"), (dict(tmax=float("nan")), "tmin"), (dict(quat=(0.0, 0.0, 0.0, 0.0)), "bad pose"),
             (dict(pos=(0.0, float("nan"), 0.0)), "bad pose"), (dict(exclude=beyond), "exclude bit %d" % ncg),
             (dict(dirs=bad_dir * [[1], [1], [0], [1]]), "direction 2 is zero"), (dict(dirs=bad_dir * [[1], [float("inf")], [1], [1]]), "direction 1 is zero or not finite"),
             (dict(n_planes=1025), "1025 hull planes")]
    assert ncg < 96
    for over, msg in cases:
        assert call(**over) == -1, over
        assert msg in err(), (over, err())
    with pytest.raises(FsimError, match="no rays set"):  # a refused set sets nothing
        sim._chk(lib().fsim_cast_rays(sim._h, out.data_ptr(), None, None))
    assert call(exclude=every) == 0  # every geom excluded on sensor 0, whose three rays miss; sensor 1 sees the scene
    assert lib().fsim_cast_rays(sim._h, None, None, None) == -1 and "no output" in err()
    assert lib().fsim_cast_rays(sim._h, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert res[:3].tolist() == [-1.0] * 3 and res[3] > 0 and res[4:].tolist() == [0.0] * 4  # nothing past the four rays
    assert call() == 0 and lib().fsim_cast_rays(sim._h, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:4] > 0).all()  # straight down from 1 m: the table or the floor
    # n_sensors == 0 clears; a cast after that fails cleanly; clearing twice is fine
    assert lib().fsim_set_rays(sim._h, 0, None, 0, None, 0, None, None, None) == 0
    assert lib().fsim_cast_rays(sim._h, out.data_ptr(), None, None) == -1 and "no rays set" in err()
    assert lib().fsim_set_rays(sim._h, 0, None, 0, None, 0, None, None, None) == 0
    sim.set_rays(RaySet([RaySensor((0, 0, 1), [(0, 0, -1)])]))
    sim.set_rays(None)
    with pytest.raises(FsimError, match="no rays set"):
        sim.cast_rays()
    sim.close()
    # a mesh collider needs its planes, and more than the cap of planes is refused before they are read
    mc, simc = _make("Sawyer", "chair_agne_0010", 1)
    tab = (FsimRaySensor * 1)()
    tab[0].body, tab[0].tmax, tab[0].n_rays = -1, 5.0, 1
    tab[0].quat[:] = (1.0, 0.0, 0.0, 0.0)
    d = np.array([[0.0, 0.0, -1.0]], dtype=np.float32)
    assert lib().fsim_set_rays(simc._h, 1, ctypes.addressof(tab), 1, d.ctypes.data, 0, None, None, None) == -1 and "hull planes" in err()
    planes, adr, num = hull_plane_table(mc)
    assert lib().fsim_set_rays(simc._h, 1, ctypes.addressof(tab), 1, d.ctypes.data, len(planes), planes.ctypes.data, adr.ctypes.data, num.ctypes.data) == 0
    simc.close()

"""Ray sensors, the parts that run without a GPU: RaySensor / RaySet validation, lidar() and camera_rays() geometry, the "body"
exclusion rule, the float64 reference (tests/rays_reference.py) on hand-made scenes, the refusals and the C-ABI of include/fsim_rays.h
(tests/test_rays_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import Camera, quat_to_mat
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.rays import MAX_RAYS, MAX_SENSORS, RaySensor, RaySet, camera_rays, check, exclude_mask, lidar, sensor_table
from tests import camera_reference as cref
from tests import rays_reference as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = [(1.0, 0.0, 0.0)]


# ---- RaySensor / RaySet -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(tmin=-0.1), dict(tmin=1.0, tmax=1.0), dict(tmin=2.0, tmax=1.0), dict(tmax=float("inf")), dict(tmax=float("nan")),
                                dict(directions=[(0.0, 0.0, 0.0)]), dict(directions=[(1.0, 0.0, 0.0), (0.0, float("nan"), 0.0)]), dict(directions=[]),
                                dict(directions=[1.0, 0.0, 0.0]), dict(quat=(0, 0, 0, 0)), dict(pos=(0, float("inf"), 0)), dict(exclude="hand"),
                                dict(exclude=[1.5])])
def test_sensor_validation(kw):
    args = dict(pos=(0, 0, 0), directions=X)
    args.update(kw)
    with pytest.raises(ValueError):
        RaySensor(**args)


def test_sensor_accepts_and_normalises():
    s = RaySensor((0, 0, 1), [(0, 0, -2.0), (3.0, 4.0, 0.0)], quat=(2, 0, 0, 0), tmin=0.0, tmax=0.5, exclude=[3, 4])
    assert s.n_rays == 2 and np.allclose(s.directions, [(0, 0, -1), (0.6, 0.8, 0)]) and np.allclose(s.quat, (1, 0, 0, 0))
    assert s.exclude == [3, 4] and s.body is None and "2 rays" in repr(s)
    assert RaySensor((0, 0, 0), X).exclude == "body" and RaySensor((0, 0, 0), X, exclude=None).exclude is None


def test_ray_set_validation():
    one = RaySensor((0, 0, 0), X)
    with pytest.raises(ValueError, match="0 sensors"):
        RaySet([])
    with pytest.raises(ValueError, match="17 sensors"):
        RaySet([one] * (MAX_SENSORS + 1))
    with pytest.raises(ValueError, match="4097 rays"):
        RaySet([RaySensor((0, 0, 0), lidar(MAX_RAYS // 2)), RaySensor((0, 0, 0), lidar(MAX_RAYS // 2 + 1))])
    with pytest.raises(TypeError, match="RaySensor"):
        RaySet([one, "lidar"])
    with pytest.raises(ValueError, match="boolean"):
        RaySet([one], normal=1)
    with pytest.raises(TypeError, match="RaySet"):
        check([one])
    rs = RaySet([RaySensor((0, 0, 0), lidar(3)), one, RaySensor((0, 0, 0), lidar(70))], normal=True)
    assert rs.n_rays == 74 and rs.normal and rs.sensor_slices() == {0: slice(0, 3), 1: slice(3, 4), 2: slice(4, 74)}
    assert RaySet(one).n_rays == 1  # a single sensor is a set of one
    RaySet([one] * MAX_SENSORS)
    RaySet([RaySensor((0, 0, 0), lidar(MAX_RAYS))])
    m = load_compiled("Sawyer", "table_lack_0825")
    with pytest.raises(ValueError, match="unknown body"):
        sensor_table(m, RaySet([RaySensor((0, 0, 0), X, body="no_such_body")]))
    with pytest.raises(ValueError, match="names geom"):
        sensor_table(m, RaySet([RaySensor((0, 0, 0), X, exclude=[10000])]))


# ---- lidar() and camera_rays() ----------------------------------------------------------------------------------------------------
def test_lidar_geometry():
    d = lidar(8, 3, elevation=(-30.0, 60.0))
    assert d.shape == (24, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0)
    el = np.degrees(np.arcsin(d[:, 2])).reshape(3, 8)
    assert np.allclose(el, np.array([-30.0, 15.0, 60.0])[:, None])  # elevation is outer
    az = np.degrees(np.arctan2(d[:, 1], d[:, 0])).reshape(3, 8) % 360.0
    assert np.allclose(az, ((np.arange(8) + 0.5) * 45.0)[None, :])  # azimuth at cell centres
    flat = lidar(4)
    assert flat.shape == (4, 3) and np.allclose(flat[:, 2], 0.0) and np.allclose(flat[0], (np.sqrt(0.5), np.sqrt(0.5), 0.0))
    assert np.allclose(np.degrees(np.arcsin(lidar(2, 1, (10.0, 30.0))[:, 2])), 20.0)  # one ring: the mean
    for bad in (dict(n_azimuth=0), dict(n_azimuth=4, n_elevation=0), dict(n_azimuth=4, elevation=(10, -10)), dict(n_azimuth=4, elevation=(-91, 0)),
                dict(n_azimuth=2.5)):
        with pytest.raises(ValueError):
            lidar(**bad)


def test_camera_rays_are_the_pixel_rays():
    cam = Camera((0.3, -0.2, 1.1), lookat=(0.0, 0.1, 0.2), fovy=63.0, width=7, height=5, znear=0.05, zfar=4.0, body="right_hand")
    s = camera_rays(cam)
    assert s.n_rays == 35 and s.body == "right_hand" and s.tmin == 0.0 and s.tmax == 4.0 and s.exclude == "body"
    assert np.array_equal(s.pos, cam.pos) and np.array_equal(s.quat, cam.quat)
    want = cref.pixel_rays(np.eye(3), cam.fovy, 7, 5).reshape(-1, 3)  # camera frame; row-major: ray j * W + i is pixel (i, j)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(s.directions - want).max() < 1e-15
    # in the world, through the sensor's pose: the reference's world rays of the same camera
    p, R = s.world_pose((0.1, 0.2, 0.3), (0.5, 0.5, -0.5, 0.5))
    pc, Rc = cam.world_pose((0.1, 0.2, 0.3), (0.5, 0.5, -0.5, 0.5))
    world = cref.pixel_rays(Rc, cam.fovy, 7, 5).reshape(-1, 3)
    assert np.allclose(p, pc) and np.abs(s.directions @ R.T - world / np.linalg.norm(world, axis=1, keepdims=True)).max() < 1e-14
    s2 = camera_rays(cam, tmin=0.1, tmax=1e3, exclude=None)
    assert (s2.tmin, s2.tmax, s2.exclude) == (0.1, 1e3, None)


# ---- the "body" exclusion rule ---------------------------------------------------------------------------------------------------------
def _bodies_of(m, mask):
    cg = np.asarray(m.arrays["cg_orig"])
    return [m.meta["body_names"][int(m.arrays["geom_bodyid"][int(g)])] for g in cg[mask]]


def test_body_exclusion_rule():
    m = load_compiled("Sawyer", "table_lack_0825")
    hand = RaySensor((0, 0, 0), X, body="right_hand")
    mask = exclude_mask(m, hand)
    cg = np.asarray(m.arrays["cg_orig"])
    gbody = np.asarray(m.arrays["geom_bodyid"])[cg]
    names = m.meta["body_names"]
    want = np.isin(gbody, [names.index("right_l6"), names.index("right_gripper_base")])
    assert want.sum() >= 2 and np.array_equal(mask, want)  # exactly the colliding geoms of those two bodies
    assert set(_bodies_of(m, mask)) == {"right_l6", "right_gripper_base"}
    # an exact-body rule would leave the sensor blind: right_hand itself has no colliding geom
    assert not (gbody == names.index("right_hand")).any()
    assert not exclude_mask(m, RaySensor((0, 0, 1), X)).any()  # a world sensor
    assert not exclude_mask(m, RaySensor((0, 0, 0), X, body="right_hand", exclude=None)).any()
    some = [int(cg[3]), int(cg[5])]
    assert np.nonzero(exclude_mask(m, RaySensor((0, 0, 0), X, exclude=some)))[0].tolist() == [3, 5]
    tab, dirs = sensor_table(m, RaySet([hand, RaySensor((0, 0, 1), lidar(5))]))
    bits = sum(int(tab[0].exclude[j]) << (32 * j) for j in range(3))
    assert [k for k in range(96) if bits >> k & 1] == np.nonzero(mask)[0].tolist()
    assert list(tab[1].exclude) == [0, 0, 0] and (tab[1].first_ray, tab[1].n_rays, tab[1].body) == (1, 5, -1) and dirs.shape == (6, 3)
    # a cursor is welded to the world: only its own geom, not the floor
    mc = load_compiled("Cursor", "toy_table")
    cur = RaySensor((0, 0, 0), X, body="cursor0")
    assert int(mc.arrays["body_red"][cur.body_id(mc)]) == 0
    assert _bodies_of(mc, exclude_mask(mc, cur)) == ["cursor0"]


# ---- the reference on hand-made scenes ---------------------------------------------------------------------------------------------
def _geom(gid, gtype, size, pos, mat=None, **kw):
    return dict(id=gid, type=gtype, size=np.asarray(size, dtype=np.float64), pos=np.asarray(pos, dtype=np.float64), mat=np.eye(3) if mat is None else mat, **kw)


def test_reference_sanity():
    o = np.zeros(3)
    sphere = _geom(4, cref.SPHERE, (0.5, 0, 0), (3.0, 0, 0))
    r = rref.cast(o, [(1, 0, 0), (-1, 0, 0), (0, 1, 0)], [sphere], 0.0, 10.0)
    assert np.allclose(r["dist"], [2.5, -1.0, -1.0]) and r["geom"].tolist() == [4, -1, -1]  # ahead; a backward ray misses
    assert np.allclose(r["normal"], [(-1, 0, 0), (0, 0, 0), (0, 0, 0)]) and r["radius"][0] == 0.5
    box = _geom(7, cref.BOX, (1.0, 2.0, 3.0), (0.2, 0, 0))
    r = rref.cast(o, [(1, 0, 0), (0, -1, 0), (0, 0, 1)], [box], 0.0, 10.0)  # origin inside a box: the exit face
    assert np.allclose(r["dist"], [1.2, 2.0, 3.0]) and np.allclose(r["normal"], [(1, 0, 0), (0, -1, 0), (0, 0, 1)])
    r = rref.cast(o, [(1, 0, 0)], [sphere], 2.6, 10.0)  # tmin beyond the entry: the exit
    assert np.allclose(r["dist"], [3.5]) and np.allclose(r["normal"], [(1, 0, 0)])
    assert rref.cast(o, [(1, 0, 0)], [sphere], 3.6, 10.0)["geom"].tolist() == [-1]  # tmin beyond the exit
    r = rref.cast(o, [(1, 0, 0)], [sphere], 0.0, 2.4)  # a hit beyond tmax is a miss
    assert r["dist"].tolist() == [-1.0] and r["geom"].tolist() == [-1] and not r["near_clip"].any()
    assert rref.cast(o, [(1, 0, 0)], [sphere], 0.0, 2.50005)["near_clip"].all() and rref.cast(o, [(1, 0, 0)], [sphere], 2.49995, 9.0)["near_clip"].all()
    assert rref.cast(o, [(1, 0, 0)], [sphere, box], 0.0, 10.0, skip=[7])["geom"].tolist() == [4]  # the box is invisible
    assert rref.cast(o, [(1, 0, 0)], [sphere, box], 0.0, 10.0)["geom"].tolist() == [7]
    floor = _geom(0, cref.PLANE, (0, 0, 0), (0, 0, -1.0))
    r = rref.cast(o, [(0, 0, -1), (0, 0, 1), (0.6, 0, -0.8)], [floor], 0.0, 10.0)
    assert np.allclose(r["dist"], [1.0, -1.0, 1.25]) and np.allclose(r["normal"][0], (0, 0, 1))
    # a cube as a hull equals the box, at any pose
    rng = np.random.RandomState(2)
    q = rng.normal(size=4)
    R = quat_to_mat(q / np.linalg.norm(q))
    half = np.array([0.3, 0.2, 0.4])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    pos = np.array([0.5, 0.1, -0.2])
    d = rng.normal(size=(400, 3))
    rb = rref.cast(o, d, [_geom(1, cref.BOX, half, pos, R)], 0.0, 5.0)
    rh = rref.cast(o, d, [_geom(1, cref.MESH, (0, 0, 0), pos, R, halfspaces=cref.mesh_halfspaces(corners))], 0.0, 5.0)
    assert 50 < (rb["geom"] >= 0).sum() < 400 and np.array_equal(rb["geom"], rh["geom"])
    assert np.abs(rb["dist"] - rh["dist"]).max() < 1e-12
    sure = (rb["geom"] >= 0) & (rb["margin"] > 1e-9)
    assert np.abs(rb["normal"][sure] - rh["normal"][sure]).max() < 1e-12
    # ambiguous: a ray that grazes the sphere's silhouette, not one through its middle
    th = np.arcsin((0.5 - 1e-3) / 3.0)  # passes 1 mm inside the silhouette; a tilt of 1e-3 rad moves it by 3 mm there
    graze = np.array([np.cos(th), np.sin(th), 0.0])
    amb = rref.ambiguous(o, [(1, 0, 0), graze], [sphere], 0.0, 10.0)
    assert amb.tolist() == [False, True]


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = RaySet([RaySensor((0, 0, 1), lidar(8))])
    with pytest.raises(TypeError, match="RaySet"):
        FurnitureBatchEnv("Sawyer", 1, rays=[RaySensor((0, 0, 1), X)])
    with pytest.raises(NotImplementedError, match="rays= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, rays=spec)
    with pytest.raises(NotImplementedError, match="rays= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(rays=spec))

    class _Handle:  # a handle with a ray set and nothing else
        cameras, points, voxels, normals, flow, rays = None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="ray-sensor outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_rays_header_symbols_are_exported():
    assert sim.RAY_SYMBOLS == ["fsim_set_rays", "fsim_cast_rays"]
    assert sorted(_declared("fsim_rays.h")) == sorted(sim.RAY_SYMBOLS)
    others = set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS) | set(sim.VOXELS_SYMBOLS) | set(sim.NORMALS_SYMBOLS) | set(sim.FLOW_SYMBOLS)
    assert not set(sim.RAY_SYMBOLS) & others
    assert not set(sim.RAY_SYMBOLS) & set().union(*[_declared(h) for h in ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h")])
    lib = ctypes.CDLL(sim.build())
    for n in sim.RAY_SYMBOLS:
        assert hasattr(lib, n), n


def test_rays_header_is_plain_c11_and_the_struct_matches(tmp_path):
    fields = [n for n, _ in sim.FsimRaySensor._fields_]
    src = tmp_path / "use_rays.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsim_rays.h"\n'
                   "int use(fsim_t *s, const fsim_ray_sensor_t *k, const float *d, float *o) { return fsim_set_rays(s, 1, k, 1, d, 0, 0, 0, 0) + fsim_cast_rays(s, o, 0, 0); }\n"
                   'int main(void) { printf("%zu %d %d", sizeof(fsim_ray_sensor_t), FSIM_RAY_MAX_SENSORS, FSIM_RAY_MAX_RAYS);\n' +
                   "".join('  printf(" %%zu", offsetof(fsim_ray_sensor_t, %s));\n' % f for f in fields) + "  return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_rays.o")])
    # the layout: a program that defines the two entry points itself prints sizeof and every offsetof
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_rays.h"\nint fsim_set_rays(fsim_t *s, int a, const fsim_ray_sensor_t *k, int b, const float *d, int c, const float *p, const int32_t *x, '
                    "const int32_t *y) { (void)s; (void)k; (void)d; (void)p; (void)x; (void)y; return a + b + c; }\n"
                    "int fsim_cast_rays(fsim_t *s, float *a, int32_t *b, float *c) { (void)s; (void)a; (void)b; (void)c; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [ctypes.sizeof(sim.FsimRaySensor), MAX_SENSORS, MAX_RAYS] and got[0] == 60
    assert got[3:] == [getattr(sim.FsimRaySensor, f).offset for f in fields]


def test_rays_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_rays.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("normalises each direction in double", "a zero or non-finite direction is FSIM_EINVAL", "A ray is o + t d in world metres",
              "cursor offset is added for a sensor on a cursor body", "t = t0 >= tmin ? t0 : t1", "accepted when tmin <= t <= tmax",
              "the smallest t wins; a strict < in colliding-geom order settles ties", "-1 when nothing is hit", "The hit point in the sensor frame is dist * dir",
              "in the numbering of the segmentation image", "R_geom * the geom's local outward normal, not flipped towards the sensor",
              "a miss gives (0, 0, 0)", "writes no state, RNG draw, look-ahead shadow or counter", "depends only on its own record and the ray set",
              "Without rays set, nothing is allocated or launched", "n_sensors == 0 clears", "keeps its own copy",
              "waits for the handle's stream before it replaces the tables", "any may be NULL, not all", "settled exactly as fsim_render settles it",
              "returns without waiting"):
        assert s in flat, s

"""Depth / segmentation cameras, the parts that run without a GPU: the reference caster's analytic cases, Camera validation, lookat,
the body-attached composition, the hull-plane tables and the exported C-ABI (tests/test_camera_gpu.py runs the device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import (LABEL_ARENA, LABEL_ROBOT, MAX_PLANES, Camera, camera_table, geom_labels, hull_plane_table, quat_to_mat,
                                  reduced_pose)
from furniture_amd.mjcf.model import load_compiled
from tests import camera_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOWN = np.eye(3)  # camera -> world rotation of a camera looking straight down: its -z is the world's -z, its +y the world's +y


def _geom(gid, gtype, size, pos=(0, 0, 0), mat=np.eye(3), **kw):
    return dict(id=gid, type=gtype, size=np.asarray(size, dtype=np.float64), pos=np.asarray(pos, dtype=np.float64), mat=np.asarray(mat), **kw)


# ---- the reference caster against closed-form answers ------------------------------------------------------------------------
def test_reference_floor_from_above_is_flat():
    h = 1.3
    d, s = ref.render((0.2, -0.1, h), DOWN, 60.0, 32, 24, 0.01, 10.0, [_geom(0, ref.PLANE, (0, 0, 0))])
    assert (s == 0).all()
    np.testing.assert_allclose(d, h, rtol=0, atol=1e-12)  # depth along the optical axis, not along the ray


def test_reference_sphere_ahead():
    dist, r = 2.0, 0.25
    d, s = ref.render((0, 0, 0), np.eye(3), 30.0, 33, 33, 0.01, 10.0, [_geom(5, ref.SPHERE, (r, 0, 0), pos=(0, 0, -dist))])
    assert s[16, 16] == 5 and abs(d[16, 16] - (dist - r)) < 1e-12
    assert s[0, 0] == -1 and d[0, 0] == 10.0


def test_reference_box_near_faces():
    # axis-aligned box centred 3 m ahead, half extents (0.5, 0.4, 0.3): the central pixels see its +z face at depth 3 - 0.3
    d, s = ref.render((0, 0, 0), np.eye(3), 40.0, 41, 41, 0.01, 10.0, [_geom(2, ref.BOX, (0.5, 0.4, 0.3), pos=(0, 0, -3))])
    assert (s[18:23, 18:23] == 2).all()
    np.testing.assert_allclose(d[18:23, 18:23], 2.7, atol=1e-12)
    # seen from the side (camera on +x), the +x face at depth 2 - 0.5
    R = np.stack([[0, 1, 0], [0, 0, 1], [1, 0, 0]], axis=1).astype(float)  # cam x -> world y, cam y -> world z, cam z -> world x
    d, s = ref.render((2.0, 0, 0), R, 40.0, 21, 21, 0.01, 10.0, [_geom(2, ref.BOX, (0.5, 0.4, 0.3))])
    assert s[10, 10] == 2 and abs(d[10, 10] - 1.5) < 1e-12


def test_reference_capsule_end_cap():
    r, h = 0.1, 0.4
    # looking down the capsule's axis from above: the centre pixel meets the top of the upper cap at z = h + r
    d, s = ref.render((0, 0, 2.0), DOWN, 20.0, 21, 21, 0.01, 10.0, [_geom(3, ref.CAPSULE, (r, h, 0))])
    assert s[10, 10] == 3 and abs(d[10, 10] - (2.0 - h - r)) < 1e-12
    # a ray off the axis meets the cap sphere, not a flat disc: the hit point lies on the sphere of radius r about (0, 0, h)
    D = ref.pixel_rays(DOWN, 20.0, 21, 21)[10, 9]
    t0, t1, hit = ref.solid_interval(ref.CAPSULE, np.array([r, h, 0]), np.array([0, 0, 2.0]), D[None])
    assert hit[0]
    p = np.array([0, 0, 2.0]) + t0[0] * D
    assert abs(np.linalg.norm(p - [0, 0, h]) - r) < 1e-9 and p[2] > h + 0.5 * r
    assert abs(d[10, 9] - t0[0]) < 1e-12 and s[10, 9] == 3


def test_reference_hull_cube_matches_box():
    verts = np.array([[x, y, z] for x in (-0.2, 0.2) for y in (-0.3, 0.3) for z in (-0.1, 0.1)])
    # the cube as a hull of its 8 vertices, seen by a camera that looks at it from (0.5, -0.8, 0.6)
    from furniture_amd.camera import lookat_quat
    R = quat_to_mat(lookat_quat((0.5, -0.8, 0.6), (0, 0, 0)))
    a = ref.render((0.5, -0.8, 0.6), R, 50.0, 40, 30, 0.01, 10.0, [_geom(1, ref.BOX, (0.2, 0.3, 0.1))])
    b = ref.render((0.5, -0.8, 0.6), R, 50.0, 40, 30, 0.01, 10.0, [_geom(1, ref.MESH, (0, 0, 0), halfspaces=ref.mesh_halfspaces(verts))])
    assert (a[1] == 1).sum() > 50
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[0], b[0], atol=1e-12)


def test_reference_near_plane_clips_to_the_far_side():
    # camera inside a sphere: the entry point lies behind znear, the surface seen is the exit point
    d, s = ref.render((0, 0, 0), np.eye(3), 30.0, 11, 11, 0.01, 10.0, [_geom(4, ref.SPHERE, (0.5, 0, 0))])
    assert s[5, 5] == 4 and abs(d[5, 5] - 0.5) < 1e-12


# ---- Camera ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(fovy=0), dict(fovy=180), dict(fovy=-5), dict(znear=0), dict(znear=-1), dict(znear=1, zfar=1),
                                dict(znear=2, zfar=1), dict(width=0), dict(height=513), dict(width=2.5), dict(quat=(0, 0, 0, 0)),
                                dict(quat=(1, 0, 0, 0), lookat=(0, 0, 0)), dict(lookat=(0, 0, 1))])
def test_camera_validation(kw):
    with pytest.raises(ValueError):
        Camera((0, 0, 1), **kw)


def test_camera_lookat():
    pos, at = np.array([1.0, -2.0, 1.5]), np.array([0.2, 0.1, 0.4])
    cam = Camera(pos, lookat=at)
    R = quat_to_mat(cam.quat)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    fwd = (at - pos) / np.linalg.norm(at - pos)
    np.testing.assert_allclose(-R[:, 2], fwd, atol=1e-12)  # the optical axis is the camera's -z
    assert abs(R[2, 0]) < 1e-12 and R[2, 1] > 0  # x horizontal, +y up
    # straight down: still a valid rotation
    R = quat_to_mat(Camera((0, 0, 2), lookat=(0, 0, 0)).quat)
    np.testing.assert_allclose(-R[:, 2], [0, 0, -1], atol=1e-12)


def test_camera_table_rows():
    m = load_compiled("Sawyer", "table_lack_0825")
    cams = [Camera((0, 0, 1), fovy=60, width=64, height=48), Camera((0, 0, 0.1), body="right_hand", width=64, height=48)]
    tab = camera_table(m, cams)
    assert tab["body"].tolist() == [-1, m.meta["body_names"].index("right_hand")]
    assert tab["width"].tolist() == [64, 64] and tab["height"].tolist() == [48, 48]
    with pytest.raises(ValueError, match="unknown body"):
        camera_table(m, [Camera((0, 0, 1), body="no_such_body")])
    with pytest.raises(ValueError, match="one size"):
        camera_table(m, [Camera((0, 0, 1)), Camera((0, 0, 1), width=32)])
    with pytest.raises(ValueError):
        camera_table(m, [Camera((0, 0, 1))] * 9)


@pytest.mark.parametrize("agent,furniture,body", [("Sawyer", "table_lack_0825", "right_hand"), ("Sawyer", "table_lack_0825", "r_gripper_l_finger_tip"),
                                                  ("Baxter", "desk_mikael_1064", "left_hand"), ("Sawyer", "table_lack_0825", "1_part1")])
def test_body_attached_composition_matches_oracle_body_pose(agent, furniture, body):
    """reduced body pose (x) (body_relpos, body_relquat) (x) camera pose == the body's own world pose (x) camera pose, with the body poses
    of the fp64 oracle's forward pass at a random configuration"""
    from oracle.oracle_sim import OracleSim
    m = load_compiled(agent, furniture)
    o = OracleSim(m)
    rng = np.random.RandomState(3)
    q = np.asarray(m.qpos0, dtype=np.float64).copy()
    q[np.asarray(m.arm_qposadr)] += rng.uniform(-0.6, 0.6, len(m.arm_qposadr))
    a = int(m.part_qposadr[1])
    q[a:a + 3] += [0.1, -0.2, 0.3]
    qq = rng.normal(size=4)
    q[a + 3:a + 7] = qq / np.linalg.norm(qq)
    o.data.qpos[:] = q
    o.forward()
    cam = Camera((0.03, -0.02, 0.11), quat=(0.9, 0.1, -0.3, 0.2), body=body)
    b = cam.body_id(m)
    want_p, want_R = cam.world_pose(o.data.xpos[b], o.data.xquat[b])
    rb, lp, lq = reduced_pose(m, cam)
    ob = int(m.arrays["r_orig"][rb])
    Rr = quat_to_mat(o.data.xquat[ob])
    np.testing.assert_allclose(o.data.xpos[ob] + Rr @ lp, want_p, atol=1e-9)
    np.testing.assert_allclose(Rr @ quat_to_mat(lq), want_R, atol=1e-9)
    o.close()


# ---- hull planes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("furniture", ["chair_agne_0010", "chair_bertil_0148", "shelf_liden_0922"])
def test_hull_plane_tables(furniture):
    m = load_compiled("Sawyer", furniture)
    A = m.arrays
    planes, adr, num = hull_plane_table(m)
    assert planes.dtype == np.float32 and 0 < len(planes) <= MAX_PLANES
    mesh = np.nonzero(np.asarray(A["cg_meshnum"]) > 0)[0]
    assert len(mesh) >= 1 and (num[mesh] >= 4).all() and (num[np.asarray(A["cg_meshnum"]) == 0] == 0).all()
    verts = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)
    for g in mesh:
        v = verts[int(A["cg_meshadr"][g]):int(A["cg_meshadr"][g]) + int(A["cg_meshnum"][g])]
        P = planes[adr[g]:adr[g] + num[g]].astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(P[:, :3], axis=1), 1.0, atol=1e-6)
        s = v @ P[:, :3].T - P[:, 3]
        assert (s <= 1e-5).all()                          # every vertex inside every plane
        assert ((np.abs(s) < 1e-5).sum(0) >= 3).all()     # every plane carries a face (3+ vertices)
        n = P[:, :3]
        assert not np.any(np.triu((n @ n.T > 1 - 1e-6) & (np.abs(P[:, 3][:, None] - P[:, 3][None]) < 1e-6), 1))  # coplanar facets merged
        from scipy.spatial import ConvexHull
        assert len(P) < len(ConvexHull(v).equations)
    if furniture == "chair_agne_0010":
        assert int(A["cg_meshnum"][mesh[0]]) == 433 and num[mesh[0]] <= MAX_PLANES


def test_models_without_meshes_have_empty_plane_tables():
    planes, adr, num = hull_plane_table(load_compiled("Sawyer", "table_lack_0825"))
    assert planes.shape == (0, 4) and not num.any()


# ---- segmentation labels --------------------------------------------------------------------------------------------------------
def test_geom_labels():
    m = load_compiled("Sawyer", "table_lack_0825")
    A = m.arrays
    lab = geom_labels(m)
    assert lab.shape == (m.ngeom,) and lab.dtype == np.int32
    assert lab[m.meta["geom_names"].index("FLOOR")] == LABEL_ARENA
    robot = np.nonzero(np.asarray(A["geom_is_robot"]) != 0)[0]
    assert len(robot) and (lab[robot] == LABEL_ROBOT).all()
    part = np.asarray(A["body_partid"])[np.asarray(A["geom_bodyid"])]
    assert (lab[part >= 0] == part[part >= 0]).all() and set(range(m.nparts)) <= set(lab.tolist())
    mc = load_compiled("Cursor", "toy_table")
    labc = geom_labels(mc)
    cursor = [i for i, n in enumerate(mc.meta["geom_names"]) if "cursor" in n]
    assert cursor and (labc[cursor] == LABEL_ROBOT).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_camera_header_symbols_are_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsim_camera.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fsim_\w+)\s*\(", src)))
    assert declared == sorted(sim.CAMERA_SYMBOLS)
    assert not set(sim.CAMERA_SYMBOLS) & set(sim.EXPORTED_SYMBOLS)
    assert not set(sim.CAMERA_SYMBOLS) & set(re.findall(r"\b(fsim_\w+)\s*\(", open(os.path.join(ROOT, "include", "fsim.h")).read()))
    lib = ctypes.CDLL(sim.build())
    for n in sim.CAMERA_SYMBOLS:
        assert hasattr(lib, n), n


def test_camera_struct_matches_header():
    from furniture_amd.camera import CAMERA_DTYPE
    src = open(os.path.join(ROOT, "include", "fsim_camera.h")).read()
    body = re.search(r"typedef struct fsim_camera \{(.*?)\} fsim_camera_t;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)(?:\[(\d)\])?\s*[,;]", body)
    assert [f for f, _ in fields] == ["body", "pos", "quat", "fovy_deg", "znear", "zfar", "width", "height"]
    assert CAMERA_DTYPE.names == ("body", "pos", "quat", "fovy", "znear", "zfar", "width", "height")
    assert CAMERA_DTYPE.itemsize == 4 * (1 + 3 + 4 + 3 + 2)
    for name in ("FSIM_CAM_MAX = 8", "FSIM_CAM_MAX_SIZE = 512", "FSIM_CAM_MAX_GEOMS = 96", "FSIM_CAM_MAX_PLANES = 1024"):
        assert name in src


def test_catalogue_fits_the_camera_caps():
    """every compiled model stays within the ray pass's LDS stage (colliding geoms) and plane cap"""
    import glob
    from furniture_amd.camera import MAX_GEOMS
    from furniture_amd.mjcf.model import CompiledModel
    worst = 0
    for p in sorted(glob.glob(os.path.join(ROOT, "furniture_amd", "assets", "compiled", "*.npz"))):
        m = CompiledModel.load(p)
        worst = max(worst, len(m.arrays["cg_orig"]))
        if "cg_meshnum" in m.arrays and (np.asarray(m.arrays["cg_meshnum"]) > 0).any():
            assert len(hull_plane_table(m)[0]) <= MAX_PLANES
    assert 0 < worst <= MAX_GEOMS

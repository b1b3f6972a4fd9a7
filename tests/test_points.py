"""Point clouds, the parts that run without a GPU: the reference FPS on clouds with known answers, PointCloud validation, geom_keep and
the exported C-ABI of include/fsim_points.h (tests/test_points_gpu.py runs the device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import LABEL_ARENA, LABEL_ROBOT, Camera, geom_labels
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.points import MAX_PIXELS, MAX_POINTS, PointCloud, check, geom_keep
from tests import points_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference FPS ----------------------------------------------------------------------------------------------------------
def test_fps_line_takes_the_ends_first():
    x = np.array([0.3, 0.0, 1.0, 0.5, 0.9, 0.1], dtype=np.float32)
    p = np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
    rows = ref.fps(p, 4)
    # row 0 = candidate 0 (0.3); the farthest from it is 1.0 (index 2); then 0.0 (index 1: 0.3 away, beats 0.5's 0.2); then 0.5 or
    # 0.1 / 0.9 ... the largest of min distances: 0.5 -> min(0.2, 0.5) = 0.2, 0.1 -> 0.1, 0.9 -> 0.1: index 3
    assert rows.tolist() == [0, 2, 1, 3]


def test_fps_square_corners():
    # candidate 0 is a corner: then the opposite corner, then the two others (a tie: the smaller index first), then the centre
    p = np.array([[0, 0, 0], [0.5, 0.5, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.25, 0.5, 0]], dtype=np.float32)
    assert ref.fps(p, 5).tolist() == [0, 3, 2, 4, 1]
    # from the centre every corner is equally far: the smallest index wins, and the corner after it is the next in index order
    # (from (0, 0) the two neighbours and the opposite corner all keep dmin = 0.5, the distance to the centre)
    assert ref.fps(p[[1, 0, 2, 3, 4]], 5).tolist() == [0, 1, 2, 3, 4]


def test_fps_tie_goes_to_the_smaller_index():
    p = np.array([[0, 0, 0], [0, 0, 2], [2, 0, 0], [0, 2, 0], [0, 0, -2]], dtype=np.float32)
    assert ref.fps(p, 2).tolist() == [0, 1]
    assert ref.fps(p[[0, 4, 3, 2, 1]], 2).tolist() == [0, 1]


def test_fps_pads_with_row_0_and_handles_empty():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    rows = ref.fps(p, 6)
    assert rows[:3].tolist() in ([0, 1, 2], [0, 2, 1]) and rows[3:].tolist() == [0, 0, 0]
    assert ref.fps(np.zeros((0, 3), np.float32), 4).tolist() == [-1] * 4


def test_fps_random_cloud_against_a_scalar_loop():
    rng = np.random.RandomState(0)
    p = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    rows = ref.fps(p, 40)
    assert len(set(rows.tolist())) == 40  # 300 distinct points: no repeats before the candidates run out
    # the rule with numpy float32 scalars, one operation at a time
    f = np.float32
    dmin, prev, want, chosen = [f(np.inf)] * len(p), 0, [0], []
    for _ in range(1, 40):
        for k in range(len(p)):
            dx, dy, dz = p[k, 0] - p[prev, 0], p[k, 1] - p[prev, 1], p[k, 2] - p[prev, 2]
            dmin[k] = min(dmin[k], f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
        best = max(dmin)
        prev = dmin.index(best)
        want.append(prev)
        chosen.append(best)
    assert rows.tolist() == want
    assert all(a >= b for a, b in zip(chosen, chosen[1:]))  # the chosen distances never grow


def test_back_project_centre_pixel():
    # a camera at (0, 0, 2) looking straight down, 3 x 3 pixels: the centre ray is the optical axis
    depth = np.full((3, 3), 1.5)
    xyz = ref.back_project(depth, (0.0, 0.0, 2.0), np.eye(3), 60.0)
    np.testing.assert_allclose(xyz[1, 1], [0.0, 0.0, 0.5], atol=1e-12)
    assert xyz[0, 0, 0] < 0 < xyz[0, 0, 1]  # top-left pixel: -x, +y (row 0 is the top of the image)


# ---- PointCloud -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(n_points=-1), dict(n_points=MAX_POINTS + 1), dict(n_points=2.5), dict(n_points=True), dict(include=()),
                                dict(include=("parts", "table")), dict(include=("parts", "parts")), dict(box=((0, 0, 0), (1, 1))),
                                dict(box=((0, 0, 0), (1, np.inf, 1))), dict(box=((0, 0, 1), (1, 1, 0))), dict(box=((0, 0, 0), (1, np.nan, 1)))])
def test_point_cloud_validation(kw):
    with pytest.raises(ValueError):
        PointCloud(**kw)


def test_point_cloud_accepts():
    pc = PointCloud()
    assert pc.n_points == 512 and pc.include == ("parts", "robot") and pc.box is None and not pc.dense
    pc = PointCloud(0, include="floor", box=[-1, -1, 0, 1, 1, 2])
    assert pc.dense and pc.include == ("floor",) and pc.box.shape == (2, 3)
    assert PointCloud(MAX_POINTS, box=((0, 0, 0), (0, 0, 0))).n_points == MAX_POINTS  # a flat box is allowed (inclusive bounds)


def test_check_against_cameras():
    with pytest.raises(ValueError, match="needs cameras"):
        check(PointCloud(), None)
    with pytest.raises(TypeError):
        check(dict(n_points=5), [Camera((0, 0, 1))])
    check(PointCloud(), [Camera((0, 0, 1), width=64, height=64)] * 4)  # 16384 pixels: at the cap
    with pytest.raises(ValueError, match="pixels per env"):
        check(PointCloud(), [Camera((0, 0, 1), width=128, height=129)])
    assert MAX_PIXELS == 16384


# ---- geom_keep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table"),
                                             ("Sawyer", "chair_agne_0010")])
def test_geom_keep(agent, furniture):
    m = load_compiled(agent, furniture)
    lab = geom_labels(m)
    parts, robot, floor = lab >= 0, lab == LABEL_ROBOT, lab == LABEL_ARENA
    assert parts.any() and robot.any() and floor.any()
    for inc, want in ((("parts",), parts), (("robot",), robot), (("floor",), floor), (("parts", "robot"), parts | robot),
                      (("parts", "robot", "floor"), np.ones_like(parts))):
        k = geom_keep(m, inc)
        assert k.dtype == np.uint8 and k.shape == (m.ngeom,)
        np.testing.assert_array_equal(k.astype(bool), want, err_msg=str(inc))
    floor_id = m.meta["geom_names"].index("FLOOR") if "FLOOR" in m.meta["geom_names"] else int(np.nonzero(floor)[0][0])
    assert geom_keep(m, ("parts", "robot"))[floor_id] == 0
    if furniture == "chair_agne_0010":  # the hull collider is a part geom
        g = int(m.arrays["cg_orig"][int(np.nonzero(np.asarray(m.arrays["cg_meshnum"]) > 0)[0][0])])
        assert geom_keep(m, ("parts",))[g] == 1


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, point_cloud=PointCloud())
    from furniture_amd.vec_env import FurnitureVecEnv
    with pytest.raises(NotImplementedError, match="mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, point_cloud=PointCloud())
    with pytest.raises(NotImplementedError, match="VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(point_cloud=PointCloud()))

    class _Handle:  # a handle with point-cloud settings and no cameras
        cameras, points = None, PointCloud()

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="point clouds"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_points_header_symbols_are_exported():
    assert sorted(_declared("fsim_points.h")) == sorted(sim.POINTS_SYMBOLS)
    assert not set(sim.POINTS_SYMBOLS) & set(sim.EXPORTED_SYMBOLS)
    assert not set(sim.POINTS_SYMBOLS) & set(sim.CAMERA_SYMBOLS)
    assert not set(sim.POINTS_SYMBOLS) & (_declared("fsim.h") | _declared("fsim_camera.h"))
    lib = ctypes.CDLL(sim.build())
    for n in sim.POINTS_SYMBOLS:
        assert hasattr(lib, n), n


def test_points_header_limits_match_python():
    src = open(os.path.join(ROOT, "include", "fsim_points.h")).read()
    assert "FSIM_PTS_MAX_PIXELS = %d" % MAX_PIXELS in src and "FSIM_PTS_MAX_POINTS = %d" % MAX_POINTS in src

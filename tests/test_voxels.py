"""Voxel grids, the parts that run without a GPU: the reference binning on hand-built maps, VoxelGrid validation, the refusals and the
exported C-ABI of include/fsim_voxels.h (tests/test_voxels_gpu.py runs the device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import Camera
from furniture_amd.voxels import MAX_CELLS, MAX_DIM, VoxelGrid, check
from tests import voxels_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ((-1.0, -0.5, 0.0), (1.0, 0.5, 2.0))


def _map(points, labels):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3), np.asarray(labels, dtype=np.int32)


# ---- the reference binning ------------------------------------------------------------------------------------------------------
def test_bounds_land_in_the_first_and_last_cell():
    xyz, seg = _map([BOX[0], BOX[1]], [5, 7])
    count, label = ref.voxelize(xyz, seg, (4, 3, 2), BOX)
    assert count[0, 0, 0] == 1 and label[0, 0, 0] == 5       # p == lo: cell 0
    assert count[3, 2, 1] == 1 and label[3, 2, 1] == 7       # p == hi: the last cell (floor gives dims, clamped)
    assert count.sum() == 2 and (label >= 0).sum() == 2
    assert ref.cells(xyz, (4, 3, 2), BOX).tolist() == [0, 4 * 3 * 2 - 1]


def test_points_just_outside_are_dropped():
    lo, hi = np.float32(BOX[0]), np.float32(BOX[1])
    out = [np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]
    pts = []
    for a in range(3):
        for v, base in ((out[0][a], lo), (out[1][a], hi)):
            q = base.copy()
            q[a] = v
            pts.append(q)
    xyz, seg = _map(pts, [1] * len(pts))
    count, label = ref.voxelize(xyz, seg, (5, 5, 5), BOX)
    assert count.sum() == 0 and (label == -1).all()
    # the same points nudged back inside are kept
    count, _ = ref.voxelize(np.clip(xyz, lo, hi), seg, (5, 5, 5), BOX)
    assert count.sum() == len(pts)


def test_unkept_pixels_are_dropped():
    xyz, seg = _map([[0, 0, 1]] * 3, [-1, 4, -1])
    count, label = ref.voxelize(xyz, seg, (2, 2, 2), BOX)
    assert count.sum() == 1 and label[1, 1, 1] == 4


def test_label_is_the_smallest_pix():
    # three pixels in one cell, the first (smallest pix) sees geom 9; a fourth pixel in another cell
    xyz, seg = _map([[0.9, 0.4, 1.9], [0.1, 0.1, 0.1], [0.95, 0.45, 1.95], [0.8, 0.3, 1.7]], [9, 2, 3, 4])
    count, label = ref.voxelize(xyz, seg, (2, 2, 2), BOX)
    assert count[1, 1, 1] == 3 and label[1, 1, 1] == 9
    assert count[1, 1, 0] == 1 and label[1, 1, 0] == 2
    assert count.sum() == 4 and (label >= 0).sum() == 2
    # reversing the pixel order makes the last pixel the first
    count2, label2 = ref.voxelize(xyz[::-1], seg[::-1], (2, 2, 2), BOX)
    assert label2[1, 1, 1] == 4 and (count2 == count).all()


def test_count_saturates():
    n = 40000
    xyz, seg = _map(np.tile([0.1, 0.1, 0.1], (n, 1)), np.arange(n) % 3)
    count, label = ref.voxelize(xyz, seg, (1, 1, 1), BOX)
    assert count.dtype == np.int16 and count[0, 0, 0] == 32767 and label[0, 0, 0] == 0
    count, _ = ref.voxelize(xyz[:32767], seg[:32767], (1, 1, 1), BOX)
    assert count[0, 0, 0] == 32767
    count, _ = ref.voxelize(xyz[:32766], seg[:32766], (1, 1, 1), BOX)
    assert count[0, 0, 0] == 32766


def test_non_cubic_dims_z_fastest():
    dims = (5, 3, 7)
    b = np.asarray(BOX, np.float32)
    rng = np.random.RandomState(0)
    p = (b[0] + rng.uniform(0, 1, (2000, 3)) * (b[1] - b[0])).astype(np.float32)
    count, label = ref.voxelize(p, np.arange(2000) % 11, dims, BOX)
    assert count.shape == dims and count.sum() == 2000
    # a scalar loop of the header's rule, one float32 operation at a time
    f = np.float32
    s = [f(dims[a]) / (f(b[1][a]) - f(b[0][a])) for a in range(3)]
    want_c, want_l = np.zeros(dims, np.int64), np.full(dims, -1, np.int64)
    for k, q in enumerate(p):
        i = [min(int(np.floor(f(f(q[a] - b[0][a]) * s[a]))), dims[a] - 1) for a in range(3)]
        want_c[tuple(i)] += 1
        if want_l[tuple(i)] < 0:
            want_l[tuple(i)] = k % 11
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(label, want_l)
    # the linear index: (i_x * dy + i_y) * dz + i_z
    c = ref.cells(p[:50], dims, BOX)
    np.testing.assert_array_equal(count.reshape(-1)[c] > 0, True)


def test_scale_is_one_float32_division():
    box = ((0.1, 0.2, 0.3), (0.7, 0.9, 1.3))
    s = ref.scale((30, 20, 17), box)
    assert s.dtype == np.float32
    b = np.asarray(box, np.float32)
    assert s.tolist() == [np.float32(d) / np.float32(b[1][a] - b[0][a]) for a, d in enumerate((30, 20, 17))]
    np.testing.assert_array_equal(VoxelGrid((30, 20, 17), box).scale, s)


# ---- VoxelGrid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dims=(0, 4, 4)), dict(dims=(4, 4, MAX_DIM + 1)), dict(dims=(4, 4)), dict(dims=(4, 4, 2.5)),
                                dict(dims=(64, 64, 65)), dict(dims=("a", 1, 1)), dict(box=None), dict(box=((0, 0, 0), (1, 1)),),
                                dict(box=((0, 0, 0), (1, np.inf, 1))), dict(box=((0, 0, 0), (1, np.nan, 1))),
                                dict(box=((0, 0, 1), (1, 1, 0))), dict(box=((0, 0, 0), (1, 1, 0))), dict(box=((0, 0, 1), (1, 1, 1 + 1e-9))),
                                dict(box=((-3e38, 0, 0), (3e38, 1, 1))), dict(include=()), dict(include=("parts", "table")),
                                dict(include=("parts", "parts"))])
def test_voxel_grid_validation(kw):
    args = dict(dims=(8, 8, 8), box=BOX)
    args.update(kw)
    with pytest.raises(ValueError):
        VoxelGrid(**args)


def test_voxel_grid_accepts():
    g = VoxelGrid((32, 32, 32), BOX)
    assert g.dims == (32, 32, 32) and g.include == ("parts", "robot") and g.n_cells == 32768
    assert g.box.dtype == np.float32 and g.box.shape == (2, 3) and g.box.tolist() == np.asarray(BOX, np.float32).tolist()
    g = VoxelGrid(np.array([64, 64, 64]), [-1, -1, 0, 1, 1, 2], include="floor")
    assert g.n_cells == MAX_CELLS and g.include == ("floor",)
    assert VoxelGrid((MAX_DIM, 1, 1), BOX).dims == (MAX_DIM, 1, 1)
    assert VoxelGrid((1, 1, 1), BOX, include=("parts", "robot", "floor")).n_cells == 1


def test_check_against_cameras():
    with pytest.raises(ValueError, match="needs cameras"):
        check(VoxelGrid((4, 4, 4), BOX), None)
    with pytest.raises(TypeError):
        check(dict(dims=(4, 4, 4)), [Camera((0, 0, 1))])
    check(VoxelGrid((4, 4, 4), BOX), [Camera((0, 0, 1), width=256, height=256)] * 8)  # no pixel cap


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    grid = VoxelGrid((8, 8, 8), BOX)
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, voxels=grid)
    with pytest.raises(TypeError, match="VoxelGrid"):
        FurnitureBatchEnv("Sawyer", 1, cameras=[Camera((0, 0, 1))], voxels=(8, 8, 8))
    with pytest.raises(NotImplementedError, match="mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, voxels=grid)
    with pytest.raises(NotImplementedError, match="VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(voxels=grid))

    class _Handle:  # a handle with voxel settings and no cameras
        cameras, points, voxels = None, None, grid

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="voxel grids"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_voxels_header_symbols_are_exported():
    assert sorted(_declared("fsim_voxels.h")) == sorted(sim.VOXELS_SYMBOLS)
    others = set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS)
    assert not set(sim.VOXELS_SYMBOLS) & others
    assert not set(sim.VOXELS_SYMBOLS) & (_declared("fsim.h") | _declared("fsim_camera.h") | _declared("fsim_points.h"))
    lib = ctypes.CDLL(sim.build())
    for n in sim.VOXELS_SYMBOLS:
        assert hasattr(lib, n), n


def test_voxels_header_limits_and_rule_match_python():
    src = open(os.path.join(ROOT, "include", "fsim_voxels.h")).read()
    assert "FSIM_VOX_MAX_DIM = %d" % MAX_DIM in src and "FSIM_VOX_MAX_CELLS = %d" % MAX_CELLS in src
    assert MAX_CELLS == 64 ** 3
    # the cell rule and the saturation the reference implements
    flat = " ".join(src.split())
    for s in ("s_a = (float)dims_a / (hi_a - lo_a)", "t = (p_a - lo_a) * s_a", "i_a = min((int)floorf(t), dims_a - 1)",
              "(i_x * dy + i_y) * dz + i_z", "saturating at %d" % ref.SATURATE, "smallest pix"):
        assert s in flat, s

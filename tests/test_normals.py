"""Normal / shaded images, the parts that run without a GPU: the reference normals on hand-built scenes, Normals validation and the
palette, the refusals, save_ppm and the exported C-ABI of include/fsim_normals.h (tests/test_normals_gpu.py runs the device)."""
import ctypes
import os
import re

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import LABEL_ARENA, LABEL_ROBOT, Camera, geom_labels, lookat_quat, quat_to_mat
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.normals import PART_COLORS, Normals, check, default_palette, save_ppm
from tests import normals_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(3)


def _geom(gtype, size, pos=(0, 0, 0), mat=EYE, gid=3, **kw):
    return dict(id=gid, type=gtype, size=np.asarray(size, dtype=np.float64), pos=np.asarray(pos, dtype=np.float64), mat=np.asarray(mat, dtype=np.float64), **kw)


def _look(pos, at, geoms, size=1, fovy=40.0, up=(0.0, 0.0, 1.0)):
    """the reference's images of a size x size camera at pos looking at `at`"""
    R = quat_to_mat(lookat_quat(pos, at, up))
    return ref.render(np.asarray(pos, dtype=np.float64), R, fovy, size, size, 0.01, 20.0, geoms)


def _centre(pos, at, geoms, **kw):
    r = _look(pos, at, geoms, **kw)
    return r["seg"][0, 0], r["normal"][0, 0], r["margin"][0, 0], r["radius"][0, 0]


# ---- the reference normals --------------------------------------------------------------------------------------------------------
def test_sphere_ahead_faces_the_camera():
    g = [_geom(ref.SPHERE, (0.5, 0, 0), pos=(0, 0, -2))]
    r = ref.render(np.zeros(3), EYE, 40.0, 1, 1, 0.01, 10.0, g)  # the one pixel looks along -z, through the sphere's centre
    assert r["seg"][0, 0] == 3 and abs(r["depth"][0, 0] - 1.5) < 1e-12
    np.testing.assert_allclose(r["normal"][0, 0], (0, 0, 1), atol=1e-12)
    assert r["margin"][0, 0] == np.inf and r["radius"][0, 0] == 0.5
    # off the centre: the normal is the unit vector from the sphere's centre to the hit point
    r = ref.render(np.zeros(3), EYE, 40.0, 9, 9, 0.01, 10.0, g)
    hit = r["seg"] == 3
    assert hit.sum() > 9
    np.testing.assert_allclose(r["normal"][hit], (r["point"][hit] - (0, 0, -2)) / 0.5, atol=1e-9)
    np.testing.assert_allclose(np.linalg.norm(r["normal"][hit], axis=1), 1.0, atol=1e-12)
    assert (r["normal"][~hit] == 0).all() and (r["margin"][~hit] == np.inf).all()


def test_box_faces():
    rot = quat_to_mat((0.9, 0.1, -0.3, 0.2))  # an arbitrary orientation: the normal is a column of the box's rotation
    for mat in (EYE, rot):
        g = [_geom(ref.BOX, (0.3, 0.2, 0.1), pos=(0.5, -0.2, 0.4), mat=mat)]
        for a in range(3):
            for sg in (1.0, -1.0):
                face = sg * mat[:, a]
                seg, n, margin, radius = _centre(np.asarray(g[0]["pos"]) + 2.0 * face, g[0]["pos"], g, up=mat[:, (a + 1) % 3])
                assert seg == 3 and radius == np.inf
                np.testing.assert_allclose(n, face, atol=1e-12)
                assert margin == pytest.approx(min(g[0]["size"][b] for b in range(3) if b != a), abs=1e-9)  # the nearest other face


def test_box_edge_has_a_small_margin():
    g = [_geom(ref.BOX, (0.3, 0.3, 0.3))]
    r = _look((2.0, 2.0, 0.0), (0, 0, 0), g, size=33)  # looking at the x / y edge: both faces in view, the margin vanishes between them
    hit = r["seg"] == 3
    nx, ny = hit & (r["normal"][..., 0] == 1.0), hit & (r["normal"][..., 1] == 1.0)
    assert nx.sum() > 50 and ny.sum() > 50 and (nx | ny)[hit].all()
    assert r["margin"][hit].min() < 0.02 and r["margin"][hit].max() > 0.2


def test_cylinder_cap_against_side():
    g = [_geom(ref.CYLINDER, (0.2, 0.4, 0))]
    seg, n, margin, radius = _centre((0.05, 0.0, 3.0), (0.05, 0.0, 0.0), g, up=(0, 1, 0))  # from above: the cap
    np.testing.assert_allclose(n, (0, 0, 1), atol=1e-12)
    assert radius == np.inf and margin == pytest.approx(0.15, abs=1e-9)
    seg, n, margin, radius = _centre((0.0, 0.0, -3.0), (0.0, 0.0, 0.0), g, up=(0, 1, 0))  # from below: the other cap
    np.testing.assert_allclose(n, (0, 0, -1), atol=1e-12)
    seg, n, margin, radius = _centre((3.0, 0.0, 0.1), (0.0, 0.0, 0.1), g)  # from the side: radial
    np.testing.assert_allclose(n, (1, 0, 0), atol=1e-12)
    assert radius == 0.2 and margin == pytest.approx(0.3, abs=1e-9)
    seg, n, _, _ = _centre((2.0, 2.0, 0.0), (0.0, 0.0, 0.0), g)
    np.testing.assert_allclose(n, (np.sqrt(0.5), np.sqrt(0.5), 0), atol=1e-12)


def test_capsule_cap_and_barrel():
    g = [_geom(ref.CAPSULE, (0.2, 0.4, 0))]
    seg, n, margin, radius = _centre((3.0, 0.0, 0.3), (0.0, 0.0, 0.3), g)  # the barrel: radial
    np.testing.assert_allclose(n, (1, 0, 0), atol=1e-12)
    assert margin == np.inf and radius == 0.2
    seg, n, _, _ = _centre((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), g, up=(0, 1, 0))  # the top of the cap
    np.testing.assert_allclose(n, (0, 0, 1), atol=1e-12)
    r = _look((3.0, 0.0, 0.5), (0.0, 0.0, 0.5), g, size=1)  # on the cap, off its axis: away from the end sphere's centre
    want = (r["point"][0, 0] - (0, 0, 0.4)) / 0.2
    assert r["point"][0, 0][2] > 0.4 and want[2] > 0.1
    np.testing.assert_allclose(r["normal"][0, 0], want, atol=1e-9)


def test_cube_as_a_hull_equals_the_box():
    verts = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.2, 0.2) for z in (-0.1, 0.1)])
    rot = quat_to_mat((0.8, -0.2, 0.3, 0.4))
    box = [_geom(ref.BOX, (0.3, 0.2, 0.1), pos=(0.1, 0.2, 0.3), mat=rot)]
    hull = [_geom(ref.MESH, (0, 0, 0), pos=(0.1, 0.2, 0.3), mat=rot, halfspaces=ref.cref.mesh_halfspaces(verts))]
    cam = ((1.5, -1.2, 1.4), (0.1, 0.2, 0.3))
    rb, rh = _look(*cam, box, size=24), _look(*cam, hull, size=24)
    assert (rb["seg"] == rh["seg"]).all() and (rb["seg"] == 3).sum() > 30
    np.testing.assert_allclose(rh["depth"], rb["depth"], atol=1e-9)
    np.testing.assert_allclose(rh["normal"], rb["normal"], atol=1e-9)
    hit = rb["seg"] == 3
    np.testing.assert_allclose(rh["margin"][hit], rb["margin"][hit], atol=1e-9)  # the two triangles of a face are one face
    assert len({tuple(np.round(n, 6)) for n in rb["normal"][hit]}) == 3  # three faces in view


def test_floor_gives_plus_z():
    g = [_geom(ref.PLANE, (0, 0, 0), gid=0)]
    r = _look((1.0, -2.0, 1.5), (0.0, 0.0, 0.0), g, size=8)
    hit = r["seg"] == 0
    assert hit.sum() > 20
    np.testing.assert_allclose(r["normal"][hit], np.tile((0, 0, 1), (hit.sum(), 1)), atol=1e-12)
    assert (r["margin"][hit] == np.inf).all() and (r["radius"][hit] == np.inf).all()
    np.testing.assert_allclose(r["point"][hit][:, 2], 0.0, atol=1e-9)


def test_exit_hit_keeps_the_outward_normal():
    cam = np.array([0.1, -0.05, 0.02])  # inside the solids: the pixel shows the exit point, the normal still points outwards
    for g in ([_geom(ref.SPHERE, (0.5, 0, 0))], [_geom(ref.BOX, (0.5, 0.4, 0.3))], [_geom(ref.CYLINDER, (0.5, 0.4, 0))]):
        r = _look(cam, cam + (1.0, 0.3, 0.1), g, size=5)
        assert (r["seg"] == 3).all()
        view = cam - r["point"]  # from the surface back to the camera
        assert ((r["normal"] * view).sum(-1) < 0).all()
        assert (np.einsum("hwk,hwk->hw", r["normal"], r["point"]) > 0).all()  # away from the solid's centre (the origin)


# ---- Normals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(normal=False, shaded=False), dict(normal=1), dict(shaded="yes"), dict(ambient=-0.1), dict(ambient=1.5),
                                dict(ambient=np.nan), dict(ambient=np.inf), dict(ambient="0.2"), dict(ambient=True), dict(background=(0, 0, 0)),
                                dict(background=(0, 0, 0, 256)), dict(background=(0, 0, -1, 0)), dict(background=(0.5, 0, 0, 0)),
                                dict(palette=np.zeros((5, 3), np.uint8)), dict(palette=np.full((5, 4), 256)), dict(palette=np.full((5, 4), 0.5)),
                                dict(palette=np.zeros(4, np.uint8))])
def test_normals_validation(kw):
    with pytest.raises(ValueError):
        Normals(**kw)


def test_normals_accepts_and_palette():
    s = Normals()
    assert s.normal and not s.shaded and s.palette is None and s.background == (30, 30, 40, 255) and s.ambient == np.float32(0.25)
    m = load_compiled("Sawyer", "table_lack_0825")
    assert s.palette_for(m) is None  # normals only: no palette goes to the library
    s = Normals(normal=False, shaded=True, ambient=0, background=[1, 2, 3, 4])
    assert s.shaded and s.background == (1, 2, 3, 4) and s.ambient == 0.0
    pal = s.palette_for(m)
    assert pal.dtype == np.uint8 and pal.shape == (m.ngeom, 4) and (pal == default_palette(m)).all()
    lab = geom_labels(m)
    assert (pal[:, 3] == 255).all()
    arena, robot = pal[lab == LABEL_ARENA, :3], pal[lab == LABEL_ROBOT, :3]
    assert len(arena) and len(robot)
    assert (arena == arena[0]).all() and arena[0][0] == arena[0][1] == arena[0][2]  # one grey
    assert (robot == robot[0]).all() and tuple(robot[0]) != tuple(arena[0])         # one colour
    for k in range(m.nparts):
        rows = pal[lab == k, :3]
        assert len(rows) and (rows == PART_COLORS[k % len(PART_COLORS)]).all()
    assert len(PART_COLORS) >= 12 and len(set(PART_COLORS)) == len(PART_COLORS)
    assert not {tuple(arena[0]), tuple(robot[0])} & set(PART_COLORS)
    # a palette of one's own: by model geom id, the model's size
    own = np.arange(4 * m.ngeom).reshape(m.ngeom, 4) % 256
    assert (Normals(shaded=True, palette=own).palette_for(m) == own).all()
    with pytest.raises(ValueError, match="rows"):
        Normals(shaded=True, palette=own[:-1]).palette_for(m)


def test_check_against_cameras():
    with pytest.raises(ValueError, match="needs cameras"):
        check(Normals(), None)
    with pytest.raises(TypeError):
        check(dict(normal=True), [Camera((0, 0, 1))])
    check(Normals(shaded=True), [Camera((0, 0, 1), width=256, height=256)] * 8)  # no pixel cap


def test_save_ppm_round_trip(tmp_path):
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (17, 33, 4)).astype(np.uint8)
    for a in (img, img[:, :, :3]):
        path = str(tmp_path / "f.ppm")
        save_ppm(path, a)
        raw = open(path, "rb").read()
        head = b"P6\n33 17\n255\n"
        assert raw.startswith(head) and len(raw) == len(head) + 17 * 33 * 3
        back = np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(17, 33, 3)
        assert (back == img[:, :, :3]).all()
    for bad in (img.astype(np.float32), img[:, :, 0], img[:, :, :2]):
        with pytest.raises(ValueError):
            save_ppm(str(tmp_path / "g.ppm"), bad)


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = Normals(shaded=True)
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, normals=spec)
    with pytest.raises(TypeError, match="Normals"):
        FurnitureBatchEnv("Sawyer", 1, cameras=[Camera((0, 0, 1))], normals=True)
    with pytest.raises(NotImplementedError, match="mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, normals=spec)
    with pytest.raises(NotImplementedError, match="VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(normals=spec))

    class _Handle:  # a handle with normals settings and nothing else
        cameras, points, voxels, normals = None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="normal / shaded images"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_normals_header_symbols_are_exported():
    assert sim.NORMALS_SYMBOLS == ["fsim_set_normals", "fsim_render_normals"]
    assert sorted(_declared("fsim_normals.h")) == sorted(sim.NORMALS_SYMBOLS)
    others = set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS) | set(sim.VOXELS_SYMBOLS)
    assert not set(sim.NORMALS_SYMBOLS) & others
    assert not set(sim.NORMALS_SYMBOLS) & (_declared("fsim.h") | _declared("fsim_camera.h") | _declared("fsim_points.h") | _declared("fsim_voxels.h"))
    lib = ctypes.CDLL(sim.build())
    for n in sim.NORMALS_SYMBOLS:
        assert hasattr(lib, n), n


def test_normals_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_normals.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("p = Rg^T (q - pos_g)", "c = (0, 0, clamp(p.z, -h, h))", "hypot(p.x, p.y) - r >= |p.z| - h", "the side wins a tie",
              "the largest |p_a| - s_a", "the smallest axis wins a tie", "the largest n_k . p - d_k", "the smallest k wins a tie", "|.| < 1e-20",
              "seg == -1 gives (0, 0, 0)", "I = ambient + (1 - ambient) * lam", "floorf(palette[seg][c] * I + 0.5f)", "one 4-byte store"):
        assert s in flat, s

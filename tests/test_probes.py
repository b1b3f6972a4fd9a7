"""Distance probes, the parts that run without a GPU: ProbeSensor / ProbeSet validation, grid_points(), the "body" exclusion rule, the
float64 reference (tests/probes_reference.py) on hand-made scenes with closed-form answers, the plane bound of chair_agne_0010's hull
against the exact distance, the refusals and the C-ABI of include/fsim_probes.h (tests/test_probes_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import quat_to_mat
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.probes import MAX_PROBES, MAX_SENSORS, ProbeSensor, ProbeSet, check, grid_points, sensor_table
from furniture_amd.rays import exclude_mask
from tests import camera_reference as cref
from tests import probes_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P0 = [(0.0, 0.0, 0.0)]


# ---- ProbeSensor / ProbeSet -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dmax=0.0), dict(dmax=-1.0), dict(dmax=float("inf")), dict(dmax=float("nan")), dict(points=[]),
                                dict(points=[0.0, 0.0, 0.0]), dict(points=[(0.0, float("nan"), 0.0)]), dict(points=[(0.0, 0.0, 0.0), (float("inf"), 0.0, 0.0)]),
                                dict(points=[(0.0, 0.0)]), dict(quat=(0, 0, 0, 0)), dict(quat=(1, 0, float("nan"), 0)), dict(pos=(0, float("inf"), 0)),
                                dict(exclude="hand"), dict(exclude=[1.5])])
def test_sensor_validation(kw):
    args = dict(pos=(0, 0, 0), points=P0)
    args.update(kw)
    with pytest.raises(ValueError):
        ProbeSensor(**args)


def test_sensor_accepts():
    pts = np.array([(0, 0, -2.0), (3.0, 4.0, 0.0)])
    s = ProbeSensor((0, 0, 1), pts, quat=(2, 0, 0, 0), dmax=0.5, exclude=[3, 4])
    assert s.n_probes == 2 and np.array_equal(s.points, pts) and np.allclose(s.quat, (1, 0, 0, 0)) and s.dmax == 0.5
    pts[0, 0] = 9.0
    assert s.points[0, 0] == 0.0  # its own copy
    assert s.exclude == [3, 4] and s.body is None and "2 probes" in repr(s)
    assert ProbeSensor((0, 0, 0), P0).exclude == "body" and ProbeSensor((0, 0, 0), P0, exclude=None).exclude is None and ProbeSensor((0, 0, 0), P0).dmax == 1.0
    p, R = ProbeSensor((0.1, 0.0, 0.0), P0, body="b").world_pose((1.0, 2.0, 3.0), (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)))  # a quarter turn about z
    assert np.allclose(p, (1.0, 2.1, 3.0)) and np.allclose(R, quat_to_mat((np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))))


def test_probe_set_validation():
    one = ProbeSensor((0, 0, 0), P0)
    with pytest.raises(ValueError, match="0 sensors"):
        ProbeSet([])
    with pytest.raises(ValueError, match="17 sensors"):
        ProbeSet([one] * (MAX_SENSORS + 1))
    with pytest.raises(ValueError, match="4097 probes"):
        ProbeSet([ProbeSensor((0, 0, 0), np.zeros((MAX_PROBES // 2, 3))), ProbeSensor((0, 0, 0), np.zeros((MAX_PROBES // 2 + 1, 3)))])
    with pytest.raises(TypeError, match="ProbeSensor"):
        ProbeSet([one, "grid"])
    with pytest.raises(ValueError, match="boolean"):
        ProbeSet([one], gradient=1)
    with pytest.raises(TypeError, match="ProbeSet"):
        check([one])
    ps = ProbeSet([ProbeSensor((0, 0, 0), np.zeros((3, 3))), one, ProbeSensor((0, 0, 0), np.zeros((70, 3)))], gradient=True)
    assert ps.n_probes == 74 and ps.gradient and ps.sensor_slices() == {0: slice(0, 3), 1: slice(3, 4), 2: slice(4, 74)} and "74 probes" in repr(ps)
    assert ProbeSet(one).n_probes == 1 and not ProbeSet(one).gradient  # a single sensor is a set of one
    ProbeSet([one] * MAX_SENSORS)
    ProbeSet([ProbeSensor((0, 0, 0), np.zeros((MAX_PROBES, 3)))])
    m = load_compiled("Sawyer", "table_lack_0825")
    with pytest.raises(ValueError, match="unknown body"):
        sensor_table(m, ProbeSet([ProbeSensor((0, 0, 0), P0, body="no_such_body")]))
    with pytest.raises(ValueError, match="names geom"):
        sensor_table(m, ProbeSet([ProbeSensor((0, 0, 0), P0, exclude=[10000])]))


def test_grid_points():
    g = grid_points((0.0, -1.0, 2.0), (4.0, 1.0, 3.0), (4, 2, 1))
    assert g.shape == (8, 3) and g.dtype == np.float64
    assert g.tolist() == [[0.5, -0.5, 2.5], [0.5, 0.5, 2.5], [1.5, -0.5, 2.5], [1.5, 0.5, 2.5], [2.5, -0.5, 2.5], [2.5, 0.5, 2.5], [3.5, -0.5, 2.5], [3.5, 0.5, 2.5]]
    big = grid_points((-0.12, -0.12, -0.05), (0.12, 0.12, 0.25), (8, 8, 8)).reshape(8, 8, 8, 3)  # x outer: reshapes to (nx, ny, nz)
    assert np.allclose(big[3, :, :, 0], -0.12 + 3.5 * 0.03) and np.allclose(big[:, 5, :, 1], -0.12 + 5.5 * 0.03) and np.allclose(big[:, :, 0, 2], -0.05 + 0.5 * 0.0375)
    for bad in (dict(shape=(2, 2)), dict(shape=(2, 0, 2)), dict(shape=(2, 2.5, 2)), dict(hi=(1.0, 1.0, 0.0)), dict(lo=(0.0, float("nan"), 0.0))):
        args = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), shape=(2, 2, 2))
        args.update(bad)
        with pytest.raises(ValueError):
            grid_points(**args)


# ---- the "body" exclusion rule (furniture_amd.rays.exclude_mask, reused) -----------------------------------------------------------------
def test_body_exclusion_rule():
    m = load_compiled("Sawyer", "table_lack_0825")
    hand = ProbeSensor((0, 0, 0), np.zeros((2, 3)), body="right_hand", dmax=0.3)
    mask = exclude_mask(m, hand)
    cg = np.asarray(m.arrays["cg_orig"])
    gbody = np.asarray(m.arrays["geom_bodyid"])[cg]
    names = m.meta["body_names"]
    want = np.isin(gbody, [names.index("right_l6"), names.index("right_gripper_base")])
    assert want.sum() >= 2 and np.array_equal(mask, want)  # exactly the colliding geoms that move rigidly with the hand
    assert not exclude_mask(m, ProbeSensor((0, 0, 1), P0)).any()  # a world sensor
    assert not exclude_mask(m, ProbeSensor((0, 0, 0), P0, body="right_hand", exclude=None)).any()
    some = [int(cg[3]), int(cg[5])]
    assert np.nonzero(exclude_mask(m, ProbeSensor((0, 0, 0), P0, exclude=some)))[0].tolist() == [3, 5]
    tab, pts = sensor_table(m, ProbeSet([hand, ProbeSensor((0, 0, 1), np.ones((5, 3)), dmax=2.0)]))
    bits = sum(int(tab[0].exclude[j]) << (32 * j) for j in range(3))
    assert [k for k in range(96) if bits >> k & 1] == np.nonzero(mask)[0].tolist()
    assert list(tab[1].exclude) == [0, 0, 0] and (tab[1].first_probe, tab[1].n_probes, tab[1].body, tab[1].dmax) == (2, 5, -1, 2.0)
    assert (tab[0].first_probe, tab[0].n_probes, tab[0].body) == (0, 2, names.index("right_hand")) and abs(tab[0].dmax - 0.3) < 1e-7
    assert pts.shape == (7, 3) and pts.dtype == np.float32 and pts[:2].tolist() == [[0.0] * 3] * 2 and pts[2:].tolist() == [[1.0] * 3] * 5
    # a cursor is welded to the world: only its own geom, not the floor
    mc = load_compiled("Cursor", "toy_table")
    cur = ProbeSensor((0, 0, 0), P0, body="cursor0")
    assert int(mc.arrays["body_red"][cur.body_id(mc)]) == 0
    cgc = np.asarray(mc.arrays["cg_orig"])
    assert [mc.meta["body_names"][int(mc.arrays["geom_bodyid"][int(g)])] for g in cgc[exclude_mask(mc, cur)]] == ["cursor0"]


# ---- the reference on hand-made scenes with closed-form answers ---------------------------------------------------------------------
def _geom(gid, gtype, size, pos=(0.0, 0.0, 0.0), mat=None, **kw):
    return dict(id=gid, type=gtype, size=np.asarray(size, dtype=np.float64), pos=np.asarray(pos, dtype=np.float64), mat=np.eye(3) if mat is None else mat, **kw)


def _one(geom, pts, dmax=10.0):
    r = pref.distance(np.asarray(pts, dtype=np.float64), [geom], dmax)
    assert (r["geom"] == geom["id"]).all()
    return r["dist"], r["grad"], r["flat"]


S2, S3 = np.sqrt(2.0), np.sqrt(3.0)


def test_reference_plane_sphere_capsule():
    d, g, f = _one(_geom(0, cref.PLANE, (0, 0, 0), (0, 0, -1.0)), [(3.0, 4.0, 0.5), (0.0, 0.0, -1.25)])
    assert np.allclose(d, [1.5, -0.25]) and np.allclose(g, [(0, 0, 1)] * 2) and f.all()
    d, g, f = _one(_geom(4, cref.SPHERE, (0.5, 0, 0), (1.0, 0, 0)), [(4.0, 4.0, 0.0), (1.0, 0.0, 0.3), (1.0, 0.0, 0.0)])
    assert np.allclose(d, [4.5, -0.2, -0.5]) and np.allclose(g, [(0.6, 0.8, 0), (0, 0, 1), (1, 0, 0)]) and not f.any()  # the centre: the local +x
    cap = _geom(2, cref.CAPSULE, (0.1, 0.4, 0))
    d, g, f = _one(cap, [(0.5, 0.0, 0.2), (0.0, 0.3, 0.8), (0.0, 0.0, 0.45), (0.05, 0.0, -0.1), (0.0, 0.0, 0.1), (0.3, 0.0, 0.8)])
    assert np.allclose(d, [0.4, 0.4, -0.05, -0.05, -0.1, 0.4])
    assert np.allclose(g, [(1, 0, 0), (0, 0.6, 0.8), (0, 0, 1), (1, 0, 0), (1, 0, 0), (0.6, 0, 0.8)]) and not f.any()  # on the axis: the local +x


def test_reference_cylinder():
    cyl = _geom(5, cref.CYLINDER, (0.5, 1.0, 0))
    pts = [(2.0, 0.0, 0.3),     # outside the side
           (0.0, 0.2, -1.5),    # outside a cap
           (0.8, 0.0, 1.4),     # outside the rim: dr = 0.3, dz = 0.4
           (0.0, 0.4, 0.0),     # inside, nearest the side
           (0.1, 0.0, -0.95),   # inside, nearest the bottom cap
           (0.25, 0.0, 0.75),   # inside, the tie dr = dz = -0.25 (exact in binary): the side
           (0.0, 0.0, 0.2)]     # on the axis, nearest the side: the local +x
    d, g, f = _one(cyl, pts)
    assert np.allclose(d, [1.5, 0.5, 0.5, -0.1, -0.05, -0.25, -0.5])
    assert np.allclose(g, [(1, 0, 0), (0, 0, -1), (0.6, 0, 0.8), (0, 1, 0), (0, 0, -1), (1, 0, 0), (1, 0, 0)])
    assert f.tolist() == [False, True, False, False, True, False, False]


def test_reference_box():
    box = _geom(7, cref.BOX, (1.0, 2.0, 3.0))
    pts = [(1.5, 0.5, -1.0),    # outside a face
           (-1.3, 2.4, 0.0),    # outside an edge: (0.3, 0.4, 0)
           (2.0, 4.0, -5.0),    # outside a corner: (1, 2, 2)
           (0.5, -1.9, 0.0),    # inside, nearest -y
           (0.0, 1.0, 2.0),     # inside, the three-way tie a = -1: the smallest axis, +x (sign(0) = +1)
           (-0.2, 1.5, 2.5),    # inside, the tie of y and z at -0.5: y
           (0.0, 0.0, 0.0)]     # the centre: x is nearest
    d, g, f = _one(box, pts)
    assert np.allclose(d, [0.5, 0.5, 3.0, -0.1, -1.0, -0.5, -1.0])
    assert np.allclose(g, [(1, 0, 0), (-0.6, 0.8, 0), (1 / 3, 2 / 3, -2 / 3), (0, -1, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0)])
    assert f.tolist() == [True, False, False, True, True, True, True]
    # at any pose: the gradient turns with the box, and p - dist * grad is the nearest surface point
    rng = np.random.RandomState(5)
    q = rng.normal(size=4)
    R = quat_to_mat(q / np.linalg.norm(q))
    pos = np.array([0.4, -0.3, 0.2])
    world = np.asarray(pts) @ R.T + pos
    r = pref.distance(world, [_geom(7, cref.BOX, (1.0, 2.0, 3.0), pos, R)], 10.0)
    assert np.allclose(r["dist"], d) and np.allclose(r["grad"], g @ R.T)
    near = (world - r["dist"][:, None] * r["grad"] - pos) @ R
    assert np.allclose(np.abs(np.abs(near) - (1.0, 2.0, 3.0)).min(axis=1), 0.0, atol=1e-12) and (np.abs(near) <= np.array([1.0, 2.0, 3.0]) + 1e-12).all()


def test_reference_hull_is_the_plane_bound():
    half = np.array([0.3, 0.2, 0.4])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * half
    hull = _geom(1, cref.MESH, (0, 0, 0), halfspaces=cref.mesh_halfspaces(corners))
    box = _geom(1, cref.BOX, half)
    pts = np.array([(0.5, 0.0, 0.1), (0.1, 0.05, 0.1), (0.0, 0.1, -0.35), (0.6, 0.6, 0.0), (0.5, 0.4, 0.7)])  # a face, inside twice, an edge, a corner
    dh, gh, fh = _one(hull, pts)
    db, gb, _ = _one(box, pts)
    assert fh.all() and np.allclose(dh[:3], db[:3]) and np.allclose(gh[:3], gb[:3])  # exact inside and outside a face
    assert np.allclose(dh[3:], [0.4, 0.3]) and np.allclose(db[3:], [0.5, np.sqrt(0.04 + 0.04 + 0.09)])  # the bound: the largest plane excess
    assert (dh[3:] < db[3:]).all() and np.allclose(gh[3], (0, 1, 0)) and np.allclose(gh[4], (0, 0, 1))


def test_reference_winner_exclusion_and_dmax():
    near = _geom(4, cref.SPHERE, (0.5, 0, 0), (1.0, 0, 0))
    far = _geom(7, cref.BOX, (0.5, 0.5, 0.5), (-3.0, 0, 0))
    p = [(0.0, 0.0, 0.0)]
    r = pref.distance(p, [near, far], 10.0)
    assert r["geom"].tolist() == [4] and np.allclose(r["dist"], [0.5]) and np.allclose(r["grad"], [(-1, 0, 0)]) and r["type"].tolist() == [cref.SPHERE]
    r = pref.distance(p, [near, far], 10.0, skip=[4])  # the nearer one is invisible
    assert r["geom"].tolist() == [7] and np.allclose(r["dist"], [2.5]) and np.allclose(r["grad"], [(1, 0, 0)]) and r["flat"].all()
    r = pref.distance(p, [near, far], 0.4)  # nothing within dmax
    assert r["geom"].tolist() == [-1] and r["dist"].tolist() == [0.4] and (r["grad"] == 0).all() and r["type"].tolist() == [-1] and not r["near_range"].any()
    assert np.allclose(r["raw"], [0.5])
    assert pref.distance(p, [near, far], 0.5)["geom"].tolist() == [4] and pref.distance(p, [near, far], 0.5)["near_range"].all()  # accepted at <= dmax
    assert pref.distance(p, [near, far], 0.50005)["near_range"].all() and pref.distance(p, [near, far], 0.49995)["near_range"].all()
    # a tie between two geoms: the first in the list
    left = _geom(9, cref.SPHERE, (0.5, 0, 0), (-1.0, 0, 0))
    assert pref.distance(p, [near, left], 10.0)["geom"].tolist() == [4] and pref.distance(p, [left, near], 10.0)["geom"].tolist() == [9]
    # inside one solid and outside another: the negative distance wins
    r = pref.distance([(0.9, 0.0, 0.0)], [far, near], 10.0)
    assert r["geom"].tolist() == [4] and np.allclose(r["dist"], [-0.4])
    # flags: halfway between two spheres the label is ambiguous; near a box edge the gradient is unstable; elsewhere neither
    amb, uns = pref.flags([(0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.3, 2.0, 0.0)], [near, left], 10.0)
    assert amb.tolist() == [True, False, False] and uns.tolist() == [True, False, False]
    box = _geom(7, cref.BOX, (1.0, 1.0, 1.0))
    amb, uns = pref.flags([(1.5, 1.00001, 0.0), (1.5, 0.5, 0.0), (1.004, 1.003, 0.0), (1.5, 1.5, 0.0)], [box], 10.0)
    assert not amb.any() and uns.tolist() == [False, False, True, False]  # (0.5 m from the edge a 1e-4 m step turns the gradient by 2e-4 rad)


# ---- chair_agne_0010's hull: the plane bound against the exact distance ----------------------------------------------------------------
def test_plane_bound_against_exact_distance_on_a_real_hull():
    m = load_compiled("Sawyer", "chair_agne_0010")
    A = m.arrays
    g = [int(k) for k in np.asarray(A["cg_orig"]) if int(A["geom_type"][int(k)]) == cref.MESH][0]  # the colliding hull
    a, n = int(A["geom_meshadr"][g]), int(A["geom_meshnum"][g])
    verts = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)[a:a + n]
    hs = cref.mesh_halfspaces(verts)
    lo, hi = verts.min(0), verts.max(0)
    rng = np.random.RandomState(7)
    pts = rng.uniform(lo - 0.3 * (hi - lo) - 0.02, hi + 0.3 * (hi - lo) + 0.02, (1500, 3))
    bound, _, flat = pref.local_distance(cref.MESH, np.zeros(3), pts, hs)
    exact, interior = pref.hull_exact_distance(pts, verts, hs)
    inside = exact < 0
    assert inside.sum() > 30 and (~inside & interior).sum() > 100 and (~inside & ~interior).sum() > 100 and flat.all()
    assert (bound <= exact + 1e-9).all()  # a lower bound everywhere
    assert np.abs(bound[inside] - exact[inside]).max() < 1e-9  # exact inside
    face = ~inside & interior
    assert np.abs(bound[face] - exact[face]).max() < 1e-9  # exact where the nearest point is in a facet's interior
    assert (exact - bound)[~inside & ~interior].max() > 1e-3  # and really smaller somewhere near an edge or a vertex


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = ProbeSet([ProbeSensor((0, 0, 1), grid_points((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1), (2, 2, 2)))])
    with pytest.raises(TypeError, match="ProbeSet"):
        FurnitureBatchEnv("Sawyer", 1, probes=[ProbeSensor((0, 0, 1), P0)])
    with pytest.raises(NotImplementedError, match="probes= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, probes=spec)
    with pytest.raises(NotImplementedError, match="probes= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(probes=spec))

    class _Handle:  # a handle with a probe set and nothing else
        cameras, points, voxels, normals, flow, rays, probes = None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="distance-probe outputs"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_probes_header_symbols_are_exported():
    assert sim.PROBE_SYMBOLS == ["fsim_set_probes", "fsim_probe_distance"]
    assert sorted(_declared("fsim_probes.h")) == sorted(sim.PROBE_SYMBOLS)
    others = set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS) | set(sim.VOXELS_SYMBOLS) | set(sim.NORMALS_SYMBOLS) | set(sim.FLOW_SYMBOLS) | set(sim.RAY_SYMBOLS)
    assert not set(sim.PROBE_SYMBOLS) & others
    assert not set(sim.PROBE_SYMBOLS) & set().union(*[_declared(h) for h in ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h", "fsim_rays.h")])
    lib = ctypes.CDLL(sim.build())
    for n in sim.PROBE_SYMBOLS:
        assert hasattr(lib, n), n


def test_probes_header_is_plain_c11_and_the_struct_matches(tmp_path):
    fields = [n for n, _ in sim.FsimProbeSensor._fields_]
    src = tmp_path / "use_probes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fsim_probes.h"\n'
                   "int use(fsim_t *s, const fsim_probe_sensor_t *k, const float *d, float *o) { return fsim_set_probes(s, 1, k, 1, d, 0, 0, 0, 0) + fsim_probe_distance(s, o, 0, 0); }\n"
                   'int main(void) { printf("%zu %d %d", sizeof(fsim_probe_sensor_t), FSIM_PROBE_MAX_SENSORS, FSIM_PROBE_MAX_PROBES);\n' +
                   "".join('  printf(" %%zu", offsetof(fsim_probe_sensor_t, %s));\n' % f for f in fields) + "  return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_probes.o")])
    # the layout: a program that defines the two entry points itself prints sizeof and every offsetof
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_probes.h"\nint fsim_set_probes(fsim_t *s, int a, const fsim_probe_sensor_t *k, int b, const float *d, int c, const float *p, const int32_t *x, '
                    "const int32_t *y) { (void)s; (void)k; (void)d; (void)p; (void)x; (void)y; return a + b + c; }\n"
                    "int fsim_probe_distance(fsim_t *s, float *a, int32_t *b, float *c) { (void)s; (void)a; (void)b; (void)c; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [ctypes.sizeof(sim.FsimProbeSensor), MAX_SENSORS, MAX_PROBES] and got[0] == 56
    assert got[3:] == [getattr(sim.FsimProbeSensor, f).offset for f in fields]


def test_probes_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_probes.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("p = o + R_s * pt", "cursor offset is added for a sensor on a cursor body", "d = q.z; gradient +z", "d = |q| - r; gradient q / |q|",
              "clamp(q.z, -h, h)", "d = hypot(max(dr, 0), max(dz, 0))", "the side wins a tie", "d = |max(a, 0)|", "the smallest axis wins a tie",
              "the PLANE BOUND d = max_i (n_i . q - c_i)", "the smallest plane index wins a tie", "This is exact inside the hull and wherever the nearest feature is a face.",
              "It is a lower bound near edges and vertices outside.", "the unit vector is the geom's local +x", "The gradient goes to the world frame with R_geom",
              "the smallest signed distance wins; a strict < in colliding-geom order settles ties", "accepted when its distance is <= dmax",
              "dist = dmax, geom = -1, grad = (0, 0, 0)", "the nearest surface point is p - dist * grad", "in the numbering of the segmentation image",
              "writes no state, RNG draw, look-ahead shadow or counter", "depends only on its own record and the probe set",
              "Without probes set, nothing is allocated or launched", "n_sensors == 0 clears", "keeps its own copy", "a non-finite point",
              "a dmax that is not 0 < dmax < inf", "waits for the handle's stream before it replaces the tables", "any may be NULL, not all",
              "settled exactly as fsim_cast_rays settles it", "returns without waiting"):
        assert s in flat, s

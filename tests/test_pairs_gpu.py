"""Geom-pair distance sensors on the device (include/fsim_pairs.h) through the library, against the float64 reference
tests/collide_reference.py evaluated at the oracle's poses of the device's own qpos: gripper against each part, every part against every
other, floor against gripper, all arm links against all parts, and a short-range sensor that sees nothing, in states whose reference can
be evaluated beforehand and after a reset and 30 steps; outputs one at a time, pair counts that end mid-wave, independence of the other
sensors and of the batch, read-only evaluation, the env surface, the C-ABI's error paths and a cross-check with the distance probes.
FSIM_TEST_POISON=<hex> also fills every CU's LDS with the pattern before each call.

What is compared.  The states hold exact ties (two pairs at the same distance), touching parts and overlaps, so nothing depends on WHICH
pair wins: the distance is held against the reference minimum over the sensor's pairs and against the reference gap of the pair the device
names.  Reference minimum > 2e-4: the bound of rays and probes, 1e-4 |ref| + 1e-5, the separation along the device's normal, the witness
points.  < -2e-4: the portal assertions of tests/test_pairs_tool_gpu.py (never shallower than the true depth).  In between (touching):
|dist| <= 2e-4 + tol."""
import ctypes

import numpy as np
import pytest
import torch

from furniture_amd.envs import FurnitureBatchEnv
from furniture_amd.pairs import PairSensor, PairSet, gripper_bodies
from furniture_amd.probes import ProbeSensor, ProbeSet
from furniture_amd.sim import FSim, FsimError, FsimPairSensor, lib
from oracle.oracle_sim import OracleSim
from tests import collide_reference as cr
from tests.collide_reference import MESH, PLANE, Shapes
from tests.test_camera_gpu import _make, _poison, _steps
from tests.test_pairs_tool_gpu import PORTAL_TOL, POS_TOL, dist_bound, radii
from tests.test_rays_gpu import _bent, _device_state, _pose_oracle

pytestmark = pytest.mark.gpu
MODELS = [("Sawyer", "table_lack_0825"), ("Sawyer", "chair_agne_0010"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table")]
TOUCH = 2e-4
NDIR = 4000  # (signed_gap at 4 000 and at 40 000 directions agree within 5e-11 on every robot-to-part pair of the four models)


def _pairs(sim, **kw):
    _poison()
    res = sim.pair_distance(**kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _arm_bodies(m):
    """every robot body that carries a collider and moves (the arm links and the gripper)"""
    A = m.arrays
    cg = np.asarray(A["cg_orig"])
    gbody = np.asarray(A["geom_bodyid"])[cg]
    red = np.asarray(A["body_red"])
    rob = np.asarray(A["cg_isrobot"]) != 0
    return [m.meta["body_names"][b] for b in sorted(set(gbody[rob & (red[gbody] != 0)].tolist()))]


def _part_bodies(m):
    A = m.arrays
    cg = np.asarray(A["cg_orig"])
    gbody = np.asarray(A["geom_bodyid"])[cg]
    pid = np.asarray(A["cg_partid"])
    return [m.meta["body_names"][int(gbody[pid == p][0])] for p in sorted(set(pid[pid >= 0].tolist()))]


def _sensors(m):
    """the sensors of the issue: gripper (or cursor0) against each part, every part against every other, floor against gripper, all arm
    links against all parts (dmax 2), one more gripper-to-part sensor with dmax 0.2"""
    parts = _part_bodies(m)
    grip = ["cursor0"] if m.meta["agent"] == "Cursor" else gripper_bodies(m)
    arm = ["cursor0", "cursor1"] if m.meta["agent"] == "Cursor" else _arm_bodies(m)
    out = [PairSensor(grip, p, dmax=3.0) for p in parts]
    out += [PairSensor(parts[i], parts[j], dmax=3.0) for i in range(len(parts)) for j in range(i + 1, len(parts))]
    # (the short-range sensor looks at a part that is more than 0.25 m from the gripper in the known states: the reference alone puts parts 0 - 2
    # of toy_table at 0.13, 0.02 and 0.13 m from cursor0, part 3 at 0.36 m)
    out += [PairSensor("world", grip, dmax=3.0), PairSensor(arm, parts, dmax=2.0), PairSensor(grip, parts[3 if m.meta["agent"] == "Cursor" else 0], dmax=0.2)]
    return out


def _shapes(geoms, idx):
    """tests.collide_reference.Shapes of the colliding geoms idx (all of one type; hulls: of one geom)"""
    g0 = geoms[idx[0]]
    verts = g0["verts"] if g0["type"] == MESH else None
    return Shapes(g0["type"], [geoms[k]["pos"] for k in idx], [geoms[k]["mat"] for k in idx], [geoms[k]["size"] for k in idx], verts)


def _with_verts(m, geoms):
    A = m.arrays
    for g in geoms:
        if g["type"] == MESH:
            a, n = int(A["geom_meshadr"][g["id"]]), int(A["geom_meshnum"][g["id"]])
            g["verts"] = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)[a:a + n]
    return geoms


def _reference_gaps(geoms, pairs):
    """{(g1, g2): (gap, A, B)} for colliding-geom index pairs, one signed_gap call per (type, type, hull) group"""
    groups = {}
    for (g1, g2) in sorted(set(pairs)):
        a, b = geoms[g1], geoms[g2]
        swap = b["type"] == PLANE  # (the reference takes a plane as its first shape; the gap is symmetric)
        key = (b["type"], a["type"], g2 if b["type"] == MESH else -1, g1 if a["type"] == MESH else -1) if swap else (a["type"], b["type"], g1 if a["type"] == MESH else -1, g2 if b["type"] == MESH else -1)
        groups.setdefault((key, swap), []).append((g1, g2))
    out = {}
    for (key, swap), lst in groups.items():
        A = _shapes(geoms, [p[1] if swap else p[0] for p in lst])
        B = _shapes(geoms, [p[0] if swap else p[1] for p in lst])
        gap = cr.signed_gap(A, B, ndir=NDIR)
        for i, p in enumerate(lst):
            out[p] = gap[i]
    return out


def _one(geoms, g):
    return _shapes(geoms, [g])


def _check_env(m, sensors, got, e, geoms, tag):
    """every sensor of one env against the reference -> the list of (sensor, reference minimum, device distance)"""
    cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
    lists = [s.pairs(m) for s in sensors]
    ref = _reference_gaps(geoms, [p for l in lists for p in l])
    rows = []
    for i, (s, pl) in enumerate(zip(sensors, lists)):
        where = "%s env %d sensor %d %r" % (tag, e, i, s)
        d, gg, ft, n = float(got["pair_distance"][e, i]), got["pair_geoms"][e, i], got["pair_fromto"][e, i].astype(np.float64), got["pair_normal"][e, i].astype(np.float64)
        rmin = min(ref[p] for p in pl)
        rows.append((i, rmin, d))
        miss = gg[0] < 0
        assert miss == (gg[1] < 0) and miss == (d == np.float32(s.dmax)) and miss == bool((ft == 0).all() and (n == 0).all()), "%s: geoms < 0, dist == dmax and zero vectors disagree (%s, %g)" % (where, gg, d)
        if rmin > s.dmax + dist_bound(s.dmax):
            assert miss, "%s: the nearest pair is %.4f away, beyond dmax, yet dist %.6f" % (where, rmin, d)
            continue
        assert not miss, "%s: the reference minimum is %.6f, the device reports nothing" % (where, rmin)
        ma, mb = s.side_masks(m)
        g1, g2 = cg.index(int(gg[0])), cg.index(int(gg[1]))
        assert ma[g1] and mb[g2] and (g1, g2) in ref, "%s: names geoms %s, not a pair of its sides" % (where, gg)
        assert abs(np.linalg.norm(n) - 1.0) <= 1e-5, "%s: a normal of length %.7f" % (where, np.linalg.norm(n))
        rnamed = ref[g1, g2]
        A, B = _one(geoms, g1), _one(geoms, g2)
        plane_b = B.type == PLANE
        sep = cr.separation_along(B, A, -n[None])[0] if plane_b else cr.separation_along(A, B, n[None])[0]
        dv = np.linalg.norm(ft[3:] - ft[:3] - d * n)
        if rmin > TOUCH:
            for r, what in ((rmin, "the minimum over its pairs"), (rnamed, "the gap of the pair it names")):
                assert abs(d - r) <= dist_bound(r), "%s: dist %.9g, %s %.9g" % (where, d, what, r)
            assert abs(sep - d) <= dist_bound(d), "%s: the geoms leave %.9g along the device's normal, dist is %.9g" % (where, sep, d)
            da, db = abs(cr.point_depth(A, ft[None, None, :3])[0, 0]), abs(cr.point_depth(B, ft[None, None, 3:])[0, 0])
            assert max(da, db, dv) <= POS_TOL, "%s: from is %.3e off its geom, to %.3e, to - from - dist * normal %.3e" % (where, da, db, dv)
        elif rmin < -TOUCH:
            assert d < 0 and d <= rmin + PORTAL_TOL, "%s: dist %.9g is shallower than the true depth %.9g" % (where, d, rmin)
            assert dv <= POS_TOL, "%s: to - from - dist * normal %.3e" % (where, dv)
            # the pair the device names: its cores are apart (the reference decides, as in tests/test_pairs_tool_gpu.py (b); a plane pair
            # is a closed form) -> the two-sided bound of (a); its cores intersect -> the portal answer, consistent with its own normal
            if PLANE in (A.type, B.type) or rnamed + radii(A)[0] + radii(B)[0] > 0:
                for r, what in ((rmin, "the minimum over its pairs"), (rnamed, "the gap of the pair it names")):
                    assert abs(d - r) <= dist_bound(r), "%s: cores apart: dist %.9g, %s %.9g" % (where, d, what, r)
                assert abs(sep - d) <= dist_bound(d), "%s: the geoms leave %.9g along the device's normal, dist is %.9g" % (where, sep, d)
                da, db = abs(cr.point_depth(A, ft[None, None, :3])[0, 0]), abs(cr.point_depth(B, ft[None, None, 3:])[0, 0])
                assert max(da, db) <= POS_TOL, "%s: from is %.3e off its geom, to %.3e" % (where, da, db)
            else:
                assert abs(sep - d) <= PORTAL_TOL, "%s: the geoms leave %.9g along the device's normal, dist is %.9g" % (where, sep, d)
        else:
            assert abs(d) <= TOUCH + PORTAL_TOL, "%s: a touching pair (reference %.3e) with dist %.6g" % (where, rmin, d)
    return rows


def _known_states(m, sim):
    q = sim.get_state("qpos")["qpos"]
    q[0] = torch.as_tensor(np.asarray(m.arrays["qpos0"], dtype=np.float32), device=q.device)
    q[1] = torch.as_tensor(_bent(m).astype(np.float32), device=q.device)
    sim.set_state(qpos=q)


def _check(m, sim, sensors, envs, tag):
    sim.set_pairs(PairSet(sensors, fromto=True, normal=True))
    got = _pairs(sim)
    qpos, cursor = _device_state(m, sim)
    osim = OracleSim(m)
    rows = {}
    for e in envs:
        geoms = _with_verts(m, _pose_oracle(osim, m, qpos, cursor, e))
        rows[e] = _check_env(m, sensors, got, e, geoms, tag)
        print("%s env %d: reference minima %s" % (tag, e, " ".join("%.4f" % r[1] for r in rows[e])))
    osim.close()
    return got, rows


# ---- 1. against the reference in states known beforehand -------------------------------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", MODELS)
def test_sensors_match_reference_in_known_states(agent, furniture):
    m, sim = _make(agent, furniture, 2)
    _known_states(m, sim)
    sensors = _sensors(m)
    got, rows = _check(m, sim, sensors, range(2), furniture)
    for e in range(2):
        mins = np.array([r[1] for r in rows[e]])
        assert got["pair_geoms"][e, -1, 0] == -1 and got["pair_distance"][e, -1] == np.float32(0.2)  # the short-range sensor: nothing within 0.2 m
        assert (got["pair_geoms"][e, :-1] >= 0).all()  # no other sensor is near its dmax
        print("%s env %d: %d sensors apart, %d touching, %d overlapping" % (furniture, e, (mins > TOUCH).sum(), (np.abs(mins) <= TOUCH).sum(), (mins < -TOUCH).sum()))
    print("%s: %d sensors, reference minima from %.4f to %.4f" % (furniture, len(sensors), min(r[1] for r in rows[0]), max(r[1] for r in rows[0])))
    sim.close()


# ---- 2. the same checks after a reset and 30 random steps -----------------------------------------------------------------------------
def test_sensors_match_reference_after_reset_and_steps():
    m, sim = _make("Sawyer", "table_lack_0825", 8)
    sensors = _sensors(m)
    _check(m, sim, sensors, range(8), "lack reset")
    _steps(sim, 30)
    got, _ = _check(m, sim, sensors, range(8), "lack 30 steps")
    assert len({got["pair_distance"][e].tobytes() for e in range(8)}) == 8
    sim.close()


# ---- 3. outputs, counts, independence ------------------------------------------------------------------------------------------------
def test_each_output_alone_and_out_buffers():
    m, sim = _make("Sawyer", "table_lack_0825", 3)
    sim.set_pairs(PairSet(_sensors(m), fromto=True, normal=True))
    full = _pairs(sim)
    shapes = sim.pair_shapes()
    assert sorted(shapes) == ["pair_distance", "pair_fromto", "pair_geoms", "pair_normal"]
    for k, (sh, dt) in shapes.items():
        buf = torch.full((3,) + sh, 77, dtype=dt, device=sim.device)
        res = _pairs(sim, out={k: buf})
        assert list(res) == [k] and np.array_equal(res[k], full[k]) and np.array_equal(buf.cpu().numpy(), full[k]), k
    with pytest.raises(ValueError, match="out holds"):
        sim.pair_distance(out={})
    with pytest.raises(ValueError, match="out holds"):
        sim.pair_distance(out={"pair_depth": torch.zeros(3, device=sim.device)})
    with pytest.raises(ValueError, match="not a contiguous"):
        sim.pair_distance(out={"pair_distance": torch.zeros((3, 1), device=sim.device)})
    sim.set_pairs(PairSet(_sensors(m)))
    assert sorted(sim.pair_shapes()) == ["pair_distance", "pair_geoms"] and sorted(_pairs(sim)) == ["pair_distance", "pair_geoms"]
    sim.set_pairs(None)
    with pytest.raises(FsimError, match="no pair set"):
        sim.pair_distance()
    sim.close()


def _brute(m, sim, sensor):
    """the sensor's answer from one single-pair sensor per pair (which the prune cannot touch), reduced on the host by the header's rule"""
    cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
    pl = sensor.pairs(m)
    best = None
    for c0 in range(0, len(pl), 64):
        chunk = pl[c0:c0 + 64]
        sim.set_pairs(PairSet([PairSensor([cg[a]], [cg[b]], dmax=sensor.dmax) for a, b in chunk], fromto=True, normal=True))
        one = _pairs(sim)
        for j in range(len(chunk)):
            if one["pair_geoms"][0, j, 0] >= 0 and (best is None or one["pair_distance"][0, j] < best[0]):
                best = (one["pair_distance"][0, j], one["pair_geoms"][0, j].copy(), one["pair_fromto"][0, j].copy(), one["pair_normal"][0, j].copy())
    return best


@pytest.mark.parametrize("agent,furniture,count", [("Sawyer", "table_lack_0825", 1), ("Sawyer", "table_lack_0825", 65), ("Cursor", "toy_table", 41 * 7)])
def test_pair_counts_that_end_mid_wave(agent, furniture, count):
    """1, 65 and 41 x 7 pairs: the chunked walk, its prune and the tie rule against one single-pair sensor per pair, bit for bit"""
    m, sim = _make(agent, furniture, 1)
    cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
    if count == 1:
        s = PairSensor([cg[12]], [cg[22]], dmax=3.0)
    elif count == 65:
        s = PairSensor(cg[1:14], cg[22:27], dmax=3.0)  # 13 robot geoms x 5 parts
    else:
        pid = np.asarray(m.arrays["cg_partid"])
        s = PairSensor([cg[k] for k in np.nonzero(pid == 1)[0]], [cg[k] for k in np.nonzero((pid >= 0) & (pid != 1))[0][:7]], dmax=3.0)
    assert len(s.pairs(m)) == count
    want = _brute(m, sim, s)
    sim.set_pairs(PairSet(s, fromto=True, normal=True))
    got = _pairs(sim)
    assert want is not None and got["pair_distance"][0, 0] == want[0] and np.array_equal(got["pair_geoms"][0, 0], want[1])
    assert np.array_equal(got["pair_fromto"][0, 0], want[2]) and np.array_equal(got["pair_normal"][0, 0], want[3])
    sim.close()


def test_sensor_alone_and_env_alone_are_bit_identical():
    m, sim = _make("Sawyer", "chair_agne_0010", 8)
    _steps(sim, 3)
    sensors = _sensors(m)
    sim.set_pairs(PairSet(sensors, fromto=True, normal=True))
    full = _pairs(sim)
    for i in (0, len(sensors) // 2, len(sensors) - 2):  # a sensor of the set is the same sensor alone
        sim.set_pairs(PairSet(sensors[i], fromto=True, normal=True))
        one = _pairs(sim)
        for k in full:
            assert one[k][:, 0].tobytes() == np.ascontiguousarray(full[k][:, i]).tobytes(), (i, k)
    state = sim.get_state("qpos")["qpos"]
    alone = FSim(m, 1, config=sim.cfg)
    alone.set_pairs(PairSet(sensors, fromto=True, normal=True))
    for e in range(8):  # an env of the batch is the same state alone
        alone.set_state(qpos=state[e:e + 1])
        one = _pairs(alone)
        for k in full:
            assert one[k][0].tobytes() == full[k][e].tobytes(), (e, k)
    assert len({full["pair_distance"][e].tobytes() for e in range(8)}) == 8  # the envs differ
    alone.close()
    sim.close()


# ---- 4. read-only evaluation ----------------------------------------------------------------------------------------------------------
def _all_state(sim):
    return {k: v.cpu().numpy().copy() for k, v in sim.get_state().items()}


def test_evaluation_is_read_only():
    from furniture_amd.rays import RaySensor, RaySet, lidar
    from tests.test_camera_gpu import _cameras
    m, sim = _make("Sawyer", "table_lack_0825", 4)
    _, twin = _make("Sawyer", "table_lack_0825", 4)
    _steps(sim, 3)
    _steps(twin, 3)
    qpos, _ = _device_state(m, sim)
    cams = _cameras(m, qpos[0].astype(np.float32), "right_hand")
    rays = RaySet([RaySensor((0.0, 0.0, 0.0), lidar(64, 4, elevation=(-60.0, 60.0)), body="right_hand", tmax=3.0)], normal=True)
    probes = ProbeSet([ProbeSensor((0.3, 0.0, 0.3), np.random.RandomState(0).uniform(-0.3, 0.3, (70, 3)))], gradient=True)
    for s_ in (sim, twin):
        s_.set_cameras(cams)
        s_.set_rays(rays)
        s_.set_probes(probes)
    plain = [t.cpu().numpy() for t in twin.render()] + [v.cpu().numpy() for _, v in sorted(twin.cast_rays().items())] + [v.cpu().numpy() for _, v in sorted(twin.probe_distance().items())]
    sim.set_pairs(PairSet(_sensors(m), fromto=True, normal=True))
    before = _all_state(sim)  # the whole record
    first = _pairs(sim)
    _pairs(sim, out={"pair_geoms": torch.empty((4, len(sim.pairs.sensors), 2), dtype=torch.int32, device=sim.device)})
    after = _all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    # fsim_render, fsim_cast_rays and fsim_probe_distance with a pair set are what they are without
    with_pairs = [t.cpu().numpy() for t in sim.render()] + [v.cpu().numpy() for _, v in sorted(sim.cast_rays().items())] + [v.cpu().numpy() for _, v in sorted(sim.probe_distance().items())]
    assert len(plain) == len(with_pairs) and all(a.tobytes() == b.tobytes() for a, b in zip(plain, with_pairs))
    again = _pairs(sim)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    # a step after a call == the same step without one, bit for bit
    _steps(sim, 2, seed=8)
    _steps(twin, 2, seed=8)
    sa, sb = _all_state(sim), _all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 5. the env surface -----------------------------------------------------------------------------------------------------------------
def test_env_surface():
    from furniture_amd.envs import FurnitureSawyerEnv, furniture_names, make_config
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    spec = PairSet([PairSensor(gripper_bodies(load_model()), "0_part0", dmax=3.0), PairSensor("world", "right_hand", dmax=3.0), PairSensor("right_hand", "1_part1", dmax=0.01)],
                   fromto=True, normal=True)
    env = FurnitureBatchEnv("Sawyer", 4, config=cfg(), pairs=spec)
    sp = env.observation_space.spaces
    ob = env.reset()
    assert list(ob.keys()) == list(sp.keys()) and list(sp.keys())[-4:] == ["pair_distance", "pair_geoms", "pair_fromto", "pair_normal"] and "probe_distance" not in ob
    assert tuple(ob["pair_distance"].shape) == (4, 3) and ob["pair_distance"].dtype == torch.float32 and sp["pair_distance"].shape == (3,)
    assert tuple(ob["pair_geoms"].shape) == (4, 3, 2) and ob["pair_geoms"].dtype == torch.int32 and sp["pair_geoms"].dtype == np.int32
    assert tuple(ob["pair_fromto"].shape) == (4, 3, 6) and tuple(ob["pair_normal"].shape) == (4, 3, 3) and sp["pair_fromto"].shape == (3, 6) and sp["pair_normal"].shape == (3, 3)
    assert np.isinf(sp["pair_distance"].low).all() and float(sp["pair_distance"].high.max()) == 3.0 and int(sp["pair_geoms"].low.min()) == -1
    assert int(sp["pair_geoms"].high.max()) == env.model.ngeom - 1
    fresh = env.sim.pair_distance()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], ob[k]), k
    g = ob["pair_geoms"].cpu().numpy()
    assert (g[:, :2] >= 0).all() and (g[:, 2] == -1).all() and (ob["pair_distance"][:, 2] == 0.01).all()
    rng = np.random.RandomState(0)
    for _ in range(3):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (4, env.dof)).astype(np.float32))
    assert bool(done.all()) and list(ob.keys()) == list(sp.keys())
    kept = {k: ob[k].clone() for k in fresh}
    fresh = env.sim.pair_distance()
    torch.cuda.synchronize()
    for k in fresh:
        assert torch.equal(fresh[k], kept[k]), k
    for e in range(4):
        for k in fresh:
            assert sp[k].contains(ob[k][e].cpu().numpy()), k
    env.close()
    # without the vectors
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg(), pairs=PairSet(spec.sensors))
    ob = env.reset()
    assert list(ob.keys()) == list(env.observation_space.spaces.keys()) and list(ob.keys())[-2:] == ["pair_distance", "pair_geoms"]
    env.close()
    # without pairs: the keys of before
    env = FurnitureBatchEnv("Sawyer", 2, config=cfg())
    assert not any(k.startswith("pair_") for k in list(env.reset()) + list(env.observation_space.spaces)) and env.sim.pairs is None
    env.close()
    # the single env keeps its pair set through reset(furniture_id)
    e1 = FurnitureSawyerEnv(config=cfg(), pairs=spec)
    first = e1.reset()
    assert first["pair_distance"].shape == (3,) and first["pair_fromto"].shape == (3, 6)
    other = e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert e1._b.furniture_name == "chair_agne_0010" and e1._b.pairs is spec and list(other.keys()) == list(first.keys())
    assert other["pair_distance"].shape == (3,) and (np.asarray(other["pair_geoms"].cpu() if hasattr(other["pair_geoms"], "cpu") else other["pair_geoms"])[:2] >= 0).all()
    e1.close()


def load_model():
    from furniture_amd.mjcf.model import load_compiled
    return load_compiled("Sawyer", "table_lack_0825")


# ---- 6. the C-ABI's error paths -----------------------------------------------------------------------------------------------------------
def test_c_abi_error_paths():
    m, sim = _make("Sawyer", "table_lack_0825", 2)
    L, h = lib(), sim._h
    ncg = len(m.arrays["cg_orig"])
    buf = torch.zeros((2, 70), device=sim.device)
    msg = lambda: L.fsim_last_error().decode()

    def table(n=1, a=(1 << 12,), b=(1 << 22,), dmax=1.0):
        t = (FsimPairSensor * n)()
        for k in t:
            k.a[:] = list(a) + [0] * (3 - len(a))
            k.b[:] = list(b) + [0] * (3 - len(b))
            k.dmax = dmax
        return t

    def refused(rc, text):
        assert rc == -1 and text in msg(), (rc, text, msg())

    def set_pairs(n, t):  # (t stays alive over the call)
        return L.fsim_set_pairs(h, n, ctypes.addressof(t) if t is not None else None)
    for call_ in (sim.pair_distance, sim.pair_shapes):
        with pytest.raises(FsimError, match="no pair set"):
            call_()
    refused(L.fsim_pair_distance(h, buf.data_ptr(), None, None, None), "no pair set")
    t0 = table()
    refused(L.fsim_set_pairs(None, 1, ctypes.addressof(t0)), "null handle")
    refused(L.fsim_pair_distance(None, buf.data_ptr(), None, None, None), "null handle")
    refused(L.fsim_set_pairs(h, 1, None), "null argument")
    refused(set_pairs(-1, table()), "-1 sensors")
    refused(set_pairs(65, table(65)), "65 sensors")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(set_pairs(1, table(dmax=bad)), "0 < dmax < inf")
    refused(set_pairs(1, table(a=(0,))), "side A is empty")
    refused(set_pairs(1, table(b=(0,))), "side B is empty")
    assert ncg < 32
    refused(set_pairs(1, table(a=(1 << ncg,))), "mask bit %d set" % ncg)
    refused(set_pairs(1, table(b=(1 << 22, 0, 1 << 31))), "mask bit 95 set")
    refused(set_pairs(1, table(a=(1,), b=(1,))), "no valid pair")  # the floor with itself
    refused(set_pairs(1, table(a=(1 << 5,), b=(1 << 5,))), "no valid pair")
    allg = ((1 << ncg) - 1,)
    n_all = ncg * (ncg - 1)
    assert n_all <= 4096
    assert set_pairs(16384 // n_all, table(16384 // n_all, a=allg, b=allg)) == 0
    refused(set_pairs(16384 // n_all + 1, table(16384 // n_all + 1, a=allg, b=allg)), "more than 16384 pairs over the set")
    assert L.fsim_pair_distance(h, buf.data_ptr(), None, None, None) == 0  # a refused set leaves the one before it
    torch.cuda.synchronize()
    assert L.fsim_set_pairs(h, 0, None) == 0  # clear
    refused(L.fsim_pair_distance(h, buf.data_ptr(), None, None, None), "no pair set")
    assert set_pairs(2, table(2)) == 0
    refused(L.fsim_pair_distance(h, None, None, None, None), "no output")
    buf.fill_(7.0)
    assert L.fsim_pair_distance(h, buf.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    res = buf.cpu().numpy().reshape(-1)
    assert ((res[:4] > 0) & (res[:4] <= 1.0)).all() and (res[4:] == 7.0).all()  # [2 envs][2 sensors], nothing past them
    assert L.fsim_set_pairs(h, 0, None) == 0 and L.fsim_set_pairs(h, 0, None) == 0  # clearing twice is fine
    sim.set_pairs(PairSet(PairSensor("right_hand", "0_part0")))
    sim.set_pairs(None)
    with pytest.raises(FsimError, match="no pair set"):
        sim.pair_distance()
    with pytest.raises(TypeError, match="PairSet"):
        sim.set_pairs([PairSensor("right_hand", "0_part0")])
    sim.close()


def test_per_sensor_cap_in_the_library():
    """4097 pairs in one sensor need 65 geoms on a side: no shipped model has them, so the cap is reached with the all-against-all sensor
    of the largest model (52 geoms, 2652 pairs: accepted) and the refusal is the host check's (tests/test_pairs.py)"""
    m, sim = _make("Cursor", "toy_table", 1)
    cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
    sim.set_pairs(PairSet(PairSensor(cg, cg, dmax=3.0)))
    got = _pairs(sim)
    assert got["pair_geoms"][0, 0, 0] >= 0
    sim.close()


# ---- 7. device against device: a probe at `from` sees side B at the same distance --------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064")])
def test_probe_at_from_returns_the_distance(agent, furniture):
    m, sim = _make(agent, furniture, 2)
    _known_states(m, sim)
    sensors = [s for s in _sensors(m)[:-1]]
    sim.set_pairs(PairSet(sensors, fromto=True))
    got = _pairs(sim)
    cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
    gtype = np.asarray(m.arrays["geom_type"])
    checked = 0
    for e in range(2):
        for i, s in enumerate(sensors):
            d, gg = got["pair_distance"][e, i], got["pair_geoms"][e, i]
            if gg[0] < 0 or d <= TOUCH or gtype[gg[1]] == MESH:  # apart winners whose B geom is not a hull (the probes measure a hull by its plane bound)
                continue
            _, mb = s.side_masks(m)
            probe = ProbeSensor((0.0, 0.0, 0.0), [got["pair_fromto"][e, i, :3]], dmax=s.dmax, exclude=[g for k, g in enumerate(cg) if not mb[k]])
            sim.set_probes(ProbeSet([probe]))
            res = sim.probe_distance()
            torch.cuda.synchronize()
            pd = float(res["probe_distance"][e, 0])
            assert abs(pd - d) <= dist_bound(d), "%s env %d sensor %d: pair distance %.9g, a probe at `from` against side B %.9g" % (furniture, e, i, d, pd)
            checked += 1
    assert checked >= 6
    sim.close()

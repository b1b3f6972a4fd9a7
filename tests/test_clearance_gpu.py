"""What-if clearance queries on the device (include/fsim_clearance.h) through the library: against the existing path (set_state + pair_distance
per candidate, bit for bit), against the float64 reference tests/clearance_reference.py with the tolerances of tests/test_pairs_gpu.py,
with the record's own values as the candidate, independence of K, of the chunking and of the batch, the carry mask per env and per rule,
`valid`, read-only evaluation, outputs one at a time, the C-ABI's error paths, coexistence with a pair set and the env surface.

3 envs (not a multiple of the four waves of a k_pair_dist workgroup) and 2 sensors, K from {1, 5}, scratch_rows 5, 6 and the default.  The
states are written with set_state: the arm at qpos0 and at two bent poses, and one part put under the right gripper's finger tips at a
reference gap of 3 cm (near), 0 (touching) and -5 mm (overlapping), found by bisection on the float64 gap.

Against the existing path the comparison is of bytes: k_clr_pose runs the stages of fsim_kin.hpp and k_cam_pose's geom stage on the same
operands, and the distance kernel is the same kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tests.test_pairs_gpu as tpg
from furniture_amd.clearance import ClearanceSet, carried_sensor, robot_clearance_sensors
from furniture_amd.envs import FurnitureBatchEnv
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.pairs import PairSensor, PairSet, gripper_bodies
from furniture_amd.sim import FSim, FsimClrCarry, FsimError, FsimPairSensor, lib
from oracle.oracle_sim import OracleSim
from tests import clearance_reference as clr
from tests.test_camera_gpu import _make, _poison, _steps
from tests.test_pairs_tool_gpu import PORTAL_TOL, POS_TOL, dist_bound
from tests.test_rays_gpu import _bent

pytestmark = pytest.mark.gpu
MODELS = [("Sawyer", "table_lack_0825"), ("Baxter", "table_liden_0921"), ("Sawyer", "chair_agne_0010")]  # (chair_agne_0010: the convex-mesh collider of tests/test_pairs_gpu.py)
N, K = 3, 5
KEYS = ("clearance_distance", "clearance_geoms", "clearance_fromto", "clearance_normal")
PAIR_KEYS = ("pair_distance", "pair_geoms", "pair_fromto", "pair_normal")
GAPS = (0.03, 0.0, -0.005)  # the placed part against the gripper, per env: near, touching, overlapping


# ---- the models' dofs, parts and states (host only, once per model) -------------------------------------------------------------------------
def _dofs(m):
    """the candidate's columns: Sawyer's arm and fingers; Baxter's two arms and four fingers, interleaved so that the columns follow
    neither dof order nor one arm; the arm alone on the third model"""
    arm = [int(d) for d in np.asarray(m.arm_dofadr).reshape(-1)]
    grip = [int(d) for d in np.asarray(m.arrays["grip_dofadr"]).reshape(-1)]
    if m.meta["agent"] == "Baxter":
        h = len(arm) // 2
        return [d for pair in zip(arm[h:], arm[:h]) for d in pair] + grip[::-1]
    return arm if m.meta["furniture_name"] == "chair_agne_0010" else arm + grip


def _held_part(m):
    """the part put under the gripper: the one with a convex-mesh collider where the model has one, else the part on the last reduced
    body (Baxter + table_liden_0921: reduced body 31)"""
    A = m.arrays
    cg = np.asarray(A["cg_orig"])
    pid = np.asarray(A["cg_partid"])
    mesh = pid[(np.asarray(A["geom_type"])[cg] == tpg.MESH) & (pid >= 0)]
    names = m.meta["part_names"]
    if len(mesh):
        return names[int(mesh[0])]
    red = np.asarray(A["body_red"])
    return max(names, key=lambda p: red[m.meta["body_names"].index(p)])


def _other_part(m):
    return [p for p in m.meta["part_names"] if p != _held_part(m)][0]


def _grip(m):
    return gripper_bodies(m, arm="right") if m.meta["agent"] == "Baxter" else gripper_bodies(m)


def _hand(m):
    return "right_hand"


def _second_carrier(m):
    return "left_hand" if m.meta["agent"] == "Baxter" else "right_l5"


@functools.lru_cache(maxsize=None)
def _setup(agent, furniture):
    """(model, float64 [N][nq] arm and held-part words of the three states (the other parts stay where the reset put them: NaN here),
    float32 [N][K][D] candidates)"""
    m = load_compiled(agent, furniture)
    part = _held_part(m)
    adr = int(np.asarray(m.part_qposadr).reshape(-1)[m.meta["part_names"].index(part)])
    pairs = PairSensor(_grip(m), part).pairs(m)
    A = m.arrays
    cg = np.asarray(A["cg_orig"])
    tips = [int(g) for g, r in zip(cg, np.asarray(A["cg_fingerrole"])) if r != 0 and m.meta["body_names"][int(A["geom_bodyid"][g])].startswith("r_")]
    q0 = np.asarray(A["qpos0"], dtype=np.float64)
    osim = OracleSim(m)
    states = []
    on_part = np.nonzero(clr.carried_geoms(m, part))[0]
    for q, target in zip((q0, _bent(m), _bent(m, seed=4)), GAPS):
        osim.data.qpos[:] = q
        osim.forward()
        tip = np.mean([np.array(osim.data.geom_xpos[g], dtype=np.float64) for g in tips], axis=0)

        def put(h):
            q2 = q.copy()
            q2[adr:adr + 3] = tip - np.array([0.0, 0.0, h])
            q2[adr + 3:adr + 7] = (1.0, 0.0, 0.0, 0.0)
            return q2
        at0 = clr.geoms_at(osim, m, put(0.0), [], [])

        def gap(h):  # (the part hangs straight: lowering it by h moves its geoms by h)
            moved = [dict(g, pos=g["pos"] - np.array([0.0, 0.0, h])) if k in on_part else g for k, g in enumerate(at0)]
            return min(tpg._reference_gaps(moved, pairs).values()) - target
        lo, hi = 0.0, 0.6
        flo, fhi = gap(lo), gap(hi)
        assert flo < 0.0 < fhi, (agent, furniture, flo, fhi)
        for _ in range(20):  # regula falsi with the Illinois step; 2e-5 m is a tenth of the band the checks call touching
            mid = hi - fhi * (hi - lo) / (fhi - flo)
            fm = gap(mid)
            if abs(fm) < 2e-5:
                break
            if fm * fhi < 0:
                lo, flo = hi, fhi
            else:
                flo *= 0.5
            hi, fhi = mid, fm
        assert abs(fm) < 2e-5, (agent, furniture, target, fm)
        states.append(put(mid))
    osim.close()
    states = np.array(states)
    keep = np.zeros(states.shape[1], dtype=bool)
    keep[:int(np.asarray(m.part_qposadr).reshape(-1).min())] = True  # the robot's words
    keep[adr:adr + 7] = True
    states[:, ~keep] = np.nan
    dofs = _dofs(m)
    qa = clr.dof_addresses(m, dofs)
    cand = states[:, None, qa] + np.random.RandomState(7).uniform(-0.3, 0.3, (N, K, len(dofs)))
    cand[:, 0] = states[:, qa]  # candidate 0: the record's own values
    return m, states, cand.astype(np.float32)


def _write_states(sim, states):
    q = sim.get_state("qpos")["qpos"]
    s = torch.as_tensor(states.astype(np.float32), device=q.device)
    q = torch.where(torch.isnan(s), q, s)
    sim.set_state(qpos=q)
    return q


def _open(agent, furniture, sensors, n=N, **kw):
    m, states, cand = _setup(agent, furniture)
    _, sim = _make(agent, furniture, n)
    _write_states(sim, states[:n])
    sim.set_clearance(ClearanceSet(_dofs(m), sensors(m), max_candidates=K, fromto=True, normal=True, **kw))
    return m, sim, torch.as_tensor(cand[:n], device=sim.device)


def _plain_sensors(m):
    return [robot_clearance_sensors(m, dmax=2.0), carried_sensor(m, _held_part(m), dmax=2.0)]


def _carry_sensors(m):
    """the carrier body against the held part (constant under carry rule 0; the fingers are bodies of their own and move with the
    candidate's finger joints), the held part against the other part (which rule 1 moves)"""
    return [PairSensor(_hand(m), _held_part(m), dmax=2.0), PairSensor(_held_part(m), _other_part(m), dmax=2.0)]


def _rules(m):
    return [(_held_part(m), _hand(m)), (_other_part(m), _second_carrier(m))]


def _clear(sim, cand, mask=None, **kw):
    _poison()
    res = sim.clearance(cand, mask, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _by_set_state(m, sim, sensors, cand):
    """the existing path: per candidate set_state, pair_distance with the same sensors, and the restoring set_state -> [n][K][S]... arrays"""
    qa = torch.as_tensor(clr.dof_addresses(m, _dofs(m)), device=sim.device)
    sim.set_pairs(PairSet(sensors, fromto=True, normal=True))
    rec = sim.get_state("qpos")["qpos"].clone()
    out = {k: [] for k in PAIR_KEYS}
    for k in range(cand.shape[1]):
        q = rec.clone()
        q[:, qa] = cand[:, k]
        sim.set_state(qpos=q)
        res = sim.pair_distance()
        torch.cuda.synchronize()
        for key in PAIR_KEYS:
            out[key].append(res[key].cpu().numpy())
    sim.set_state(qpos=rec)
    sim.set_pairs(None)
    return {"clearance_" + k[len("pair_"):]: np.stack(v, axis=1) for k, v in out.items()}


def _same(a, b, keys=KEYS, where=""):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s %s: largest difference %g" % (where, k, np.abs(a[k].astype(np.float64) - b[k]).max())


# ---- 1. against the existing path, 3. candidate = the record's own values ------------------------------------------------------------------
@pytest.mark.parametrize("agent,furniture", MODELS)
def test_matches_set_state_and_pair_distance_bit_for_bit(agent, furniture):
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    got = _clear(sim, cand)
    assert got["clearance_valid"].shape == (N, K) and (got["clearance_valid"] == 1).all()
    # 3. first, before any set_state of this test: candidate 0 is the record -> pair_distance of the state as it is
    sim.set_pairs(PairSet(_plain_sensors(m), fromto=True, normal=True))
    now = {k: v.cpu().numpy() for k, v in sim.pair_distance().items()}
    for key in PAIR_KEYS:
        assert got["clearance_" + key[len("pair_"):]][:, 0].tobytes() == now[key].tobytes(), key
    want = _by_set_state(m, sim, _plain_sensors(m), cand)
    for key in KEYS:
        print("%s + %s %s: largest difference %g" % (agent, furniture, key, np.abs(got[key].astype(np.float64) - want[key]).max()))
    _same(got, want, where=furniture)
    d = got["clearance_distance"]
    assert len({d[e, k].tobytes() for e in range(N) for k in range(K)}) == N * K  # the rows differ
    # the three regimes are there: near, touching and overlapping at the record's own values (the robot sensor sees the placed part nearest)
    print("%s + %s: robot sensor at the record %s" % (agent, furniture, d[:, 0, 0]))
    assert d[0, 0, 0] > 0.02 and abs(d[1, 0, 0]) < 1e-3 and d[2, 0, 0] < -0.004
    sim.close()


# ---- 2. against float64 -----------------------------------------------------------------------------------------------------------------------
def _against_float64(m, sim, sensors, got, rules, mask, tag, cands=range(K)):
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    _, _, cand = _setup(m.meta["agent"], m.meta["furniture_name"])
    osim = OracleSim(m)
    kept = {}
    for e in range(N):
        carry = [r for i, r in enumerate(rules) if (int(mask[e]) >> i) & 1]
        for k in cands:
            geoms = clr.geoms_at(osim, m, qpos[e], _dofs(m), cand[e, k], carry)
            kept[e, k] = geoms
            one = {"pair_" + key[len("clearance_"):]: got[key][:, k] for key in KEYS}
            tpg._check_env(m, sensors, one, e, geoms, "%s candidate %d" % (tag, k))
    osim.close()
    return kept


@pytest.mark.parametrize("agent,furniture", MODELS)
def test_matches_float64_without_carry(agent, furniture):
    """The tolerances of tests/test_pairs_gpu.py, unchanged.  The robot sensor has hundreds of pairs, a second of reference each row: it
    is held against float64 at candidate 0 (the record: near, touching, overlapping) and candidate 3 of every env; the first test ties
    every row, these included, to pair_distance bit for bit, and the carry test below holds all fifteen rows of its smaller sensors."""
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    _against_float64(m, sim, _plain_sensors(m), _clear(sim, cand), [], np.zeros(N, dtype=np.uint8), furniture, cands=(0, 3))
    sim.close()


def _carry_extra(m, qpos, mask):
    """4 x the largest effect on a carried geom's position of the carried-pose composition restated in numpy float32 (the issue's rule)"""
    _, _, cand = _setup(m.meta["agent"], m.meta["furniture_name"])
    osim = OracleSim(m)
    worst = max(clr.composition_error_fp32(osim, m, qpos[e], _dofs(m), cand[e], [r for i, r in enumerate(_rules(m)) if (int(mask[e]) >> i) & 1]) for e in range(N))
    osim.close()
    return 4.0 * worst


@pytest.mark.parametrize("agent,furniture", MODELS[:2])
def test_carry_mask_per_env_and_rule_and_float64(agent, furniture, monkeypatch):
    """5. and 2. with carry.  env 0: nothing carried, env 1: rule 0, env 2: rules 0 and 1."""
    m, sim, cand = _open(agent, furniture, _carry_sensors, carry=_rules(_setup(agent, furniture)[0]))
    mask = np.array([0, 1, 3], dtype=np.uint8)
    none = _clear(sim, cand)
    got = _clear(sim, cand, torch.as_tensor(mask, device=sim.device))
    for key in KEYS:  # the bit clear: the answer without carry, bit for bit
        assert got[key][0].tobytes() == none[key][0].tobytes(), key
    zero = _clear(sim, cand, torch.zeros(N, dtype=torch.uint8, device=sim.device))
    _same(zero, none, where="a zero mask")
    hi = _clear(sim, cand, torch.as_tensor(mask | 0xf0, device=sim.device))  # bits beyond the rules are ignored
    _same(hi, got, where="mask bits beyond the rules")
    only1 = _clear(sim, cand, torch.as_tensor(np.array([0, 2, 2], dtype=np.uint8), device=sim.device))  # rule 1 alone moves the OTHER part:
    for key in KEYS:  # the hand-to-held-part sensor is what it is without carry
        assert only1[key][:, :, 0].tobytes() == none[key][:, :, 0].tobytes(), key
    assert only1["clearance_distance"][1:, 1:, 1].tobytes() != none["clearance_distance"][1:, 1:, 1].tobytes()
    qpos = sim.get_state("qpos")["qpos"].cpu().numpy().astype(np.float64)
    extra = _carry_extra(m, qpos, mask)
    print("%s + %s: carried-pose composition in float32, 4 x its largest effect on a geom position: %.3e m" % (agent, furniture, extra))
    assert extra < 1e-5
    # candidate 0 is the record: a carried part stays where it is, up to the composition's rounding
    apart = none["clearance_distance"][:, 0] > tpg.TOUCH  # (an exact distance moves by no more than its geoms do; a portal depth promises less)
    assert np.abs(got["clearance_distance"][:, 0].astype(np.float64) - none["clearance_distance"][:, 0])[apart].max() <= 2 * dist_bound(0.6) + extra
    # the tolerances of tests/test_pairs_gpu.py, widened by `extra`
    monkeypatch.setattr(tpg, "dist_bound", lambda r: dist_bound(r) + extra)
    monkeypatch.setattr(tpg, "POS_TOL", POS_TOL + extra)
    monkeypatch.setattr(tpg, "PORTAL_TOL", PORTAL_TOL + extra)
    geoms = _against_float64(m, sim, _carry_sensors(m), got, _rules(m), mask, furniture + " carry")
    for e in (1, 2):  # the reference's own check, then the device: the distance from the carrier to the part is constant over the candidates
        spread = clr.check_carry_is_rigid(m, tpg._reference_gaps, [geoms[e, k] for k in range(K)], *_rules(m)[0])
        d = got["clearance_distance"][e, :, 0].astype(np.float64)
        print("%s + %s env %d: carrier to carried part %s (reference spread %.1e)" % (agent, furniture, e, d, spread))
        assert d.max() - d.min() <= 2 * (tpg.dist_bound(d.mean()) + tpg.PORTAL_TOL)
    d0 = none["clearance_distance"][1, :, 0]
    assert d0.max() - d0.min() > 1e-3  # ... and it is not without carry
    sim.close()


# ---- 4. independence --------------------------------------------------------------------------------------------------------------------------
def test_independent_of_k_of_the_chunking_and_of_the_batch():
    agent, furniture = MODELS[0]
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    full = _clear(sim, cand)
    allk = KEYS + ("clearance_valid",)
    one = _clear(sim, cand[:, 3:4].contiguous())  # candidate 3 of K = 5 is the same candidate alone
    for key in allk:
        assert one[key][:, 0].tobytes() == np.ascontiguousarray(full[key][:, 3]).tobytes(), key
    spec = dict(max_candidates=K, fromto=True, normal=True)
    for rows in (5, 6):  # floor(rows / 5) = 1 env per chunk: three chunks; K = 1: one chunk of the three envs
        sim.set_clearance(ClearanceSet(_dofs(m), _plain_sensors(m), scratch_rows=rows, **spec))
        _same(_clear(sim, cand), full, allk, "scratch_rows %d" % rows)
        _same(_clear(sim, cand[:, 3:4].contiguous()), one, allk, "scratch_rows %d, K = 1" % rows)
    # two envs per chunk: a full chunk and a ragged last one
    sim.set_clearance(ClearanceSet(_dofs(m), _plain_sensors(m), max_candidates=1, scratch_rows=2, fromto=True, normal=True))
    _same(_clear(sim, cand[:, 3:4].contiguous()), one, allk, "scratch_rows 2, K = 1")
    state = sim.get_state("qpos")["qpos"]
    alone = FSim(m, 1, config=sim.cfg)  # env 1 alone in a 1-env handle
    alone.set_state(qpos=state[1:2])
    alone.set_clearance(ClearanceSet(_dofs(m), _plain_sensors(m), **spec))
    got = _clear(alone, cand[1:2].contiguous())
    for key in allk:
        assert got[key][0].tobytes() == full[key][1].tobytes(), key
    alone.close()
    sim.close()


# ---- 6. valid ---------------------------------------------------------------------------------------------------------------------------------
def test_valid_and_the_substitution():
    agent, furniture = MODELS[0]
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    full = _clear(sim, cand)
    bad = cand.clone()
    bad[1, 2, 0], bad[1, 2, 3] = float("nan"), float("-inf")
    got = _clear(sim, bad)
    want = np.ones((N, K), dtype=np.uint8)
    want[1, 2] = 0
    assert np.array_equal(got["clearance_valid"], want)
    sub = cand.clone()
    qa = clr.dof_addresses(m, _dofs(m))
    rec = sim.get_state("qpos")["qpos"]
    sub[1, 2, 0], sub[1, 2, 3] = rec[1, int(qa[0])], rec[1, int(qa[3])]
    fixed = _clear(sim, sub)
    assert (fixed["clearance_valid"] == 1).all()
    _same(got, fixed, where="the env's own values in place of the two")
    for key in KEYS:  # the neighbours are untouched, the row itself is not the candidate's
        keep = np.ones((N, K), dtype=bool)
        keep[1, 2] = False
        assert got[key][keep].tobytes() == full[key][keep].tobytes(), key
    assert got["clearance_distance"][1, 2].tobytes() != full["clearance_distance"][1, 2].tobytes()
    sim.close()


# ---- 7. read-only -----------------------------------------------------------------------------------------------------------------------------
def test_evaluation_is_read_only():
    agent, furniture = MODELS[0]
    m, _, cand = _setup(agent, furniture)
    _, sim = _make(agent, furniture, N)
    _, twin = _make(agent, furniture, N)
    _steps(sim, 3)
    _steps(twin, 3)
    sim.set_clearance(ClearanceSet(_dofs(m), _carry_sensors(m), carry=_rules(m), max_candidates=K, scratch_rows=6, fromto=True, normal=True))
    c = torch.as_tensor(cand, device=sim.device)
    before = tpg._all_state(sim)  # the whole record
    first = _clear(sim, c, torch.as_tensor(np.array([1, 0, 3], dtype=np.uint8), device=sim.device))
    _clear(sim, c[:, :1].contiguous())
    after = tpg._all_state(sim)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    again = _clear(sim, c, torch.as_tensor(np.array([1, 0, 3], dtype=np.uint8), device=sim.device))
    _same(first, again, KEYS + ("clearance_valid",), "the same call twice")
    # a step after a call == the same step without one, bit for bit
    _steps(sim, 2, seed=8)
    _steps(twin, 2, seed=8)
    sa, sb = tpg._all_state(sim), tpg._all_state(twin)
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    sim.close()
    twin.close()


# ---- 8. outputs one at a time, wrong tensors, the C-ABI, a pair set beside it, the env surface ------------------------------------------------------
def test_each_output_alone_and_wrong_tensors():
    agent, furniture = MODELS[0]
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    full = _clear(sim, cand)
    shapes = sim.clearance_shapes(K)
    assert list(shapes) == ["clearance_distance", "clearance_geoms", "clearance_valid", "clearance_fromto", "clearance_normal"]
    assert shapes["clearance_distance"] == ((K, 2), torch.float32) and shapes["clearance_valid"] == ((K,), torch.uint8) and shapes["clearance_geoms"] == ((K, 2, 2), torch.int32)
    for k in KEYS:
        buf = torch.full((N,) + shapes[k][0], 77, dtype=shapes[k][1], device=sim.device)
        res = _clear(sim, cand, out={k: buf})
        assert list(res) == [k] and res[k].tobytes() == full[k].tobytes() and buf.cpu().numpy().tobytes() == full[k].tobytes(), k
    vbuf = torch.full((N, K), 77, dtype=torch.uint8, device=sim.device)
    res = _clear(sim, cand, out={"clearance_valid": vbuf, "clearance_geoms": torch.empty((N, K, 2, 2), dtype=torch.int32, device=sim.device)})
    assert sorted(res) == ["clearance_geoms", "clearance_valid"] and (vbuf == 1).all() and res["clearance_geoms"].tobytes() == full["clearance_geoms"].tobytes()
    with pytest.raises(ValueError, match="clearance_valid alone"):
        sim.clearance(cand, out={"clearance_valid": vbuf})
    with pytest.raises(ValueError, match="out holds"):
        sim.clearance(cand, out={})
    with pytest.raises(ValueError, match="not a contiguous"):
        sim.clearance(cand, out={"clearance_distance": torch.zeros((N, K, 3), device=sim.device)})
    D = cand.shape[2]
    for bad in (cand.double(), cand[:, :, :D - 1].contiguous(), cand[:2].contiguous(), cand.transpose(0, 1).contiguous().transpose(0, 1), cand.cpu(), cand.cpu().numpy(), cand[:, 0]):
        with pytest.raises(ValueError, match="cand is not a contiguous float32 tensor of shape"):
            sim.clearance(bad)
    with pytest.raises(ValueError, match="K = 6 candidates"):
        sim.clearance(torch.zeros((N, K + 1, D), device=sim.device))
    with pytest.raises(ValueError, match="K = 0 candidates"):
        sim.clearance(torch.zeros((N, 0, D), device=sim.device))
    ok = torch.zeros(N, dtype=torch.uint8, device=sim.device)
    for bad in (ok.int(), ok[:2].contiguous(), torch.zeros((N, 2), dtype=torch.uint8, device=sim.device)[:, 0], ok.cpu(), [0, 0, 0]):
        with pytest.raises(ValueError, match="carry_mask is not a contiguous uint8 tensor of shape"):
            sim.clearance(cand, bad)
    # without the vectors
    sim.set_clearance(ClearanceSet(_dofs(m), _plain_sensors(m), max_candidates=K))
    res = _clear(sim, cand)
    assert sorted(res) == ["clearance_distance", "clearance_geoms", "clearance_valid"] and res["clearance_distance"].tobytes() == full["clearance_distance"].tobytes()
    sim.set_clearance(None)
    for call_ in (lambda: sim.clearance(cand), lambda: sim.clearance_shapes(1)):
        with pytest.raises(FsimError, match="no clearance set"):
            call_()
    with pytest.raises(TypeError, match="ClearanceSet"):
        sim.set_clearance(_plain_sensors(m))
    sim.close()


def test_c_abi_set_refused_set_clear_and_a_pair_set_beside_it():
    agent, furniture = MODELS[0]
    m, sim, cand = _open(agent, furniture, _plain_sensors)
    L, h = lib(), sim._h
    msg = lambda: L.fsim_last_error().decode()
    names = m.meta["body_names"]
    nv = len(m.arrays["dof_bodyid"])
    D = cand.shape[2]

    def table(a=(1 << 12,), b=(1 << 22,), dmax=1.0):
        t = (FsimPairSensor * 1)()
        t[0].a[:] = list(a) + [0] * (3 - len(a))
        t[0].b[:] = list(b) + [0] * (3 - len(b))
        t[0].dmax = dmax
        return t

    def rule(part, carrier):
        r = (FsimClrCarry * 1)()
        r[0].part_body, r[0].carrier_body = part, carrier
        return r

    def set_clr(dofs, t=None, carry=None, maxc=K, rows=0, n_sens=1):
        d = np.ascontiguousarray(dofs, dtype=np.int32)
        t = table() if t is None else t  # (d, t and carry stay alive over the call)
        return L.fsim_set_clearance(h, len(d), d.ctypes.data if len(d) else None, n_sens, ctypes.addressof(t), 0 if carry is None else len(carry),
                                    None if carry is None else ctypes.addressof(carry), maxc, rows)

    def refused(rc, text):
        assert rc == -1 and text in msg(), (rc, text, msg())
    full = _clear(sim, cand)
    dist = torch.zeros((N, K, 2), device=sim.device)

    def run():
        rc = L.fsim_clearance(h, K, cand.data_ptr(), None, dist.data_ptr(), None, None, None, None)
        torch.cuda.synchronize()
        return rc
    part0, hand = names.index("0_part0"), names.index("right_hand")
    refused(L.fsim_set_clearance(None, 1, None, 1, None, 0, None, 1, 0), "null handle")
    refused(set_clr([]), "no dofs listed")
    refused(set_clr(list(range(7)) + list(range(7)) + list(range(7)) + list(range(7)) + list(range(5))), "33 dofs")
    refused(set_clr([nv]), "out of range")
    refused(set_clr([0, 1, 0]), "listed twice")
    refused(set_clr([int(m.arrays["part_dofadr"][0])]), "not the dof of a hinge or slide joint")
    refused(set_clr(range(7), t=table(dmax=0.0)), "0 < dmax < inf")  # what fsim_set_pairs refuses, in its words
    refused(set_clr(range(7), t=table(a=(0,))), "side A is empty")
    refused(set_clr(range(7), t=table(a=(1,), b=(1,))), "no valid pair")
    refused(set_clr(range(7), n_sens=65), "65 sensors")
    refused(set_clr(range(7), carry=rule(hand, part0)), "is not a furniture part")
    refused(set_clr(range(7), carry=rule(part0, len(names))), "unknown carrier body")
    refused(set_clr(range(7), carry=rule(part0, part0)), "belongs to the part it carries")
    two = (FsimClrCarry * 2)()
    two[0].part_body, two[0].carrier_body, two[1].part_body, two[1].carrier_body = part0, hand, part0, names.index("right_l5")
    refused(set_clr(range(7), carry=two), "carried by rule 0 already")
    refused(set_clr(range(7), carry=(FsimClrCarry * 9)()), "9 carry rules")
    refused(set_clr(range(7), maxc=0), "max_candidates 0")
    refused(set_clr(range(7), maxc=1025), "max_candidates 1025")
    refused(set_clr(range(7), maxc=8, rows=7), "scratch_rows 7")
    assert run() == 0 and dist.cpu().numpy().tobytes() == full["clearance_distance"].tobytes()  # a refused set leaves the one before it
    refused(L.fsim_clearance(None, K, cand.data_ptr(), None, dist.data_ptr(), None, None, None, None), "null handle")
    refused(L.fsim_clearance(h, 0, cand.data_ptr(), None, dist.data_ptr(), None, None, None, None), "K = 0 candidates")
    refused(L.fsim_clearance(h, K + 1, cand.data_ptr(), None, dist.data_ptr(), None, None, None, None), "K = 6 candidates")
    refused(L.fsim_clearance(h, K, None, None, dist.data_ptr(), None, None, None, None), "null argument")
    valid = torch.zeros((N, K), dtype=torch.uint8, device=sim.device)
    refused(L.fsim_clearance(h, K, cand.data_ptr(), None, None, None, None, None, valid.data_ptr()), "no output")
    # a pair set beside it: neither knows of the other
    pairs = PairSet(_carry_sensors(m), fromto=True, normal=True)
    sim.set_pairs(pairs)
    with_pairs = {k: v.cpu().numpy() for k, v in sim.pair_distance().items()}
    _same(_clear(sim, cand), full, where="with a pair set")
    assert L.fsim_set_clearance(h, 0, None, 0, None, 0, None, 0, 0) == 0  # clear
    refused(L.fsim_clearance(h, K, cand.data_ptr(), None, dist.data_ptr(), None, None, None, None), "no clearance set")
    again = {k: v.cpu().numpy() for k, v in sim.pair_distance().items()}
    for k in with_pairs:
        assert with_pairs[k].tobytes() == again[k].tobytes(), k
    assert L.fsim_set_clearance(h, 0, None, 0, None, 0, None, 0, 0) == 0  # clearing twice is fine
    assert set_clr(range(D), maxc=K, rows=K) == 0  # one sensor, the smallest scratch
    dist.fill_(7.0)
    assert run() == 0
    res = dist.cpu().numpy().reshape(-1)
    assert ((res[:N * K] > 0) & (res[:N * K] <= 1.0)).all() and (res[N * K:] == 7.0).all()  # [3 envs][5 candidates][1 sensor], nothing past them
    sim.set_pairs(None)
    sim.close()


def test_env_surface():
    from furniture_amd.envs import FurnitureSawyerEnv, furniture_names, make_config
    cfg = lambda **kw: make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", max_episode_steps=3, seed=4, **kw)
    m = load_compiled("Sawyer", "table_lack_0825")
    sensors = [PairSensor(gripper_bodies(m), "1_part1", dmax=3.0), PairSensor("1_part1", "world", dmax=3.0)]  # (names the chair has too)
    spec = ClearanceSet(_dofs(m), sensors, carry=[("1_part1", "right_hand")], max_candidates=K, normal=True)
    plain = FurnitureBatchEnv("Sawyer", N, config=cfg())
    env = FurnitureBatchEnv("Sawyer", N, config=cfg(), clearance=spec)
    assert list(env.observation_space.spaces) == list(plain.observation_space.spaces)
    ob, ob0 = env.reset(), plain.reset()
    assert list(ob.keys()) == list(ob0.keys()) and not any(k.startswith("clearance") for k in ob) and all(torch.equal(ob[k], ob0[k]) for k in ob)
    with pytest.raises(ValueError, match="no clearance set"):
        plain.clearance(torch.zeros((N, 1, len(_dofs(m))), device=plain.sim.device))
    plain.close()
    rec = env.sim.get_state("qpos")["qpos"]
    qa = torch.as_tensor(clr.dof_addresses(m, _dofs(m)), device=rec.device)
    cand = (rec[:, qa][:, None, :] + torch.linspace(0.0, 0.2, K, device=rec.device)[None, :, None]).contiguous()
    res = env.clearance(cand, torch.ones(N, dtype=torch.uint8, device=rec.device))
    torch.cuda.synchronize()
    assert sorted(res) == ["clearance_distance", "clearance_geoms", "clearance_normal", "clearance_valid"]
    assert tuple(res["clearance_distance"].shape) == (N, K, 2) and tuple(res["clearance_geoms"].shape) == (N, K, 2, 2) and tuple(res["clearance_normal"].shape) == (N, K, 2, 3)
    assert tuple(res["clearance_valid"].shape) == (N, K) and bool((res["clearance_valid"] == 1).all()) and bool((res["clearance_geoms"] >= 0).all())
    env.sim.set_pairs(PairSet(sensors, normal=True))  # candidate 0 is the state itself
    now = env.sim.pair_distance()
    assert torch.equal(env.clearance(cand)["clearance_distance"][:, 0], now["pair_distance"])
    env.sim.set_pairs(None)
    rng = np.random.RandomState(0)
    for _ in range(2):
        ob, rew, done, info = env.step(rng.uniform(-1, 1, (N, env.dof)).astype(np.float32))
        assert list(ob.keys()) == list(ob0.keys())
    env.close()
    # the single env keeps its clearance set through reset(furniture_id)
    e1 = FurnitureSawyerEnv(config=cfg(), clearance=spec)
    first = e1.reset()
    assert not any(k.startswith("clearance") for k in first) and e1._b.clearance_set is spec
    e1.reset(furniture_id=furniture_names().index("chair_agne_0010"))
    assert e1._b.furniture_name == "chair_agne_0010" and e1._b.clearance_set is spec and e1._b.sim.clearance_set is spec and tuple(e1._b.clearance(cand[:1].contiguous())["clearance_distance"].shape) == (1, K, 2)
    e1.close()

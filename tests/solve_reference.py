"""One Newton solve per factorisation path of csrc/fsim_solver.hpp fs_chol_solve against float64: the stored states
(tests/golden/solve_states.npz, written by scripts/make_golden_solve_states.py with the CPU checker alone), the conditions every stored
state meets, the float64 reference of one solve and of one substep, and the three measures.  Shared by tests/test_solve.py (CPU: the
conditions, the generator, what fp32 alone does) and tests/test_solve_gpu.py (the device).  Pure numpy + oracle/.

A state is a row of the fields of contacts_reference.FIELDS plus qacc_warmstart, float32 values held in float64 arrays.  A case is a
handful of states (at most 8) of one model that put their largest constraint island on one factorisation path:

  case         model                        largest island (dofs)   path
  free         Sawyer table_lack_0825       9 (+ parts of 6)        fs_chol_phase<12> / <6>
  limit        same                         9                       the same rows with an active joint-limit row
  pinch        same                         15                      fs_chol_phase<16>, cached body pairs
  grip_table   same                         21                      the matrix-core tile, contacts only
  weld         same                         21 with a weld row, 12  the tile with weld / contact cross blocks
  table30      same                         30                      top of the tile: four welds, the table on the floor
  welded39     same                         39                      fs_chol_lds (FSIM_MW=all: mw_chol_big)
  pile2..10    Sawyer bookcase_billy_0191   12, 18, 30, 36, 60      rows, tile, fs_chol_lds, all behind the second row pass (nv = 75 > 64)
  pile11       same                         66                      fs_chol_all_lds (512 contact slots)
  baxter       Baxter desk_mikael_1064      as it comes, recorded   a second robot tree

Parts that lie at rest (free, table30, the piles) are pushed by a wrench of the order of their weight in the stored state: at rest qacc = 0, which is
also where the solve starts, and a solve that does nothing would pass (START_FLOORS).  The planks of a pile are turned about the vertical: laid
square, each plank's spin is decoupled from every other dof, and it is the last pivot of the pile's island.

The measures (all through the float64 mass matrix M, so that they are forces):
  force   max |M (qacc_x - qacc_smooth) - qfrc_constraint| over the env's largest |qfrc_constraint| (contacts_reference.force_measure)
  island  the same error per constraint island, over the larger of the island's largest |qfrc_constraint| and its largest
          |M qacc_smooth|: a resting part is judged against its own weight, not against zero and not against the gripper's force; the
          worst island of the env.  Trees that no constraint touches are not islands of the solve and are left to `force`.
  step    (qvel after one substep - qvel) / h against the oracle's, through M, on the scale of `force`: the damped integrator's own
          fs_chol_solve call on top of the solve"""
import contextlib
import ctypes
import os

import numpy as np

from tests import contacts_reference as cref
from tests.solve_bits_common import island_dofs, tree_of_geom, tree_of_part

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_states.npz")
FIELDS = tuple(cref.FIELDS) + ("qacc_warmstart",)
INT_FIELDS = ("eq_active", "geom_contype", "geom_conaffinity")
LACK, BILLY, DESK = ("Sawyer", "table_lack_0825"), ("Sawyer", "bookcase_billy_0191"), ("Baxter", "desk_mikael_1064")
# name -> model, the largest island every state of the case must show (None: as it comes; the file records it) and the contact slots the
# state must fit
CASES = {
    "free": dict(model=LACK, island=(9,), slots=48),
    "limit": dict(model=LACK, island=(9,), slots=48),
    "pinch": dict(model=LACK, island=(15,), slots=48),
    "grip_table": dict(model=LACK, island=(21,), slots=48),
    "weld": dict(model=LACK, island=(21, 12), slots=48),
    "table30": dict(model=LACK, island=(30,), slots=48),
    "welded39": dict(model=LACK, island=(39,), slots=48),
    "pile2": dict(model=BILLY, island=(12,), slots=128),
    "pile3": dict(model=BILLY, island=(18,), slots=128),
    "pile5": dict(model=BILLY, island=(30,), slots=128),
    "pile6": dict(model=BILLY, island=(36,), slots=128),
    "pile10": dict(model=BILLY, island=(60,), slots=128),
    "pile11": dict(model=BILLY, island=(66,), slots=512),
    "baxter": dict(model=DESK, island=None, slots=64),
}
MAX_ENVS = 8
# The reference's own consistency (tests/test_solve.py): M (qacc - qacc_smooth) = qfrc_constraint relative to the largest |qfrc_constraint|,
# and the cold against the warm start, relative to the largest |qacc|
IDENTITY_TOL, COLD_WARM_TOL = 1e-12, 1e-10
# How far from a threshold a stored state must stay (conditions).  A listed contact's float64 distance stays CONTACT_BAND away from the
# pair's margin: eight times what float32 does to a distance between bodies a metre or two from the origin (spacing 1.2e-7 to 2.4e-7 m;
# the device's closed-form distances were measured within 1.3e-7 m of the oracle's).  The band of the collision sweep (EDGE,
# 1e-4 m) cannot be asked of these states: a table leg at rest sinks 3e-5 m into the floor and a plank of 22 g 6e-6 m into the plank below,
# and the cases are parts at rest.  A limited joint stays
# LIMIT_ULPS float32 spacings of its limit away from the limit's threshold: the distance is the difference of two float32 values, exact in
# float32, so that the builds can only disagree through the rounding of the limit itself (Sawyer's open fingers rest 3.5e-7 m beyond theirs).
# What guards the comparison itself is stronger than either band: both CPU builds must list the same pairs, and the device's list is held to
# the reference's with the rule of tests/test_contacts_gpu.py (a pair that one side alone lists is within EDGE of its margin).
CONTACT_BAND, LIMIT_ULPS = 1e-6, 4
# A solve that does nothing must not pass: in every env the cold start's two candidates, qacc = 0 and qacc = qacc_smooth, miss the solution by at least
# START_FLOORS x the case's fp32 floor in the `island` measure (a part at rest has qacc = 0: such states are pushed by the generator)
START_FLOORS = 100.0
# A case whose fp32 floor exceeds this on `force` or `island` is no usable test state: rebuild it
VACUITY = 1e-2
# What fp32 alone does, per case: the three measures of the checker's float32 build (oracle/libfsim_cpu32.so through the C-ABI: one
# fsim_physics_forward for qacc, one fsim_physics_step for qvel) against the float64 reference, the largest over the states of the case,
# cold and warm start; tests/test_solve.py::test_what_fp32_alone_does prints them and checks that they still hold.  Rounded up in the last digit.
FLOOR = {
    "free": dict(force=1.567e-05, island=1.900e-04, step=1.595e-05),
    "limit": dict(force=3.761e-06, island=2.121e-06, step=3.884e-06),
    "pinch": dict(force=1.006e-06, island=1.004e-06, step=9.498e-07),
    "grip_table": dict(force=5.594e-06, island=5.501e-06, step=5.436e-06),
    "weld": dict(force=4.687e-05, island=4.687e-05, step=4.687e-05),
    "table30": dict(force=3.460e-06, island=3.448e-06, step=3.459e-06),
    "welded39": dict(force=1.888e-03, island=1.733e-03, step=1.888e-03),  # 1.3e-4 to 1.9e-3 per env: four stiff weld rows and a single pad contact
    "pile2": dict(force=1.079e-05, island=1.198e-05, step=1.079e-05),
    "pile3": dict(force=6.038e-06, island=6.962e-06, step=6.038e-06),
    "pile5": dict(force=4.490e-06, island=3.909e-06, step=4.490e-06),
    "pile6": dict(force=3.731e-06, island=2.663e-06, step=3.734e-06),
    "pile10": dict(force=1.990e-05, island=1.390e-05, step=1.989e-05),
    "pile11": dict(force=3.654e-05, island=2.777e-05, step=3.654e-05),
    "baxter": dict(force=1.440e-03, island=1.440e-03, step=1.440e-03),  # env 1; the others 3.3e-4 to 3.8e-4
}

_models = {}


def model(case, cases=None):
    from furniture_amd.mjcf.model import load_compiled
    key = (cases or CASES)[case]["model"]
    if key not in _models:
        _models[key] = load_compiled(*key)
    return _models[key]


def load(path=GOLDEN, cases=None):
    """name -> dict(st: state dict of [n, .] arrays, island: [n] the largest island of each env) of the cases (default: CASES) stored at path"""
    out = {}
    with np.load(path) as z:
        for name in (cases or CASES):
            st = {k: (z["%s/%s" % (name, k)].astype(np.int32) if k in INT_FIELDS else z["%s/%s" % (name, k)].astype(np.float64)) for k in FIELDS}
            st["cursor"] = None
            out[name] = dict(st=st, island=z["%s/island" % name].astype(np.int64))
    return out


def pack(cases):
    """the arrays of the file from {name: dict(st, island)}: float fields as float32"""
    out = {}
    for name, c in cases.items():
        for k in FIELDS:
            out["%s/%s" % (name, k)] = np.ascontiguousarray(c["st"][k], dtype=np.int32 if k in INT_FIELDS else np.float32)
        out["%s/island" % name] = np.asarray(c["island"], dtype=np.int32)
    return out


def robot_dofs(m):
    """every dof that is not one of a part's six"""
    part = (np.asarray(m.part_dofadr, dtype=np.int64)[:, None] + np.arange(6)[None, :]).reshape(-1)
    return np.setdiff1d(np.arange(m.nv), part)


def tree_dofs(m):
    adr = np.cumsum([0] + [int(k) for k in m.tree_dofnum])
    return [np.arange(adr[t], adr[t + 1]) for t in range(len(m.tree_dofnum))]


def island_sets(m, pairs, eq_active, constrained_dofs=()):
    """the constraint islands: [dof index array], largest first -- the trees that the contact pairs and the active welds join, and the single
    trees that a contact with static geometry or a row on one of `constrained_dofs` (an active joint limit) touches"""
    gt, pt, td = tree_of_geom(m), tree_of_part(m), tree_dofs(m)
    root = list(range(len(td)))

    def find(i):
        while root[i] != i:
            i = root[i]
        return i
    links = [(int(gt[a]), int(gt[b])) for a, b in pairs if a >= 0 and b >= 0]
    links += [(int(pt[int(m.eq_part1[k])]), int(pt[int(m.eq_part2[k])])) for k in range(m.neq) if eq_active[k]]
    dof_tree = np.asarray(m.dof_tree, dtype=np.int64)
    touched = {t for ab in links for t in ab if t >= 0} | {int(dof_tree[d]) for d in constrained_dofs}
    for a, b in links:
        if a >= 0 and b >= 0 and find(a) != find(b):
            root[find(b)] = find(a)
    groups = {}
    for t in sorted(touched):
        groups.setdefault(find(t), []).append(t)
    return sorted((np.concatenate([td[t] for t in ts]) for ts in groups.values()), key=lambda d: -len(d))


def put(osim, m, st, e, warm, iterations=200, tolerance=1e-14):
    """env e of a state dict into the oracle (contacts_reference.set_state without the forward(), with the warm start)"""
    d, mo = osim.data, osim.model
    osim.reset()
    d.qpos[:], d.qvel[:], d.ctrl[:], d.qfrc_applied[:] = st["qpos"][e], st["qvel"][e], st["ctrl"][e], st["qfrc_applied"][e]
    d.qacc_warmstart[:] = st["qacc_warmstart"][e] if warm else 0.0
    d.xfrc_applied[:] = 0.0
    for i, b in enumerate(np.asarray(m.arrays["part_bodyid"], dtype=np.int64)):
        d.xfrc_applied[int(b)] = st["xfrc_applied"][e][6 * i:6 * i + 6]
    if m.neq:
        mo.eq_data[:] = st["eq_data"][e].reshape(-1, 7)
        mo.eq_active[:] = st["eq_active"][e]
    mo.geom_contype[:], mo.geom_conaffinity[:] = st["geom_contype"][e], st["geom_conaffinity"][e]
    if st.get("cursor") is not None:  # (the Cursor agent: its cursor bodies stand where the env's cursor says, as contacts_reference.set_state puts them)
        for k, b in enumerate(m.arrays["cursor_bodyid"]):
            mo.body_pos[int(b)] = st["cursor"][e][3 * k:3 * k + 3]
    osim.set_solver(iterations, tolerance, "newton")


def reference(osim, m, st, e, warm=False, iterations=200, tolerance=1e-14, step=True):
    """dict at env e: qacc, qfrc_constraint, qacc_smooth, M, contacts [(g1, g2)], dists, iters of one forward(); islands (dof index arrays,
    largest first); and acc_step = (qvel after one step() - qvel) / h"""
    put(osim, m, st, e, warm, iterations, tolerance)
    osim.forward()
    d = osim.data
    c = lambda a: np.array(a, dtype=np.float64)
    ref = dict(qacc=c(d.qacc), qfrc_constraint=c(d.qfrc_constraint), qacc_smooth=c(d.qacc_smooth), M=osim.full_M(), contacts=osim.contacts(),
               dists=np.array(osim.contact_dists()), iters=int(osim.last_solver_iters))
    ref["islands"] = island_sets(m, ref["contacts"], st["eq_active"][e], constrained_dofs=np.nonzero(ref["qfrc_constraint"])[0])
    if step:
        put(osim, m, st, e, warm, iterations, tolerance)
        osim.step()
        ref["acc_step"] = (c(d.qvel) - st["qvel"][e]) / float(m.arrays["opt"][0])
    return ref


# ---- the measures -------------------------------------------------------------------------------------------------------------------------
def force(qacc, ref):
    return cref.force_measure(ref["M"] @ (np.asarray(qacc, dtype=np.float64) - ref["qacc_smooth"]), ref["qfrc_constraint"])


def island(qacc, ref):
    err = np.abs(ref["M"] @ (np.asarray(qacc, dtype=np.float64) - ref["qacc_smooth"]) - ref["qfrc_constraint"])
    smooth = np.abs(ref["M"] @ ref["qacc_smooth"])
    worst = 0.0
    for dofs in ref["islands"]:
        scale = max(np.abs(ref["qfrc_constraint"][dofs]).max(), smooth[dofs].max())
        worst = max(worst, err[dofs].max() / (scale if scale > 0 else 1.0))
    return worst


def step(acc_step, ref):
    scale = np.abs(ref["qfrc_constraint"]).max()
    return np.abs(ref["M"] @ (np.asarray(acc_step, dtype=np.float64) - ref["acc_step"])).max() / (scale if scale > 0 else 1.0)


MEASURES = ("force", "island", "step")


def measure(qacc, acc_step, ref):
    return dict(force=force(qacc, ref), island=island(qacc, ref), step=step(acc_step, ref))


# ---- the conditions on a stored state --------------------------------------------------------------------------------------------------------
def robot_geom(m):
    return np.asarray(m.arrays["body_partid"])[np.asarray(m.arrays["geom_bodyid"])] < 0


def pair_key(g1, g2):
    return (int(min(g1, g2)), int(max(g1, g2)))


def conditions(m, case, st, e, ref, pairs32, cases=None):
    """the problems of env e as a list of strings (empty: the state is usable).  ref: reference() at the state, pairs32: the contact pairs
    the checker's float32 build lists there, cases: the table that holds `case` (default: CASES).
    Threshold-free: both builds list the same pairs; no float64 contact distance within CONTACT_BAND of the pair's margin; no limited joint
    within LIMIT_ULPS float32 spacings of the threshold of its limit.  The one exception: what sits EXACTLY on a threshold -- a pair of two robot geoms whose float64
    distance is the margin to 1e-9 m or that only the float32 build lists (Sawyer's l0 sphere on the base cylinder, distance 0: it carries no
    force), and a joint whose float32 position is its float32 limit (Sawyer's open fingers).
    Path reached: the largest island is the case's.  Slot capacity: the contacts fit the case's slots."""
    bad = []
    robot, margin = robot_geom(m), np.asarray(m.arrays["geom_margin"], dtype=np.float64)
    p64, p32 = sorted(pair_key(*p) for p in ref["contacts"]), sorted(pair_key(*p) for p in pairs32)
    for k in set(p64) ^ set(p32):
        if not (robot[k[0]] and robot[k[1]] and k not in set(p64)):
            bad.append("pair %s is listed by one build only" % (k,))
    if not bad and [p for p in p64] != [p for p in p32 if p in set(p64)]:
        bad.append("the builds list different numbers of contacts for a pair")
    for (g1, g2), d in zip(ref["contacts"], ref["dists"]):
        gap = abs(d - max(margin[g1], margin[g2]))
        if gap <= CONTACT_BAND and not (robot[g1] and robot[g2] and gap <= 1e-9):
            bad.append("pair %s at %.3e m is within %.0e m of its margin" % (pair_key(g1, g2), d, CONTACT_BAND))
    A = m.arrays
    lim = np.asarray(A["jnt_limited"]).astype(bool)
    qa = np.asarray(A["jnt_qposadr"], dtype=np.int64)[lim]
    rg = np.asarray(A["jnt_range"], dtype=np.float64).reshape(-1, 2)[lim]
    mg = np.asarray(A["jnt_margin"], dtype=np.float64)[lim] if "jnt_margin" in A else np.zeros(int(lim.sum()))
    q = np.asarray(st["qpos"][e])[qa]
    for j in range(len(qa)):
        for dist, end in ((q[j] - rg[j, 0], rg[j, 0]), (rg[j, 1] - q[j], rg[j, 1])):
            if abs(dist - mg[j]) <= LIMIT_ULPS * np.spacing(np.float32(abs(end))) and not (mg[j] == 0 and np.float32(q[j]) == np.float32(end)):
                bad.append("joint at qpos[%d] is %.3e from the threshold of its limit" % (qa[j], dist - mg[j]))
    cases = cases or CASES
    want = cases[case]["island"]
    size = island_dofs(m, ref["contacts"], st["eq_active"][e])[0]
    if want is not None and size not in want:
        bad.append("the largest island has %d dofs, the case wants %s" % (size, want))
    if len(ref["contacts"]) > cases[case]["slots"] or len(pairs32) > cases[case]["slots"]:
        bad.append("%d contacts do not fit %d slots" % (max(len(ref["contacts"]), len(pairs32)), cases[case]["slots"]))
    return bad


# ---- the checker's builds through the C-ABI ------------------------------------------------------------------------------------------------
def abi_solve(path, m, st, warm):
    """(qacc [n, nv] of one fsim_physics_forward, (qvel after one fsim_physics_step - qvel) / h, contact pairs per env) of the library at
    `path` (host pointers: oracle/libfsim_cpu.so, oracle/libfsim_cpu32.so) on every env of the state"""
    from furniture_amd import sim
    from tests.abi_session import Abi, Session
    n = len(st["qpos"])
    ws = st["qacc_warmstart"] if warm else np.zeros((n, m.nv))
    ses = Session(Abi(path), m.to_blob(), n, auto_reset=0)
    more = dict(cursor=st["cursor"]) if st.get("cursor") is not None else {}
    write = lambda: ses.set_state(m, **dict({k: st[k] for k in cref.FIELDS if st[k].shape[1] > 0}, qacc_warmstart=ws, **more))
    write()
    ses.forward()
    buf, sp = np.zeros((n, m.nv), np.float32), sim.StatePtrs()  # (qacc is not among the fields Session.get_state knows)
    sp.qacc = buf.ctypes.data
    ses.abi.check(ses.abi.L.fsim_get_state(ses.h, ctypes.byref(sp)))
    got = ses.get_state(m, "contact_geoms", "ncon")
    pairs = [[(int(a), int(b)) for a, b in got["contact_geoms"][e].reshape(-1, 2) if a >= 0] for e in range(n)]
    write()
    ses.abi.L.fsim_physics_step.argtypes = [ctypes.c_void_p, ctypes.c_int]
    ses.abi.check(ses.abi.L.fsim_physics_step(ses.h, 1))
    qvel = ses.get_state(m, "qvel")["qvel"].astype(np.float64)
    ses.close()
    return buf.astype(np.float64), (qvel - st["qvel"]) / float(m.arrays["opt"][0]), pairs


# ---- the kernel sets of the device ----------------------------------------------------------------------------------------------------------
ENV_VARS = ("FSIM_MW", "FSIM_GENERIC", "FSIM_NCON_MAX")
# kernel set -> model, the environment fsim_create reads, the variant the handle must report and its contact slots
KSETS = {
    "spec-mw0": dict(model=LACK, env=dict(FSIM_MW="0"), variant="sawyer_table_lack_0825", slots=48),
    "spec-mwall": dict(model=LACK, env=dict(FSIM_MW="all"), variant="sawyer_table_lack_0825", slots=48),
    "generic-mw0": dict(model=LACK, env=dict(FSIM_MW="0", FSIM_GENERIC="1"), variant="generic", slots=48),
    "generic-mwall": dict(model=LACK, env=dict(FSIM_MW="all", FSIM_GENERIC="1"), variant="generic", slots=48),
    "generic2": dict(model=LACK, env=dict(FSIM_MW="0", FSIM_NCON_MAX="128"), variant="generic2", slots=128),
    "generic8": dict(model=LACK, env=dict(FSIM_MW="0", FSIM_NCON_MAX="512"), variant="generic8", slots=512),
    "billy-generic2": dict(model=BILLY, env=dict(FSIM_MW="0"), variant="generic2", slots=128),
    "billy-generic8": dict(model=BILLY, env=dict(FSIM_MW="0", FSIM_NCON_MAX="512"), variant="generic8", slots=512),
    "desk-mw0": dict(model=DESK, env=dict(FSIM_MW="0"), variant="generic", slots=64),
    "desk-mwall": dict(model=DESK, env=dict(FSIM_MW="all"), variant="generic", slots=64),
}


@contextlib.contextmanager
def environment(env):
    """the variables fsim_create reads, set for the creation of a handle and restored (as test_specialised_and_generic_kernels_agree does)"""
    saved = {k: os.environ.get(k) for k in ENV_VARS}
    for k in ENV_VARS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def handle(cache, ks, n=MAX_ENVS):
    """the handle of a kernel set and its twin, n envs each, made once per cache (a dict that the caller closes with close_handles)"""
    if ks not in cache:
        from furniture_amd.mjcf.model import load_compiled
        from furniture_amd.sim import FSim
        k = KSETS[ks]
        with environment(k["env"]):
            cache[ks] = (FSim(load_compiled(*k["model"]), n), FSim(load_compiled(*k["model"]), n))
        for sim in cache[ks]:
            assert sim.kernel_variant == k["variant"] and sim.max_contacts == k["slots"], (ks, sim.kernel_variant, sim.max_contacts)
    return cache[ks]


def close_handles(cache):
    for pair in cache.values():
        for sim in pair:
            sim.close()
    cache.clear()

"""Generate tests/golden/solve_bits.npz: the raw bits the step kernels leave on a handful of small seeded scenarios of Sawyer + table_lack_0825 that
between them reach every factorisation path of the Newton solve (tests/solve_bits_common.py), under FSIM_MW = 0, 1 and all.

Run ONCE, on the GPU, against the library whose arithmetic is to be pinned (FSIM_LIB=<that libfsim.so>): tests/test_solve_bits_gpu.py then holds every
later library to those bits.  The start snapshots and the actions are stored in the file, so the test replays exactly these inputs.  The island sizes each
scenario is meant to produce are checked here twice: from the device's own contact list after every step, and from the CPU checker's (oracle/) contact
list at the state the device left after the first step that shows the wanted island."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from furniture_amd.mjcf.model import load_compiled  # noqa: E402
from furniture_amd import transform_utils as T  # noqa: E402
from tests.scenarios import pinch_attach_state  # noqa: E402
from tests.solve_bits_common import CASES, FLOAT_FIELDS, GOLDEN, LIMIT_JOINT, MODES, SNAP, island_dofs, record  # noqa: E402


def post_reset(m, n):
    """SNAP fields + body poses of n freshly reset envs (numpy)"""
    import torch
    from furniture_amd.envs import ResetTableSampler, make_config
    from furniture_amd.sim import FSim, default_config
    cfg = default_config()
    cfg.max_episode_steps, cfg.auto_reset, cfg.multi_wave = 1000, 0, 1
    sim = FSim(m, n, config=cfg)
    sim.set_reset_tables(*ResetTableSampler(m, make_config(), 123, 0, n).draw())
    obs = torch.zeros((n, sim.obs_dim), device=sim.device)
    sim.reset(None, obs)
    sim.sync()
    sim.physics_forward()
    st = {k: v.cpu().numpy() for k, v in sim.get_state(*(SNAP + ["xpos", "xquat"])).items()}
    sim.close()
    return st


def start_states(m):
    base = post_reset(m, 16)
    nv = m.nv

    def take(n):
        s = {k: base[k][:n].copy() for k in SNAP}
        s["qvel"], s["qacc_warmstart"] = np.zeros((n, nv), np.float32), np.zeros((n, nv), np.float32)
        return s

    def pinch(s, gaps, ghost_table, press=0.0):
        for e, gap in enumerate(gaps):
            q, xf, masks = pinch_attach_state(m, base["qpos"][e].astype(np.float64), base["xpos"][e].reshape(-1, 3).astype(np.float64),
                                              base["xquat"][e].reshape(-1, 4).astype(np.float64), gap=gap)
            if ghost_table:
                for g, (t, a) in masks.items():
                    s["geom_contype"][e, g], s["geom_conaffinity"][e, g] = t, a
            if press:  # a constant force on the floating table, through its connector and along the connector axis, that keeps it pressed on the leg's end
                tp, la = int(m.conn_partid[4]), m.part_qposadr[0]
                ta = m.part_qposadr[tp]
                up = T.quat2mat_wxyz(q[la + 3:la + 7])[:, 2]
                site = q[ta:ta + 3] + T.quat2mat_wxyz(q[ta + 3:ta + 7]) @ m.site_pos[m.conn_siteid[4]]
                f = -press * 9.81 * float(m.body_mass[m.part_bodyid[tp]]) * up
                xf = xf.reshape(-1, 6).copy()
                xf[tp, :3] += f
                xf[tp, 3:] += np.cross(site - q[ta:ta + 3], f)
                xf = xf.reshape(-1)
            s["qpos"][e], s["xfrc_applied"][e] = q, xf
        return s

    rng = np.random.RandomState(5)

    def grip_actions(n, steps, connect):
        a = rng.uniform(-0.3, 0.3, (steps, n, 9)).astype(np.float32)
        a[:, :, 7], a[:, :, 8] = 1.0, connect  # gripper closed on the leg
        return a

    out = {}
    c = CASES["free"]
    a = rng.uniform(-1, 1, (c["steps"], c["n"], 9)).astype(np.float32)
    a[:, :, 8] = -1.0  # no connect
    out["free"] = (take(c["n"]), a)
    c = CASES["pinch"]
    out["pinch"] = (pinch(take(c["n"]), [0.02] * c["n"], True), grip_actions(c["n"], c["steps"], -1.0))
    c = CASES["grip_table"]  # the table stays solid, starts a hair inside the leg's connector face and is pressed on it with a fifth of its weight
    out["grip_table"] = (pinch(take(c["n"]), [-0.0005] * c["n"], False, press=0.2), grip_actions(c["n"], c["steps"], -1.0))
    c = CASES["limit"]
    s = take(c["n"])
    s["qpos"][:, LIMIT_JOINT] = m.jnt_range[LIMIT_JOINT][1] + 0.01
    a = np.zeros((c["steps"], c["n"], 9), np.float32)
    a[:, :, 8] = -1.0
    out["limit"] = (s, a)
    c = CASES["weld"]
    out["weld"] = (pinch(take(c["n"]), [0.02] * c["n"], True), grip_actions(c["n"], c["steps"], 1.0))
    return out


def oracle_islands(m, rec_last, n):
    """largest island per env from the CPU checker's contact list at the state the device ended in"""
    from oracle.oracle_sim import OracleSim
    out = []
    for e in range(n):
        o = OracleSim(m)
        o.reset()
        o.data.qpos[:] = rec_last["qpos"][e].view(np.float32)
        o.model.geom_contype[:], o.model.geom_conaffinity[:] = rec_last["geom_contype"][e], rec_last["geom_conaffinity"][e]
        o.model.eq_active[:] = rec_last["eq_active"][e]
        o.forward()
        out.append(island_dofs(m, o.contacts(), rec_last["eq_active"][e])[0])
        o.close()
    return np.array(out, dtype=np.int32)


def main():
    m = load_compiled("Sawyer", "table_lack_0825")
    out, missed = {}, []

    def expect(ok, *what):
        if not ok:
            missed.append(what)
            print("MISSED", what, flush=True)

    for name, (snap, acts) in start_states(m).items():
        c = CASES[name]
        lo, hi = c["island"]
        snap = {k: (np.ascontiguousarray(v, dtype=np.float32).view(np.int32) if k in FLOAT_FIELDS else np.ascontiguousarray(v, dtype=np.int32)) for k, v in snap.items()}
        for k, v in snap.items():
            out["%s/snap/%s" % (name, k)] = v
        out["%s/actions" % name] = acts
        for mode in MODES:
            rec = record(m, mode, snap, acts)
            isl = rec["island"]
            print("%-10s FSIM_MW=%-3s island (max per step over envs) %s  Newton iterations per step (max over envs) %s  team steps %s" % (
                name, mode, isl.max(axis=1).tolist(), rec["niter"].max(axis=1).tolist(), rec["mw_steps"][-1].tolist()), flush=True)
            expect(((isl >= lo) & (isl <= hi)).any(), name, mode, "no env reached an island of %d..%d dofs" % (lo, hi), isl.tolist())
            if mode == "0":  # the CPU checker's view of the islands, at the state the device left after the first step that shows the wanted island
                hit = ((isl >= lo) & (isl <= hi)).any(axis=1)
                t = int(np.argmax(hit)) if hit.any() else len(hit) - 1
                last = dict(qpos=rec["qpos"][t], eq_active=rec["eq_active"][t], geom_contype=snap["geom_contype"], geom_conaffinity=snap["geom_conaffinity"])
                if name != "weld":  # (a connect rewrites the geom masks of both groups: the weld case is checked on its welds alone)
                    oi = oracle_islands(m, last, c["n"])
                    print("%-10s CPU checker, state after step %d: largest island per env %s (device: %s)" % (name, t + 1, oi.tolist(), isl[t].tolist()), flush=True)
                    expect(((oi >= lo) & (oi <= hi)).any(), name, "the CPU checker finds no island of %d..%d dofs" % (lo, hi), oi.tolist())
            if name == "weld":
                expect(rec["eq_active"][-1].any(axis=1).all(), name, mode, "no weld became active")
            if name == "limit":
                q0, q1 = snap["qpos"].view(np.float32)[:, LIMIT_JOINT], rec["qpos"][0].view(np.float32)[:, LIMIT_JOINT]
                print("limit      wrist joint: start %s, after step 1 %s (range end %.4f)" % (q0.tolist(), q1.tolist(), m.jnt_range[LIMIT_JOINT][1]), flush=True)
                expect((q1 < q0 - 1e-4).all(), name, mode, "the limit row did not push the wrist joint back", q1.tolist())
            for k, v in rec.items():
                out["%s/%s/%s" % (name, mode, k)] = v
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN) // 1024, "KB")
    assert not missed, missed


if __name__ == "__main__":
    main()

"""Shared by scripts/make_golden_solve_bits.py (writes tests/golden/solve_bits.npz) and tests/test_solve_bits_gpu.py (replays it): stepping a stored
start snapshot with stored actions and recording every word the step kernel leaves, plus the constraint islands of each env -- the quantity that
selects the factorisation path of the Newton solve (csrc/fsim_solver.hpp fs_chol_solve):

  * islands of <= 16 dofs are factored in the wave's 16-lane rows: fs_chol_phase<6> / <12> / <16> by the fullest row (the free Sawyer is 9 dofs, a
    part 6, the Sawyer holding a part 15);
  * an island of 17..31 dofs is one tile on the matrix cores (fs_chol_mfma / fs_newton_mfma).

Pure numpy except for `record`, which needs a GPU."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_bits.npz")
MODES = ("0", "1", "all")  # FSIM_MW: one wave per env, the scheduler's rule (bundles + four-wave teams), four waves for every env
MW_K = "51"                # FSIM_MW_K: the rule's threshold (Newton iterations of the previous step), lowered so that gripping envs do join a team
SNAP = ["qpos", "qvel", "qacc_warmstart", "qfrc_bias", "ctrl", "qfrc_applied", "xfrc_applied", "eq_active", "eq_data", "geom_contype", "geom_conaffinity", "group", "env_block"]
FLOAT_FIELDS = ("qpos", "qvel", "qacc_warmstart", "qfrc_bias", "ctrl", "qfrc_applied", "xfrc_applied", "eq_data")
# name -> (envs, steps, what the islands of the case must show: (lo, hi) of the largest island of the case, in dofs)
CASES = {
    "free": dict(n=16, steps=6, island=(9, 9)),          # rows of 9 and 6 dofs: fs_chol_phase<12> (robot + a part in one row), <6> once only parts still move
    "pinch": dict(n=8, steps=6, island=(15, 15)),        # robot + the leg it pinches: one 15-dof row, fs_chol_phase<16>, cached body pairs
    "grip_table": dict(n=8, steps=6, island=(17, 31)),   # the pinched leg touches the (solid) table: robot + leg + table, the MFMA tile
    "limit": dict(n=2, steps=6, island=(9, 9)),          # wrist joint beyond its upper limit: an active limit row in the robot's island
    "weld": dict(n=2, steps=6, island=(17, 31)),         # pinch + connect: the leg is welded to the table in step 1 (anyweld), robot + leg + table
}
LIMIT_JOINT = 6  # right_j6, range +-4.7124


def tree_of_geom(m):
    """geom -> kinematic tree (-1: static geometry), via the nearest ancestor body that has dofs"""
    out = np.full(m.ngeom, -1, dtype=np.int64)
    for g in range(m.ngeom):
        b = int(m.geom_bodyid[g])
        while b > 0 and int(m.body_dofnum[b]) == 0:
            b = int(m.body_parentid[b])
        if b > 0:
            out[g] = int(m.dof_tree[int(m.body_dofadr[b])])
    return out


def tree_of_part(m):
    return np.array([int(m.dof_tree[int(a)]) for a in m.part_dofadr])


def island_dofs(m, pairs, eq_active):
    """sizes (dofs, descending) of the islands that the contact pairs [(geom, geom)] and the active welds join the trees into"""
    gt, pt = tree_of_geom(m), tree_of_part(m)
    ntree = len(m.tree_dofnum)
    root = list(range(ntree))

    def find(i):
        while root[i] != i:
            i = root[i]
        return i
    links = [(gt[a], gt[b]) for a, b in pairs if a >= 0 and b >= 0]
    links += [(pt[int(m.eq_part1[k])], pt[int(m.eq_part2[k])]) for k in range(m.neq) if eq_active[k]]
    for a, b in links:
        if a >= 0 and b >= 0:
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                root[rb] = ra
    size = {}
    for t in range(ntree):
        size[find(t)] = size.get(find(t), 0) + int(m.tree_dofnum[t])
    return sorted(size.values(), reverse=True)


def record(m, mode, snap, acts):
    """Step the envs of the snapshot (dict of numpy arrays, SNAP fields; float fields stored as their int32 bits) under FSIM_MW=mode; returns a dict of
    int32 arrays [steps, n, ...]: the raw bits of everything the step leaves, and the device's own account of the path it took."""
    import torch
    from furniture_amd.sim import E_MW_STEPS, E_NITER, FSim, INFO_DIM, default_config
    saved = {k: os.environ.get(k) for k in ("FSIM_MW", "FSIM_MW_K")}
    os.environ["FSIM_MW"], os.environ["FSIM_MW_K"] = mode, MW_K  # (read by fsim_create)
    try:
        n = acts.shape[1]
        cfg = default_config()
        cfg.max_episode_steps, cfg.auto_reset = 1000, 0
        sim = FSim(m, n, config=cfg)
        probe = FSim(m, n, config=cfg)  # (the contact list is a read-back of the raw physics entry points: taken on a copy of the state, so that the stepped handle is left alone)
        sim.set_state(**{k: (torch.as_tensor(v).view(torch.float32) if k in FLOAT_FIELDS else v) for k, v in snap.items()})
        dev = sim.device
        act, obs, rew = torch.zeros((n, sim.dof_action), device=dev), torch.zeros((n, sim.obs_dim), device=dev), torch.zeros(n, device=dev)
        done, info = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, INFO_DIM), dtype=torch.int32, device=dev)
        out = {}
        for t in range(acts.shape[0]):
            act.copy_(torch.as_tensor(acts[t]))
            torch.cuda.synchronize()
            sim.step(act, obs, rew, done, info)
            sim.sync()
            full = sim.get_state(*SNAP)
            probe.set_state(**full)
            probe.physics_forward()
            st = {k: v.cpu().numpy() for k, v in full.items()}
            st.update({k: v.cpu().numpy() for k, v in probe.get_state("ncon", "contact_geoms").items()})
            row = dict(qpos=st["qpos"].view(np.int32), qvel=st["qvel"].view(np.int32), qacc_warmstart=st["qacc_warmstart"].view(np.int32),
                       obs=obs.cpu().numpy().view(np.int32), reward=rew.cpu().numpy().view(np.int32), done=done.cpu().numpy().astype(np.int32),
                       info=info.cpu().numpy(), niter=st["env_block"][:, E_NITER], mw_steps=st["env_block"][:, E_MW_STEPS],
                       ncon=st["ncon"][:, 0], eq_active=st["eq_active"],
                       island=np.array([island_dofs(m, st["contact_geoms"][e].reshape(-1, 2)[:st["ncon"][e, 0]], st["eq_active"][e])[0] for e in range(n)], dtype=np.int32))
            for k, v in row.items():
                out.setdefault(k, []).append(np.ascontiguousarray(v))
        sim.close()
        probe.close()
        return {k: np.stack(v) for k, v in out.items()}
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v

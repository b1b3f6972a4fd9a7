"""Time fsim_dynamics (include/fsim_dynamics.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random steps.
Cases: all four outputs over all dofs; the arm tree's nine dofs with minv alone; and, to see which stage binds, each output alone over all
dofs and mass + bias over the arm's seven dofs.  HIP events around calls on the handle's stream (one launch: k_dynamics), median of the
repeats (second argument, 20) after 5 warm-up launches.  One JSON line per case; bound_ms is the bytes bound of the case -- the env record
read once plus each requested output written once, at 8 TB/s -- and ratio = ms over it."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from furniture_amd.dynamics import Dynamics, arm_dofs, tree_dofs
from furniture_amd.envs import ResetTableSampler, make_config
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import INFO_DIM, FSim, default_config

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
HBM_BYTES_PER_MS = 8e9  # 8 TB/s

furniture = "table_lack_0825"
m = load_compiled("Sawyer", furniture)
ecfg = make_config(unity=False, record_vid=False, furniture_name=furniture, seed=7)
cfg = default_config()
cfg.auto_reset = 0
sim = FSim(m, n, config=cfg)
p, nz = ResetTableSampler(m, ecfg, 7, 0, n).draw()
sim.set_reset_tables(p, nz)
dev = sim.device
obs, rew = torch.zeros((n, sim.obs_dim), device=dev), torch.zeros(n, device=dev)
done, info = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, INFO_DIM), dtype=torch.int32, device=dev)
sim.reset(None, obs)
sim.sync()
rng = np.random.RandomState(0)
for _ in range(3):
    act = torch.as_tensor(rng.uniform(-1, 1, (n, sim.dof_action)).astype(np.float32), device=dev)
    torch.cuda.synchronize()
    sim.step(act, obs, rew, done, info)
    sim.sync()


def median_ms(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    with torch.cuda.stream(sim.torch_stream):
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


arm, tree = arm_dofs(m)[0], tree_dofs(m, 0)
off = dict(mass=False, inverse=False, bias=False, gravity=False)
cases = [("all_dofs_all_four", None, dict(mass=True, inverse=True, bias=True, gravity=True)), ("arm_tree_minv", tree, dict(off, inverse=True)),
         ("all_dofs_mass", None, dict(off, mass=True)), ("all_dofs_minv", None, dict(off, inverse=True)), ("all_dofs_bias", None, dict(off, bias=True)),
         ("all_dofs_gravity", None, dict(off, gravity=True)), ("arm_mass_bias", arm, dict(off, mass=True, bias=True))]
for name, dofs, kw in cases:
    sim.set_dynamics(Dynamics(dofs=dofs, **kw))
    out = sim.dynamics()
    t = median_ms(lambda: sim.dynamics(out=out))
    torch.cuda.synchronize()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    rec_bytes = n * sim.stride * 4
    bound = (out_bytes + rec_bytes) / HBM_BYTES_PER_MS
    print(json.dumps(dict(case=name, envs=n, dofs=m.nv if dofs is None else len(dofs), nv=m.nv, outputs=sorted(out), reps=reps, ms=round(t, 4), record_mb=round(rec_bytes / 1e6, 2),
                          output_mb=round(out_bytes / 1e6, 2), bound_ms=round(bound, 4), ratio=round(t / bound, 2), gb_per_s=round((out_bytes + rec_bytes) / t / 1e6, 1))), flush=True)
sim.close()

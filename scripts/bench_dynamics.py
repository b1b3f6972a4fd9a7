"""Time fsim_dynamics (include/fsim_dynamics.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random steps.
Cases: all four outputs over all dofs; the arm tree's nine dofs with minv alone; and, to see which stage binds, each output alone over all
dofs and mass + bias over the arm's seven dofs.  HIP events around calls on the handle's stream (one launch: k_dynamics), median of the
repeats (second argument, 20) after 5 warm-up launches.  One JSON line per case; bound_ms is the bytes bound of the case -- the env record
read once plus each requested output written once, at 8 TB/s -- and ratio = ms over it."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.dynamics import Dynamics, arm_dofs, tree_dofs

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
HBM_BYTES_PER_MS = 8e9  # 8 TB/s

m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps, warmup=5)


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

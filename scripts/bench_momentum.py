"""Time fsim_momenta (include/fsim_momentum.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random steps.
Cases: one sensor per part, without and with the Jacobian; the parts, all parts together and the robot with the Jacobian and the energy; 64
sensors with everything.  For scale, from the same session: fsim_dynamics of all dofs with mass and bias, the pass whose first stages
k_momenta repeats.  HIP events around calls on the handle's stream (one launch each), median of the repeats (second argument, 20) after 5
warm-up launches.  One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.dynamics import Dynamics
from furniture_amd.momentum import MomentumSensor, MomentumSet, all_parts_sensor, part_sensors, robot_sensor

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20

m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps, warmup=5)


def report(name, t, out, **kw):
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    print(json.dumps(dict(case=name, envs=n, reps=reps, ms=round(t, 4), us_per_env=round(1e3 * t / n, 4), output_mb=round(out_bytes / 1e6, 2), **kw)), flush=True)


parts = part_sensors(m)
groups = parts + [all_parts_sensor(m), robot_sensor(m)]
links = [MomentumSensor(b) for b in m.meta["body_names"] if b.startswith("right_l")]  # each arm link with its subtree
many = (groups + 8 * links)[:64]  # (a set may hold a sensor more than once)
for name, sensors, jac, energy in [("parts", parts, False, False), ("parts_jacobian", parts, True, False), ("parts_all_robot_jacobian_energy", groups, True, True),
                                   ("%d_sensors_jacobian_energy" % len(many), many, True, True)]:
    sim.set_momenta(MomentumSet(sensors, jacobian=jac, energy=energy))
    out = sim.momenta()
    t = median_ms(lambda: sim.momenta(out=out))
    torch.cuda.synchronize()
    report(name, t, out, sensors=len(sensors))
sim.set_momenta(None)

sim.set_dynamics(Dynamics())
out = sim.dynamics()
report("dynamics_mass_bias_all_dofs", median_ms(lambda: sim.dynamics(out=out)), out)
sim.set_dynamics(None)
sim.close()

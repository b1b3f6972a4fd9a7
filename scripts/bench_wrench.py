"""Time fsim_wrenches (include/fsim_wrench.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random steps.
Cases: the wrist sensor alone; the wrist and one sensor per part with external, qacc and qfrc_constraint; 64 sensors with everything.  For
scale, from the same session: fsim_contact_forces of one sensor per part with the contact list, and -- last, it rewrites the records' warm
start -- fsim_physics_forward, the pass both repeat on the generic one-wave kernel.  HIP events around calls on the handle's stream (one
launch each), median of the repeats (second argument, 20) after 5 warm-up launches.  One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.contacts import ContactSet
from furniture_amd.contacts import part_sensors as contact_part_sensors
from furniture_amd.frames import Frame
from furniture_amd.wrench import WrenchSensor, WrenchSet, part_sensors, wrist_sensor

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20

m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps, warmup=5)


def report(name, t, out, **kw):
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    print(json.dumps(dict(case=name, envs=n, reps=reps, ms=round(t, 4), us_per_env=round(1e3 * t / n, 4), output_mb=round(out_bytes / 1e6, 2), **kw)), flush=True)


wrist, parts = wrist_sensor(m), part_sensors(m)
bodies = [WrenchSensor(Frame(body=b)) for b in m.meta["body_names"] if b.startswith("right_l")]
many = (wrist + parts + 8 * bodies)[:64]  # (a set may hold a sensor more than once)
for name, sensors, ext, joint in [("wrist", wrist, False, False), ("wrist_and_parts_external_joint", wrist + parts, True, True), ("%d_sensors_external_joint" % len(many), many, True, True)]:
    sim.set_wrenches(WrenchSet(sensors, external=ext, joint=joint))
    out = sim.wrenches()
    t = median_ms(lambda: sim.wrenches(out=out))
    torch.cuda.synchronize()
    report(name, t, out, sensors=len(sensors), slots=sim.max_contacts, status_or=int(out["wrench_status"].max()))
sim.set_wrenches(None)

sim.set_contacts(ContactSet(contact_part_sensors(m), contacts=True))
out = sim.contact_forces()
report("contact_forces_part_sensors_with_list", median_ms(lambda: sim.contact_forces(out=out)), out)
sim.set_contacts(None)
report("physics_forward", median_ms(sim.physics_forward), {}, kernel=sim.kernel_variant)
sim.close()

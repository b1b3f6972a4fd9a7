"""Time fsim_contact_forces (include/fsim_contacts.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: one sensor per part (the net-contact-force tensor) alone; the same with the contact list; 64 sensors with the list.  For
scale, from the same session: fsim_frame_state of 8 site frames with Jacobians, fsim_dynamics with all four outputs over all dofs, and --
last, it rewrites the records' warm start -- fsim_physics_forward, the pass fsim_contact_forces repeats on the generic one-wave kernel.
HIP events around calls on the handle's stream (one launch each), median of the repeats (second argument, 20) after 5 warm-up launches.
One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench_common
from furniture_amd.contacts import ContactSensor, ContactSet, part_sensors
from furniture_amd.dynamics import Dynamics
from furniture_amd.frames import Frame, FrameSensor, FrameSet

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20

m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps, warmup=5)


def report(name, t, out, **kw):
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    print(json.dumps(dict(case=name, envs=n, reps=reps, ms=round(t, 4), us_per_env=round(1e3 * t / n, 4), output_mb=round(out_bytes / 1e6, 2), **kw)), flush=True)


parts = part_sensors(m)
cg = [int(g) for g in np.asarray(m.arrays["cg_orig"])]
many = (parts + 3 * [ContactSensor([g]) for g in cg])[:64]  # (a set may hold a sensor more than once)
for name, sensors, lst in [("part_sensors", parts, False), ("part_sensors_with_list", parts, True), ("%d_sensors_with_list" % len(many), many, True)]:
    sim.set_contacts(ContactSet(sensors, contacts=lst))
    out = sim.contact_forces()
    t = median_ms(lambda: sim.contact_forces(out=out))
    torch.cuda.synchronize()
    report(name, t, out, sensors=len(sensors), slots=sim.max_contacts, listed_per_env=round(float(out["contact_count"].sum()) / n, 2) if name == "part_sensors" else None,
           status_or=int(out["contact_status"].max()))
sim.set_contacts(None)

sites = [s for s in m.meta["site_names"]][:8]
sim.set_frames(FrameSet([FrameSensor(Frame(site=s)) for s in sites], velocity=True, jacobian=True))
out = sim.frame_state()
report("frame_state_8_sites_jacobian", median_ms(lambda: sim.frame_state(out=out)), out)
sim.set_frames(None)
sim.set_dynamics(Dynamics(mass=True, inverse=True, bias=True, gravity=True))
out = sim.dynamics()
report("dynamics_all_dofs_all_four", median_ms(lambda: sim.dynamics(out=out)), out)
sim.set_dynamics(None)
report("physics_forward", median_ms(sim.physics_forward), {}, kernel=sim.kernel_variant)
sim.close()

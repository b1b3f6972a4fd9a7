"""Time fsim_frame_state (include/fsim_frames.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: 8 sensors (the four connector pairs, the grip site in the world, the grip site in the table top's frame, two legs in the
world) with pose only, with pose + vel and with everything; 64 sensors (the same, repeated) with everything.  HIP events around calls on the
handle's stream (one launch: k_frame_state), median of the repeats (second argument, 20).  One JSON line per case; bound_ms is the bytes bound
of the case -- the env record read once plus each requested output written once, at 8 TB/s -- and ratio = ms over it."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.frames import Frame, FrameSensor, FrameSet, connector_pairs

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
HBM_BYTES_PER_MS = 8e9  # 8 TB/s

m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


grip, top = Frame(site="grip_site"), Frame(body=m.meta["part_names"][-1])
eight = [FrameSensor(Frame(site=a), ref=Frame(site=b)) for a, b in connector_pairs(m)]
eight += [FrameSensor(grip), FrameSensor(grip, ref=top), FrameSensor(Frame(body=m.meta["part_names"][0])), FrameSensor(Frame(body=m.meta["part_names"][1]))]
assert len(eight) == 8
for name, sensors, vel, jac in (("8_pose", eight, False, False), ("8_pose_vel", eight, True, False), ("8_all", eight, True, True), ("64_all", eight * 8, True, True)):
    sim.set_frames(FrameSet(sensors, velocity=vel, jacobian=jac))
    out = sim.frame_state()
    t = median_ms(lambda: sim.frame_state(out=out))
    torch.cuda.synchronize()
    out_bytes = sum(v.numel() * v.element_size() for v in out.values())
    rec_bytes = n * sim.stride * 4
    bound = (out_bytes + rec_bytes) / HBM_BYTES_PER_MS
    print(json.dumps(dict(case=name, envs=n, sensors=len(sensors), nv=m.nv, velocity=vel, jacobian=jac, reps=reps, ms=round(t, 4), record_mb=round(rec_bytes / 1e6, 2),
                          output_mb=round(out_bytes / 1e6, 2), bound_ms=round(bound, 4), ratio=round(t / bound, 2), gb_per_s=round((out_bytes + rec_bytes) / t / 1e6, 1))), flush=True)
sim.close()

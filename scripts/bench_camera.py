"""Time fsim_render (include/fsim_camera.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and a few random steps,
{1, 2} cameras x {64 x 64, 128 x 128}: device time per render (HIP events around the two launches on the handle's stream, median of
the repeats).  One JSON line per configuration.  The kernels' own times: run under rocprofv3 --kernel-trace --stats (k_cam_pose,
k_cam_ray)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench_common
from furniture_amd.camera import Camera

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dev = sim.device
world = dict(pos=(1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50)                      # the robot, the table and the parts
wrist = dict(pos=(0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, body="right_hand")  # along the gripper
for ncam in (1, 2):
    for size in (64, 128):
        cams = [Camera(width=size, height=size, **c) for c in (world, wrist)[:ncam]]
        sim.set_cameras(cams)
        shape = (n, ncam, size, size)
        out = (torch.empty(shape, device=dev), torch.empty(shape, dtype=torch.int32, device=dev))
        ms = bench_common.times_ms(sim, lambda: sim.render(out=out), reps)
        seg = out[1]
        print(json.dumps(dict(envs=n, cameras=ncam, width=size, height=size, ms_per_render=round(float(np.median(ms)), 4),
                              ms_min=round(float(np.min(ms)), 4), mrays_per_s=round(n * ncam * size * size / np.median(ms) / 1e3, 1),
                              hit_fraction=round(float((seg >= 0).float().mean()), 3))), flush=True)
sim.close()

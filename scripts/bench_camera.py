"""Time fsim_render (include/fsim_camera.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and a few random steps,
{1, 2} cameras x {64 x 64, 128 x 128}: device time per render (HIP events around the two launches on the handle's stream, median of
the repeats).  One JSON line per configuration.  The kernels' own times: run under rocprofv3 --kernel-trace --stats (k_cam_pose,
k_cam_ray)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from furniture_amd.camera import Camera
from furniture_amd.envs import ResetTableSampler, make_config
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import INFO_DIM, FSim, default_config

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m = load_compiled("Sawyer", "table_lack_0825")
ecfg = make_config(unity=False, record_vid=False, furniture_name="table_lack_0825", seed=7)
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
world = dict(pos=(1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50)                      # the robot, the table and the parts
wrist = dict(pos=(0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, body="right_hand")  # along the gripper
for ncam in (1, 2):
    for size in (64, 128):
        cams = [Camera(width=size, height=size, **c) for c in (world, wrist)[:ncam]]
        sim.set_cameras(cams)
        shape = (n, ncam, size, size)
        out = (torch.empty(shape, device=dev), torch.empty(shape, dtype=torch.int32, device=dev))
        for _ in range(3):
            sim.render(out=out)
        torch.cuda.synchronize()
        ms = []
        with torch.cuda.stream(sim.torch_stream):
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sim.render(out=out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        seg = out[1]
        print(json.dumps(dict(envs=n, cameras=ncam, width=size, height=size, ms_per_render=round(float(np.median(ms)), 4),
                              ms_min=round(float(np.min(ms)), 4), mrays_per_s=round(n * ncam * size * size / np.median(ms) / 1e3, 1),
                              hit_fraction=round(float((seg >= 0).float().mean()), 3))), flush=True)
sim.close()

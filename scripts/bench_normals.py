"""Time fsim_render_normals (include/fsim_normals.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: one world camera and world + wrist camera, 64 x 64 each, and one 128 x 128 world camera; normal and shaded image both,
then each alone.  HIP events around calls on the handle's stream, median of the repeats (second argument, 20):
  rays    = fsim_render alone (k_cam_pose + k_cam_ray);
  normals = fsim_render_normals minus rays (k_cam_normal);
  total   = fsim_render_normals.
The bytes bound of the normal pass: depth and segmentation read once (8 B per pixel) and the outputs written once (12 B of normal, 4 B
of shaded picture per pixel), over the 8 TB/s HBM peak.  The per-kernel time comes from rocprofv3 --kernel-trace --stats
(k_cam_normal).  One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.camera import Camera
from furniture_amd.normals import Normals

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dev = sim.device
world = dict(pos=(1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50)                      # the robot, the table and the parts
wrist = dict(pos=(0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, body="right_hand")  # along the gripper


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


cases = [("world64", 1, 64, True, True), ("world_wrist64", 2, 64, True, True), ("world128", 1, 128, True, True),
         ("world64_normal_only", 1, 64, True, False), ("world64_shaded_only", 1, 64, False, True)]
for name, ncam, size, normal, shaded in cases:
    cams = [Camera(width=size, height=size, **c) for c in (world, wrist)[:ncam]]
    sim.set_cameras(cams)
    img = (torch.empty((n, ncam, size, size), device=dev), torch.empty((n, ncam, size, size), dtype=torch.int32, device=dev))
    t_rays = median_ms(lambda: sim.render(out=img))
    sim.set_normals(Normals(normal=normal, shaded=shaded))
    out = sim.render_normals(images=True)
    t_all = median_ms(lambda: sim.render_normals(images=True, out=out))
    torch.cuda.synchronize()
    pixels = n * ncam * size * size
    bytes_ = pixels * (8 + (12 if normal else 0) + (4 if shaded else 0))
    bound_ms = bytes_ / HBM_BYTES_PER_S * 1e3
    row = dict(case=name, envs=n, cameras=ncam, width=size, height=size, normal=normal, shaded=shaded, reps=reps,
               ms_rays=round(t_rays, 4), ms_normals=round(t_all - t_rays, 4), ms_total=round(t_all, 4),
               hit_fraction=round(float((out["camera_segmentation"] >= 0).double().mean()), 3), bytes_bound_mb=round(bytes_ / 1e6, 1),
               bytes_bound_ms=round(bound_ms, 4))
    row["normals_over_bound"] = round(row["ms_normals"] / bound_ms, 2)
    print(json.dumps(row), flush=True)
sim.close()

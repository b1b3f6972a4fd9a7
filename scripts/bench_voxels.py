"""Time fsim_render_voxels (include/fsim_voxels.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: one world camera and world + wrist camera, 64 x 64 each; grids 32^3 and 64 x 64 x 16 over the robot's workspace (parts
and robot kept); and a contention case -- the floor kept too, over a 4 x 4 x 4 grid, so that most pixels land in a few cells.  HIP
events around calls on the handle's stream, median of the repeats (second argument, 20):
  rays    = fsim_render alone (k_cam_pose + k_cam_ray);
  binning = fsim_render_voxels minus rays (k_vox_bin);
  total   = fsim_render_voxels.
The bytes bound of the binning: the two int16 outputs written once (n_envs x cells x 4 B) plus the images read once per LDS chunk of
16384 cells (n_envs x chunks x pixels x 8 B: depth and segmentation), over the 8 TB/s HBM peak.  The per-kernel time comes from
rocprofv3 --kernel-trace --stats (k_vox_bin).  One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.camera import Camera
from furniture_amd.voxels import VoxelGrid

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
CHUNK = 16384             # cells per k_vox_bin workgroup (VOX_CHUNK)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dev = sim.device
world = dict(pos=(1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50)                      # the robot, the table and the parts
wrist = dict(pos=(0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, body="right_hand")  # along the gripper
BOX = ((-0.6, -0.8, -0.05), (1.0, 0.8, 1.55))                                             # the workspace above the table


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


cases = [("world64_32cubed", 1, (32, 32, 32), ("parts", "robot")), ("world_wrist64_32cubed", 2, (32, 32, 32), ("parts", "robot")),
         ("world64_64x64x16", 1, (64, 64, 16), ("parts", "robot")), ("world_wrist64_64x64x16", 2, (64, 64, 16), ("parts", "robot")),
         ("world_wrist64_4cubed_floor", 2, (4, 4, 4), ("parts", "robot", "floor"))]
for name, ncam, dims, include in cases:
    cams = [Camera(width=64, height=64, **c) for c in (world, wrist)[:ncam]]
    sim.set_cameras(cams)
    img = (torch.empty((n, ncam, 64, 64), device=dev), torch.empty((n, ncam, 64, 64), dtype=torch.int32, device=dev))
    t_rays = median_ms(lambda: sim.render(out=img))
    sim.set_voxels(VoxelGrid(dims, BOX, include=include))
    out = sim.render_voxels(images=True)
    t_all = median_ms(lambda: sim.render_voxels(images=True, out=out))
    torch.cuda.synchronize()
    cnt = out["voxel_count"].reshape(n, -1).double()
    cells = dims[0] * dims[1] * dims[2]
    chunks = -(-cells // CHUNK)
    bytes_ = n * cells * 4 + n * chunks * ncam * 64 * 64 * 8
    bound_ms = bytes_ / HBM_BYTES_PER_S * 1e3
    row = dict(case=name, envs=n, cameras=ncam, width=64, height=64, dims=list(dims), include=list(include), reps=reps,
               ms_rays=round(t_rays, 4), ms_binning=round(t_all - t_rays, 4), ms_total=round(t_all, 4),
               binned_mean=round(float(cnt.sum(1).mean()), 1), max_cell_mean=round(float(cnt.max(1).values.mean()), 1),
               occupied_mean=round(float((cnt > 0).sum(1).double().mean()), 1), bytes_bound_mb=round(bytes_ / 1e6, 1),
               bytes_bound_ms=round(bound_ms, 4))
    row["binning_over_bound"] = round(row["ms_binning"] / bound_ms, 2)
    print(json.dumps(row), flush=True)
sim.close()

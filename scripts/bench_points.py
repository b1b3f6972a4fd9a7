"""Time fsim_render_points (include/fsim_points.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and a few random
steps, three cases -- one world camera 64 x 64 with N = 512, world + wrist camera 64 x 64 each with N = 1024, and the world camera in
dense mode.  HIP events around calls on the handle's stream, median of the repeats (second argument, 20):
  rays   = fsim_render alone (k_cam_pose + k_cam_ray);
  gather = a dense-mode fsim_render_points minus rays (k_pts_gather writing every pixel's point);
  fps    = the sampled-mode fsim_render_points minus the dense one (k_pts_fps, plus the gather's candidate writes in place of the dense
           outputs).
Every pixel the cameras see is kept (include parts, robot and floor), so that K, the kept pixels per env, is close to the image size
the issue's cost model assumes.  The per-kernel times come from rocprofv3 --kernel-trace --stats (k_pts_gather, k_pts_fps<PER>).  The
VALU bound of the FPS: n_envs x N x K distance updates at 10 lane-operations each (K: the mean kept-pixel count; the kernel updates
ceil(K / 512) x 512 slots per row), over 7.9e13 fp32 lane-operations per second.  One JSON line per case."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.camera import Camera
from furniture_amd.points import PointCloud

VALU_LANE_OPS_PER_S = 7.9e13  # fp32 vector issue rate of the MI355X: 256 CUs x 128 lanes per clock x 2.4 GHz (non-packed)
OPS_PER_UPDATE = 10           # dx, dy, dz, three products, two sums, the min, the compare of the running best

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dev = sim.device
world = dict(pos=(1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50)                      # the robot, the table and the parts
wrist = dict(pos=(0.0, 0.05, -0.05), quat=(0.0, 1.0, 0.0, 0.0), fovy=80, body="right_hand")  # along the gripper


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


for name, ncam, N in (("world64_n512", 1, 512), ("world_wrist64_n1024", 2, 1024), ("world64_dense", 1, 0)):
    cams = [Camera(width=64, height=64, **c) for c in (world, wrist)[:ncam]]
    sim.set_cameras(cams)
    img = (torch.empty((n, ncam, 64, 64), device=dev), torch.empty((n, ncam, 64, 64), dtype=torch.int32, device=dev))
    t_rays = median_ms(lambda: sim.render(out=img))
    sim.set_points(PointCloud(0))
    dense_out = sim.render_points(images=True)
    t_dense = median_ms(lambda: sim.render_points(images=True, out=dense_out))
    row = dict(case=name, envs=n, cameras=ncam, width=64, height=64, n_points=N, include=["parts", "robot", "floor"], reps=reps,
               ms_rays=round(t_rays, 4), ms_gather=round(t_dense - t_rays, 4))
    spec = PointCloud(N, include=("parts", "robot", "floor"))
    sim.set_points(spec)
    out = sim.render_points(images=True)
    torch.cuda.synchronize()
    K = out["point_cloud_count"].double()
    if N:
        t_all = median_ms(lambda: sim.render_points(images=True, out=out))
        ops_k = n * N * float(K.mean()) * OPS_PER_UPDATE
        ops_p = n * N * float((torch.ceil(K / 512) * 512).mean()) * OPS_PER_UPDATE
        row.update(ms_fps=round(t_all - t_dense, 4), ms_total=round(t_all, 4), kept_mean=round(float(K.mean()), 1), kept_min=int(K.min()),
                   kept_max=int(K.max()), valu_bound_ms_kept=round(ops_k / VALU_LANE_OPS_PER_S * 1e3, 4),
                   valu_bound_ms_slots=round(ops_p / VALU_LANE_OPS_PER_S * 1e3, 4))
        row["fps_over_bound_slots"] = round(row["ms_fps"] / row["valu_bound_ms_slots"], 2)
    else:
        row.update(ms_total=round(t_dense, 4), kept_mean=round(float(K.mean()), 1))
    print(json.dumps(row), flush=True)
sim.close()

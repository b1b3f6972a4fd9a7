"""Time fsim_cast_rays (include/fsim_rays.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: a 4-ray finger sensor on right_hand, a 64 x 16 lidar on right_hand, a 1024-ray world lidar, each with and without the
normal; as the yardstick of the same session, fsim_render of one 32 x 32 world camera (1024 rays behind the camera's tile cull).  HIP
events around calls on the handle's stream (both launches of a call: k_cam_pose + k_ray_cast, or k_cam_pose + k_cam_ray), median of the
repeats (second argument, 20).  One JSON line per case; ratio = ms per ray over the yardstick's ms per pixel."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench_common
from furniture_amd.camera import Camera
from furniture_amd.rays import RaySensor, RaySet, lidar

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dev = sim.device


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


# the yardstick: 1024 coherent rays per env through the camera's tile cull
sim.set_cameras([Camera((1.6, -1.1, 1.3), lookat=(0.3, 0.0, 0.3), fovy=50, width=32, height=32)])
img = (torch.empty((n, 1, 32, 32), device=dev), torch.empty((n, 1, 32, 32), dtype=torch.int32, device=dev))
t_cam = median_ms(lambda: sim.render(out=img))
print(json.dumps(dict(case="render_32x32", envs=n, rays=1024, reps=reps, ms=round(t_cam, 4), ns_per_ray=round(t_cam * 1e6 / (n * 1024), 4),
                      hit_fraction=round(float((img[1] >= 0).double().mean()), 3))), flush=True)
sensors = {"finger4": RaySensor((0.0, 0.0, 0.06), [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.0, 1.0)], body="right_hand", tmax=0.5),
           "hand_lidar_64x16": RaySensor((0.0, 0.0, 0.0), lidar(64, 16, elevation=(-75.0, 75.0)), body="right_hand"),
           "world_lidar_1024": RaySensor((0.3, 0.0, 1.1), lidar(64, 16, elevation=(-60.0, 20.0)), tmax=6.0)}
for name, sensor in sensors.items():
    for normal in (False, True):
        sim.set_rays(RaySet([sensor], normal=normal))
        out = sim.cast_rays()
        t = median_ms(lambda: sim.cast_rays(out=out))
        torch.cuda.synchronize()
        rays = sensor.n_rays
        print(json.dumps(dict(case=name, envs=n, rays=rays, normal=normal, reps=reps, ms=round(t, 4), ns_per_ray=round(t * 1e6 / (n * rays), 4),
                              ratio_to_render=round((t / rays) / (t_cam / 1024), 2), hit_fraction=round(float((out["ray_geom"] >= 0).double().mean()), 3))), flush=True)
sim.close()

"""Time fsim_probe_distance (include/fsim_probes.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases: 8 pad probes (four per finger) on right_hand, the 10 x 10 x 10 hand grid, a 16 x 16 x 4 world grid, each with and without
the gradient; as the yardstick of the same session, fsim_cast_rays of the 64 x 16 lidar on right_hand (1024 rays).  HIP events around
calls on the handle's stream (both launches of a call: k_cam_pose + k_probe_dist, or k_cam_pose + k_ray_cast), median of the repeats
(second argument, 20).  Then Sawyer + chair_agne_0010, whose seat is a 459-plane hull: the hand grid again and a grid around the seat.  One JSON line per case;
ratio = ms per probe over the yardstick's ms per ray."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench_common
from furniture_amd.probes import ProbeSensor, ProbeSet, grid_points
from furniture_amd.rays import RaySensor, RaySet, lidar

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


# the yardstick: the 1024-ray hand lidar of scripts/bench_rays.py
sim.set_rays(RaySet([RaySensor((0.0, 0.0, 0.0), lidar(64, 16, elevation=(-75.0, 75.0)), body="right_hand")]))
rout = sim.cast_rays()
t_ray = median_ms(lambda: sim.cast_rays(out=rout))
print(json.dumps(dict(case="cast_rays_hand_lidar_64x16", envs=n, rays=1024, reps=reps, ms=round(t_ray, 4), ns_per_ray=round(t_ray * 1e6 / (n * 1024), 4),
                      hit_fraction=round(float((rout["ray_geom"] >= 0).double().mean()), 3))), flush=True)
sim.set_rays(None)
pads = [(sx * 0.03, sy * 0.01, 0.12 + dz) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for dz in (0.0, 0.02)]
sensors = {"pads8": ProbeSensor((0.0, 0.0, 0.0), pads, body="right_hand", dmax=0.1),
           "hand_grid_10x10x10": ProbeSensor((0.0, 0.0, 0.0), grid_points((-0.12, -0.12, -0.05), (0.12, 0.12, 0.25), (10, 10, 10)), body="right_hand", dmax=0.3),
           "world_grid_16x16x4": ProbeSensor((0.0, 0.0, 0.0), grid_points((-0.3, -0.6, -0.02), (0.9, 0.6, 0.6), (16, 16, 4)), dmax=1.0)}
def run(tag, sensors):
    for name, sensor in sensors.items():
        for gradient in (False, True):
            sim.set_probes(ProbeSet([sensor], gradient=gradient))
            out = sim.probe_distance()
            t = median_ms(lambda: sim.probe_distance(out=out))
            torch.cuda.synchronize()
            k = sensor.n_probes
            print(json.dumps(dict(case=tag + name, envs=n, probes=k, gradient=gradient, reps=reps, ms=round(t, 4), ns_per_probe=round(t * 1e6 / (n * k), 4),
                                  ratio_to_rays=round((t / k) / (t_ray / 1024), 2), within_dmax=round(float((out["probe_geom"] >= 0).double().mean()), 3),
                                  inside=round(float((out["probe_distance"] < 0).double().mean()), 4))), flush=True)


run("", sensors)
sim.close()
# a model with a hull collider: chair_agne_0010's seat, a disc of 459 face planes.  The hand grid again (the hull is walked only by the
# probes its bound does not prune) and a 10 x 10 x 10 grid in the seat's own frame, 0.2 m around it, where most probes walk the planes
m, sim = bench_common.make("Sawyer", "chair_agne_0010", n)
hull = [int(g) for g in np.asarray(m.arrays["cg_orig"]) if int(m.arrays["geom_type"][int(g)]) == 7][0]
seat = m.meta["body_names"][int(m.arrays["geom_bodyid"][hull])]
run("chair_", {"hand_grid_10x10x10": sensors["hand_grid_10x10x10"],
               "seat_grid_10x10x10": ProbeSensor((0.0, 0.0, 0.0), grid_points((-0.2, -0.2, -0.2), (0.2, 0.2, 0.2), (10, 10, 10)), body=seat, dmax=0.25, exclude=None)})
sim.close()

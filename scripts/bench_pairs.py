"""Time fsim_pair_distance (include/fsim_pairs.h): Sawyer + table_lack_0825, 4096 envs (first argument) after a reset and three random
steps.  Cases, each a pair set of its own: the gripper against the five parts (five sensors), the arm links against all parts (one sensor,
dmax 2), every part against every other (ten sensors); as the yardstick of the same session, fsim_probe_distance of the 8 pad probes of
scripts/bench_probes.py.  HIP events around calls on the handle's stream (both launches of a call: k_cam_pose + k_pair_dist, or k_cam_pose +
k_probe_dist), median of the repeats (second argument, 20).  Then Sawyer + chair_agne_0010, whose seat is a convex hull of 433 vertices:
the gripper against the seat.  One JSON line per case; ratio = ms over the yardstick's ms."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench_common
from furniture_amd.pairs import PairSensor, PairSet, gripper_bodies
from furniture_amd.probes import ProbeSensor, ProbeSet

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20


m, sim = bench_common.make("Sawyer", "table_lack_0825", n)


def median_ms(fn):
    return bench_common.median_ms(sim, fn, reps)


def parts(m):
    cg = np.asarray(m.arrays["cg_orig"])
    gbody = np.asarray(m.arrays["geom_bodyid"])[cg]
    pid = np.asarray(m.arrays["cg_partid"])
    return [m.meta["body_names"][int(gbody[pid == p][0])] for p in sorted(set(pid[pid >= 0].tolist()))]


def arm(m):
    cg = np.asarray(m.arrays["cg_orig"])
    gbody = np.asarray(m.arrays["geom_bodyid"])[cg]
    red = np.asarray(m.arrays["body_red"])
    rob = np.asarray(m.arrays["cg_isrobot"]) != 0
    return [m.meta["body_names"][b] for b in sorted(set(gbody[rob & (red[gbody] != 0)].tolist()))]


# the yardstick: the 8 pad probes of scripts/bench_probes.py
pads = [(sx * 0.03, sy * 0.01, 0.12 + dz) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for dz in (0.0, 0.02)]
sim.set_probes(ProbeSet([ProbeSensor((0.0, 0.0, 0.0), pads, body="right_hand", dmax=0.1)]))
pout = sim.probe_distance()
t_pad = median_ms(lambda: sim.probe_distance(out=pout))
print(json.dumps(dict(case="probe_distance_pads8", envs=n, probes=8, reps=reps, ms=round(t_pad, 4))), flush=True)
sim.set_probes(None)


def run(tag, m, cases):
    for name, sensors in cases.items():
        for vectors in (False, True):
            sim.set_pairs(PairSet(sensors, fromto=vectors, normal=vectors))
            out = sim.pair_distance()
            t = median_ms(lambda: sim.pair_distance(out=out))
            torch.cuda.synchronize()
            k = sum(len(s.pairs(m)) for s in sensors)
            print(json.dumps(dict(case=tag + name, envs=n, sensors=len(sensors), pairs=k, vectors=vectors, reps=reps, ms=round(t, 4), ns_per_pair=round(t * 1e6 / (n * k), 3),
                                  ratio_to_pads8=round(t / t_pad, 2), within_dmax=round(float((out["pair_geoms"][..., 0] >= 0).double().mean()), 3),
                                  overlapping=round(float((out["pair_distance"] < 0).double().mean()), 4), mean_distance=round(float(out["pair_distance"].double().mean()), 4))), flush=True)


P, G = parts(m), gripper_bodies(m)
run("", m, {"gripper_to_5_parts": [PairSensor(G, p, dmax=3.0) for p in P], "arm_to_parts": [PairSensor(arm(m), P, dmax=2.0)],
            "all_part_pairs": [PairSensor(P[i], P[j], dmax=3.0) for i in range(len(P)) for j in range(i + 1, len(P))]})
sim.close()
# a model with a hull collider: chair_agne_0010's seat (433 hull vertices: every support evaluation walks them)
m, sim = bench_common.make("Sawyer", "chair_agne_0010", n)
hull = [int(g) for g in np.asarray(m.arrays["cg_orig"]) if int(m.arrays["geom_type"][int(g)]) == 7][0]
run("chair_", m, {"gripper_to_hull": [PairSensor(gripper_bodies(m), [hull], dmax=3.0)]})
sim.close()

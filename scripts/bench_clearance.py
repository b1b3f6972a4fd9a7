"""Time fsim_clearance (include/fsim_clearance.h): Sawyer + table_lack_0825, 4096 envs (--envs) after a reset and three random steps, the
robot against every part and the floor (furniture_amd.clearance.robot_clearance_sensors) over the arm's seven joints and the two fingers,
K = 1, 16 and 64 candidates per env, without and with a carried leg (one carry rule, set in every env, and the leg's own sensor).
Next to each: the only way to the same answers without it, K rounds of set_state(candidate), pair_distance and a restoring set_state with
the same sensors.  (With the carried leg that loop is handed the leg's K poses for nothing -- it writes qpos words it was given -- while
the call composes them on the device: the comparison flatters the loop.)

Wall-clock time of the whole call or loop including the device work it enqueues (perf_counter around it and a device synchronize), since
the loop's cost is host calls that each settle the handle; median of the repeats after 2 warm-up rounds.  One JSON line per case.

Run without --case, the script is a driver: every case runs in a fresh child process under a time limit of its own (--limit seconds,
default 120), one after the other, and the first that fails, or runs out of time, ends the run."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 16, 64)
CASES = ["%s_k%d%s" % (path, k, c) for c in ("", "_carry") for k in KS for path in ("call", "loop")]

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--limit", type=int, default=120)
ap.add_argument("--case", choices=CASES)
args = ap.parse_args()

if args.case is None:
    for case in CASES:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(args.envs), "--reps", str(args.reps), "--case", case], timeout=args.limit).returncode
        if rc != 0:
            sys.exit("bench_clearance: case %s ended with status %d; nothing more is started" % (case, rc))
    sys.exit(0)

import numpy as np
import torch
import bench_common
from furniture_amd.clearance import ClearanceSet, carried_sensor, robot_clearance_sensors
from furniture_amd.pairs import PairSet

path, k, carry = args.case.split("_")[0], int(args.case.split("_")[1][1:]), args.case.endswith("_carry")
n = args.envs
m, sim = bench_common.make("Sawyer", "table_lack_0825", n)
dofs = [int(d) for d in np.asarray(m.arm_dofadr).reshape(-1)] + [int(d) for d in np.asarray(m.arrays["grip_dofadr"]).reshape(-1)]
leg = m.meta["part_names"][1]
sensors = [robot_clearance_sensors(m)] + ([carried_sensor(m, leg)] if carry else [])
qa = torch.as_tensor(np.asarray(m.arrays["dof_qposadr"]).astype(np.int64)[dofs], device=sim.device)
rec = sim.get_state("qpos")["qpos"].clone()
gen = torch.Generator(device=sim.device).manual_seed(3)
cand = (rec[:, qa][:, None, :] + 0.4 * (torch.rand((n, k, len(dofs)), device=sim.device, generator=gen) - 0.5)).contiguous()


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


if path == "call":
    sim.set_clearance(ClearanceSet(dofs, sensors, carry=[(leg, "right_hand")] if carry else (), max_candidates=k))
    mask = torch.ones(n, dtype=torch.uint8, device=sim.device) if carry else None
    out = sim.clearance(cand, mask)
    ms = timed(lambda: sim.clearance(cand, mask, out=out), args.reps)
    launches = 2 * -(-n // (min(n * k, 32768) // k))
else:
    sim.set_pairs(PairSet(sensors))
    outs = [sim.pair_distance() for _ in range(k)]
    padr = int(np.asarray(m.part_qposadr).reshape(-1)[1])
    qk = rec[:, None, :].repeat(1, k, 1)  # the K states to write, built outside the timing (with carry: the leg's words as well, given)
    qk[:, :, qa] = cand
    if carry:
        qk[:, :, padr:padr + 3] += 0.01
    qk = [qk[:, j].contiguous() for j in range(k)]

    def loop():
        for j in range(k):
            sim.set_state(qpos=qk[j])
            sim.pair_distance(out=outs[j])
            sim.set_state(qpos=rec)
    ms = timed(loop, max(2, args.reps // 3))
    launches = None
print(json.dumps(dict(case=args.case, envs=n, K=k, carry=carry, sensors=len(sensors), pairs=sum(len(s.pairs(m)) for s in sensors), ms=round(ms, 3),
                      us_per_candidate=round(1e3 * ms / (n * k), 4), launches=launches)), flush=True)
sim.close()

"""What the scripts/bench_*.py of the observation and sensor families share: the handle they measure on and the timing of one call.
Seed 7, a reset and three random steps (RandomState(0)), so that the figures of earlier profiles/*.jsonl stay comparable."""
import numpy as np
import torch
from furniture_amd.envs import ResetTableSampler, make_config
from furniture_amd.mjcf.model import load_compiled
from furniture_amd.sim import INFO_DIM, FSim, default_config


def make(agent, furniture, n):
    """-> (model, handle) of n envs of agent + furniture after a reset and three random steps"""
    m = load_compiled(agent, furniture)
    ecfg = make_config(unity=False, record_vid=False, furniture_name=furniture, seed=7)
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
    return m, sim


def times_ms(sim, fn, reps, warmup=3):
    """the times of reps calls of fn, each between HIP events on the handle's stream, after warmup calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    with torch.cuda.stream(sim.torch_stream):
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return ms


def median_ms(sim, fn, reps, warmup=3):
    return float(np.median(times_ms(sim, fn, reps, warmup)))

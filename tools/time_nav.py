"""The navigator's three costs on one GPU, the default world, by events, in alternating rounds:

(a) se_nav_actions at n envs beside se_sample_actions on the same states (the same kind of
    kernel: one lane per env, the world read in place);
(b) se_rollout_nav at m rollouts of K positions beside se_rollout (max_steps = max_attempts = K)
    and the agent-index se_rollout_plan of K random unit moves, from the same states;
(c) the wall time of se_nav_create (host breadth-first passes, two allocations, two uploads) at
    the default world's 5 ports and at 64 random ports.

The legs of (a) and of (b) alternate within a round; one JSON line per leg and round (events ms
per launch), then a summary line per part with each leg's median and range over the rounds.

    python tools/time_nav.py [--n 1048576] [--steps 100] [--rounds 7] [--launches 3] [--warm 30]
                             [--load 0] [--out profiles/nav/time_nav.jsonl]

--warm launches of every leg run first, unrecorded, as tools/time_rollout_plan.py does. The
states are those after reset() and --preroll random steps (default 0: every ship in port, bound
for another).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rounds(legs, a, count, emit, part):
    for _ in range(max(a.warm, 1)):
        for run in legs.values():
            run(0)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    base = count
    for r in range(a.rounds):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kept = []
            e0.record()
            for _ in range(a.launches):
                kept.append(run(base))
                base += count
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.launches
            times[name].append(ms)
            row = {"part": part, "leg": name, "round": r, "n": count, "launches": a.launches, "kernel_ms": round(ms, 4)}
            if kept[0] is not None:
                row["counted_steps_per_launch"] = sum(int(s.sum().item()) for s in kept) / a.launches
            emit(row)
    emit({"part": part, "summary": {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                                           "max_ms": round(max(v), 4)} for name, v in times.items()},
          "n": count, "steps": a.steps, "rounds": a.rounds, "load": a.load, "preroll": a.preroll,
          "device": torch.cuda.get_device_name(0)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--launches", type=int, default=3)
    p.add_argument("--warm", type=int, default=30)
    p.add_argument("--load", type=int, default=0)
    p.add_argument("--preroll", type=int, default=0)
    p.add_argument("--seed", type=int, default=2026)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from shippingenv_amd import _native as N
    from shippingenv_amd.nav import VecNavigator
    from shippingenv_amd.vec import VecEnv, random_water_ports

    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    n, K = a.n, a.steps
    env = VecEnv(n, seed=a.seed, device="cuda:0")
    env.reset()
    for t in range(a.preroll):
        env.step(env.gen_actions(t))
    nav = VecNavigator(env, load=a.load)
    emit({"part": "world", "max_leg": nav.max_leg, "refuel_below": nav.refuel_below, "P": env.P, "H": env.H, "W": env.W})
    out3 = tuple(torch.empty(n, dtype=torch.int32, device=env.device) for _ in range(3))

    # (a) the policy kernels
    def run_nav_actions(_):
        nav.actions()

    def run_nav_actions_all(_):
        nav.actions(agent=True, dist=True)

    def run_sample(base):
        env.sample_actions(base // n, out=out3)

    rounds({"nav_actions": run_nav_actions, "nav_actions_agent_dist": run_nav_actions_all, "sample_actions": run_sample},
           a, n, emit, "a")

    # (b) the rollouts
    src = torch.arange(n, dtype=torch.int32, device=env.device)
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    idx = torch.randint(0, 4, (K, n), dtype=torch.int32, device=env.device, generator=gen)
    legs = {
        "rollout_nav": lambda base: nav.rollout(src, steps=K, rollout_base=base).steps,
        "rollout": lambda base: env.rollout(src, max_steps=K, max_attempts=K, rollout_base=base)[1],
        "plan_agent": lambda base: env.rollout_plan(src, actions=idx, rollout_base=base).steps,
    }
    rounds(legs, a, n, emit, "b")
    nav.close()

    # (c) se_nav_create, wall time (it synchronises through its two blocking copies)
    lib = N.lib()
    for label, ports in (("default_5_ports", None), ("random_64_ports", random_water_ports(env.water, 64, a.seed))):
        small = VecEnv(1024, seed=a.seed, device="cuda:0") if ports is None else VecEnv(1024, seed=a.seed, device="cuda:0", ports=ports)
        torch.cuda.synchronize()
        walls = []
        for _ in range(a.rounds + 2):
            h = C.c_void_p()
            t0 = time.perf_counter()
            N.check(lib.se_nav_create(C.byref(h), small._h))
            walls.append((time.perf_counter() - t0) * 1e3)
            lib.se_nav_destroy(h)
        walls = walls[2:]  # the first two warm the allocator
        emit({"part": "c", "leg": label, "P": small.P, "create_ms": [round(v, 4) for v in walls],
              "median_ms": round(statistics.median(walls), 4), "min_ms": round(min(walls), 4), "max_ms": round(max(walls), 4)})
        small.close()
    env.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()

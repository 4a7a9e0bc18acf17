"""Scripted rollouts (se_rollout_plan) beside the random rollouts (se_rollout) they restate, from
the same states: m rollouts from ships after reset(), plans of K random unit moves (typed, and
as agent indices), against se_rollout with max_steps = max_attempts = K. The three legs
alternate within a round; one JSON line per leg and round (events ms per launch, counted steps
per launch), then one summary line with each leg's median and spread over the rounds.

    python tools/time_rollout_plan.py [--m 1048576] [--steps 100] [--rounds 5] [--launches 3] [--warm 30]

--warm launches of every leg run first, unrecorded: the clocks take a few hundred launches' worth
of time to settle, and the first rounds otherwise read up to 8% high.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--m", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--launches", type=int, default=3)
    p.add_argument("--warm", type=int, default=30)
    p.add_argument("--seed", type=int, default=2026)
    a = p.parse_args()
    from shippingenv_amd.vec import VecEnv

    m, K = a.m, a.steps
    env = VecEnv(m, seed=a.seed, device="cuda:0")
    env.reset()
    src = torch.arange(m, dtype=torch.int32, device=env.device)
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    idx = torch.randint(0, 4, (K, m), dtype=torch.int32, device=env.device, generator=gen)  # N, E, S, W
    dx = torch.tensor([0, -1, 0, 1], dtype=torch.int32, device=env.device)[idx.long()]
    dy = torch.tensor([-1, 0, 1, 0], dtype=torch.int32, device=env.device)[idx.long()]
    one = torch.ones_like(idx)

    legs = {
        "plan_typed": lambda base: env.rollout_plan(src, one, dx, dy, rollout_base=base).steps,
        "plan_agent": lambda base: env.rollout_plan(src, actions=idx, rollout_base=base).steps,
        "rollout": lambda base: env.rollout(src, max_steps=K, max_attempts=K, rollout_base=base)[1],
    }
    for _ in range(max(a.warm, 1)):
        for run in legs.values():
            run(0)
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    base = m
    for r in range(a.rounds):
        for name, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kept = []
            e0.record()
            for _ in range(a.launches):
                kept.append(run(base))
                base += m
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.launches
            times[name].append(ms)
            steps = sum(int(s.sum().item()) for s in kept) / a.launches
            print(json.dumps({"leg": name, "round": r, "m": m, "steps": K, "launches": a.launches,
                              "kernel_ms": round(ms, 4), "counted_steps_per_launch": steps}), flush=True)
    print(json.dumps({"summary": {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                                         "max_ms": round(max(v), 4)} for name, v in times.items()},
                      "m": m, "steps": K, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
